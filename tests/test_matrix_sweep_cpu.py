"""The threshold-swept matrix (`python -m commet_amd.matrix --max-t T`, commet_amd/matrix_sweep.py), host logic on the CPU:
what --max-t refuses; the sweep's job DAG with the CPU checker standing in for the two thresholds calls, against the checker driven
through Commet.py's job sequence at every t; and the numpy model of hits_tags_kernel's contract (hits_tags_cases.py, which the GPU
test compares the kernel with) against the host code it replaces: api.tags_at, matrix_io.split_bits + popcount."""
import os
import sys

import numpy as np
import pytest

import hits_tags_cases as htc
from conftest import ROOT
from oracle_engine import OracleEngine
from sweep_sets import four_sets

GOLD = os.path.join(ROOT, "tests", "golden")


# ---- what --max-t refuses -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,why", [(["--max-t", "3", "--gpus", "2"], "one rank"), (["--max-t", "3", "--set-budget-gb", "1"], "set-budget-gb"),
                                       (["--max-t", "3", "-l", "50"], "depend on t"), (["--max-t", "0"], "1..255"), (["--max-t", "256"], "1..255")])
def test_max_t_refusals(tmp_path, capsys, monkeypatch, extra, why):
    from commet_amd import matrix
    for v in ("WORLD_SIZE", "RANK", "COMMET_MATRIX_SET_BUDGET_GB"):
        monkeypatch.delenv(v, raising=False)
    (tmp_path / "sets.txt").write_text("a: a.fa\nb: b.fa\n")
    with pytest.raises(SystemExit) as ex:
        matrix.main([str(tmp_path / "sets.txt"), "-k", "20", "-o", str(tmp_path / "out")] + extra)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert "error:" in err and why in err, err
    assert not (tmp_path / "out").exists()


def test_a_launchers_ranks_are_refused(tmp_path, capsys, monkeypatch):
    from commet_amd import matrix, matrix_sweep
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit):
        matrix.main([str(tmp_path / "sets.txt"), "-k", "20", "--max-t", "2"])
    assert "one rank" in capsys.readouterr().err
    with pytest.raises(ValueError, match="one rank"):
        matrix_sweep.run(str(tmp_path / "sets.txt"), str(tmp_path / "out"), k=20, max_t=2)


# ---- the sweep's DAG on the CPU checker ----------------------------------------------------------------------------------------------------------
class SweepOracle(OracleEngine):
    """the two thresholds calls, by running the checker once per t"""
    calls = None

    def __init__(self, k, t, local_rank):
        super().__init__(k, t, local_rank)
        SweepOracle.calls = dict(single=0, many=[])

    @staticmethod
    def _per_file(bits, counts):
        import util
        bools, out, pos = util.bools_from_bits(bits, sum(counts)), [], 0
        for c in counts:
            out.append(int(bools[pos:pos + c].sum()))
            pos += c
        return np.array(out, dtype=np.uint64)

    def index_and_thresholds(self, index, searches, isel, ssels, max_t):
        SweepOracle.calls["single"] += 1
        tags, shared = [[None] * max_t for _ in searches], [[None] * max_t for _ in searches]
        for t in range(1, max_t + 1):
            self.t = t
            tg, _st, info = self.index_and_search(index, searches, isel, ssels)
            for s, rs in enumerate(searches):
                tags[s][t - 1], shared[s][t - 1] = tg[s], self._per_file(tg[s], rs["counts"])
        return tags, shared, info

    def index_many_and_thresholds(self, indexes, search, isels, ssel, ts):
        SweepOracle.calls["many"].append(len(indexes))
        tags, shared = [], []
        for index, isel, t in zip(indexes, isels, ts):
            self.t = t
            tg, _st, info = self.index_and_search(index, [search], isel, [ssel])
            tags.append(tg[0])
            shared.append(self._per_file(tg[0], search["counts"]))
        return tags, shared, info


def checker_matrix(names, files, bvs, k, t, out):
    """the checker through Commet.py's job sequence at one t: its .bv files and the three csv files in `out`/"""
    import oracle_binding as ob
    import util
    from commet_amd.matrix_io import write_matrices
    sys.path.insert(0, GOLD)
    from make_golden import commet_jobs

    def cfg(si, restrict_to=None):
        return names[si] + ":" + ";".join(f + "," + (b if restrict_to is None else f"{out}/{f}_in_{names[restrict_to]}.bv") for f, b in zip(files[si], bvs[si]))

    os.makedirs(out)
    for _kind, idx, searches, restr in commet_jobs(names):
        open("i.txt", "w").write(cfg(idx, restr) + "\n")
        open("s.txt", "w").write("".join(cfg(s) + "\n" for s in searches))
        rc, *_ = ob.index_and_search("i.txt", "s.txt", out, out, k, t)
        assert rc == 0
    N = len(names)
    count = lambda path: int(util.bools_from_bits(util.read_bv(path)[2], util.read_bv(path)[1]).sum())
    considered = [sum(count(b) for b in bvs[s]) for s in range(N)]
    mat = [[considered[a] if a == b else sum(count(f"{out}/{f}_in_{names[b]}.bv") for f in files[a]) for b in range(N)] for a in range(N)]
    write_matrices(out + "/", names, considered, mat)
    return mat


def same_outputs(got_dir, want_dir):
    """every .bv and .csv of want_dir is in got_dir, byte for byte, and got_dir holds no other -> how many .bv"""
    want = sorted(f for f in os.listdir(want_dir) if f.endswith((".bv", ".csv")))
    assert sorted(os.listdir(got_dir)) == want, (sorted(os.listdir(got_dir)), want)
    for f in want:
        assert open(os.path.join(got_dir, f), "rb").read() == open(os.path.join(want_dir, f), "rb").read(), (got_dir, f)
    return sum(f.endswith(".bv") for f in want)


def test_sweep_dag_matches_the_checker_at_every_t(tmp_path, monkeypatch):
    from commet_amd import matrix_sweep
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    names, files, bvs = four_sets()
    k, T = 20, 3
    res = matrix_sweep.run("sets.txt", "out/", k=k, max_t=T, verbose=False, engine_factory=SweepOracle)
    # per reference set one J1 call and one J2 call of (targets x T) jobs; per target one J3 call of (references x T) jobs
    assert SweepOracle.calls["single"] == 3 and SweepOracle.calls["many"] == [9, 3, 6, 6, 3, 9], SweepOracle.calls
    for t in range(1, T + 1):
        mat = checker_matrix(names, files, bvs, k, t, f"orc{t}")
        assert same_outputs(f"out/t{t}", f"orc{t}") == 5 * 3          # 5 files, each searched in the 3 other sets
        assert res["matrices"][t] == mat
    assert not [f for f in os.listdir("out") if f.endswith(".log") or "_in_" in f]
    assert res["matrices"][1] != res["matrices"][3]                    # (the thresholds do tell the sets apart)


# ---- the model of the kernel's contract against the host code it replaces --------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in htc.SIZES if n <= 1025])
def test_model_matches_tags_at_and_popcount(n):
    from commet_amd import api, matrix_io
    for cut, file_reads in htc.file_cuts(n).items():
        assert sum(file_reads) == n and all(c >= 0 for c in file_reads), (n, cut, file_reads)
        for rot, (t_first, n_t) in enumerate(htc.RANGES):
            if n_t > 8 and n > 65:
                continue                                          # (the read-by-read model at 255 thresholds: small sizes only)
            hits = htc.designed_bytes(n, file_reads, t_first, n_t, rot)
            tags, shared = htc.model(hits, file_reads, t_first, n_t)
            fast_tags, fast_shared = htc.fast_model(hits, file_reads, t_first, n_t)
            assert np.array_equal(shared, fast_shared)
            for ti in range(n_t):
                assert np.array_equal(tags[ti], fast_tags[ti])
                assert np.array_equal(tags[ti], api.tags_at(hits, t_first + ti)), (n, cut, t_first, ti)
                per_file = [matrix_io.popcount(b, c) for b, c in zip(matrix_io.split_bits(tags[ti], file_reads), file_reads)]
                assert shared[ti].tolist() == per_file, (n, cut, t_first, ti)


def test_designed_bytes_hold_every_edge_value():
    """0, t - 1, t, t + 1 and 255 all occur either side of a boundary, for the first and the last threshold of the range"""
    n, file_reads = 4099, htc.file_cuts(4099)["two_in_word"]
    seen = set()
    for rot in range(10):
        h = htc.designed_bytes(n, file_reads, 3, 2, rot)
        seen.update(int(h[p]) for p in htc.boundaries(n, file_reads))
        assert int(h[0]) in (0, 2, 3, 4, 5, 255) and int(h[n - 1]) in (0, 2, 3, 4, 5, 255)
    assert seen == {0, 2, 3, 4, 5, 255}
