"""commet_amd.matrix.run under a set budget (--set-budget-gb), host logic on the CPU: the CPU checker stands in for the GPU engine, with
sets that can leave and come back.  Every file of the budgeted run equals the unconstrained run's (logs: apart from their times, as
tests/test_gpu_read_filter.py compares them)."""
import os
import subprocess
import threading

import pytest

from conftest import ROOT
from oracle_engine import OracleEngine

BIN = os.path.join(ROOT, "commet_amd", "bin")


@pytest.fixture(scope="module", autouse=True)
def _filter_tool():
    if not os.path.exists(os.path.join(BIN, "filter_reads")):
        os.makedirs(BIN, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(BIN, "filter_reads"),
                        os.path.join(ROOT, "commet_amd", "csrc", "host", "filter_reads.cpp"), "-lz"], check=True)


class BudgetedOracle(OracleEngine):
    """sets that can be offloaded: a resident flag per set, counters, and the two things the driver must never do"""
    budget = None
    log = None

    def __init__(self, k, t, local_rank):
        super().__init__(k, t, local_rank)
        self.mu = threading.Lock()
        self.resident_bytes = 0
        BudgetedOracle.log = dict(offloads=0, restores=0, parses=0, peak=0, jobs_on_offloaded=0)

    def packed_bytes(self, files):
        return sum(os.path.getsize(f) for f in files)

    def _add(self, rs, sign):
        with self.mu:
            self.resident_bytes += sign * rs["bytes"]
            BudgetedOracle.log["peak"] = max(BudgetedOracle.log["peak"], self.resident_bytes)
            if BudgetedOracle.budget is not None and self.resident_bytes > BudgetedOracle.budget:
                raise RuntimeError(f"{self.resident_bytes} bytes of sets resident, the budget is {BudgetedOracle.budget}")

    def parse(self, files):
        rs = super().parse(files)
        rs["bytes"], rs["resident"] = self.packed_bytes(files), True
        BudgetedOracle.log["parses"] += 1
        self._add(rs, +1)
        return rs

    def offload(self, rs):
        assert rs["resident"]
        rs["resident"] = False
        BudgetedOracle.log["offloads"] += 1
        self._add(rs, -1)

    def restore(self, rs):
        assert not rs["resident"]
        rs["resident"] = True
        BudgetedOracle.log["restores"] += 1
        self._add(rs, +1)

    def release(self, rs):
        if rs.get("resident"):
            rs["resident"] = False
            self._add(rs, -1)

    def index_and_search(self, index, searches, isel, ssels):
        for rs in [index] + list(searches):
            if not rs["resident"]:
                BudgetedOracle.log["jobs_on_offloaded"] += 1
                raise RuntimeError("a job names an offloaded set")
        return super().index_and_search(index, searches, isel, ssels)


def _six_sets(tmp_path):
    from commet_amd import synth
    L = 80
    shape = [(500, 2), (700, 1), (400, 3), (650, 2), (550, 1), (600, 2)]      # (reads, files) per set
    names, files = [f"s{s}" for s in range(6)], []
    for s, (n, nf) in enumerate(shape):
        b, o = synth.synth_set(s, n, L, copy_frac=0.3)
        fl, per = [], n // nf
        for j in range(nf):
            lo, hi = j * per, (n if j == nf - 1 else (j + 1) * per)
            path = str(tmp_path / f"s{s}_{j}.fa")
            synth.write_fasta(path, b[lo * L:hi * L], o[lo:hi + 1] - o[lo])
            fl.append(path)
        files.append(fl)
    (tmp_path / "sets.txt").write_text("".join(f"{names[s]}: " + "; ".join(files[s]) + "\n" for s in range(6)))
    sizes = [sum(os.path.getsize(f) for f in fl) for fl in files]
    return str(tmp_path / "sets.txt"), sizes


def _same_files(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    n_bv = 0
    for f in fa:
        x, y = open(os.path.join(a, f), "rb").read(), open(os.path.join(b, f), "rb").read()
        if f.endswith(".log"):                                    # times differ; the counts do not
            x, y = x.split(b"\n")[-2], y.split(b"\n")[-2]
        assert x == y, f
        n_bv += f.endswith(".bv")
    return n_bv


@pytest.mark.parametrize("opts", [dict(), dict(l=45, e=1.9, m=900)], ids=["default_filters", "l_e_m"])
def test_budget_of_three_sets_leaves_the_unconstrained_runs_files(tmp_path, opts):
    from commet_amd import matrix, residency
    sets_txt, sizes = _six_sets(tmp_path)
    BudgetedOracle.budget = None
    free = matrix.run(sets_txt, str(tmp_path / "free"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle, **opts)
    assert "set_reloads" not in free and "set_budget_bytes" not in free          # without the option: the report it always was
    budget = sum(sorted(sizes)[-3:])
    BudgetedOracle.budget = budget
    res = matrix.run(sets_txt, str(tmp_path / "tight"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle,
                     set_budget_gb=(budget + 0.5) / 2**30, **opts)
    log = BudgetedOracle.log
    n_files = sum(len(open(sets_txt).read().split("\n")[s].split(";")) for s in range(6))
    assert _same_files(str(tmp_path / "free"), str(tmp_path / "tight")) == n_files * 5 + n_files    # every file in the 5 other sets + its filter
    assert res["matrix"] == free["matrix"] and res["considered"] == free["considered"]
    assert res["set_budget_bytes"] == budget
    assert res["set_reloads"] > 0 and res["set_reloads"] == log["restores"] == res["set_loads"] - 6
    assert res["set_offloads"] == log["offloads"] >= res["set_reloads"]
    assert log["parses"] == 6 and log["jobs_on_offloaded"] == 0
    assert log["peak"] <= budget and res["peak_set_bytes"] <= budget
    assert res["set_loads"] == sum(1 for st in residency.plan(sizes, budget) if st[0] == "load")
    assert res["j1_builds"] >= 5 and res["reload_s"] >= 0 and res["set_wait_s"] >= 0
    if opts:
        assert any(c < n for c, n in zip(res["considered"], (500, 700, 400, 650, 550, 600)))    # the filters removed reads


def test_env_variable_sets_the_budget(tmp_path, monkeypatch):
    from commet_amd import matrix
    sets_txt, sizes = _six_sets(tmp_path)
    budget = sum(sorted(sizes)[-2:])
    BudgetedOracle.budget = budget
    monkeypatch.setenv("COMMET_MATRIX_SET_BUDGET_GB", repr((budget + 0.5) / 2**30))
    res = matrix.run(sets_txt, str(tmp_path / "out"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle)
    assert res["set_budget_bytes"] == budget and res["peak_set_bytes"] <= budget and res["set_reloads"] > 0


def test_budget_below_the_two_largest_sets_names_them(tmp_path):
    from commet_amd import matrix
    sets_txt, sizes = _six_sets(tmp_path)
    BudgetedOracle.budget = None
    with pytest.raises(ValueError) as ei:
        matrix.run(sets_txt, str(tmp_path / "out"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle,
                   set_budget_gb=(sum(sorted(sizes)[-2:]) - 1) / 2**30)
    assert "s1" in str(ei.value) and "s3" in str(ei.value)
    assert BudgetedOracle.log["parses"] == 0                       # before any set was loaded, let alone a job run
    assert not any("_in_" in f for f in os.listdir(tmp_path / "out"))


def test_several_ranks_with_a_budget_are_refused(tmp_path):
    from commet_amd import matrix
    sets_txt, _ = _six_sets(tmp_path)

    class TwoRanks:
        world, rank, local_rank = 2, 0, 0

    with pytest.raises(ValueError, match="one rank"):
        matrix.run(sets_txt, str(tmp_path / "out"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle, ranks=TwoRanks(),
                   set_budget_gb=1.0)


def test_an_engine_whose_sets_cannot_leave_is_refused(tmp_path):
    from commet_amd import matrix
    sets_txt, _ = _six_sets(tmp_path)
    with pytest.raises(RuntimeError, match="offload"):
        matrix.run(sets_txt, str(tmp_path / "out"), k=20, t=2, verbose=False, engine_factory=OracleEngine, set_budget_gb=1.0)


def test_given_filter_files_under_a_budget(tmp_path):
    """the set file names a .bv per file (Commet.py then runs no filter): the budgeted run reads them at a set's first load as the
    unconstrained run does when the set arrives — the vectors are a default run's, a few reads taken out by hand"""
    from commet_amd import matrix
    sets_txt, sizes = _six_sets(tmp_path)
    BudgetedOracle.budget = None
    matrix.run(sets_txt, str(tmp_path / "prior"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle)
    os.makedirs(tmp_path / "given")
    lines, reads = [], []
    for ln in open(sets_txt).read().split("\n")[:6]:
        name, fl = ln.split(":")[0], [f.strip() for f in ln.split(":")[1].split(";")]
        items, total = [], 0
        for f in fl:
            nb, bits = matrix.read_bv(str(tmp_path / "prior" / (os.path.basename(f) + ".bv")))
            bits = bits.copy()
            for r in (0, 9, nb // 2, nb - 1):                     # (the first and the last read of the file among them)
                bits[r >> 3] &= 0xFF ^ (1 << (r & 7))
            bv = str(tmp_path / "given" / (os.path.basename(f) + ".bv"))
            matrix.write_filter_bv(bv, f, nb, bits)
            items.append(f + "," + bv)
            total += nb
        lines.append(name + ": " + "; ".join(items) + "\n")
        reads.append(total)
    (tmp_path / "sets_bv.txt").write_text("".join(lines))
    free = matrix.run(str(tmp_path / "sets_bv.txt"), str(tmp_path / "free"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle)
    budget = sum(sorted(sizes)[-3:])
    BudgetedOracle.budget = budget
    res = matrix.run(str(tmp_path / "sets_bv.txt"), str(tmp_path / "tight"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle,
                     set_budget_gb=(budget + 0.5) / 2**30)
    n_files = sum(ln.count(",") for ln in lines)
    assert _same_files(str(tmp_path / "free"), str(tmp_path / "tight")) == n_files * 5       # (no filter files: they were given)
    assert res["matrix"] == free["matrix"] and res["considered"] == free["considered"]
    assert reads == [500, 700, 400, 650, 550, 600]
    assert all(c < r for c, r in zip(res["considered"], reads))
    assert res["considered"] == [r - 4 * ln.count(",") for r, ln in zip(reads, lines)]
    assert res["set_reloads"] > 0 and BudgetedOracle.log["peak"] <= budget


def test_job_order_of_one_rank_with_everything_loaded_first(tmp_path, monkeypatch):
    """COMMET_MATRIX_PIPELINE=0 on one rank: the reference sets in their order, J1 then the J2 jobs of each, a target's J3 jobs as soon as
    its last reference set is through — the [kind, search set or reference, other sets] of every library call (the CPU checker has no
    call for several jobs on one search set: one row per job), as the driver made them before its scheduler was a function of its own"""
    from commet_amd import matrix
    sets_txt, _ = _six_sets(tmp_path)
    monkeypatch.setenv("COMMET_MATRIX_PIPELINE", "0")
    BudgetedOracle.budget = None
    res = matrix.run(sets_txt, str(tmp_path / "out"), k=20, t=2, verbose=False, engine_factory=BudgetedOracle)
    assert [row[:3] for row in res["per_rank"][0]["job_log"]] == [
        ["J1", 0, [1, 2, 3, 4, 5]], ["J2", 0, [1]], ["J2", 0, [2]], ["J2", 0, [3]], ["J2", 0, [4]], ["J2", 0, [5]], ["J3", 1, [0]],
        ["J1", 1, [2, 3, 4, 5]], ["J2", 1, [2]], ["J2", 1, [3]], ["J2", 1, [4]], ["J2", 1, [5]], ["J3", 2, [0]], ["J3", 2, [1]],
        ["J1", 2, [3, 4, 5]], ["J2", 2, [3]], ["J2", 2, [4]], ["J2", 2, [5]], ["J3", 3, [0]], ["J3", 3, [1]], ["J3", 3, [2]],
        ["J1", 3, [4, 5]], ["J2", 3, [4]], ["J2", 3, [5]], ["J3", 4, [0]], ["J3", 4, [1]], ["J3", 4, [2]], ["J3", 4, [3]],
        ["J1", 4, [5]], ["J2", 4, [5]], ["J3", 5, [0]], ["J3", 5, [1]], ["J3", 5, [2]], ["J3", 5, [3]], ["J3", 5, [4]]]
    assert all(len(row) == 6 for row in res["per_rank"][0]["job_log"])
