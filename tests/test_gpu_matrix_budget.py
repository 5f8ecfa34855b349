"""The N x N driver under --set-budget-gb on the device: a 12-set matrix (fixed-length and ragged sets mixed, one set of two files) whose
sets may hold a third of what they hold together — every .bv and CSV byte for byte what the unconstrained run leaves, with the default
filters and with -l -n -e -m (the device filter runs while a set is resident, before its first offload)."""
import os

import pytest

pytestmark = pytest.mark.gpu

N_SETS, READS = 12, 30000


@pytest.fixture(scope="module", autouse=True)
def _tools():
    from commet_amd import build
    build.build_lib()
    build.build_tools()


@pytest.fixture(scope="module")
def twelve(tmp_path_factory):
    from commet_amd import synth
    d = tmp_path_factory.mktemp("twelve")
    lines = []
    for s in range(N_SETS):
        if s % 3 == 1:                                               # ragged: 40 .. 160 bases
            b, o = synth.synth_set_ragged(s, READS, 40, 160)
            path = str(d / f"r{s}.fa")
            synth.write_fasta_ragged(path, b, o)
            fl = [path]
        elif s == 5:                                                 # two files
            b, o = synth.synth_set(s, READS, 100)
            h = READS // 2
            fl = [str(d / "m5a.fa"), str(d / "m5b.fa")]
            synth.write_fasta(fl[0], b[: h * 100], o[: h + 1])
            synth.write_fasta(fl[1], b[h * 100:], o[h:] - o[h])
        else:
            b, o = synth.synth_set(s, READS, 100)
            path = str(d / f"f{s}.fa")
            synth.write_fasta_fast(path, b, READS, 100)
            fl = [path]
        lines.append(f"set{s}: " + "; ".join(fl) + "\n")
    (d / "sets.txt").write_text("".join(lines))
    return d


def _same_outputs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    n_bv = 0
    for f in fa:
        x, y = open(os.path.join(a, f), "rb").read(), open(os.path.join(b, f), "rb").read()
        if f.endswith(".log"):                                    # times differ; the counts do not (as tests/test_gpu_read_filter.py)
            x, y = x.split(b"\n")[-2], y.split(b"\n")[-2]
        assert x == y, f
        n_bv += f.endswith(".bv")
    return n_bv


@pytest.mark.parametrize("opts", [dict(), dict(l=70, n=2, e=1.8, m=20000)], ids=["default_filters", "l_n_e_m"])
def test_budget_of_four_sets_leaves_the_unconstrained_runs_files(twelve, tmp_path, opts):
    import commet_amd
    from commet_amd import matrix, residency
    lines = open(twelve / "sets.txt").read().strip().split("\n")
    files = [[f.strip() for f in ln.split(":")[1].split(";")] for ln in lines]
    sizes = [commet_amd.files_packed_bytes(fl)[2] for fl in files]
    budget = 4 * max(sizes)
    assert sum(sizes) > 2.5 * budget
    free = matrix.run(str(twelve / "sets.txt"), str(tmp_path / "free"), k=32, t=2, verbose=False, **opts)
    assert "set_reloads" not in free
    res = matrix.run(str(twelve / "sets.txt"), str(tmp_path / "tight"), k=32, t=2, verbose=False, set_budget_gb=(budget + 0.5) / 2**30, **opts)
    print({f: res[f] for f in ("set_budget_bytes", "set_loads", "set_reloads", "set_offloads", "peak_set_bytes", "reload_s", "set_wait_s",
                               "jobs_s", "total_s", "j1_builds")}, "unconstrained:", free["jobs_s"], free["total_s"])
    n_files = sum(len(fl) for fl in files)
    assert _same_outputs(str(tmp_path / "free"), str(tmp_path / "tight")) == n_files * (N_SETS - 1) + n_files
    assert res["matrix"] == free["matrix"] and res["considered"] == free["considered"]
    assert res["set_budget_bytes"] == budget
    assert res["set_reloads"] > 0
    assert res["peak_set_bytes"] <= budget
    assert N_SETS <= res["set_loads"] <= residency.equal_size_load_bound(N_SETS, 4) == 30
    assert res["set_loads"] - N_SETS == res["set_reloads"] <= res["set_offloads"]
    if opts:
        assert any(c < READS for c in res["considered"])
