"""What the many-job hit profile's GPU tests (test_gpu_hit_profile_jobs.py) presuppose, proved without a GPU: the planted fixtures
reach the designed bytes on the CPU checker, job by job; and the sweep command's --full mode — its arguments, and against a stub
context which selections go into which call and which files come out."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_jobs_sets as js
import util
from conftest import ROOT


# ---- the fixtures on the checker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", js.FIXTURES)
def test_fixture_reaches_its_design_on_the_checker(tmp_path, name, strand):
    f = js.fixture(name, strand)
    got, chunks = js.checker_bytes(tmp_path, name, strand)
    assert chunks == f["chunks"]
    search = f["search"]
    r = search[0]
    for j, cap in enumerate(f["caps"]):
        h = got[j]
        print(name, strand, "job", j, "cap", cap, h[:9].tolist())
        assert int(h[0]) == f["design"][j], (name, strand, j, h[:9].tolist())
        assert int(h.max()) <= min(cap, js.T_TOP)
        # (e) the copies of the planted read get its byte, in lower case too, and its reverse complement; reads shorter than k get none
        for i, x in enumerate(search):
            if x == r or x == r.lower() or x == util.revcomp(r):
                assert h[i] == h[0], (name, j, i)
            if len(x) < js.K:
                assert h[i] == 0, (name, j, i)
    assert sum(1 for x in search if x == r) == 41 and any(b"N" in x for x in search) and any(len(x) < js.K for x in search)
    # the N inside a planted window costs the job that owns the window a hit
    with_n = search[1]
    assert with_n[45:46] == b"N"
    owner = {"stop": 1, "crosstalk": 0, "max": 0}[name]
    if f["caps"][owner] > 1:
        assert got[owner][1] < got[owner][0], (name, got[owner][:3].tolist())


def test_the_wrong_kernels_would_show():
    """the designs, spelled out with the greedy rule: what a global stop, a shared `free` and a sum over slots would give instead"""
    k = js.K
    g = js.gs.greedy
    # (a) a walk that ends at the first capped job never reaches window 40
    assert g(range(0, 11), k) == 1 and g(range(40, 81), k) == 3
    # (b) one `free` for both slots: job 0 takes 0, 20, 40 and job 1 is left with 20 and 40
    free, cnt = 0, [0, 0]
    for s in range(0, 51):
        takers = [j for j, (lo, hi) in enumerate(((0, 40), (10, 50))) if lo <= s <= hi and s >= free]
        for j in takers:
            cnt[j] += 1
        if takers:
            free = s + k
    assert cnt == [3, 2] and g(range(0, 41), k) == 3 and g(range(10, 51), k) == 3
    # (c) max, not sum
    assert g(range(0, 21), k) == 2 and g(range(40, 81), k) == 3


# ---- the sweep command: --full -----------------------------------------------------------------------------------------------------------
def _run_sweep(cwd, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "commet_amd.sweep"] + list(args), cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_sweep_full_argument_handling(tmp_path):
    r = _run_sweep(tmp_path, "--help")
    assert r.returncode == 0 and b"--full" in r.stdout and b"index_and_search -f" in r.stdout
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "two.txt", "w").write("A:a.fa\nZ:z.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    r = _run_sweep(tmp_path, "-i", "two.txt", "-s", "s.txt", "-k", "20", "-o", "out", "--max-t", "3", "--full")
    assert r.returncode == 2 and b"Only one set of files is allowed for indexing" in r.stderr
    for bad in ("0", "256"):
        r = _run_sweep(tmp_path, "-i", "i.txt", "-s", "s.txt", "-k", "20", "-o", "out", "--max-t", bad, "--full")
        assert r.returncode == 2 and b"--max-t" in r.stderr
    r = _run_sweep(tmp_path, "-i", "i.txt", "-s", "s.txt", "-k", "20", "-o", "out", "--max-t", "3", "--full=1")
    assert r.returncode == 2
    assert not os.path.exists(tmp_path / "out")


class _StubSet:
    def __init__(self, files, counts):
        self.files, self.counts = list(files), [counts[f] for f in files]
        self.num_reads = sum(self.counts)

    def file_reads(self):
        return list(self.counts)


class _StubApi:
    """Context / ReadSet / tags_at as sweep.py uses them; the hit counts are made up from the selections so that every call's
    inputs show in the next call's"""

    def __init__(self, counts):
        from commet_amd.api import tags_at
        api = self
        self.tags_at = tags_at
        self.calls, self.counts = [], counts

        class ReadSet:
            @staticmethod
            def from_fasta(ctx, files):
                return _StubSet(files, api.counts)

        class Context:
            def __init__(self, k, t=2, device=0):
                self.k = k

            def __enter__(self):
                return self

            def __exit__(self, *a):
                pass

            def set_option(self, name, value):
                api.calls.append(("option", name, value))

            def index_and_profile(self, index_rs, search_sets, index_select=None, search_selects=None, max_hits=8):
                api.calls.append(("profile", index_rs, list(search_sets), index_select, list(search_selects), max_hits))
                hits = []
                for q, rs in enumerate(search_sets):
                    h = (np.arange(rs.num_reads) * 7 + int(max_hits)) % (int(max_hits) + 2)
                    sel = search_selects[q]
                    if sel is not None:
                        h = np.where(util.bools_from_bits(sel, rs.num_reads), h, 0)
                    hits.append(np.minimum(h, max_hits).astype(np.uint8))
                return hits, dict(n_chunks=1, search_launches=len(search_sets))

            def index_many_and_profile(self, index_sets, search_rs, index_selects=None, search_select=None, max_hits=8):
                api.calls.append(("many", list(index_sets), search_rs, list(index_selects), search_select, list(max_hits)))
                hits = []
                for j, cap in enumerate(max_hits):
                    n_sel = int(util.bools_from_bits(index_selects[j], index_sets[j].num_reads).sum())
                    h = (np.arange(search_rs.num_reads) * 3 + n_sel) % (cap + 2)
                    hits.append(np.minimum(h, cap).astype(np.uint8))
                return hits, dict(n_chunks=len(max_hits), search_launches=1)

        self.ReadSet, self.Context = ReadSet, Context


def test_sweep_full_pass_sequence_against_a_stub(tmp_path, capsys):
    from commet_amd import matrix_io, sweep
    d = tmp_path
    counts = {"dir/a1.fa": 13, "a2.fa": 8, "b1.fa": 17, "sub/b2.fa": 9, "c.fa": 5}
    a_sel = np.arange(13) % 3 != 0
    matrix_io.write_bv(str(d / "a1.bv"), "filter", 13, util.bits_from_bools(a_sel))
    open(d / "i.txt", "w").write("A:dir/a1.fa,a1.bv;a2.fa\n")
    open(d / "s.txt", "w").write("C:c.fa\nB:b1.fa;sub/b2.fa\n")           # (sorted by tag: B is the first search set)
    api = _StubApi(counts)
    T = 3
    cwd = os.getcwd()
    os.chdir(d)
    try:
        assert sweep.main(["-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", str(T), "-o", "out", "--full"], api=api) == 0
    finally:
        os.chdir(cwd)
    err = capsys.readouterr().err
    assert "first search set only (B)" in err and "1 more set(s) ignored" in err
    calls = [c for c in api.calls if c[0] != "option"]
    assert [c[0] for c in calls] == ["profile", "many"] + ["profile"] * T
    n_a, n_b = 21, 26
    a_bits = util.bits_from_bools(np.concatenate([a_sel, np.ones(8, bool)]))
    # pass 1: A under its own selection -> B (no selection), max_hits = T
    _, irs, srs, isel, ssels, cap = calls[0]
    assert irs.files == ["dir/a1.fa", "a2.fa"] and [s.files for s in srs] == [["b1.fa", "sub/b2.fa"]] and cap == T
    assert isel.tobytes() == a_bits.tobytes() and ssels == [None]
    rs_a, rs_b = irs, srs[0]
    h1 = api.Context(20).index_and_profile(rs_a, [rs_b], isel, [None], T)[0][0]
    api.calls.pop()
    t1 = [api.tags_at(h1, t) for t in range(1, T + 1)]
    assert len({x.tobytes() for x in t1}) == T                         # (the thresholds tell the reads apart)
    # pass 2: T jobs, job t indexes B under T1(t); all search A under A's selection; caps 1..T
    _, isets, srs2, isels, ssel2, caps = calls[1]
    assert all(s is rs_b for s in isets) and len(isets) == T and srs2 is rs_a and caps == [1, 2, 3]
    assert [x.tobytes() for x in isels] == [x.tobytes() for x in t1] and ssel2.tobytes() == a_bits.tobytes()
    h2 = api.Context(20).index_many_and_profile(isets, rs_a, isels, ssel2, caps)[0]
    api.calls.pop()
    rows = []
    for t in range(1, T + 1):
        # pass 3 of t: A under T2(t) -> B under T1(t), max_hits = t
        _, irs3, srs3, isel3, ssels3, cap3 = calls[1 + t]
        t2 = api.tags_at(h2[t - 1], t)
        assert irs3 is rs_a and srs3 == [rs_b] and cap3 == t
        assert isel3.tobytes() == t2.tobytes() and [x.tobytes() for x in ssels3] == [t1[t - 1].tobytes()]
        h3 = api.Context(20).index_and_profile(rs_a, [rs_b], isel3, ssels3, t)[0][0]
        api.calls.pop()
        assert sorted(os.listdir(d / "out" / f"t{t}")) == ["a1.fa_in_B.bv", "a2.fa_in_B.bv", "b1.fa_in_A.bv", "b2.fa_in_A.bv"]
        for tag, files, h, other in (("A", [("dir/a1.fa", 13), ("a2.fa", 8)], h2[t - 1], "B"), ("B", [("b1.fa", 17), ("sub/b2.fa", 9)], h3, "A")):
            pos = 0
            for f, n in files:
                want = (h[pos:pos + n] >= t)
                pos += n
                data = open(d / "out" / f"t{t}" / (os.path.basename(f) + "_in_" + other + ".bv"), "rb").read()
                assert data == f"{f} in {other}\n#{n}\n".encode() + util.bits_from_bools(want).tobytes()[:n // 8 + 1], (t, f)
                rows.append(f"{t};{tag};{f};{n};{int(want.sum())}")
    assert n_a == rs_a.num_reads and n_b == rs_b.num_reads
    assert open(d / "out" / "sweep.csv").read().strip().split("\n") == ["t;set;file;reads;shared"] + rows


def test_sweep_without_full_makes_one_profile_call(tmp_path):
    from commet_amd import sweep
    d = tmp_path
    open(d / "i.txt", "w").write("A:a2.fa\n")
    open(d / "s.txt", "w").write("C:c.fa\nB:b1.fa\n")
    api = _StubApi({"a2.fa": 8, "b1.fa": 17, "c.fa": 5})
    cwd = os.getcwd()
    os.chdir(d)
    try:
        assert sweep.main(["-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", "2", "-o", "out"], api=api) == 0
    finally:
        os.chdir(cwd)
    calls = [c for c in api.calls if c[0] != "option"]
    assert [c[0] for c in calls] == ["profile"] and [s.files for s in calls[0][2]] == [["b1.fa"], ["c.fa"]]
    assert sorted(os.listdir(d / "out" / "t2")) == ["b1.fa_in_A.bv", "c.fa_in_A.bv"]


# ---- the scenario cases: their jobs have the chunks they are meant to have -------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(js.SCENARIO_CASES))
def test_scenario_case_has_its_chunks_on_the_checker(tmp_path, name):
    case = js.scenario_case(name, tmp_path)
    truth, chunks = js.scenario_truth(name, tmp_path)
    print(name, "max_kmer", case["max_kmer"], "chunks", chunks, "found", [int((h > 0).sum()) for h in truth], "of", truth[0].size)
    assert chunks == [job["chunks"] for job in case["jobs"]]
    for (want, cap), job, h in zip(js.SCENARIO_CASES[name]["jobs"], case["jobs"], truth):
        assert want in ("all", "empty") or job["chunks"] == want
        assert int(h.max(initial=0)) <= cap
        assert (want == "empty") == (job["chunks"] == 0) and (job["chunks"] > 0 or not h.any())
    assert sum(1 for h in truth if h.any()) >= 2                       # (the jobs find reads of the searched set)
    if name in ("k8_mixed", "k20_eight", "k32_nine"):                  # one set under several selections, no two of them equal
        by_source = {}
        for job in case["jobs"]:
            by_source.setdefault(job["source"], []).append(job["sel"].tobytes())
        assert any(len(v) >= 2 for v in by_source.values()) and all(len(set(v)) == len(v) for v in by_source.values())


def test_scenario_cases_cover_the_pass_shapes():
    shapes = {n: [c if isinstance(c, int) else 0 for c, _ in s["jobs"]] for n, s in js.SCENARIO_CASES.items() if all(c != "all" for c, _ in s["jobs"])}
    assert js.passes_of(shapes["k20_eight"]) == (1, 0) and js.passes_of(shapes["k32_nine"]) == (1, 1)
    assert js.passes_of(shapes["k8_mixed"]) == (2, 3)                  # 3 + 2 + 3 | 1 + 1; alone: 9 chunks, the empty one, 8 chunks (a pass of one job)
    slots = {(s["k"] > 32, 2 if sum(x) <= 2 else 4 if sum(x) <= 4 else 8) for n, s in js.SCENARIO_CASES.items() if n in shapes
             for x in [[c for c in shapes[n] if 0 < c <= 8]] if sum(x) <= 8}
    assert slots >= {(w, nf) for w in (False, True) for nf in (2, 4, 8)}
    assert {c for s in js.SCENARIO_CASES.values() for _, c in s["jobs"]} >= {1, 2, 5, 255}
    assert {c for s in js.SCENARIO_CASES.values() for c, _ in s["jobs"]} >= {1, 2, 3, 8, 9, "empty"}
    assert {len(s["jobs"]) for s in js.SCENARIO_CASES.values()} >= {2, 3, 8, 9}
