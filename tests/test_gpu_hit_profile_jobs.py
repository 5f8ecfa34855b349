"""commet_index_many_and_profile (capi/multi_profile.hpp; hits_jobs_kernel, hit_profile_jobs.hpp): several hit-profile jobs on one search
set, their chunk filters side by side in one hits pass.  Every job's bytes must be what commet_index_and_profile gives for it alone,
and what the CPU checker gives at every t: on planted fixtures that a global stop, a shared `free` or a sum over a job's slots get
wrong (hit_profile_jobs_sets.py, proved on the checker in test_hit_profile_jobs_cpu.py), over scenario sets in every pass shape, with
the passes really shared, without room for them, after poison, and through `python -m commet_amd.sweep --full`."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_jobs_sets as js
import util
from conftest import ROOT
from scenarios import Scenario

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "commet_amd", "bin", "index_and_search")
GOLD = os.path.join(ROOT, "tests", "golden")


def _commet():
    import commet_amd
    return commet_amd


def _load(ctx, reads):
    return _commet().ReadSet.from_files(ctx, [util.to_batch(reads)])


def _timed(ctx, call):
    """-> (the call's result, {kernel: launches})"""
    ctx.set_option("kernel_timing", 1)
    try:
        out = call()
        times = ctx.kernel_times()
    finally:
        ctx.set_option("kernel_timing", 0)
    return out, {n: times[n][0] for n in times}


@pytest.fixture(scope="module")
def truth_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("jobs_truth")


@pytest.fixture(scope="module")
def wide_ctx():
    """ONE context for the k = 33 cases: its eight 4 GiB filter slots are asked for once"""
    with _commet().Context(k=33, t=2) as ctx:
        yield ctx


# ---- 1. the planted fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", js.FIXTURES)
def test_planted_fixture(truth_dir, name, strand):
    f = js.fixture(name, strand)
    want, chunks = js.checker_bytes(truth_dir, name, strand)
    with _commet().Context(k=js.K, t=2) as ctx:
        ctx.set_option("max_kmer", f["max_kmer"])
        sets, qrs = [_load(ctx, index) for index in f["jobs"]], _load(ctx, f["search"])
        (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=f["caps"]))
        alone = [ctx.index_and_profile(rs, [qrs], max_hits=cap)[0][0] for rs, cap in zip(sets, f["caps"])]
    for j in range(len(sets)):
        print(name, strand, "job", j, "cap", f["caps"][j], "got", hits[j][:9].tolist(), "checker", want[j][:9].tolist())
    assert ran.get("hits_jobs_kernel") == 1 and info["search_launches"] == 1, (ran, info)
    assert info["n_chunks"] == sum(chunks) and info["probes"] == 0 and info["reads_scanned"] == len(f["search"])
    for j in range(len(sets)):
        assert np.array_equal(hits[j], want[j]), (name, strand, j, hits[j][:9].tolist(), want[j][:9].tolist())
        assert np.array_equal(hits[j], alone[j]), (name, strand, j)
        assert int(hits[j][0]) == f["design"][j]


# ---- 2. scenario sets: the many-job call against the single calls and the checker ----------------------------------------------------------
def _scenario_sets(ctx, case):
    """-> (search set, its selection bits or None, [index set per job], [selection bits per job])"""
    commet, scn = _commet(), case["scn"]
    loaded = {}

    def load(nme):
        if nme not in loaded:
            loaded[nme] = commet.ReadSet.from_files(ctx, [util.to_batch(util.parse_reads(os.path.join(scn.dir, fa))) for fa, _, _, _ in scn.sets[nme]])
        return loaded[nme]

    bits = lambda sel: None if sel is None else util.bits_from_bools(sel)
    return (load(case["search"]), bits(case["search_sel"]), [load(job["source"]) for job in case["jobs"]], [bits(job["sel"]) for job in case["jobs"]]), loaded


def _run_scenario_case(ctx, case, truth, chunks, name):
    ctx.set_option("max_kmer", case["max_kmer"])
    (qrs, qsel, sets, sels), loaded = _scenario_sets(ctx, case)
    caps = [job["cap"] for job in case["jobs"]]
    try:
        (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, index_selects=sels, search_select=qsel, max_hits=caps))
        alone = [ctx.index_and_profile(rs, [qrs], sel, [qsel], max_hits=cap) for rs, sel, cap in zip(sets, sels, caps)]
    finally:
        for rs in loaded.values():
            rs.close()
    shared, n_alone = js.passes_of(chunks)
    print(name, "chunks", chunks, "shared passes", shared, "alone", n_alone, ran.get("hits_jobs_kernel"), info["search_launches"])
    for j, (h, (a, ainfo)) in enumerate(zip(hits, alone)):
        print(name, "job", j, "cap", caps[j], "found", int((h > 0).sum()), "of", h.size, "max", int(h.max(initial=0)))
        assert np.array_equal(h, a[0]), (name, j, np.nonzero(h != a[0])[0][:10].tolist())
        assert np.array_equal(h, truth[j]), (name, j, np.nonzero(h != truth[j])[0][:10].tolist())
        assert ainfo["n_chunks"] == chunks[j], (name, j, ainfo["n_chunks"], chunks[j])
    assert ran.get("hits_jobs_kernel", 0) == shared, (name, ran)
    assert info["n_chunks"] == sum(chunks) and info["probes"] == 0
    assert info["kmers_indexed"] == sum(a[1]["kmers_indexed"] for a in alone) and info["reads_indexed"] == sum(a[1]["reads_indexed"] for a in alone)
    return info


@pytest.mark.parametrize("name", sorted(n for n, s in js.SCENARIO_CASES.items() if s["k"] != 33))
def test_scenario_case(truth_dir, name):
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [job["chunks"] for job in case["jobs"]]
    with _commet().Context(k=case["k"], t=2) as ctx:
        _run_scenario_case(ctx, case, truth, chunks, name)


@pytest.mark.parametrize("name", sorted(n for n, s in js.SCENARIO_CASES.items() if s["k"] == 33))
def test_scenario_case_wide_keys(truth_dir, wide_ctx, name):
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [job["chunks"] for job in case["jobs"]]
    _run_scenario_case(wide_ctx, case, truth, chunks, name)


def test_bad_arguments():
    commet = _commet()
    f = js.fixture("stop", 0)
    with commet.Context(k=js.K, t=2) as ctx:
        sets, qrs = [_load(ctx, index) for index in f["jobs"]], _load(ctx, f["search"])
        for bad in ([0, 1], [1, 256], [1, -1]):
            with pytest.raises(commet.CommetError, match="max_hits"):
                ctx.index_many_and_profile(sets, qrs, max_hits=bad)
        with pytest.raises(commet.CommetError, match="one entry per job"):
            ctx.index_many_and_profile(sets, qrs, max_hits=[1])
        with pytest.raises(commet.CommetError, match="against itself"):
            ctx.index_many_and_profile([sets[0], qrs], qrs, max_hits=2)
        hits, info = ctx.index_many_and_profile([], qrs)
        assert hits == [] and info["search_launches"] == 0
        hits, info = ctx.index_many_and_profile(sets[:1], qrs, max_hits=1)      # one job: the single call
        assert hits[0][0] == 1 and info["search_launches"] == 1


# ---- 3. the passes are really shared -----------------------------------------------------------------------------------------------------
def test_eight_one_chunk_jobs_share_one_pass(truth_dir):
    name = "k20_eight"
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [1] * 8
    caps = [job["cap"] for job in case["jobs"]]
    with _commet().Context(k=case["k"], t=2) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        (qrs, qsel, sets, sels), _ = _scenario_sets(ctx, case)
        call = lambda: ctx.index_many_and_profile(sets, qrs, index_selects=sels, search_select=qsel, max_hits=caps)
        (shared, info), ran = _timed(ctx, call)
        assert info["search_launches"] == 1 and ran.get("hits_jobs_kernel") == 1 and info["reads_scanned"] == qrs.num_reads, (info, ran)
        for option, value in (("multi_job", 1), ("chunk_group", 1)):
            ctx.set_option(option, value)
            (single, info1), ran1 = _timed(ctx, call)
            ctx.set_option(option, 0 if option == "multi_job" else 8)
            assert info1["search_launches"] == 8 and "hits_jobs_kernel" not in ran1, (option, info1, ran1)
            assert all(np.array_equal(a, b) for a, b in zip(shared, single)), option
        ctx.set_option("multi_job", 2)
        (again, info2), ran2 = _timed(ctx, call)
        assert info2["search_launches"] == 1 and all(np.array_equal(a, b) for a, b in zip(shared, again))
        # groups of four slots: two passes of four jobs
        ctx.set_option("multi_job", 0)
        ctx.set_option("chunk_group", 4)
        (fours, info4), ran4 = _timed(ctx, call)
        assert info4["search_launches"] == 2 and ran4.get("hits_jobs_kernel") == 2 and all(np.array_equal(a, b) for a, b in zip(shared, fours))
    assert all(np.array_equal(a, b) for a, b in zip(shared, truth))


# ---- 4., 5. no room, poison: k = 26, the bucketed build under the options of the filter-byte tests ----------------------------------------
_SLOT_CASE = {}


def _slot_case(d):
    """three jobs of 2, 3 and 1 chunks (six slots: a pass at stride 8) and a search set that every job finds reads of; the checker's bytes"""
    import test_gpu_alloc_refusal as tar
    if not _SLOT_CASE:
        k = tar.SLOT_K
        jobs = [tar.slot_job(k, c, seed=20 + j) for j, c in enumerate((2, 3, 1))]
        assert len({j["max_kmer"] for j in jobs}) == 1
        search = [jobs[i // 3 % len(jobs)]["search"][i] for i in range(len(jobs[0]["search"]))]
        caps = [1, 5, 2]
        truth = []
        for j, (job, cap) in enumerate(zip(jobs, caps)):
            counts, chunks = js.checker_counts(os.path.join(str(d), f"slot_j{j}"), k, job["index"], search, job["max_kmer"], cap)
            assert chunks == job["n_chunks"] and counts.any()
            truth.append(counts)
        _SLOT_CASE.update(k=k, jobs=jobs, search=search, caps=caps, truth=truth)
    return _SLOT_CASE


def test_no_room_for_the_slots(truth_dir):
    import test_gpu_alloc_refusal as tar
    c = _slot_case(truth_dir)
    k, caps = c["k"], c["caps"]
    fresh = lambda ctx: ([tar.load(ctx, j["index"]) for j in c["jobs"]], tar.load(ctx, c["search"]))
    with tar.context(k, c["jobs"][0]["max_kmer"]) as ctx:
        sets, qrs = fresh(ctx)
        (base, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=caps))
        assert ran.get("hits_jobs_kernel") == 1 and info["search_launches"] == 1 and info["n_chunks"] == 6, (ran, info)
        for j in range(3):
            assert np.array_equal(base[j], c["truth"][j]), j
    with tar.context(k, c["jobs"][0]["max_kmer"]) as ctx:
        sets, qrs = fresh(ctx)
        with tar.refusing(at_least=4 * tar.filter_bytes(k)) as r:              # six slots, asked for as eight, then as six: neither is granted
            (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=caps))
        print("no room", ran, r.seen, info)
        assert r.seen["refused"] >= 2 and r.seen["last_refused_bytes"] % tar.filter_bytes(k) == 0, r.seen
        assert "hits_jobs_kernel" not in ran and ran.get("hits_group_kernel") == 2 and ran.get("hits_kernel") == 1, ran
        assert info["n_chunks"] == 6 and info["search_launches"] == 3, info        # the jobs alone, not doubled
        for j in range(3):
            assert np.array_equal(hits[j], base[j]), j
        (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=caps))   # disarmed: shared again
        assert ran.get("hits_jobs_kernel") == 1 and info["search_launches"] == 1 and all(np.array_equal(a, b) for a, b in zip(hits, base)), ran


def test_no_room_for_the_byte_arrays(truth_dir):
    """the jobs' byte arrays refused by count: the context has run the call job by job, so they are the first thing a sharing call asks for"""
    import test_gpu_alloc_refusal as tar
    c = _slot_case(truth_dir)
    k, caps = c["k"], c["caps"]
    with tar.context(k, c["jobs"][0]["max_kmer"], multi_job=1) as ctx:
        sets, qrs = [tar.load(ctx, j["index"]) for j in c["jobs"]], tar.load(ctx, c["search"])
        base, _ = ctx.index_many_and_profile(sets, qrs, max_hits=caps)
        ctx.set_option("multi_job", 0)
        with tar.refusing(nth=1) as r:
            (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=caps))
        print("no bytes", ran, r.seen)
        n_lines = (len(c["search"]) + 255) // 256
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 3 * 256 * n_lines, r.seen
        assert "hits_jobs_kernel" not in ran and info["search_launches"] == 3, (ran, info)
        for j in range(3):
            assert np.array_equal(hits[j], base[j]) and np.array_equal(hits[j], c["truth"][j]), j


def test_after_poison(truth_dir):
    import job_filters as jf
    import test_gpu_alloc_refusal as tar
    c = _slot_case(truth_dir)
    with tar.context(c["k"], c["jobs"][0]["max_kmer"]) as ctx:                  # chunks that take the bucketed build: slots never zeroed
        sets, qrs = [tar.load(ctx, j["index"]) for j in c["jobs"]], tar.load(ctx, c["search"])
        for byte in (None,) + tuple(jf.POISONS):
            if byte is not None:
                ctx.poison(byte)
            (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=c["caps"]))
            assert ran.get("hits_jobs_kernel") == 1 and "filter_memset" not in ran, (byte, ran)
            for j in range(3):
                assert np.array_equal(hits[j], c["truth"][j]), (byte, j)
    name = "k20_three"                                                           # small chunks: the atomic kernel into slots zeroed by the pass
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    with _commet().Context(k=case["k"], t=2) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        (qrs, qsel, sets, sels), _ = _scenario_sets(ctx, case)
        for byte in jf.POISONS:
            ctx.poison(byte)
            (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, index_selects=sels, search_select=qsel,
                                                                                 max_hits=[job["cap"] for job in case["jobs"]]))
            assert ran.get("hits_jobs_kernel") == 1, (byte, ran)
            for j in range(len(sets)):
                assert np.array_equal(hits[j], truth[j]), (byte, j)


# ---- 6. the sweep ------------------------------------------------------------------------------------------------------------------------
FULL_MODE_SEEDS = (1000, 1002)                      # two of the seeds the golden -f scenarios were made on


def _sweep_against_the_tool(d, index_cfg, search_cfg, k, max_t):
    """`sweep --full` in directory d against `index_and_search -f -t t` for every t; -> {t: {file: shared reads}}"""
    if not os.path.exists(TOOL):
        from commet_amd import build
        build.build_lib()
        build.build_tools()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", index_cfg, "-s", search_cfg, "-k", str(k), "--max-t", str(max_t), "-o", "sweep", "--full"],
                       cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    print(r.stdout.decode().strip())
    rows = [ln.split(";") for ln in open(os.path.join(d, "sweep", "sweep.csv")).read().strip().split("\n")]
    assert rows[0] == ["t", "set", "file", "reads", "shared"]
    csv = {(int(t), os.path.basename(f)): (int(n), int(s)) for t, _, f, n, s in rows[1:]}
    shared = {}
    for t in range(1, max_t + 1):
        p = subprocess.run([TOOL, "-i", index_cfg, "-s", search_cfg, "-o", f"tool{t}", "-l", f"tool{t}", "-k", str(k), "-t", str(t), "-f"], cwd=str(d),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 0, p.stderr.decode()[-500:]
        names = sorted(f for f in os.listdir(os.path.join(d, f"tool{t}")) if f.endswith(".bv"))
        assert names and sorted(os.listdir(os.path.join(d, "sweep", f"t{t}"))) == names, (t, names)
        shared[t] = {}
        for nme in names:
            exp = open(os.path.join(d, f"tool{t}", nme), "rb").read()
            got = open(os.path.join(d, "sweep", f"t{t}", nme), "rb").read()
            assert got == exp, (t, nme)
            _, n, bits = util.read_bv(os.path.join(d, f"tool{t}", nme))
            shared[t][nme] = int(util.bools_from_bits(bits, n).sum())
            assert csv[(t, nme.split("_in_")[0])] == (n, shared[t][nme]), (t, nme)
        print("t", t, shared[t])
    assert len(rows) == 1 + sum(len(s) for s in shared.values())
    return shared


def test_sweep_full_on_the_golden_sets(tmp_path):
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f, copies in (("A", "A"), ("B", "BD"), ("C", "CE")):
        data = gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read()
        for c in copies:
            open(d / "ABCDE_bench" / (c + ".fa"), "wb").write(data)
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("D:ABCDE_bench/D.fa\nCE:ABCDE_bench/C.fa;ABCDE_bench/E.fa\n")     # (CE is the first set: the tool takes it alone)
    shared = _sweep_against_the_tool(str(d), "i.txt", "s.txt", 32, 4)
    assert sorted(shared[1]) == ["A.fa_in_CE.bv", "C.fa_in_A.bv", "E.fa_in_A.bv"]
    assert all(v > 0 for v in shared[1].values())
    assert not any(shared[4].values())                                                   # no read of these sets holds four 32-mers: T1(4) is empty


@pytest.mark.parametrize("seed", FULL_MODE_SEEDS)
def test_sweep_full_on_scenarios(tmp_path, seed):
    scn = Scenario(str(tmp_path / "scn"), seed)
    shared = _sweep_against_the_tool(scn.dir, scn.index_cfg, scn.search_cfg, scn.k, 4)
    assert set(shared) == {1, 2, 3, 4}
