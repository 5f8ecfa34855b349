"""commet_index_many_and_profile on search sets of long reads (capi/multi_profile.hpp; hits_jobs_wave_kernel, hit_profile_jobs.hpp):
under option multi_job = 2 the jobs of such a set share wave-per-read hits passes.  Every job's bytes must be what
commet_index_and_profile gives for it alone, and what the CPU checker gives at every t: on block fixtures that a state not carried
between blocks, a walk that ends with the first decided job, a sum over a job's slots and a block bound off by one get wrong
(hit_profile_jobs_wave_sets.py, proved on the checker in test_hit_profile_jobs_wave_cpu.py), on the lane form's fixtures and scenario
cases, with the passes really shared — and not shared in auto —, in the auto regime of long_search, and through
`python -m commet_amd.sweep --full --multi-job 2`."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_jobs_sets as js
import hit_profile_jobs_wave_sets as ws
import util
from conftest import ROOT
from scenarios import Scenario

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "commet_amd", "bin", "index_and_search")
SHARED = "hits_jobs_wave_kernel"
ONE_JOB = ("hits_wave_kernel", "hits_group_wave_kernel")
LANE = ("hits_kernel", "hits_group_kernel", "hits_jobs_kernel")


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


def _wave_context(k, long_search=2, multi_job=2):
    ctx = _commet().Context(k=k, t=2)
    ctx.set_option("long_search", long_search)
    ctx.set_option("multi_job", multi_job)
    return ctx


@pytest.fixture(scope="module")
def truth_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("jobs_wave_truth")


@pytest.fixture(scope="module")
def wide_ctx():
    """ONE context for the k = 33 cases: its eight 4 GiB filter slots are asked for once"""
    with _wave_context(33) as ctx:
        yield ctx


def _run_fixture(f, want, chunks, tag, long_search=2):
    """one shared pass of hits_jobs_wave_kernel: its launches, its account, its bytes against the checker and the jobs alone"""
    with _wave_context(ws.K, long_search) as ctx:
        ctx.set_option("max_kmer", f["max_kmer"])
        sets, qrs = [_load(ctx, index) for index in f["jobs"]], _load(ctx, f["search"])
        (hits, info), ran = _timed(ctx, lambda: ctx.index_many_and_profile(sets, qrs, max_hits=f["caps"]))
        alone = [ctx.index_and_profile(rs, [qrs], max_hits=cap)[0][0] for rs, cap in zip(sets, f["caps"])]
    n = len(f["design"][0])
    for j in range(len(sets)):
        print(tag, "job", j, "cap", f["caps"][j], "got", hits[j][:9].tolist(), "checker", want[j][:9].tolist(), "design", f["design"][j])
    print(tag, ran, {x: info[x] for x in ("search_launches", "reads_scanned", "n_chunks")})
    assert ran.get(SHARED) == 1 and not any(x in ran for x in ONE_JOB + LANE), ran
    assert info["search_launches"] == 1, info
    assert info["reads_scanned"] == len(f["search"]), info
    assert info["n_chunks"] == sum(chunks) and info["probes"] == 0, info
    for j in range(len(sets)):
        assert np.array_equal(hits[j], want[j]), (tag, j, hits[j][:9].tolist(), want[j][:9].tolist())
        assert np.array_equal(hits[j], alone[j]), (tag, j)
        assert hits[j][:n].tolist() == f["design"][j], (tag, j)


# ---- 1. the block fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", ws.FIXTURES)
def test_block_fixture(truth_dir, name, strand):
    want, chunks = ws.checker_bytes(truth_dir, name, strand)
    _run_fixture(ws.fixture(name, strand), want, chunks, f"{name}{strand}")


# ---- 2. the lane form's fixtures and scenario cases, wave form ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", js.FIXTURES)
def test_lane_fixture_on_the_wave_form(truth_dir, name, strand):
    f = js.fixture(name, strand)
    want, chunks = js.checker_bytes(truth_dir, name, strand)
    _run_fixture(dict(f, design={j: [b] for j, b in f["design"].items()}), want, chunks, f"lane_{name}{strand}")


def _scenario_sets(ctx, case):
    """-> (search set, its selection bits or None, [index set per job], [selection bits per job]), the loaded sets by name"""
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
    print(name, "chunks", chunks, "shared passes", shared, "alone", n_alone, ran, info["search_launches"])
    for j, (h, (a, ainfo)) in enumerate(zip(hits, alone)):
        print(name, "job", j, "cap", caps[j], "found", int((h > 0).sum()), "of", h.size, "max", int(h.max(initial=0)))
        assert np.array_equal(h, truth[j]), (name, j, np.nonzero(h != truth[j])[0][:10].tolist())
        assert np.array_equal(h, a[0]), (name, j, np.nonzero(h != a[0])[0][:10].tolist())
        assert ainfo["n_chunks"] == chunks[j], (name, j, ainfo["n_chunks"], chunks[j])
    assert ran.get(SHARED, 0) == shared and not any(x in ran for x in LANE), (name, ran)
    assert info["n_chunks"] == sum(chunks) and info["probes"] == 0


@pytest.mark.parametrize("name", sorted(n for n, s in js.SCENARIO_CASES.items() if s["k"] != 33))
def test_scenario_case(truth_dir, name):
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [job["chunks"] for job in case["jobs"]]
    with _wave_context(case["k"]) as ctx:
        _run_scenario_case(ctx, case, truth, chunks, name)


@pytest.mark.parametrize("name", sorted(n for n, s in js.SCENARIO_CASES.items() if s["k"] == 33))
def test_scenario_case_wide_keys(truth_dir, wide_ctx, name):
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [job["chunks"] for job in case["jobs"]]
    _run_scenario_case(wide_ctx, case, truth, chunks, name)


# ---- 3. the passes are really shared, and auto is as it was ------------------------------------------------------------------------------------
def test_eight_one_chunk_jobs_share_one_wave_pass(truth_dir):
    name = "k20_eight"
    case = js.scenario_case(name, truth_dir)
    truth, chunks = js.scenario_truth(name, truth_dir)
    assert chunks == [1] * 8
    caps = [job["cap"] for job in case["jobs"]]
    with _wave_context(case["k"]) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        (qrs, qsel, sets, sels), _ = _scenario_sets(ctx, case)
        call = lambda: ctx.index_many_and_profile(sets, qrs, index_selects=sels, search_select=qsel, max_hits=caps)
        (shared, info), ran = _timed(ctx, call)
        print("multi_job 2", ran, info["search_launches"], info["reads_scanned"])
        assert info["search_launches"] == 1 and ran.get(SHARED) == 1 and not any(x in ran for x in ONE_JOB + LANE), (info, ran)
        assert qsel is None and info["reads_scanned"] == qrs.num_reads, (info, qrs.num_reads)
        for multi_job in (0, 1):                                                     # auto stays job by job on such a set
            ctx.set_option("multi_job", multi_job)
            (single, info1), ran1 = _timed(ctx, call)
            print("multi_job", multi_job, ran1, info1["search_launches"])
            assert info1["search_launches"] == 8 and ran1.get("hits_wave_kernel") == 8 and SHARED not in ran1 and "hits_jobs_kernel" not in ran1, (multi_job, info1, ran1)
            assert all(np.array_equal(a, b) for a, b in zip(shared, single)), multi_job
        ctx.set_option("multi_job", 2)
        ctx.set_option("chunk_group", 4)                                             # groups of four slots: two passes of four jobs
        (fours, info4), ran4 = _timed(ctx, call)
        assert info4["search_launches"] == 2 and ran4.get(SHARED) == 2 and not any(x in ran4 for x in ONE_JOB), (info4, ran4)
        assert all(np.array_equal(a, b) for a, b in zip(shared, fours))
    assert all(np.array_equal(a, b) for a, b in zip(shared, truth))


# ---- 4. the auto regime of long_search: a ragged set whose longest read has 5000 bases and more ------------------------------------------------
def test_auto_regime_takes_the_shared_wave_pass(truth_dir):
    f = ws.auto_fixture()
    want, chunks = ws.auto_bytes(truth_dir)
    _run_fixture(f, want, chunks, "auto", long_search=0)


# ---- 5. the sweep ----------------------------------------------------------------------------------------------------------------------------
def _sweep_against_the_tool(d, index_cfg, search_cfg, k, max_t, sweep_args, sweep_env):
    """`sweep --full` with the given arguments and environment in directory d against `index_and_search -f -t t` for every t: the .bv
    files byte for byte.  -> (shared reads by t and file, the sweep's stdout, its stderr)"""
    if not os.path.exists(TOOL):
        from commet_amd import build
        build.build_lib()
        build.build_tools()
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **sweep_env)
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", index_cfg, "-s", search_cfg, "-k", str(k), "--max-t", str(max_t), "-o", "sweep", "--full"] +
                       list(sweep_args), cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    shared = {}
    for t in range(1, max_t + 1):
        if not os.path.isdir(os.path.join(d, f"tool{t}")):                       # (a second sweep in d compares with the same runs of the tool)
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
    return shared, r.stdout.decode(), r.stderr.decode()


SWEEP_ENV = {"COMMET_LONG_SEARCH": "2", "COMMET_JOB_VERBOSE": "1"}          # every set takes the wave-per-read kernels; a line per many-job call that shares


def _shared_passes(err, max_t):
    """the shared passes of pass 2 as the library reports them (it prints the line only for a call that shares)"""
    print("\n".join(ln for ln in err.split("\n") if ln.startswith("[profiles")))
    m = re.search(r"\[profiles x%d\] (\d+) shared pass" % max_t, err)
    return int(m.group(1)) if m else 0


def test_sweep_full_multi_job_2_on_a_scenario(tmp_path):
    import test_gpu_hit_profile_jobs as lane_form
    scn = Scenario(str(tmp_path / "scn"), lane_form.FULL_MODE_SEEDS[1])       # one of the seeds the golden -f scenarios were made on
    max_t = 4
    shared, out, err = _sweep_against_the_tool(scn.dir, scn.index_cfg, scn.search_cfg, scn.k, max_t, ["--multi-job", "2"], SWEEP_ENV)
    print(out.strip(), "shared passes", _shared_passes(err, max_t))
    assert set(shared) == set(range(1, max_t + 1)) and any(shared[1].values())
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", scn.index_cfg, "-s", scn.search_cfg, "-k", str(scn.k), "--max-t", "2", "-o", "refused", "--full",
                        "--multi-job", "3"], cwd=scn.dir, env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", "")),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--multi-job" in r.stderr and not os.path.exists(os.path.join(scn.dir, "refused"))


def test_sweep_full_multi_job_2_shares_wave_passes_on_the_golden_sets(tmp_path):
    """the scenario's jobs of pass 2 each hold a file without a selected read and run alone; here B is one file, every job with a read
    found is planned on the device, and the jobs share a pass of hits_jobs_wave_kernel: same .bv bytes"""
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f, copies in (("A", "A"), ("B", "D")):
        data = gzip.open(os.path.join(ROOT, "tests", "golden", "abcde", f + ".fa.gz")).read()
        for c in copies:
            open(d / "ABCDE_bench" / (c + ".fa"), "wb").write(data)
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("D:ABCDE_bench/D.fa\n")
    max_t = 3
    shared, out, err = _sweep_against_the_tool(str(d), "i.txt", "s.txt", 32, max_t, ["--multi-job", "2"], SWEEP_ENV)
    print(out.strip())
    assert sorted(shared[1]) == ["A.fa_in_D.bv", "D.fa_in_A.bv"] and all(v > 0 for t in (1, 2) for v in shared[t].values()), shared
    assert _shared_passes(err, max_t) >= 1, err[-800:]
    # ... and job by job without the option: such sets stay as they were in auto
    shared0, out0, err0 = _sweep_against_the_tool(str(d), "i.txt", "s.txt", 32, max_t, [], SWEEP_ENV)
    assert shared0 == shared and _shared_passes(err0, max_t) == 0, err0[-800:]
