"""What the wave-per-read many-job hit profile's GPU tests (test_gpu_hit_profile_jobs_wave.py) presuppose, proved without a GPU: the
block fixtures and the auto-regime set reach the designed bytes on the CPU checker, job by job; a model of the block walk gives the
designs and, with one rule broken at a time, the bytes the fixtures are meant to catch; and the sweep command's --multi-job."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_jobs_wave_sets as ws
import util
from conftest import ROOT

js = ws.js


# ---- the fixtures on the checker ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strand", ws.FIXTURES)
def test_block_fixture_reaches_its_design_on_the_checker(tmp_path, name, strand):
    f = ws.fixture(name, strand)
    got, chunks = ws.checker_bytes(tmp_path, name, strand)
    assert chunks == f["chunks"]
    search = f["search"]
    n_planted = len(f["design"][0])
    r = search[n_planted - 1] if name != "edge" else search[3]
    assert len(r) == ws.L and len(r) - ws.K + 1 == 181
    for j, cap in enumerate(f["caps"]):
        h = got[j]
        print(name, strand, "job", j, "cap", cap, h[:9].tolist())
        assert h[:n_planted].tolist() == f["design"][j], (name, strand, j, h[:9].tolist())
        assert int(h.max()) <= min(cap, ws.T_TOP)
        first = search.index(r)
        for i, x in enumerate(search):
            if x == r or x == r.lower() or x == util.revcomp(r):
                assert h[i] == h[first], (name, j, i)
            if len(x) < ws.K:
                assert h[i] == 0, (name, j, i)
    assert sum(1 for x in search if x == r) == 41 and any(b"N" in x for x in search) and any(len(x) < ws.K for x in search)
    if name == "edge":
        assert [len(x) - ws.K + 1 for x in search[:3]] == [63, 64, 65]


def test_auto_fixture_reaches_its_design_on_the_checker(tmp_path):
    f = ws.auto_fixture()
    got, chunks = ws.auto_bytes(tmp_path)
    assert chunks == [1, 1] and max(f["caps"]) <= 5
    lens = [len(x) for x in f["search"]]
    print("auto", lens, [h.tolist() for h in got])
    assert len(lens) == 20 and max(lens) == lens[0] >= ws.AUTO_MIN_MAX_LEN and sorted(lens)[-2] < ws.AUTO_MIN_MAX_LEN
    assert sum(1 for n in lens if n >= 200) >= 18 and len(set(lens)) > 12
    for j in (0, 1):
        assert int(got[j][0]) == f["design"][j][0] and int(got[j].max()) <= f["caps"][j]
        assert int((got[j] > 0).sum()) >= 4                        # (the pieces and the reverse complement of x are found as well)
    assert got[0][4] < got[0][0]                                   # the N inside job 0's window 86 costs it a hit


# ---- a model of the block walk: the designs, and what breaking one rule gives ------------------------------------------------------------
def _walk(slots, job_of, caps, n_win, k=ws.K, carry=True, any_stop=False, fold=max, bound=0):
    """hits_jobs_wave_kernel's walk of one strand of one read.  slots: per slot, the window starts that are full hits in its filter;
    job_of: its job.  Block by block, slot by slot, greedy up to the job's cap; a job at its cap wants no window any more.
    carry = False: next_free starts at the block's first window again; any_stop: the block loop and the walk end when any job is
    decided; fold: over the counts of a job's slots; bound: the read is taken to have n_win - bound windows"""
    n = len(slots)
    next_free, count, done = [0] * n, [0] * n, set()
    for base in range(0, n_win - bound, ws.BLOCK):
        if (any_stop and done) or all(job_of[i] in done for i in range(n)):
            break
        if not carry:
            next_free = [0] * n
        for i in range(n):
            for s in sorted(h for h in slots[i] if base <= h < min(base + ws.BLOCK, n_win - bound)):
                if job_of[i] in done:
                    break
                if s >= next_free[i] and count[i] < caps[job_of[i]]:
                    count[i], next_free[i] = count[i] + 1, s + k
                    if count[i] >= caps[job_of[i]]:
                        done.add(job_of[i])
    return [min(caps[j], fold([count[i] for i in range(n) if job_of[i] == j] or [0])) for j in range(max(job_of) + 1)]


def test_the_wrong_kernels_would_show():
    k = ws.K
    n_win = ws.L - k + 1
    # carry: job 0 at 50, 66, 86; job 1 at 64 .. 104
    slots, jobs, caps = [[50, 66, 86], list(range(64, 105))], [0, 1], [255, 255]
    assert _walk(slots, jobs, caps, n_win) == [2, 3]
    assert _walk(slots, jobs, caps, n_win, carry=False) == [3, 3]
    # (one `free` for both slots, window by window: job 1 is left with 70 and 90)
    free, cnt = 0, [0, 0]
    for s in range(n_win):
        takers = [j for j in (0, 1) if s in slots[j] and s >= free]
        for j in takers:
            cnt[j] += 1
        if takers:
            free = s + k
    assert cnt[1] == 2 and js.gs.greedy(slots[1], k) == 3
    # stop_far: job 0 (cap 1) at 0 .. 10, job 1 (cap 3) at 130 .. 170
    slots, jobs, caps = [list(range(0, 11)), list(range(130, 171))], [0, 1], [1, 3]
    assert _walk(slots, jobs, caps, n_win) == [1, 3]
    assert _walk(slots, jobs, caps, n_win, any_stop=True) == [1, 0]
    assert min(slots[1]) >= 2 * ws.BLOCK                             # (block 2: two block bounds behind the decided job)
    # max_far: one job of two slots (0 .. 20 and 100 .. 140), another of one slot without a hit
    slots, jobs, caps = [list(range(0, 21)), list(range(100, 141)), []], [0, 0, 1], [255, 255]
    assert _walk(slots, jobs, caps, n_win) == [3, 0]
    assert _walk(slots, jobs, caps, n_win, fold=sum) == [5, 0]
    # edge: reads of 63, 64, 65 windows; job 0 holds the last window, job 1 the first
    for w in (63, 64, 65):
        slots, jobs, caps = [[w - 1], [0]], [0, 1], [255, 255]
        assert _walk(slots, jobs, caps, w) == [1, 1]
        assert _walk(slots, jobs, caps, w, bound=1) == [0, 1]
    # the auto-regime read: job 0 (cap 5) carry's plants and one hit four blocks on, job 1 (cap 3) decided in between
    a, b = ws.AUTO_AT, ws.AUTO_AT + 4 * ws.BLOCK
    slots, jobs, caps = [[a + 50, a + 66, a + 86] + list(range(b, b + 11)), list(range(a + 64, a + 105)) + list(range(b + 130, b + 171))], [0, 1], ws.AUTO_CAPS
    assert a % ws.BLOCK == 0 and _walk(slots, jobs, caps, 6000 - k + 1) == [3, 3]
    assert _walk(slots, jobs, caps, 6000 - k + 1, carry=False) == [4, 3]
    assert _walk(slots, jobs, caps, 6000 - k + 1, any_stop=True) == [2, 3]


def test_mates_counted_behind_the_capping_hit_change_no_byte():
    """within one block a mate in front of the capped slot in the slot loop has walked the whole block before the cap is reached: its
    count may hold hits behind the capping hit, which a window-by-window walk never takes.  The byte is the cap either way"""
    # one job of two slots, cap 3: slot 0 hits at 0 and 60, slot 1 at 5, 25, 45.  The job is decided at 45; slot 0, walked first, has
    # counted 60 as well (2, window by window 1): min(3, max(2, 3)) = min(3, max(1, 3))
    assert _walk([[0, 60], [5, 25, 45]], [0, 0], [3], 100) == [3]
    # ... and a cap that slot 0 reaches first: slot 1 takes nothing more
    assert _walk([[0, 20], [10, 30]], [0, 0], [2], 100) == [2]


# ---- the sweep command: --multi-job -------------------------------------------------------------------------------------------------------
def _run_sweep(cwd, *args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "commet_amd.sweep"] + list(args), cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_sweep_multi_job_argument_handling(tmp_path):
    r = _run_sweep(tmp_path, "--help")
    assert r.returncode == 0 and b"--multi-job {0,1,2}" in r.stdout and b"hits_jobs_wave_kernel" in r.stdout
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    for bad in ("3", "-1", "x"):
        r = _run_sweep(tmp_path, "-i", "i.txt", "-s", "s.txt", "-k", "20", "-o", "out", "--max-t", "3", "--full", "--multi-job", bad)
        assert r.returncode == 2 and b"--multi-job" in r.stderr, (bad, r.stderr)
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("value", [None, 0, 1, 2])
def test_sweep_passes_multi_job_on(tmp_path, value):
    import test_hit_profile_jobs_cpu as cpu
    from commet_amd import sweep
    d = tmp_path
    open(d / "i.txt", "w").write("A:a2.fa\n")
    open(d / "s.txt", "w").write("B:b1.fa\n")
    api = cpu._StubApi({"a2.fa": 8, "b1.fa": 17})
    cwd = os.getcwd()
    os.chdir(d)
    try:
        extra = [] if value is None else ["--multi-job", str(value)]
        assert sweep.main(["-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", "2", "-o", "out", "--full", "--chunk-group", "4"] + extra, api=api) == 0
    finally:
        os.chdir(cwd)
    options = [c[1:] for c in api.calls if c[0] == "option"]
    assert ("chunk_group", 4) in options
    assert [o for o in options if o[0] == "multi_job"] == ([] if value is None else [("multi_job", value)])
    first_call = min(i for i, c in enumerate(api.calls) if c[0] != "option")
    assert all(c[0] != "option" for c in api.calls[first_call:])    # (set in front of the first job)
    assert [c[0] for c in api.calls if c[0] != "option"] == ["profile", "many", "profile", "profile"]
