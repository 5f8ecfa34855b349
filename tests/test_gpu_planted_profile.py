"""The hit-profile kernels on planted windows and lane decoys (planted_sets.py): hits_wide_kernel, hits_sliced_kernel<1 | 2 | 4 | 8>,
tq_probe_kernel + tq_hits_replay_kernel and hits_jobs_kernel<., 2 | 4 | 8> on the fixtures of test_gpu_planted_search.py.

Random reads never hold a window that is a candidate in some lanes of a chunk filter and a hit in none, so byte equality with the slot
loop on such reads cannot see a kernel that skips a plane, ANDs the wrong column of a 32-chunk word or mixes the lanes of two slots or
two jobs.  Family A (the lane ladder) is made of such windows; families B, C and D put real hits at every mask and block edge.

Every read has a designed count, which IS the hit byte of commet_index_and_profile (test_planted_sets_cpu.py proves design == checker
at every t in 1 .. max + 1 for every case imported here; this file builds no case of its own).  Every test
  - compares the hit arrays byte for byte with min(design, cap), at cap 1 (a false first hit of a partial ladder) and max(design) + 1,
  - compares them with the same call through the slot loop (profile_wide = profile_slice = profile_tiled = 1; jobs: job by job),
  - holds kernel_times() to the intended kernel, launch count included, and to no other hits kernel beside it."""
import numpy as np
import pytest

import hit_profile_slice_sets as ss
import hit_profile_wide_sets as ws
import planted_sets as ps
import util

pytestmark = pytest.mark.gpu

SLOT_HITS = ("hits_kernel", "hits_group_kernel", "hits_wave_kernel", "hits_group_wave_kernel")
TABLE_HITS = ("hits_wide_kernel", "hits_sliced_kernel", "tq_probe_kernel", "tq_hits_replay_kernel", "hits_jobs_kernel")
SLOT_LOOP = dict(profile_wide=1, profile_slice=1, profile_tiled=1)
DEFAULTS = dict(SLOT_LOOP, chunk_group=8, slice_words=0, slice_wide_words=0, tq_hit_cap=1024, long_search=1, multi_job=0, count_probes=0)


def _commet():
    import commet_amd
    return commet_amd


def _load(ctx, reads):
    return _commet().ReadSet.from_files(ctx, [util.to_batch(reads)])


def _timed(ctx, opts, call):
    """the call under DEFAULTS + opts -> (its result, {hits kernel: launches} of that call alone)"""
    for name, value in dict(DEFAULTS, **opts).items():
        ctx.set_option(name, value)
    ctx.set_option("kernel_timing", 1)                            # (the totals start again)
    try:
        out = call()
        times = ctx.kernel_times()
    finally:
        ctx.set_option("kernel_timing", 0)
    return out, {n: times[n][0] for n in SLOT_HITS + TABLE_HITS if n in times}


def _caps(designs):
    return (1, max(int(d.max()) for d in designs) + 1)


def _check_case(ctx, what, case, names, runs):
    """one index_and_profile case in ctx.  names: the sets of the case that are searched; runs: [(options, {kernel: launches})], the
    launches as the dispatch's own rule gives them for this case.  Per cap the slot loop runs once, then every option set"""
    reads = [case["sets"][n][0] for n in names]
    designs = [case["sets"][n][1] for n in names]
    assert max(int(d.max()) for d in designs) >= 1 and all(len(r) for r in reads)
    ctx.set_option("max_kmer", case["max_kmer"])
    irs = _load(ctx, case["index"])
    qrs = [_load(ctx, r) for r in reads]
    try:
        for cap in _caps(designs):
            (slot, info1), ran1 = _timed(ctx, SLOT_LOOP, lambda: ctx.index_and_profile(irs, qrs, max_hits=cap))
            assert ran1 and set(ran1) <= set(SLOT_HITS), (what, cap, ran1)
            assert info1["n_chunks"] == case["n_chunks"], (what, info1["n_chunks"])
            for opts, want in runs:
                (hits, info), ran = _timed(ctx, opts, lambda: ctx.index_and_profile(irs, qrs, max_hits=cap))
                print(what, "cap", cap, opts, ran)
                assert ran == want, (what, cap, opts, ran, want)
                assert info["n_chunks"] == case["n_chunks"] and info["probes"] == 0
                for n, h, s, d in zip(names, hits, slot, designs):
                    exp = np.minimum(d, cap)
                    wrong = np.flatnonzero(h != exp)
                    assert h.dtype == np.uint8 and wrong.size == 0, (what, cap, opts, n, wrong[:10].tolist(), h[wrong[:10]].tolist(), exp[wrong[:10]].tolist())
                    assert np.array_equal(h, s), (what, cap, opts, n, np.flatnonzero(h != s)[:10].tolist())
    finally:
        for rs in qrs + [irs]:
            rs.close()


def _case_in_its_own_context(what, case, names, runs):
    with _commet().Context(k=case["k"], t=2) as ctx:
        _check_case(ctx, what, case, names, runs)


# ---- the wide rows: hits_wide_kernel ----------------------------------------------------------------------------------------------------
def _wide_runs(n_chunks, n_sets):
    """the rows uncapped, and capped at 8 words: 256 chunks a pass, the ladder's anchors 255 / 256 in different passes (the fold over
    passes is the byte array's max)"""
    return [(dict(profile_wide=2, slice_wide_words=w), {"hits_wide_kernel": ws.passes_of(n_chunks, w)[0] * n_sets}) for w in (0, 8)]


@pytest.mark.parametrize("k,n_chunks", ps.WIDE_PROFILE_LADDERS)
def test_lane_ladder_in_the_wide_rows(k, n_chunks):
    assert (k, n_chunks) in ps.SLICED_LADDERS                   # (where test_planted_sets_cpu.py proves it)
    c = ps.ladder_case(k, n_chunks)
    runs = _wide_runs(n_chunks, 1)
    assert [r[1]["hits_wide_kernel"] for r in runs] == [1, 2]
    _case_in_its_own_context(("wide", "ladder", k), c, ["ladder"], runs)


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", [s for s in ps.SLICED_SWEEPS if s[0] <= max(ps.WIDE_PROFILE_KS)])
def test_positions_in_the_wide_rows(k, t, n_chunks, fhws, per_chunk):
    c = ps.sweep_case(k, t, n_chunks, fhws, per_chunk)
    names = list(c["sets"])
    _case_in_its_own_context(("wide", "sweep", k, t), c, names, _wide_runs(c["n_chunks"], len(names)))


# ---- the narrow tables: hits_sliced_kernel<1 | 2 | 4 | 8> -----------------------------------------------------------------------------
def _narrow_runs(k, n_chunks, n_sets):
    """32, 64, 128 and 256 chunk filters a pass (k = 24: the tables of 256 pass 1 GiB, slice_words = 8 runs as 4: ss.plan)"""
    return [(dict(profile_slice=2, slice_words=w), {"hits_sliced_kernel": ss.plan(n_chunks, k, w)[1] * n_sets}) for w in (1, 2, 4, 8)]


@pytest.mark.parametrize("k,n_chunks", ps.SLICED_LADDERS)
def test_lane_ladder_in_the_narrow_tables(k, n_chunks):
    """the decoys of a k-mer in neighbouring columns of every 32-chunk word and on both sides of every pass boundary: a read whose
    only candidates are partial leaves the block counters at 0 from both sides"""
    c = ps.ladder_case(k, n_chunks)
    runs = _narrow_runs(k, n_chunks, 1)
    assert {ss.plan(n_chunks, k, w)[0] for w in (1, 2, 4, 8)} == ({1, 2, 4, 8} if k < 24 else {1, 2, 4})
    assert [r[1]["hits_sliced_kernel"] for r in runs][:3] == [10, 5, 3]
    _case_in_its_own_context(("narrow", "ladder", k), c, ["ladder"], runs)


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLICED_SWEEPS)
def test_positions_in_the_narrow_tables(k, t, n_chunks, fhws, per_chunk):
    c = ps.sweep_case(k, t, n_chunks, fhws, per_chunk)
    names = list(c["sets"])
    _case_in_its_own_context(("narrow", "sweep", k, t), c, names, _narrow_runs(k, c["n_chunks"], len(names)))


# ---- the tiled probe: tq_probe_kernel + tq_hits_replay_kernel ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def context_of():
    """ONE context per k, open while that k's cases run: the 4 / 8 GiB filter slots of k = 33 / 34 are asked for once"""
    held = {}

    def get(k):
        for other in [o for o in held if o != k]:
            held.pop(other).close()
        if k not in held:
            held[k] = _commet().Context(k=k, t=2)
        return held[k]

    yield get
    for ctx in held.values():
        ctx.close()


def _tiled_runs(n_chunks, n_sets):
    """one and two filters a pass; the hit lists at their size, at two entries and at none (the overflow walks)"""
    runs = []
    for g, cap in ((2, 1024), (1, 1024), (2, 2), (1, 0), (2, 0), (1, 2)):
        launches = -(-n_chunks // g) * n_sets
        runs.append((dict(profile_tiled=2, chunk_group=g, tq_hit_cap=cap), {"tq_probe_kernel": launches, "tq_hits_replay_kernel": launches}))
    return runs


@pytest.mark.parametrize("k,n_chunks", ps.TILED_LADDERS)
def test_lane_ladder_in_the_tiled_profile(context_of, k, n_chunks):
    """the ladder, and the whole-read ladders: every window of a read a candidate in one, two or three lanes and a hit in none"""
    c = ps.ladder_case(k, n_chunks)
    names = ps.tiled_sets(c)
    assert names == ["ladder", "whole"]
    _check_case(context_of(k), ("tiled", "ladder", k), c, names, _tiled_runs(n_chunks, len(names)))


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.TILED_SWEEPS)
def test_positions_in_the_tiled_profile(context_of, k, t, n_chunks, fhws, per_chunk):
    """t = 1: every set of the sweep; t = 3 (counts up to 3): the sets within 255 complete windows per read — every fixed-length set"""
    c = ps.sweep_case(k, t, n_chunks, fhws, per_chunk)
    names = ps.tiled_sets(c)
    assert set(names) >= {f"f{fhw}" for fhw in fhws}
    _check_case(context_of(k), ("tiled", "sweep", k, t), c, names, _tiled_runs(c["n_chunks"], len(names)))


# ---- jobs that share a hits pass: hits_jobs_kernel<., 2 | 4 | 8> ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_chunks", ps.PROFILE_JOB_LADDERS)
def test_lane_ladder_split_between_two_jobs(context_of, k, n_chunks):
    """LO and BOTH of a k-mer in job 0, HI and ROT in job 1, in the same chunk number of each: found by neither job, whichever job's
    slots stand first in the pass and whichever job stops at its first hit"""
    c = ps.ladder_jobs(k, n_chunks)
    assert c["n_chunks"] == n_chunks and max(int(d.max()) for d in c["counts"]) == 2
    ctx = context_of(k)
    ctx.set_option("max_kmer", c["max_kmer"])
    sets = [_load(ctx, s) for s in c["index_sets"]]
    qrs = _load(ctx, c["search"])
    try:
        alone = {}
        for j in range(2):
            for cap in (1, 255):
                (h, info), ran = _timed(ctx, SLOT_LOOP, lambda: ctx.index_and_profile(sets[j], [qrs], max_hits=cap))
                assert ran and set(ran) <= set(SLOT_HITS) and info["n_chunks"] == n_chunks, (k, n_chunks, j, cap, ran)
                alone[j, cap] = h[0]
        for order in ((0, 1), (1, 0)):
            for caps in ((1, 255), (255, 1)):
                for multi_job in (0, 2):
                    (hits, info), ran = _timed(ctx, dict(multi_job=multi_job),
                                               lambda: ctx.index_many_and_profile([sets[j] for j in order], qrs, max_hits=list(caps)))
                    print(k, n_chunks, order, caps, multi_job, ran)
                    assert ran == {"hits_jobs_kernel": 1} and info["search_launches"] == 1 and info["n_chunks"] == 2 * n_chunks, (order, caps, ran)
                    for j, cap, h in zip(order, caps, hits):
                        exp = np.minimum(c["counts"][j], cap)
                        wrong = np.flatnonzero(h != exp)
                        assert h.dtype == np.uint8 and wrong.size == 0, (k, n_chunks, order, caps, multi_job, j, wrong[:10].tolist(), h[wrong[:10]].tolist())
                        assert np.array_equal(h, alone[j, cap]), (k, n_chunks, order, caps, multi_job, j)
    finally:
        for rs in sets + [qrs]:
            rs.close()
