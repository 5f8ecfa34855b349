"""The thresholds calls (capi/thresholds.hpp; hits_tags_kernel, hits_tags.hpp): tags of every wanted t and per-file counts made on the
device from the hit-count bytes of a profile.
  1. commet_hits_to_tags on designed bytes against the numpy model of hits_tags_cases.py: poisoned outputs, every size, file cut and
     threshold range of the model's lists, and a workgroup that walks several tiles (option hits_tags_blocks).
  2. commet_index_and_thresholds / commet_index_many_and_thresholds against the profile calls + tags_at on the same context, and
     against commet_index_and_search on contexts of t = 1..3: the four synthetic sets of the matrix driver's test at k = 20 (one set
     of two files, one file emptied by its filter, selections that are not all ones, a job with an empty selection between two that
     share), a pair at k = 32; and the same with the tag words refused (the host loop)."""
import numpy as np
import pytest

import hits_tags_cases as htc
import util

pytestmark = pytest.mark.gpu


def _commet():
    import commet_amd
    return commet_amd


def _timed(ctx, call):
    ctx.set_option("kernel_timing", 1)
    try:
        out = call()
        times = ctx.kernel_times()
    finally:
        ctx.set_option("kernel_timing", 0)
    return out, {n: times[n][0] for n in times}


# ---- 1. the kernel on designed bytes ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_ctx():
    with _commet().Context(k=12, t=2) as ctx:
        yield ctx


# (n, most workgroups): the issue's sizes at the default; 4099 reads in ONE workgroup of two tiles, 20 000 reads (five tiles) in two
# workgroups of three and two tiles — the walk over several tiles, its per-file sums and their hand-over at a file boundary
WALKS = [(n, 2048) for n in htc.SIZES] + [(4099, 1), (20000, 2), (20000, 1)]


@pytest.mark.parametrize("n,blocks", WALKS)
def test_hits_to_tags_on_designed_bytes(small_ctx, n, blocks):
    ctx = small_ctx
    ctx.set_option("hits_tags_blocks", blocks)
    try:
        for cut, file_reads in htc.file_cuts(n).items():
            for rot, (t_first, n_t) in enumerate(htc.RANGES):
                hits = htc.designed_bytes(n, file_reads, t_first, n_t, rot)
                want_tags, want_shared = htc.fast_model(hits, file_reads, t_first, n_t)
                (tags, shared), ran = _timed(ctx, lambda: ctx.hits_to_tags(hits, file_reads, t_first, n_t, fill=0xA5))
                assert ran.get("hits_tags_kernel") == 1, ran
                for ti in range(n_t):
                    assert tags[ti].size == n // 8 + 1
                    assert np.array_equal(tags[ti], want_tags[ti]), (n, cut, t_first, ti, np.nonzero(tags[ti] != want_tags[ti])[0][:8].tolist())
                    assert int(tags[ti][-1]) >> (n & 7) == 0                     # padding bits
                assert np.array_equal(shared, want_shared), (n, cut, t_first, n_t, shared[:2].tolist(), want_shared[:2].tolist())
                tags2, none = ctx.hits_to_tags(hits, file_reads, t_first, n_t, want_shared=False, fill=0x5A)
                assert none is None and all(np.array_equal(a, b) for a, b in zip(tags2, want_tags))
    finally:
        ctx.set_option("hits_tags_blocks", 2048)


def test_hits_to_tags_bad_arguments(small_ctx):
    commet = _commet()
    h = np.zeros(10, dtype=np.uint8)
    for kw in (dict(t_first=0), dict(t_first=255, n_t=2), dict(n_t=0), dict(file_reads=[4, 5])):
        with pytest.raises(commet.CommetError):
            small_ctx.hits_to_tags(h, **kw)
    assert commet.hits_to_tags(small_ctx, h + 3, t_first=3)[1].tolist() == [[10]]


# ---- 2. the calls ---------------------------------------------------------------------------------------------------------------------------------
def _four_sets():
    """the four synthetic sets of test_matrix_driver_matches_oracle_on_synthetic_sets: 6000 x 80 bp, set 1 in two files, filters
    that keep 90 % of the reads and none of set 1's second file -> ([files of (bases, offsets)], [set-wide filter bits])"""
    from commet_amd import synth
    n, L = 6000, 80
    rng = np.random.default_rng(1)
    sets, sels = [], []
    for s in range(4):
        b, o = synth.synth_set(s, n, L, copy_frac=0.3)
        h = n // 2
        files = [(b, o)] if s != 1 else [(b[: h * L], o[: h + 1]), (b[h * L:], o[h:] - o[h])]
        sel = []
        for j, (_, fo) in enumerate(files):
            keep = rng.random(len(fo) - 1) < 0.9
            if (s, j) == (1, 1):
                keep[:] = False
            sel.append(keep)
        sets.append(files)
        sels.append(util.bits_from_bools(np.concatenate(sel)))
    return sets, sels


def _pair32():
    from commet_amd import synth
    sets = [[synth.synth_set(s, 5000, 100, copy_frac=0.4)] for s in (10, 11)]
    return sets, [None, None]


def _per_file(bits, counts):
    from commet_amd.matrix_io import popcount, split_bits
    return [popcount(b, c) for b, c in zip(split_bits(bits, counts), counts)]


def _check_single(ctx, rs, sels, ref, targets, T, searches):
    """index_and_thresholds(ref, targets) against index_and_profile + tags_at and against the searches at t = 1..T -> tags[s][t - 1]"""
    commet = _commet()
    args = (rs[ref], [rs[i] for i in targets], sels[ref], [sels[i] for i in targets])
    (tags, shared, info), ran = _timed(ctx, lambda: ctx.index_and_thresholds(*args, max_t=T))
    hits, pinfo = ctx.index_and_profile(*args, max_hits=T)
    assert ran.get("hits_tags_kernel") == len(targets), ran
    assert info["n_chunks"] == pinfo["n_chunks"] and info["search_launches"] == pinfo["search_launches"]
    for s, i in enumerate(targets):
        counts = rs[i].file_reads()
        for t in range(1, T + 1):
            assert np.array_equal(tags[s][t - 1], commet.tags_at(hits[s], t)), (ref, i, t)
            assert shared[s][t - 1].tolist() == _per_file(tags[s][t - 1], counts), (ref, i, t)
            assert np.array_equal(tags[s][t - 1], searches[t][(ref, i)]), (ref, i, t)
    return tags


def _searches(sets, sels, k, T, pairs):
    """{t: {(index, search): tags}} from commet_index_and_search on a context of every t"""
    commet = _commet()
    out = {}
    for t in range(1, T + 1):
        with commet.Context(k=k, t=t) as ctx:
            rs = [commet.ReadSet.from_files(ctx, fl) for fl in sets]
            out[t] = {(a, b): ctx.index_and_search(rs[a], [rs[b]], sels[a], [sels[b]])[0][0] for a, b in pairs}
    return out


@pytest.fixture(scope="module")
def four():
    sets, sels = _four_sets()
    pairs = [(0, i) for i in (1, 2, 3)]
    return sets, sels, _searches(sets, sels, 20, 3, pairs)


def _j2_jobs(rs, tags1, targets, T):
    """the J2 jobs (i, t) of reference set 0: index S_i restricted to J1's tags at t; an empty selection between two that share"""
    jobs = [(i, t, tags1[s][t - 1]) for s, i in enumerate(targets) for t in range(1, T + 1)]
    empty = np.zeros(rs[targets[-1]].num_reads // 8 + 1, dtype=np.uint8)
    at = len(jobs) - T + 1                                                          # behind the last target's first job: both neighbours share
    return jobs[:at] + [(targets[-1], 2, empty)] + jobs[at:]


def _check_many(ctx, rs, sels, jobs, k, refuse=False, passes=1, against_search=True):
    commet = _commet()
    sets, isel, ts = [rs[i] for i, _, _ in jobs], [b for _, _, b in jobs], [t for _, t, _ in jobs]
    hits, pinfo = ctx.index_many_and_profile(sets, rs[0], isel, sels[0], max_hits=ts)
    if refuse:
        with commet.refusing_device_allocs(nth=1) as r:
            (tags, shared, info), ran = _timed(ctx, lambda: ctx.index_many_and_thresholds(sets, rs[0], isel, sels[0], t=ts))
        print("refused", r.seen, ran)
        assert r.seen["refused"] == 1, r.seen
    else:
        (tags, shared, info), ran = _timed(ctx, lambda: ctx.index_many_and_thresholds(sets, rs[0], isel, sels[0], t=ts))
    print("many", k, "jobs", len(jobs), "chunks", info["n_chunks"], ran)
    assert info["n_chunks"] == pinfo["n_chunks"] and info["search_launches"] == pinfo["search_launches"]
    assert ran.get("hits_jobs_kernel", 0) >= passes, ran                                # the jobs really share passes
    counts = rs[0].file_reads()
    for j, t in enumerate(ts):
        assert np.array_equal(tags[j], commet.tags_at(hits[j], t)), (j, t)
        assert shared[j].tolist() == _per_file(tags[j], counts), (j, t)
    e = next(j for j, (_, _, b) in enumerate(jobs) if not b.any())
    assert not tags[e].any() and not shared[e].any()                                   # the empty selection finds nothing
    # against the search at each job's own t
    for t in sorted(set(ts)) if against_search else []:
        with commet.Context(k=k, t=t) as c2:
            loaded = {}
            for j, (i, tj, b) in enumerate(jobs):
                if tj != t:
                    continue
                for x in (i, 0):
                    if x not in loaded:
                        loaded[x] = commet.ReadSet.from_files(c2, _SETS[k][0][x])
                got = c2.index_and_search(loaded[i], [loaded[0]], b, [sels[0]])[0][0]
                assert np.array_equal(tags[j], got), (j, i, t)
    return tags


_SETS = {}


@pytest.mark.parametrize("refuse", [False, True], ids=["device", "tag_words_refused"])
def test_thresholds_calls_on_the_four_sets(four, refuse):
    commet = _commet()
    sets, sels, searches = four
    _SETS[20] = (sets, sels)
    with commet.Context(k=20, t=2) as ctx:
        rs = [commet.ReadSet.from_files(ctx, fl) for fl in sets]
        assert rs[1].file_reads() == [3000, 3000]
        if refuse:
            # every buffer but the tag words exists after the profile: their request is the first one, refused -> the host loop
            args = (rs[0], [rs[1], rs[2], rs[3]], sels[0], [sels[1], sels[2], sels[3]])
            hits, _ = ctx.index_and_profile(*args, max_hits=3)
            with commet.refusing_device_allocs(nth=1) as r:
                (tags1, shared1, _), ran = _timed(ctx, lambda: ctx.index_and_thresholds(*args, max_t=3))
            words = sum(3 * (6000 // 64 + 1) + (1 + 3) * rs[i].num_files for i in (1, 2, 3))
            assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 8 * words, r.seen
            assert "hits_tags_kernel" not in ran, ran
            for s, i in enumerate((1, 2, 3)):
                for t in (1, 2, 3):
                    assert np.array_equal(tags1[s][t - 1], commet.tags_at(hits[s], t)) and np.array_equal(tags1[s][t - 1], searches[t][(0, i)])
                    assert shared1[s][t - 1].tolist() == _per_file(tags1[s][t - 1], rs[i].file_reads())
            with commet.Context(k=20, t=2) as fresh:                                  # (the many-job call below warms its own context)
                rs2 = [commet.ReadSet.from_files(fresh, fl) for fl in sets]
                fresh.set_option("chunk_group", 4)                                    # (two passes: the first on the host, the second on the device)
                _check_many(fresh, rs2, sels, _j2_jobs(rs2, tags1, [1, 2, 3], 3), 20, refuse=True, passes=2)
            return
        tags1 = _check_single(ctx, rs, sels, 0, [1, 2, 3], 3, searches)
        _check_many(ctx, rs, sels, _j2_jobs(rs, tags1, [1, 2, 3], 3), 20)
        ctx.set_option("chunk_group", 4)                                            # four slots a pass: the sharing jobs split into two passes
        _check_many(ctx, rs, sels, _j2_jobs(rs, tags1, [1, 2, 3], 3), 20, passes=2, against_search=False)


def test_thresholds_calls_on_a_pair_at_k32():
    commet = _commet()
    sets, sels = _pair32()
    _SETS[32] = (sets, sels)
    searches = _searches(sets, sels, 32, 3, [(0, 1)])
    with commet.Context(k=32, t=2) as ctx:
        rs = [commet.ReadSet.from_files(ctx, fl) for fl in sets]
        tags1 = _check_single(ctx, rs, sels, 0, [1], 3, searches)
        _check_many(ctx, rs, sels, _j2_jobs(rs, tags1, [1], 3), 32)


def test_thresholds_bad_arguments():
    commet = _commet()
    sets, sels = _pair32()
    with commet.Context(k=20, t=2) as ctx:
        a, b = (commet.ReadSet.from_files(ctx, fl) for fl in sets)
        for T in (0, 256):
            with pytest.raises(commet.CommetError):
                ctx.index_and_thresholds(a, [b], max_t=T)
            with pytest.raises(commet.CommetError):
                ctx.index_many_and_thresholds([a, a], b, t=[1, T])
        with pytest.raises(commet.CommetError):
            ctx.index_many_and_thresholds([a, a], b, t=[1])
