"""The hit profile through the tiled probe (option profile_tiled = 2; tq_probe_kernel + tq_hits_replay_kernel, hit_profile_tiled.hpp;
try_hits_tiled, capi/profile.hpp).  Ground truth is the same call at profile_tiled = 1, the slot loop, with byte-equal hit arrays;
where a set is designed, its designed bytes (proved on the CPU checker by test_hit_profile_tiled_cpu.py); for some the checker's tags at
every t.  Every tiled call is held to have launched both kernels (kernel_times).  The read sets come from hit_profile_tiled_sets.py."""
import os
import re

import numpy as np
import pytest

import hit_profile_tiled_sets as ts
import util
from scenarios import Scenario, run_oracle
from test_hit_profile_groups_cpu import checker_tags

pytestmark = pytest.mark.gpu

TILED = ("tq_probe_kernel", "tq_hits_replay_kernel")
SLOT_HITS = ("hits_kernel", "hits_group_kernel", "hits_wave_kernel", "hits_group_wave_kernel")
ALLOC_MESSAGE = re.compile(r"memory|allocat", re.I)


def _commet():
    import commet_amd
    return commet_amd


def _context(k, t=2, **opts):
    ctx = _commet().Context(k=k, t=t)
    for name, value in opts.items():
        ctx.set_option(name, value)
    return ctx


def _load(ctx, reads):
    return _commet().ReadSet.from_files(ctx, [util.to_batch(reads)])


def _profile(ctx, irs, srs, tiled, max_hits, selects=None, index_select=None):
    """one profile call at profile_tiled = tiled -> (hits, info, {kernel: launches})"""
    ctx.set_option("profile_tiled", tiled)
    ctx.set_option("kernel_timing", 1)                            # (the totals start again)
    try:
        hits, info = ctx.index_and_profile(irs, srs, index_select, selects, max_hits=max_hits)
        times = ctx.kernel_times()
    finally:
        ctx.set_option("kernel_timing", 0)
    return hits, info, {n: times[n][0] for n in times}


def _both(ctx, irs, srs, max_hits, n_tiled_sets, passes, selects=None):
    """the call through the tiled probe and through the slot loop: byte-equal arrays, equal plans and walked reads, both tiled kernels
    launched once per pass and tiled set and no hits kernel beside them (n_tiled_sets = len(srs)), none of them in the slot loop"""
    hits, info, ran = _profile(ctx, irs, srs, 2, max_hits, selects)
    one, info1, ran1 = _profile(ctx, irs, srs, 1, max_hits, selects)
    for name in TILED:
        assert ran.get(name, 0) == passes * n_tiled_sets and name not in ran1, (name, ran, ran1)
    if n_tiled_sets == sum(1 for s in srs if s.num_reads):
        assert not any(n in ran for n in SLOT_HITS), ran
    assert any(n in ran1 for n in SLOT_HITS), ran1
    for f in ("n_chunks", "kmers_indexed", "reads_indexed", "search_launches", "reads_scanned", "index_launches"):
        assert info[f] == info1[f], (f, info[f], info1[f])
    assert info["probes"] == 0
    for q, (a, b) in enumerate(zip(hits, one)):
        assert np.array_equal(a, b), (q, np.flatnonzero(a != b)[:10], a[a != b][:10], b[a != b][:10])
    return hits, info, ran


# ---- 1. window sweep -------------------------------------------------------------------------------------------------------------------
def _sweep_case(tmp_path, ctx, k, n_chunks, caps=(None,)):
    index, max_kmer, sets = ts.window_sweep(k, n_chunks)
    T = max(max(exp) for _, exp in sets.values()) + 1
    ctx.set_option("max_kmer", max_kmer)
    irs = _load(ctx, index)
    srs = [_load(ctx, sets[W][0]) for W in ts.WINDOWS]
    try:
        for cap in caps:
            if cap is not None:
                ctx.set_option("tq_hit_cap", cap)
            hits, info, ran = _both(ctx, irs, srs, T, len(srs), 1)
            assert info["n_chunks"] == n_chunks and info["search_launches"] == len(srs)
            for W, h in zip(ts.WINDOWS, hits):
                assert h.tolist() == sets[W][1], (k, n_chunks, cap, W, [(i, int(g), e) for i, (g, e) in enumerate(zip(h, sets[W][1])) if g != e][:8])
        if (k, n_chunks) in ts.CHECKED_SWEEPS:
            for t in range(1, T + 1):
                tags, chunks = checker_tags(tmp_path / f"orc{k}_{n_chunks}", k, t, index, [sets[W][0] for W in ts.WINDOWS], max_kmer=max_kmer)
                assert chunks == n_chunks
                for h, tg in zip(hits, tags):
                    assert np.array_equal(h >= t, tg), (k, n_chunks, t)
    finally:
        ctx.set_option("tq_hit_cap", 1024)
        for rs in srs + [irs]:
            rs.close()


@pytest.mark.parametrize("n_chunks", [1, 2])
@pytest.mark.parametrize("k", ts.SWEEP_KS)
def test_window_sweep(tmp_path, k, n_chunks):
    """reads of 1 .. 255 windows (mask widths 2, 2, 2, 3, 4, 6, 8, 8), hits at the first and the last window, at bits 31 / 32 and 63 / 64 of
    the mask words, k - 1 and k apart, on either strand, with one and two chunk filters"""
    with _context(k) as ctx:
        _sweep_case(tmp_path, ctx, k, n_chunks)


def test_window_sweep_with_wide_keys(tmp_path):
    """k = 33: the 64-bit builds, one and two filters, in one context"""
    with _context(ts.WIDE_K) as ctx:
        for n_chunks in (1, 2):
            _sweep_case(tmp_path, ctx, ts.WIDE_K, n_chunks)


@pytest.mark.parametrize("n_chunks", [1, 2])
def test_hit_list_overflow(tmp_path, n_chunks):
    """tq_hit_cap = 0 and 3: the pieces' hit lists overflow and every scan walks its own candidates: the same bytes"""
    with _context(25) as ctx:
        _sweep_case(tmp_path, ctx, 25, n_chunks, caps=(0, 3))


# ---- 1b. the two consumers of the replay's shared steps ------------------------------------------------------------------------------------
def _first_hit_windows(k, t, max_len):
    """first_hit_windows of capi/search_dispatch.hpp: max_len - t_eff k + 1 with t_eff = min(t, max_len / k + 1)"""
    return max_len - min(t, max_len // k + 1) * k + 1


def _left_out(k, T):
    """the (W, t) pairs, t in 1..T, at which the sweep's set of W-window reads (all of k + W - 1 bases) has no first-hit window: the
    tiled search does not take it (tq_geometry_ok asks for 1..255), so it is not searched at that t"""
    return [(W, t) for W in ts.WINDOWS for t in range(1, T + 1) if _first_hit_windows(k, t, k + W - 1) < 1]


def _largest_t(k, designed):
    """T = the largest designed count + 1, lowered until at most a quarter of the (set, t) pairs are left out — from the sets' lengths
    alone.  k = 25: T = 4, 8 of 32 pairs left out (W = 1 from t = 2, W = 32 and 33 from t = 3, W = 65 at t = 4).  k = 33: the designed
    T = 4 would leave out 12 of 32 and T = 3 7 of 24 (a window costs 33 bases per further hit), so T = 2: 3 of 16"""
    T = designed + 1
    while T > 1 and 4 * len(_left_out(k, T)) > len(ts.WINDOWS) * T:
        T -= 1
    return T


@pytest.mark.parametrize("cap", [1024, 3, 0])
@pytest.mark.parametrize("n_chunks", [1, 2])
@pytest.mark.parametrize("k", [25, ts.WIDE_K])
def test_search_and_profile_agree_on_the_window_sweep(k, n_chunks, cap):
    """tq_replay_kernel and tq_hits_replay_kernel share the collect and the sweep (tq_collect, tq_sweep: tile_search.hpp): on the window
    sweep's sets (mask widths 2, 3, 4, 6 and 8 by mask_words_of, capi/search_dispatch.hpp; hits at bits 31 / 32 and 63 / 64, either
    strand) the tiled search's found flags at every t in 1..T are the tiled profile's hits >= t, read by read, at every hit-list cap.
    T comes from the quarter rule (_largest_t: 4 at k = 25, 2 at k = 33).  Beyond it, up to the largest designed count + 1 (where no
    read is found), the sets that still have a first-hit window are compared as well (k = 33: W >= 97 at t = 3, W >= 129 at t = 4);
    those pairs stand outside the quarter count.  The profile runs once, at max_hits = the largest designed count + 1"""
    commet = _commet()
    index, max_kmer, sets = ts.window_sweep(k, n_chunks)
    top = max(max(exp) for _, exp in sets.values()) + 1
    T = _largest_t(k, top - 1)
    left_out = _left_out(k, T)
    assert 2 <= T <= top and 4 * len(left_out) <= len(ts.WINDOWS) * T, (k, T, left_out)
    no_window = _left_out(k, top)
    opts = dict(max_kmer=max_kmer, chunk_group=2, tq_hit_cap=cap)
    with _context(k, **opts) as ctx:
        irs, srs = _load(ctx, index), [_load(ctx, sets[W][0]) for W in ts.WINDOWS]
        hits, info, ran = _profile(ctx, irs, srs, 2, top)
        assert info["n_chunks"] == n_chunks and all(ran.get(n) == len(srs) for n in TILED) and "tq_replay_kernel" not in ran, ran
    compared = 0
    for t in range(1, top + 1):
        took = [i for i, W in enumerate(ts.WINDOWS) if (W, t) not in no_window]
        assert took, (k, t)
        with _context(k, t=t, tiled_search=2, **opts) as ctx:
            irs, srs = _load(ctx, index), [_load(ctx, sets[ts.WINDOWS[i]][0]) for i in took]
            ctx.set_option("kernel_timing", 1)
            tags, _, sinfo = ctx.index_and_search(irs, srs)
            ran = {n: v[0] for n, v in ctx.kernel_times().items()}
        assert sinfo["n_chunks"] == n_chunks and ran.get("tq_replay_kernel") == ran.get("tq_probe_kernel") == len(took), (t, ran)
        assert "tq_hits_replay_kernel" not in ran and not any(n.startswith("search_") for n in ran), (t, ran)
        for i, tg in zip(took, tags):
            found = util.bools_from_bits(tg, len(hits[i]))
            assert np.array_equal(found, hits[i] >= t), (k, n_chunks, cap, t, ts.WINDOWS[i], np.flatnonzero(found != (hits[i] >= t))[:8])
            assert t < top or not found.any(), (k, t, ts.WINDOWS[i])
            compared += t <= T
    assert compared == len(ts.WINDOWS) * T - len(left_out)


# ---- 2. filter and strand independence ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_filter_and_strand_independence(case):
    name, index, search, exp, max_kmer, n_chunks = ts.independence_sets()[case]
    with _context(25, max_kmer=max_kmer) as ctx:
        hits, info, _ = _both(ctx, _load(ctx, index), [_load(ctx, search)], max(exp) + 1, 1, 1)
        assert info["n_chunks"] == n_chunks == 2
        assert hits[0].tolist() == exp, name


# ---- 3. heavy scans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_hits", [1, 3, 255])
def test_heavy_scans(max_hits):
    """reads copied from the index set: more than 20 lane-a candidates on one strand; saturation stops their walk, their other strand and
    the other filter stay in the sweep"""
    index, max_kmer, sets = ts.heavy_sets()
    with _context(ts.HEAVY_K, max_kmer=max_kmer) as ctx:
        hits, info, _ = _both(ctx, _load(ctx, index), [_load(ctx, sets[L][0]) for L in (100, 280)], max_hits, 2, 1)
        assert info["n_chunks"] == 2
        for L, h in zip((100, 280), hits):
            assert h.tolist() == [min(max_hits, e) for e in sets[L][1]], (L, max_hits)


# ---- 4. piece edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ts.PIECE_SIZES)
def test_piece_edges(n):
    index, search, max_kmer = ts.related_case(25, 2, n)
    sel = ts.piece_selection(n)
    with _context(25, max_kmer=max_kmer) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        full, info, _ = _both(ctx, irs, [srs], 5, 1, 1)
        assert info["n_chunks"] == 2 and info["reads_scanned"] == n
        part, info, _ = _both(ctx, irs, [srs], 5, 1, 1, selects=[util.bits_from_bools(sel)])
        assert np.array_equal(part[0], np.where(sel, full[0], 0)) and info["reads_scanned"] == int(sel.sum())
        assert int(full[0][0]) == 4                                # (100 bases of an index read: windows 0, 25, 50, 75)
        if n >= 255:
            assert {0, 4} <= set(full[0].tolist()) and len(set(full[0].tolist())) >= 4


# ---- 5. short and unclean reads ----------------------------------------------------------------------------------------------------------------
def test_short_and_unclean_reads(tmp_path):
    """a ragged set with reads shorter than k, N runs and lower-case bases, an empty set, a set whose reads are all shorter than k, a second
    copy of some reads: four search sets in one call"""
    k, T = 25, 5
    index, search, max_kmer = ts.related_case(k, 2, 513)
    short = [r[:k - 1] for r in search[:40]]
    with _context(k, max_kmer=max_kmer) as ctx:
        irs = _load(ctx, index)
        srs = [_load(ctx, s) for s in (search, [], short, search[100:170])]
        hits, info, ran = _both(ctx, irs, srs, T, 2, 1)            # (the set without a k-mer keeps hits_group_kernel)
        assert ran.get("hits_group_kernel") == 1 and info["search_launches"] == 3
        assert hits[1].size == 0 and not hits[2].any() and np.array_equal(hits[3], hits[0][100:170])
        assert {0, 4} <= set(hits[0].tolist()) and len(set(hits[0].tolist())) >= 4
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
        assert chunks == 2 and np.array_equal(hits[0] >= t, tags[0]), t


# ---- 6. fold across passes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chunks", [3, 5])
def test_fold_across_passes(n_chunks):
    """chunk_group = 2: tiled passes of two filters and of one, folded with max; a saturated read is not walked again"""
    index, search, exp, max_kmer, _ = ts.planted_slots(25, n_chunks=n_chunks)
    passes = (n_chunks + 1) // 2
    with _context(25, max_kmer=max_kmer, chunk_group=2) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        hits, info, ran = _both(ctx, irs, [srs], 4, 1, passes)
        assert info["n_chunks"] == n_chunks and info["search_launches"] == passes
        assert hits[0].tolist() == exp == [3] * n_chunks and info["reads_scanned"] == passes * n_chunks
        assert ran.get("interleave_a_kernel") == n_chunks // 2
        hits, info, _ = _both(ctx, irs, [srs], 1, 1, passes)
        assert hits[0].tolist() == [1] * n_chunks
        # read p is saturated by the pass that holds chunk p or chunk p + 1, and the first pass sees reads 0, 1 and the last one
        assert n_chunks <= info["reads_scanned"] < passes * n_chunks
        assert info["reads_scanned"] == sum(n_chunks - min(n_chunks, 2 * p + (1 if p else 0)) for p in range(passes))


# ---- 7. against the checker ------------------------------------------------------------------------------------------------------------------------
def _load_set(commet, ctx, files, sdir):
    batches = [util.to_batch(util.parse_reads(os.path.join(sdir, fa))) for fa, _, _, _ in files]
    rs = commet.ReadSet.from_files(ctx, batches)
    sel = np.concatenate([s for _, _, _, s in files]) if files else np.zeros(0, bool)
    has_bv = any(bv for _, bv, _, _ in files)
    return rs, (util.bits_from_bools(sel) if has_bv else None)


@pytest.mark.parametrize("seed", ts.RANDOM_SEEDS)
def test_random_scenarios_match_checker(tmp_path, seed):
    commet = _commet()
    T, k = 6, ts.random_k(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    names = sorted(scn.search_names)
    with _context(k, max_kmer=ts.RANDOM_MAX_KMER, chunk_group=2) as ctx:
        irs, isel = _load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
        loaded = [_load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
        hits, info, ran = _profile(ctx, irs, [r for r, _ in loaded], 2, T, [s for _, s in loaded], isel)
        one, info1, ran1 = _profile(ctx, irs, [r for r, _ in loaded], 1, T, [s for _, s in loaded], isel)
    assert info["n_chunks"] == info1["n_chunks"] >= 3
    assert all(ran.get(n, 0) >= 2 for n in TILED) and not any(n in ran1 for n in TILED), (ran, ran1)
    for a, b in zip(hits, one):
        assert np.array_equal(a, b)
    for t in range(1, T + 1):
        scn.t = t
        out_o = str(tmp_path / f"out{t}")
        rc, res, chunks, kmers = run_oracle(scn, out_o, str(tmp_path / f"log{t}"), max_kmer=ts.RANDOM_MAX_KMER)
        assert rc == 0 and info["n_chunks"] == chunks and info["kmers_indexed"] == kmers
        for nme, h in zip(names, hits):
            pos = 0
            for fa, _, reads, _ in scn.sets[nme]:
                _, n, bits = util.read_bv(os.path.join(out_o, os.path.basename(fa) + "_in_" + scn.index_name + ".bv"))
                assert np.array_equal(h[pos:pos + n] >= t, util.bools_from_bits(bits, n)), (seed, k, t, nme, fa)
                pos += n
            assert pos == h.size


# ---- 8. lists --------------------------------------------------------------------------------------------------------------------------------------
def test_second_profile_builds_no_list():
    index, search, max_kmer = ts.related_case(25, 2, 513)
    with _context(25, max_kmer=max_kmer) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        first, _, ran = _profile(ctx, irs, [srs], 2, 5)
        assert ran.get("tq_fill_kernel") == ran.get("tq_count_kernel") == 1 and srs.cache_bytes > 0
        second, _, ran = _profile(ctx, irs, [srs], 2, 5)
        assert "tq_fill_kernel" not in ran and "tq_count_kernel" not in ran and all(n in ran for n in TILED)
        assert np.array_equal(first[0], second[0])


@pytest.mark.parametrize("t", [1, 2])
def test_job_and_profile_keep_their_lists(t):
    """job, profile, job, profile on one set: at t = 2 two lists are live at once and each is built once; at t = 1 the profile scans the
    search's own list, built once.  cache_bytes covers what is live, drop_cache() frees it"""
    index, search, max_kmer = ts.related_case(25, 2, 513)
    with _context(25, t=t, max_kmer=max_kmer, tiled_search=1, profile_tiled=1) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        want_tags, want_stats, _ = ctx.index_and_search(irs, [srs])
        want_hits, _ = ctx.index_and_profile(irs, [srs], max_hits=5)
        assert srs.cache_bytes == 0
        ctx.set_option("tiled_search", 2)
        ctx.set_option("profile_tiled", 2)
        ctx.set_option("kernel_timing", 1)
        sizes = []
        for _ in range(2):
            tags, stats, _ = ctx.index_and_search(irs, [srs])
            assert tags[0].tobytes() == want_tags[0].tobytes() and stats[0]["shared"] == want_stats[0]["shared"]
            sizes.append(srs.cache_bytes)
            hits, _ = ctx.index_and_profile(irs, [srs], max_hits=5)
            assert np.array_equal(hits[0], want_hits[0])
            sizes.append(srs.cache_bytes)
        ran = {n: v[0] for n, v in ctx.kernel_times().items()}
        ctx.set_option("kernel_timing", 0)
        assert ran["tq_replay_kernel"] == 2 and ran["tq_hits_replay_kernel"] == 2 and ran["tq_probe_kernel"] == 4, ran
        assert ran["tq_fill_kernel"] == ran["tq_count_kernel"] == (2 if t == 2 else 1), ran
        assert sizes[0] > 0 and sizes[1:] == [sizes[1]] * 3 and (sizes[1] > sizes[0]) == (t == 2), sizes
        assert ctx.cache_stats()["bytes"] == sizes[-1]
        srs.drop_cache()
        assert srs.cache_bytes == 0 and ctx.cache_stats()["bytes"] == 0
        hits, _, ran = _profile(ctx, irs, [srs], 2, 5)
        assert np.array_equal(hits[0], want_hits[0]) and ran.get("tq_fill_kernel") == 1


def test_budget_too_small_for_both_lists_evicts_one():
    """20 000 reads of 100 bases at k = 25: the search's list (t = 2, 51 windows per read) holds about 6 MB, the profile's (76) about
    9 MB; a budget of 10 MB keeps one"""
    from commet_amd import synth
    (ib, io), (sb, so) = synth.synth_set(0, 20000, 100), synth.synth_set(1, 20000, 100)
    commet = _commet()
    with _context(25, max_kmer=800000, tiled_search=2, profile_tiled=2) as ctx:
        irs, srs = commet.ReadSet.from_files(ctx, [(ib, io)]), commet.ReadSet.from_files(ctx, [(sb, so)])
        tags, _, jinfo = ctx.index_and_search(irs, [srs])
        job_list = srs.cache_bytes
        hits, info = ctx.index_and_profile(irs, [srs], max_hits=6)
        both = srs.cache_bytes
        assert jinfo["n_chunks"] == info["n_chunks"] == 2
        assert 5 << 20 < job_list < 8 << 20 and 8 << 20 < both - job_list < 10 << 20, (job_list, both)
        before = ctx.cache_stats()["evictions"]
        ctx.set_option("query_list_budget_mb", 10)
        assert srs.cache_bytes == both - job_list and ctx.cache_stats()["evictions"] == before + 1     # (the job's list was used longest ago)
        _, _, ran = _profile(ctx, irs, [srs], 2, 6)
        assert "tq_fill_kernel" not in ran                          # the profile's list is the one that stayed
        tags2, _, _ = ctx.index_and_search(irs, [srs])             # builds the job's list again (no list of a running call is evicted)
        hits2, _ = ctx.index_and_profile(irs, [srs], max_hits=6)
        assert tags2[0].tobytes() == tags[0].tobytes() and np.array_equal(hits2[0], hits[0])
        assert commet.tags_at(hits[0], 2).tobytes() == tags[0].tobytes() and int((hits[0] > 0).sum()) > 100


def test_offload_and_restore_then_a_profile():
    index, search, max_kmer = ts.related_case(25, 2, 513)
    with _context(25, max_kmer=max_kmer) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        want, _, _ = _profile(ctx, irs, [srs], 2, 5)
        assert srs.cache_bytes > 0
        srs.offload()
        assert srs.cache_bytes == 0 and ctx.cache_stats()["bytes"] == 0
        srs.restore()
        hits, _, ran = _profile(ctx, irs, [srs], 2, 5)
        assert np.array_equal(hits[0], want[0]) and ran.get("tq_fill_kernel") == 1 and all(n in ran for n in TILED)


def test_auto_takes_sets_of_a_million_reads_within_the_list_cap():
    """profile_tiled = 0: the tiled profile for a set of 2^20 reads whose list estimate (8 bytes per k-mer) lies within query_list_max_mb;
    the slot loop for a set of 2^20 - 1 reads, and for the first when the cap is below its estimate.  40-base reads at k = 25: 16 k-mers"""
    commet = _commet()
    n, L, k = 1 << 20, 40, 25
    rng = np.random.default_rng(5)
    bases = util.ACGT[rng.integers(0, 4, size=n * L, dtype=np.uint8)]
    offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    index = [bases[i * L:(i + 1) * L].tobytes() for i in range(0, n, n // 300)]
    with _context(k, max_kmer=2500) as ctx:                        # 305 reads of 16 k-mers: two chunks
        irs = _load(ctx, index)
        big = commet.ReadSet.from_files(ctx, [(bases, offs)])
        small = commet.ReadSet.from_files(ctx, [(bases[:-L], offs[:-1])])
        want, info1, ran1 = _profile(ctx, irs, [big, small], 1, 3)
        hits, info, ran = _profile(ctx, irs, [big, small], 0, 3)
        assert info["n_chunks"] == info1["n_chunks"] == 2
        assert all(ran.get(name) == 1 for name in TILED) and ran.get("hits_group_kernel") == 1 and ran1.get("hits_group_kernel") == 2, (ran, ran1)
        assert big.cache_bytes > n * (L - k + 1) * 6 and small.cache_bytes == 0
        ctx.set_option("query_list_max_mb", (n * (L - k + 1) * 8 >> 20) - 1)
        capped, _, ran = _profile(ctx, irs, [big, small], 0, 3)
        assert not any(name in ran for name in TILED) and ran.get("hits_group_kernel") == 2, ran
        for q in range(2):
            assert np.array_equal(hits[q], want[q]) and np.array_equal(capped[q], want[q])
        assert int((want[0] > 0).sum()) >= len(index) - 2 and np.array_equal(want[1], want[0][:-1])


def test_option_range():
    with _context(25) as ctx:
        for bad in (-1, 3):
            with pytest.raises(_commet().CommetError, match="profile_tiled"):
                ctx.set_option("profile_tiled", bad)
        ctx.set_option("profile_tiled", 0)


# ---- 9. no room ------------------------------------------------------------------------------------------------------------------------------------
def test_every_request_of_a_tiled_profile_refused_in_turn():
    """the sweep of test_gpu_alloc_refusal.py: every device allocation of one tiled profile call on a fresh context refused in turn (the
    nth request from arming on, once).  The call returns the unarmed bytes — through the slot loop where the list or the result bytes
    found no room — or raises an allocation message, and then succeeds, disarmed, on the same context and sets"""
    commet = _commet()
    index, search, max_kmer = ts.related_case(25, 2, 513)

    def make():
        ctx = _context(25, max_kmer=max_kmer, profile_tiled=2)
        return ctx, _load(ctx, index), _load(ctx, search)

    def call(state):
        ctx, irs, srs = state
        ctx.set_option("kernel_timing", 1)
        hits, info = ctx.index_and_profile(irs, [srs], max_hits=5)
        return hits[0], info["n_chunks"], {n for n in ctx.kernel_times()}

    state = make()
    try:
        with commet.refusing_device_allocs() as r:
            base = call(state)
        n_requests = r.seen["requests"]
    finally:
        state[0].close()
    assert n_requests >= 6 and all(n in base[2] for n in TILED), (n_requests, base[2])     # (the list alone is five blocks)
    returned = raised = through_slots = 0
    for n in range(1, n_requests + 1):
        state = make()
        try:
            outcome, out = "returned", None
            with commet.refusing_device_allocs(nth=n) as r:
                try:
                    out = call(state)
                except commet.CommetError as e:
                    outcome = "raised: " + str(e)
            print(f"tiled profile: n = {n}, last_refused_bytes = {r.seen['last_refused_bytes']}, {outcome}")
            assert r.seen["refused"] == 1, (n, r.seen)
            if out is None:
                raised += 1
                assert ALLOC_MESSAGE.search(outcome) and "internal error" not in outcome, (n, outcome)
                out = call(state)
            else:
                returned += 1
                through_slots += "tq_hits_replay_kernel" not in out[2]
            assert np.array_equal(out[0], base[0]) and out[1] == base[1], (n, outcome)
        finally:
            state[0].close()
    print(f"tiled profile: N = {n_requests}, returned {returned} ({through_slots} through the slot loop), raised {raised}")
    assert through_slots >= 5                                        # the list's blocks and the result bytes promise a fallback


# ---- 10. fallback ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["long_read", "long_search", "sparse"])
def test_sets_outside_the_tiled_profile_run_what_they_ran(kind):
    k = 25
    index, search, max_kmer = ts.related_case(k, 2, 513)
    opts, selects, kernel = {}, None, "hits_group_kernel"
    if kind == "long_read":
        search = search + [index[0] + index[1] + index[2][:k + 255 - 220]]           # k + 255 bases: 256 windows
        assert len(search[-1]) == k + 255
    elif kind == "long_search":
        opts, kernel = dict(long_search=2), "hits_group_wave_kernel"
    else:
        opts, selects = dict(sparse_search=2), [util.bits_from_bools(np.arange(len(search)) % 5 == 0)]
    with _context(k, max_kmer=max_kmer, **opts) as ctx:
        irs, srs = _load(ctx, index), _load(ctx, search)
        hits, info, ran = _profile(ctx, irs, [srs], 2, 5, selects)
        one, info1, ran1 = _profile(ctx, irs, [srs], 1, 5, selects)
        assert ran == ran1 and kernel in ran and not any(n in ran for n in TILED), (ran, ran1)
        assert np.array_equal(hits[0], one[0]) and info["reads_scanned"] == info1["reads_scanned"]
        assert int((hits[0] > 0).sum()) > 5
        assert srs.cache_bytes == 0
