"""The hit profile through the narrow bit-sliced tables (option profile_slice = 2; hits_sliced_kernel, hit_profile_sliced.hpp;
run_profile_sliced, capi/profile.hpp).  Ground truth is always (a) the same call at profile_slice = 1, the slot loop, with byte-equal hit
arrays and equal plans, and, where stated, (b) the CPU checker once per t (hits >= t equals its bits).  Every case checks the launches:
hits_sliced_kernel ran passes x non-empty sets times, no other hits kernel ran, and the tables were built once per pass.  The read sets
come from hit_profile_slice_sets.py; test_hit_profile_slice_cpu.py proves their chunk counts, designed counts and the kernel's bounds
without a GPU."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_slice_sets as ss
import oracle_pool
import util
from conftest import ROOT
from scenarios import Scenario, run_oracle
from test_hit_profile_groups_cpu import checker_tags

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
SLOT_KERNELS = ("hits_kernel", "hits_wave_kernel", "hits_group_kernel", "hits_group_wave_kernel")
OTHER_TABLE_KERNELS = ("hits_wide_kernel", "tq_hits_replay_kernel")


def _profile(index, search_sets, k, max_hits, max_kmer, slice_opt, words=0, index_select=None, search_selects=None, **opts):
    """-> (hits, info, {kernel: (launches, ms)})"""
    import commet_amd as commet
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in search_sets]
        # (profile_wide = 1 unless a case says otherwise: the wide rows come first, and auto takes them from 257 chunks on)
        for name, value in dict({"profile_wide": 1, **opts}, max_kmer=max_kmer, profile_slice=slice_opt, slice_words=words, kernel_timing=1).items():
            ctx.set_option(name, value)
        hits, info = ctx.index_and_profile(irs, srs, index_select, search_selects, max_hits=max_hits)
        return hits, info, ctx.kernel_times()


def _timed(ctx, call):
    """-> (the call's result, the kernel times of that call alone): the totals start again at every set_option("kernel_timing", 1)"""
    ctx.set_option("kernel_timing", 1)
    out = call()
    return out, ctx.kernel_times()


def _check_sliced(times, info, passes, n_sets):
    """the narrow tables ran, launch for launch, and no other hits kernel did"""
    if passes * n_sets:
        assert times["hits_sliced_kernel"][0] == passes * n_sets, (times.get("hits_sliced_kernel"), passes, n_sets)
    else:
        assert "hits_sliced_kernel" not in times
    assert info["search_launches"] == passes * n_sets and info["index_launches"] == 2 * passes and info["probes"] == 0
    assert not [n for n in SLOT_KERNELS + OTHER_TABLE_KERNELS if n in times], sorted(times)
    if passes:
        assert times["slice_build_kernel"][0] == times["slice_transpose_kernel"][0] == passes
    assert "interleave_a_kernel" not in times


def _check_slots(times):
    assert "hits_sliced_kernel" not in times and "hits_wide_kernel" not in times and [n for n in SLOT_KERNELS if n in times], sorted(times)


def _both(index, search_sets, k, max_hits, max_kmer, words=0):
    """the call at profile_slice = 2 and at 1 -> (hits, info, passes): byte-equal arrays, equal plans"""
    hits, info, times = _profile(index, search_sets, k, max_hits, max_kmer, 2, words)
    slot, info1, times1 = _profile(index, search_sets, k, max_hits, max_kmer, 1, words)
    passes = ss.plan(info["n_chunks"], k, words)[1]
    _check_sliced(times, info, passes, sum(1 for s in search_sets if len(s)))
    _check_slots(times1)
    for f in ("n_chunks", "kmers_indexed", "reads_indexed"):
        assert info[f] == info1[f], f
    for q, (h, s) in enumerate(zip(hits, slot)):
        assert h.dtype == np.uint8 and np.array_equal(h, s), (q, np.nonzero(h != s)[0][:10], h[h != s][:10], s[h != s][:10])
    # a pass walks a visited read of at least k bases unless it stands at its cap already: every such read in the first pass
    walkable = sum(sum(1 for r in s if len(r) >= k) for s in search_sets)
    assert walkable <= info["reads_scanned"] <= passes * walkable, (walkable, info["reads_scanned"], passes)
    return hits, info, passes


# ---- 1. every instantiation and the word and pass edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("k,L,n_chunks,words,gw,passes", ss.ROWS)
def test_every_instantiation_matches_the_slot_loop_and_the_checker(k, L, n_chunks, words, gw, passes):
    index, queries = ss.row_set(k, L, n_chunks)
    hits, info, got_passes = _both(index, [queries], k, ss.ROW_T, 1, words)
    assert info["n_chunks"] == n_chunks and got_passes == passes and ss.plan(n_chunks, k, words)[0] == gw
    h = hits[0]
    print(k, L, n_chunks, gw, passes, np.bincount(h, minlength=ss.ROW_T + 1).tolist(), info["reads_scanned"])
    assert int(h.max()) <= min(ss.ROW_T, L // k) and int((h > 0).sum()) > 60 and len(set(h.tolist())) >= 3
    if k <= ss.CHECKER_MAX_K:
        import oracle_binding as ob
        ib, io = util.to_batch(index)
        qb, qo = util.to_batch(queries)
        chunks = oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, k), 1)
        assert len(chunks) == n_chunks
        for t in range(1, 5):
            tags = util.bools_from_bits(oracle_pool.chunk_loop_in_threads(k, t, ib, io, qb, qo, chunks, len(queries))[0], len(queries))
            assert np.array_equal(h >= t, tags), (k, t, np.nonzero((h >= t) != tags)[0][:10])


# ---- 2. planted reads ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ss.PLANTED_KS)
def test_planted_reads(tmp_path, k):
    T = 4
    index, search, exp, names = ss.planted(k)
    hits, info, passes = _both(index, [search], k, T, 1)
    assert info["n_chunks"] == ss.PLANTED_CHUNKS and passes == 3
    got = hits[0].tolist()
    print(k, list(zip(names, got, exp)))
    assert got == [min(T, e) for e in exp], [(n, g, e) for n, g, e in zip(names, got, exp) if g != min(T, e)]
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=1)
        assert chunks == ss.PLANTED_CHUNKS and np.array_equal(hits[0] >= t, tags[0]), t


@pytest.mark.parametrize("k", ss.PLANTED_KS)
def test_saturation_of_counter_and_cap(tmp_path, k):
    index, search, exact = ss.saturation(k)
    for max_hits in (3, exact, exact + 1, 255):
        hits, info, _ = _both(index, [search], k, max_hits, 1)
        assert info["n_chunks"] == 12
        h = hits[0]
        assert int(h[0]) == int(h[1]) == min(max_hits, exact) and int(h[2]) == min(max_hits, 100 // k) and int(h[3]) == 0, (max_hits, h.tolist())
    for t in (1, exact, exact + 1):
        tags, _ = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=1)
        assert np.array_equal(hits[0] >= t, tags[0]), t


@pytest.mark.parametrize("words", [0, 2])
def test_palindromic_kmer(tmp_path, words):
    """a k-mer that is its own reverse complement has its own partner in plane A: the `selfp` entry, in the pair load of gw <= 2"""
    k = 20
    index, search, exp, max_kmer, n_chunks = ss.planted_palindrome(k)
    T = max(exp) + 1
    hits, info, _ = _both(index, [search], k, T, max_kmer, words)
    assert info["n_chunks"] == n_chunks and hits[0].tolist() == exp and ss.plan(n_chunks, k, words)[0] == (words or 1)
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
        assert chunks == n_chunks and np.array_equal(hits[0] >= t, tags[0]), t


def test_lower_bounds(tmp_path):
    """counter 1 everywhere: the count is 1 without a replay; blocks i and i + 2 of one chunk only: counter 2, count 2"""
    k, T = ss.BOUNDS_K, 4
    index, search, exp, names = ss.bounds_set(k)
    hits, info, passes = _both(index, [search], k, T, 1)
    assert info["n_chunks"] == ss.BOUNDS_CHUNKS and passes == 1
    assert hits[0].tolist() == exp, list(zip(names, hits[0].tolist(), exp))
    for t in range(1, 4):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=1)
        assert chunks == ss.BOUNDS_CHUNKS and np.array_equal(hits[0] >= t, tags[0]), t
    hits1 = _profile(index, [search], k, 1, 1, 2)[0]                              # cap 1: the lower bound 2 is cut to it
    assert hits1[0].tolist() == [min(1, e) for e in exp]


# ---- 3. selections and edges ----------------------------------------------------------------------------------------------------------
def test_selections_sets_and_edges(tmp_path):
    import commet_amd as commet
    k, T = ss.EDGE_K, 5
    index, fixed, ragged = ss.edge_cut()
    n = len(fixed)
    rng = np.random.default_rng(8)
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("max_kmer", 1)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(fixed)])
        prefix = commet.ReadSet.from_files(ctx, [util.to_batch(fixed[:257])])
        rag = commet.ReadSet.from_files(ctx, [util.to_batch(ragged)])
        tags0, _, jinfo = ctx.index_and_search(irs, [srs])
        ctx.set_option("profile_slice", 1)
        slot, info1 = ctx.index_and_profile(irs, [srs, rag], max_hits=T)
        ctx.set_option("profile_slice", 2)
        (full, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [srs, rag], max_hits=T))
        n_chunks = info["n_chunks"]
        assert n_chunks == info1["n_chunks"] == jinfo["n_chunks"] and abs(n_chunks - ss.EDGE_CHUNKS) <= 4
        assert ss.plan(n_chunks, k) == (8, 1)
        _check_sliced(times, info, 1, 2)
        assert np.array_equal(full[0], slot[0]) and np.array_equal(full[1], slot[1])
        assert int((full[0] > 0).sum()) > n // 10 and int((full[1] > 0).sum()) > 50
        # ragged reads: those shorter than k are not walked and hold zero
        short = np.array([len(r) < k for r in ragged])
        assert short.sum() > 5 and not full[1][short].any()
        assert info["reads_scanned"] == n + int((~short).sum())
        for t in range(1, 4):
            tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [fixed, ragged], max_kmer=1)
            assert chunks == n_chunks
            for q in range(2):
                assert np.array_equal(full[q] >= t, tags[q]), (t, q)
        # selections of the search set; two sets in one call, the second a prefix of the first
        for frac in (0.7, 0.02, 0.0):
            sel = rng.random(n) < frac
            (hits, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [srs, prefix], search_selects=[util.bits_from_bools(sel), None], max_hits=T))
            assert np.array_equal(hits[0], np.where(sel, full[0], 0)), frac
            assert np.array_equal(hits[1], full[0][:257])
            assert info["reads_scanned"] == int(sel.sum()) + 257 and info["search_launches"] == 2
            _check_sliced(times, info, 1, 2)
        # several passes fold with max, under a selection as well
        ctx.set_option("slice_words", 2)
        sel = rng.random(n) < 0.5
        (hits, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [srs], search_selects=[util.bits_from_bools(sel)], max_hits=T))
        passes = ss.plan(n_chunks, k, 2)[1]
        assert passes == 4 and np.array_equal(hits[0], np.where(sel, full[0], 0))
        _check_sliced(times, info, passes, 1)
        ctx.set_option("slice_words", 0)
        # device memory full of ones before the call: the same bytes
        ctx.poison(0xFF)
        (hits, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [srs, rag], max_hits=T))
        assert np.array_equal(hits[0], full[0]) and np.array_equal(hits[1], full[1])
        _check_sliced(times, info, 1, 2)
        # an index selection of all zeros; no search set
        (hits, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [srs], index_select=util.bits_from_bools(np.zeros(len(index), bool)), max_hits=T))
        assert not hits[0].any() and info["n_chunks"] == 0 and info["reads_indexed"] == 0 and info["search_launches"] == 0
        assert not [n for n in times if n.startswith("hits_")], sorted(times)
        (hits, info), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [], max_hits=T))
        assert hits == [] and info["n_chunks"] == n_chunks
        _check_sliced(times, info, 1, 0)
        # the job is what it was
        ctx.set_option("kernel_timing", 0)
        tags, _, _ = ctx.index_and_search(irs, [srs])
        assert tags[0].tobytes() == tags0[0].tobytes() == commet.tags_at(full[0], 2).tobytes()
        with pytest.raises(Exception):
            ctx.set_option("profile_slice", 3)


_EDGE_FULL = {}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_read_counts_at_wave_and_workgroup_edges(n):
    """n reads: the last wave and workgroup are partly empty"""
    index, fixed, _ = ss.edge_cut()
    ref = _EDGE_FULL.get("h")
    if ref is None:
        ref = _EDGE_FULL["h"] = _profile(index, [fixed], ss.EDGE_K, 5, 1, 1)[0][0]
    hits, info, times = _profile(index, [fixed[:n]], ss.EDGE_K, 5, 1, 2)
    _check_sliced(times, info, 1, 1)
    assert np.array_equal(hits[0], ref[:n]) and info["reads_scanned"] == n


# ---- 4. where it does not apply ---------------------------------------------------------------------------------------------------------
def test_outside_the_regime_other_kernels_run():
    index, fixed, _ = ss.edge_cut()
    ref = _profile(index[:120], [fixed[:200]], ss.EDGE_K, 4, 1, 1)[0][0]
    # k = 25 has no bit-sliced tables; auto (0) is never; count_probes keeps the slot kernels
    for k, opt, max_kmer, extra in ((25, 2, 300, {}), (ss.EDGE_K, 0, 1, {}), (ss.EDGE_K, 2, 1, dict(count_probes=1))):
        hits, info, times = _profile(index[:120], [fixed[:200]], k, 4, max_kmer, opt, **extra)
        _check_slots(times)
        assert info["n_chunks"] >= 2
        if k == ss.EDGE_K:
            assert info["n_chunks"] == 60 and np.array_equal(hits[0], ref)
    # the wide rows come first
    hits, info, times = _profile(index[:120], [fixed[:200]], ss.EDGE_K, 4, 1, 2, profile_wide=2)
    assert times["hits_wide_kernel"][0] == 1 and "hits_sliced_kernel" not in times and not [n for n in SLOT_KERNELS if n in times]
    assert np.array_equal(hits[0], ref)


# ---- 5. no room ---------------------------------------------------------------------------------------------------------------------------
def test_narrow_tables_without_room():
    import commet_amd as commet
    k, L, n_chunks, words, gw, passes = ss.ROWS[2]
    index, queries = ss.row_set(k, L, n_chunks)
    size = ss.table_bytes(k, gw)
    with commet.Context(k=k, t=2) as ctx:
        for name, value in (("max_kmer", 1), ("profile_slice", 2)):
            ctx.set_option(name, value)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(queries)])
        with commet.refusing_device_allocs(at_least=size) as r:
            (hits, info), ran = _timed(ctx, lambda: ctx.index_and_profile(irs, [qrs], max_hits=ss.ROW_T))
        print(r.seen, sorted(ran))
        assert r.seen["refused"] > 0 and r.seen["last_refused_bytes"] == size, r.seen
        assert "hits_group_kernel" in ran and "hits_sliced_kernel" not in ran and "slice_build_kernel" not in ran, sorted(ran)
        assert info["n_chunks"] == n_chunks and info["search_launches"] == -(-n_chunks // 8)
        (again, info2), times = _timed(ctx, lambda: ctx.index_and_profile(irs, [qrs], max_hits=ss.ROW_T))   # disarmed: the narrow tables again
        _check_sliced(times, info2, passes, 1)
        assert np.array_equal(hits[0], again[0]) and int((again[0] > 0).sum()) > 60


# ---- 6. randomised ------------------------------------------------------------------------------------------------------------------------
def _load_set(commet, ctx, files, sdir):
    batches = [util.to_batch(util.parse_reads(os.path.join(sdir, fa))) for fa, _, _, _ in files]
    rs = commet.ReadSet.from_files(ctx, batches)
    sel = np.concatenate([s for _, _, _, s in files]) if files else np.zeros(0, bool)
    has_bv = any(bv for _, bv, _, _ in files)
    return rs, (util.bits_from_bools(sel) if has_bv else None)


@pytest.mark.parametrize("seed", ss.RANDOM_SEEDS)
def test_random_scenarios_match_checker(tmp_path, seed):
    import commet_amd as commet
    T = 6
    k, max_kmer = ss.random_case(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    names = sorted(scn.search_names)
    with commet.Context(k=k, t=2) as ctx:
        irs, isel = _load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
        loaded = [_load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
        ctx.set_option("max_kmer", max_kmer)
        ctx.set_option("profile_wide", 1)                     # (auto would take the wide rows from 257 chunks on)
        ctx.set_option("profile_slice", 1)
        slot, info1 = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T)
        ctx.set_option("profile_slice", 2)
        ctx.set_option("kernel_timing", 1)
        hits, info = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T)
        times = ctx.kernel_times()
    assert info["n_chunks"] == info1["n_chunks"]
    passes = ss.plan(info["n_chunks"], k)[1] if info["n_chunks"] else 0
    _check_sliced(times, info, passes, sum(1 for h in hits if h.size))
    for h, s in zip(hits, slot):
        assert np.array_equal(h, s)
    for t in range(1, T + 1):
        scn.t = t
        out_o = str(tmp_path / f"out{t}")
        rc, res, chunks, kmers = run_oracle(scn, out_o, str(tmp_path / f"log{t}"), max_kmer=max_kmer)
        assert rc == 0 and info["n_chunks"] == chunks and info["kmers_indexed"] == kmers
        for nme, h in zip(names, hits):
            pos = 0
            for fa, _, reads, _ in scn.sets[nme]:
                _, n, bits = util.read_bv(os.path.join(out_o, os.path.basename(fa) + "_in_" + scn.index_name + ".bv"))
                assert np.array_equal(h[pos:pos + n] >= t, util.bools_from_bits(bits, n)), (seed, k, t, nme, fa)
                pos += n
            assert pos == h.size


# ---- 7. the sweep command -------------------------------------------------------------------------------------------------------------------
def test_sweep_profile_slice_writes_the_same_vectors(tmp_path):
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f in "ABC":
        open(d / "ABCDE_bench" / (f + ".fa"), "wb").write(gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read())
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("B:ABCDE_bench/B.fa\nC:ABCDE_bench/C.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    passes = {}
    for ps in (1, 2):                                         # k = 20: the index set makes several chunk filters
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", "3", "-o", f"sweep{ps}",
                            "--profile-slice", str(ps)], cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-800:]
        line = r.stdout.decode().strip().split("\n")[-1]
        passes[ps] = (int(line.split(" chunk filter(s)")[0].split()[-1]), int(line.split(" search pass(es)")[0].split()[-1]))
    chunks = passes[1][0]
    assert chunks >= 2 and passes[2][0] == chunks
    assert passes[1][1] == 2 * -(-chunks // 8) and passes[2][1] == 2 * ss.plan(chunks, 20)[1]
    for t in range(1, 4):
        names = sorted(os.listdir(d / "sweep1" / f"t{t}"))
        assert names == ["B.fa_in_A.bv", "C.fa_in_A.bv"] and sorted(os.listdir(d / "sweep2" / f"t{t}")) == names
        for nme in names:
            assert open(d / "sweep1" / f"t{t}" / nme, "rb").read() == open(d / "sweep2" / f"t{t}" / nme, "rb").read(), (t, nme)
    assert open(d / "sweep1" / "sweep.csv", "rb").read() == open(d / "sweep2" / "sweep.csv", "rb").read()
