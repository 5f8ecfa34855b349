"""The hit profile through the wide bit-sliced rows (option profile_wide = 2; hits_wide_kernel, hit_profile_wide.hpp; run_profile_wide,
capi/profile.hpp).  Ground truth is always both (a) the same call at profile_wide = 1, the slot loop, with byte-equal hit arrays, and
(b) the CPU checker once per t (hits >= t equals its bits).  The read sets come from hit_profile_wide_sets.py;
test_hit_profile_wide_cpu.py proves their chunk counts and designed counts without a GPU."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_wide_sets as ws
import oracle_pool
import util
from conftest import ROOT
from hit_profile_group_sets import planted_palindrome
from scenarios import Scenario, run_oracle
from test_hit_profile_groups_cpu import checker_tags

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
SLOT_KERNELS = ("hits_kernel", "hits_wave_kernel", "hits_group_kernel", "hits_group_wave_kernel")


def _profile(index, search_sets, k, max_hits, max_kmer, wide, cap_words=0, index_select=None, search_selects=None):
    """-> (hits, info, {kernel: (launches, ms)})"""
    import commet_amd as commet
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in search_sets]
        for name, value in (("max_kmer", max_kmer), ("profile_wide", wide), ("slice_wide_words", cap_words), ("kernel_timing", 1)):
            ctx.set_option(name, value)
        hits, info = ctx.index_and_profile(irs, srs, index_select, search_selects, max_hits=max_hits)
        return hits, info, ctx.kernel_times()


def _check_wide(times, info, passes, n_sets):
    """the wide path ran, launch for launch, and no slot kernel did"""
    assert times["hits_wide_kernel"][0] == passes * n_sets == info["search_launches"], (times.get("hits_wide_kernel"), passes, n_sets, info["search_launches"])
    assert not [n for n in SLOT_KERNELS if n in times], sorted(times)
    assert "interleave_a_kernel" not in times and times["slice_build_kernel"][0] == times["slice_transpose_kernel"][0]


def _check_slots(times):
    assert "hits_wide_kernel" not in times and [n for n in SLOT_KERNELS if n in times], sorted(times)


def _both(index, search_sets, k, max_hits, max_kmer, cap_words, passes=None):
    """the call at profile_wide = 2 and at 1 -> (hits, info, passes): byte-equal arrays, equal plans"""
    hits, info, times = _profile(index, search_sets, k, max_hits, max_kmer, 2, cap_words)
    slot, info1, times1 = _profile(index, search_sets, k, max_hits, max_kmer, 1, cap_words)
    if passes is None:
        passes = ws.passes_of(info["n_chunks"], cap_words)[0]
    _check_wide(times, info, passes, sum(1 for s in search_sets if len(s)))
    _check_slots(times1)
    for f in ("n_chunks", "kmers_indexed", "reads_indexed"):
        assert info[f] == info1[f], f
    assert info["probes"] == 0
    for q, (h, s) in enumerate(zip(hits, slot)):
        assert h.dtype == np.uint8 and np.array_equal(h, s), (q, np.nonzero(h != s)[0][:10], h[h != s][:10], s[h != s][:10])
    # a pass walks a visited read of at least k bases unless it stands at its cap already: every such read in the first pass
    walkable = sum(sum(1 for r in s if len(r) >= k) for s in search_sets)
    assert walkable <= info["reads_scanned"] <= passes * walkable, (walkable, info["reads_scanned"], passes)
    return hits, info, passes


# ---- 1. every instantiation, one pass and several ---------------------------------------------------------------------------------
_TRUTH = {}


def _row_truth(k, L, n_chunks, t_max=4):
    """the checker's bits per t for row_set(k, L, n_chunks), computed once"""
    import oracle_binding as ob
    key = (k, L, n_chunks)
    if key not in _TRUTH:
        index, queries = ws.row_set(k, L, n_chunks)
        ib, io = util.to_batch(index)
        qb, qo = util.to_batch(queries)
        chunks = oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, k), 1)
        _TRUTH[key] = (len(chunks), [util.bools_from_bits(oracle_pool.chunk_loop_in_threads(k, t, ib, io, qb, qo, chunks, len(queries))[0], len(queries))
                                     for t in range(1, t_max + 1)])
    return _TRUTH[key]


@pytest.mark.parametrize("k,L,n_chunks,cap_words,inst", ws.ROWS)
def test_every_instantiation_matches_the_slot_loop_and_the_checker(k, L, n_chunks, cap_words, inst):
    index, queries = ws.row_set(k, L, n_chunks)
    hits, info, passes = _both(index, [queries], k, ws.ROW_T, 1, cap_words)
    assert abs(info["n_chunks"] - n_chunks) <= n_chunks // 50
    assert ws.passes_of(info["n_chunks"], cap_words)[2] == inst and passes == ws.passes_of(n_chunks, cap_words)[0]
    h = hits[0]
    print(k, L, info["n_chunks"], passes, np.bincount(h, minlength=ws.ROW_T + 1).tolist(), info["reads_scanned"])
    assert int(h.max()) <= min(ws.ROW_T, L // k) and int((h > 0).sum()) > 60
    if k == 21:
        assert set(range(5)) <= set(h.tolist())
    if n_chunks <= ws.CHECKER_MAX_CHUNKS:
        chunks, per_t = _row_truth(k, L, n_chunks)
        assert chunks == info["n_chunks"]
        for t, tags in enumerate(per_t, start=1):
            assert np.array_equal(h >= t, tags), (k, t, np.nonzero((h >= t) != tags)[0][:10])


def test_last_pass_with_fewer_groups_than_the_rows_hold():
    """five groups of 256 chunks under rows capped at three groups: the second pass fills two of the three, and the columns of the
    third still hold the first pass's chunks — the kernel must not look at them"""
    k, L, n_chunks, _, _ = ws.ROWS[1]
    index, queries = ws.row_set(k, L, n_chunks)
    hits, info, passes = _both(index[:2 * 1100], [queries], k, ws.ROW_T, 1, 24)
    assert 1024 < info["n_chunks"] <= 1280 and passes == 2 and ws.passes_of(info["n_chunks"], 24)[1] == 24
    assert int((hits[0] > 0).sum()) > 60


# ---- 2. planted reads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap_words", [0, 8])
@pytest.mark.parametrize("k", ws.PLANTED_KS)
def test_planted_reads(tmp_path, k, cap_words):
    T = 4
    index, search, exp, names = ws.planted(k)
    hits, info, passes = _both(index, [search], k, T, 1, cap_words)
    assert info["n_chunks"] == ws.PLANTED_CHUNKS and passes == (3 if cap_words else 1)
    got = hits[0].tolist()
    print(k, cap_words, list(zip(names, got, exp)))
    assert got == [min(T, e) for e in exp], [(n, g, e) for n, g, e in zip(names, got, exp) if g != min(T, e)]   # (the checker confirms exp: test_hit_profile_wide_cpu.py)
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=1)
        assert chunks == ws.PLANTED_CHUNKS and np.array_equal(hits[0] >= t, tags[0]), t


@pytest.mark.parametrize("k", ws.PLANTED_KS)
def test_saturation_of_counter_and_cap(tmp_path, k):
    index, search, exact = ws.saturation(k)
    for max_hits in (3, exact, exact + 1, 255):
        hits, info, _ = _both(index, [search], k, max_hits, 1, 0)
        assert info["n_chunks"] == 12
        h = hits[0]
        assert int(h[0]) == int(h[1]) == min(max_hits, exact) and int(h[2]) == min(max_hits, 100 // k) and int(h[3]) == 0, (max_hits, h.tolist())
    for t in (1, exact, exact + 1):
        tags, _ = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=1)
        assert np.array_equal(hits[0] >= t, tags[0]), t


def test_palindromic_kmer(tmp_path):
    """a k-mer that is its own reverse complement has its own partner in plane A: the `selfp` rows of the row pass"""
    k = 20
    index, search, exp, max_kmer, n_chunks = planted_palindrome(k)
    T = max(exp) + 1
    hits, info, _ = _both(index, [search], k, T, max_kmer, 0)
    assert info["n_chunks"] == n_chunks and hits[0].tolist() == exp
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
        assert chunks == n_chunks and np.array_equal(hits[0] >= t, tags[0]), t


# ---- 3. selections and edges -----------------------------------------------------------------------------------------------------------
def test_selections_sets_and_edges(tmp_path):
    import commet_amd as commet
    k, T = ws.EDGE_K, 5
    index, fixed, ragged = ws.edge_set()
    n = len(fixed)
    rng = np.random.default_rng(8)
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("max_kmer", 1)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(fixed)])
        prefix = commet.ReadSet.from_files(ctx, [util.to_batch(fixed[:257])])
        rag = commet.ReadSet.from_files(ctx, [util.to_batch(ragged)])
        tags0, _, jinfo = ctx.index_and_search(irs, [srs])
        ctx.set_option("profile_wide", 1)
        slot, info1 = ctx.index_and_profile(irs, [srs, rag], max_hits=T)
        ctx.set_option("profile_wide", 2)
        ctx.set_option("kernel_timing", 1)
        full, info = ctx.index_and_profile(irs, [srs, rag], max_hits=T)
        _check_wide(ctx.kernel_times(), info, 1, 2)
        n_chunks = info["n_chunks"]
        assert n_chunks == info1["n_chunks"] == jinfo["n_chunks"] and abs(n_chunks - ws.EDGE_CHUNKS) <= 8
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
            hits, info = ctx.index_and_profile(irs, [srs, prefix], search_selects=[util.bits_from_bools(sel), None], max_hits=T)
            assert np.array_equal(hits[0], np.where(sel, full[0], 0)), frac
            assert np.array_equal(hits[1], full[0][:257])
            assert info["reads_scanned"] == int(sel.sum()) + 257 and info["search_launches"] == 2
        # several passes fold with max, under a selection as well
        ctx.set_option("slice_wide_words", 8)
        sel = rng.random(n) < 0.5
        hits, info = ctx.index_and_profile(irs, [srs], search_selects=[util.bits_from_bools(sel)], max_hits=T)
        assert info["search_launches"] == ws.passes_of(n_chunks, 8)[0] == 2 and np.array_equal(hits[0], np.where(sel, full[0], 0))
        ctx.set_option("slice_wide_words", 0)
        # an index selection of all zeros; no search set
        hits, info = ctx.index_and_profile(irs, [srs], index_select=util.bits_from_bools(np.zeros(len(index), bool)), max_hits=T)
        assert not hits[0].any() and info["n_chunks"] == 0 and info["reads_indexed"] == 0 and info["search_launches"] == 0
        hits, info = ctx.index_and_profile(irs, [], max_hits=T)
        assert hits == [] and info["n_chunks"] == n_chunks and info["search_launches"] == 0
        # the job is what it was
        ctx.set_option("kernel_timing", 0)
        tags, _, _ = ctx.index_and_search(irs, [srs])
        assert tags[0].tobytes() == tags0[0].tobytes() == commet.tags_at(full[0], 2).tobytes()
        with pytest.raises(Exception):
            ctx.set_option("profile_wide", 3)


_EDGE_FULL = {}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_read_counts_at_wave_and_workgroup_edges(n):
    """n reads: the last group of lanes, wave and workgroup are partly empty"""
    index, fixed, _ = ws.edge_set()
    ref = _EDGE_FULL.get("h")
    if ref is None:
        ref = _EDGE_FULL["h"] = _profile(index, [fixed], ws.EDGE_K, 5, 1, 1)[0][0]
    hits, info, times = _profile(index, [fixed[:n]], ws.EDGE_K, 5, 1, 2)
    _check_wide(times, info, 1, 1)
    assert np.array_equal(hits[0], ref[:n]) and info["reads_scanned"] == n


def test_auto_takes_the_measured_shape_only():
    """auto (0): more than 256 chunk filters and no search read of more than 300 bases; with a longer read in any set the slot loop"""
    index, fixed, ragged = ws.edge_set()
    ref = _profile(index, [fixed[:300], ragged[:100]], ws.EDGE_K, 5, 1, 1)[0]
    hits, info, times = _profile(index, [fixed[:300], ragged[:100]], ws.EDGE_K, 5, 1, 0)
    assert info["n_chunks"] > 256
    _check_wide(times, info, 1, 2)
    long_read = (fixed[0] * 6)[:301]
    hits2, info2, times2 = _profile(index, [fixed[:300], ragged[:100] + [long_read]], ws.EDGE_K, 5, 1, 0)
    _check_slots(times2)
    for q in range(2):
        assert np.array_equal(hits[q], ref[q]) and np.array_equal(hits2[q][:len(ref[q])], ref[q])


def test_outside_the_regime_the_slot_loop_runs():
    """k = 25 has no bit-sliced rows, and auto (0) leaves jobs of at most 256 chunk filters alone: both take the kernels of today"""
    index, fixed, _ = ws.edge_set()
    for k, wide, max_kmer in ((25, 2, 300), (ws.EDGE_K, 0, 1)):
        hits, info, times = _profile(index[:120], [fixed[:200]], k, 4, max_kmer, wide)
        _check_slots(times)
        assert info["n_chunks"] >= 2


# ---- 4. randomised -----------------------------------------------------------------------------------------------------------------------
def _load_set(commet, ctx, files, sdir):
    batches = [util.to_batch(util.parse_reads(os.path.join(sdir, fa))) for fa, _, _, _ in files]
    rs = commet.ReadSet.from_files(ctx, batches)
    sel = np.concatenate([s for _, _, _, s in files]) if files else np.zeros(0, bool)
    has_bv = any(bv for _, bv, _, _ in files)
    return rs, (util.bits_from_bools(sel) if has_bv else None)


@pytest.mark.parametrize("seed", ws.RANDOM_SEEDS)
def test_random_scenarios_match_checker(tmp_path, seed):
    import commet_amd as commet
    T = 6
    k, max_kmer = ws.random_case(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    names = sorted(scn.search_names)
    with commet.Context(k=k, t=2) as ctx:
        irs, isel = _load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
        loaded = [_load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
        ctx.set_option("max_kmer", max_kmer)
        ctx.set_option("profile_wide", 1)
        slot, info1 = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T)
        ctx.set_option("profile_wide", 2)
        ctx.set_option("kernel_timing", 1)
        hits, info = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T)
        times = ctx.kernel_times()
    assert info["n_chunks"] == info1["n_chunks"]
    if info["n_chunks"]:
        _check_wide(times, info, ws.passes_of(info["n_chunks"], 0)[0], sum(1 for h in hits if h.size))
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


# ---- 5. the sweep command ------------------------------------------------------------------------------------------------------------------
def test_sweep_profile_wide_writes_the_same_vectors(tmp_path):
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f in "ABC":
        open(d / "ABCDE_bench" / (f + ".fa"), "wb").write(gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read())
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("B:ABCDE_bench/B.fa\nC:ABCDE_bench/C.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    passes = {}
    for pw in (1, 2):                                         # k = 20: the index set makes several chunk filters
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", "3", "-o", f"sweep{pw}",
                            "--profile-wide", str(pw)], cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-800:]
        line = r.stdout.decode().strip().split("\n")[-1]
        passes[pw] = (int(line.split(" chunk filter(s)")[0].split()[-1]), int(line.split(" search pass(es)")[0].split()[-1]))
    chunks = passes[1][0]
    assert chunks >= 2 and passes[2][0] == chunks
    assert passes[1][1] == 2 * -(-chunks // 8) and passes[2][1] == 2 * ws.passes_of(chunks, 0)[0]
    for t in range(1, 4):
        names = sorted(os.listdir(d / "sweep1" / f"t{t}"))
        assert names == ["B.fa_in_A.bv", "C.fa_in_A.bv"] and sorted(os.listdir(d / "sweep2" / f"t{t}")) == names
        for nme in names:
            assert open(d / "sweep1" / f"t{t}" / nme, "rb").read() == open(d / "sweep2" / f"t{t}" / nme, "rb").read(), (t, nme)
    assert open(d / "sweep1" / "sweep.csv", "rb").read() == open(d / "sweep2" / "sweep.csv", "rb").read()
    rows = [ln.split(";") for ln in open(d / "sweep1" / "sweep.csv").read().strip().split("\n")][1:]
    assert len({int(r[4]) for r in rows}) > 2
