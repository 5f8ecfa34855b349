"""The grouped hits passes of commet_index_and_profile (capi/profile.hpp; hits_group_kernel and hits_group_wave_kernel,
hit_profile_group.hpp): up to eight chunk filters per pass over a search set.  Ground truth is always (a) the CPU checker once per t
(hits >= t equals its .bv bits) and (b) the same call at chunk_group = 1, one filter per pass, with byte-equal hit arrays.  The read
sets come from hit_profile_group_sets.py; test_hit_profile_groups_cpu.py proves their chunk counts and planted counts without a GPU."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_group_sets as gs
import util
from conftest import ROOT
from scenarios import Scenario, run_oracle
from test_hit_profile_groups_cpu import checker_tags

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
GROUP_KERNEL = {1: "hits_group_kernel", 2: "hits_group_wave_kernel"}     # by option long_search
ONE_KERNEL = {1: "hits_kernel", 2: "hits_wave_kernel"}


def _profile(index, search_sets, k, max_hits, max_kmer, chunk_group, long_search, opts=()):
    """-> (hits, info, kernel names)"""
    import commet_amd as commet
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in search_sets]
        for name, value in (("max_kmer", max_kmer), ("chunk_group", chunk_group), ("long_search", long_search), ("kernel_timing", 1)) + tuple(opts):
            ctx.set_option(name, value)
        hits, info = ctx.index_and_profile(irs, srs, max_hits=max_hits)
        return hits, info, set(ctx.kernel_times())


def _check_kernels(names, long_search, n_chunks, chunk_group):
    passes, grouped, single = gs.groups_of(n_chunks, chunk_group)
    assert (GROUP_KERNEL[long_search] in names) == grouped and (ONE_KERNEL[long_search] in names) == single, (names, n_chunks, chunk_group)
    assert GROUP_KERNEL[3 - long_search] not in names and ONE_KERNEL[3 - long_search] not in names, names
    assert ("interleave_a_kernel" in names) == grouped
    return passes


# ---- 1. groups of every size and remainder -------------------------------------------------------------------------------------
_CHECKER = {}


def _group_truth(tmp_path, k, n_chunks, t_max):
    """the checker's tags per t for group_set(k, n_chunks), computed once"""
    if (k, n_chunks) not in _CHECKER:
        index, search, max_kmer = gs.group_set(k, n_chunks)
        per_t = []
        for t in range(1, t_max + 1):
            tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
            assert chunks == n_chunks
            per_t.append(tags[0])
        _CHECKER[(k, n_chunks)] = per_t
    return _CHECKER[(k, n_chunks)]


def _group_case(tmp_path, k, long_search, n_chunks, chunk_group):
    T = 5
    index, search, max_kmer = gs.group_set(k, n_chunks)
    hits, info, names = _profile(index, [search, search[:70]], k, T, max_kmer, chunk_group, long_search)
    one, info1, names1 = _profile(index, [search, search[:70]], k, T, max_kmer, 1, long_search)
    assert info["n_chunks"] == info1["n_chunks"] == n_chunks and info["probes"] == 0
    passes = _check_kernels(names, long_search, n_chunks, chunk_group)
    assert _check_kernels(names1, long_search, n_chunks, 1) == n_chunks
    assert info["search_launches"] == passes * 2 and info1["search_launches"] == n_chunks * 2
    assert info["kmers_indexed"] == info1["kmers_indexed"] and info["reads_indexed"] == info1["reads_indexed"]
    assert len(search) + 70 <= info["reads_scanned"] <= info1["reads_scanned"]
    for q in range(2):
        assert np.array_equal(hits[q], one[q]), (k, long_search, n_chunks, chunk_group, q)
    assert np.array_equal(hits[1], hits[0][:70])
    assert {0, 1, 2, 3} <= set(hits[0].tolist())
    for t, tags in enumerate(_group_truth(tmp_path, k, n_chunks, T), start=1):
        assert np.array_equal(hits[0] >= t, tags), (k, long_search, n_chunks, chunk_group, t)


@pytest.mark.parametrize("n_chunks,chunk_group", gs.GROUP_CASES)
@pytest.mark.parametrize("long_search", [1, 2])
@pytest.mark.parametrize("k", gs.GROUP_KS)
def test_groups_of_every_size_and_remainder(tmp_path, k, long_search, n_chunks, chunk_group):
    _group_case(tmp_path, k, long_search, n_chunks, chunk_group)


@pytest.mark.parametrize("n_chunks", gs.WIDE_CHUNKS)
@pytest.mark.parametrize("long_search", [1, 2])
def test_groups_with_wide_keys(tmp_path, long_search, n_chunks):
    """k = 33: the 64-bit instantiations, NF = 2, 4, 8 (eight slots of 4 GiB and their interleaved planes)"""
    _group_case(tmp_path, gs.WIDE_K, long_search, n_chunks, 8)


# ---- 2. state is per filter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["states", "slots", "palindrome"])
@pytest.mark.parametrize("long_search", [1, 2])
def test_state_is_per_filter(tmp_path, long_search, case):
    k = 20 if case == "palindrome" else 25
    index, search, exp, max_kmer, n_chunks = {"states": gs.planted_states, "slots": gs.planted_slots, "palindrome": gs.planted_palindrome}[case](k)
    T = max(exp) + 1
    hits, info, names = _profile(index, [search], k, T, max_kmer, 8, long_search)
    one, info1, _ = _profile(index, [search], k, T, max_kmer, 1, long_search)
    assert info["n_chunks"] == info1["n_chunks"] == n_chunks
    assert info["search_launches"] == _check_kernels(names, long_search, n_chunks, 8)
    print(case, long_search, hits[0].tolist(), one[0].tolist(), exp)
    assert np.array_equal(hits[0], one[0])
    for t in range(1, T + 1):
        tags, chunks = checker_tags(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
        assert chunks == n_chunks and np.array_equal(hits[0] >= t, tags[0]), t
    assert hits[0].tolist() == exp                            # (the checker confirms these: test_hit_profile_groups_cpu.py)


# ---- 3. the wave form at block edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 32, 33])                   # (33: the loader's three-word path, 64-bit keys)
def test_wave_form_at_block_edges(tmp_path, k):
    index, ragged, exp_r, fixed, exp_f, max_kmer = gs.wave_sets(k)
    got = {}
    for long_search, chunk_group in ((2, 8), (1, 8), (2, 1)):
        got[(long_search, chunk_group)], info, names = _profile(index, [ragged, fixed], k, 4, max_kmer, chunk_group, long_search)
        assert info["n_chunks"] == 3
        assert info["search_launches"] == 2 * _check_kernels(names, long_search, 3, chunk_group)
    wave = got[(2, 8)]
    for other in ((1, 8), (2, 1)):
        for q in range(2):
            assert np.array_equal(wave[q], got[other][q]), (other, q)
    for h, exp in ((wave[0], exp_r), (wave[1], exp_f)):
        for i, e in enumerate(exp):
            if e is not None:
                assert int(h[i]) == min(4, e), (i, e, int(h[i]))
    assert {1, 2, 3, 4} <= set(wave[0].tolist())              # (the N-run reads saturate)
    for t in range(1, 5):
        tags, _ = checker_tags(tmp_path / "orc", k, t, index, [ragged, fixed], max_kmer=max_kmer)
        for q in range(2):
            assert np.array_equal(wave[q] >= t, tags[q]), (t, q)


# ---- 4. saturation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_search", [1, 2])
def test_saturation_over_groups(long_search):
    index, search, exact, max_kmer = gs.saturation_set()
    for max_hits in (1, exact, exact + 1, 255):
        hits, info, names = _profile(index, [search], 8, max_hits, max_kmer, 8, long_search)
        one, info1, _ = _profile(index, [search], 8, max_hits, max_kmer, 1, long_search)
        assert info["n_chunks"] == info1["n_chunks"] >= 9
        assert GROUP_KERNEL[long_search] in names
        assert np.array_equal(hits[0], one[0]), max_hits
        assert int(hits[0][0]) == int(hits[0][2]) == min(max_hits, exact) and int(hits[0].max()) <= max_hits
        assert len(search) <= info["reads_scanned"] <= info1["reads_scanned"], (max_hits, info["reads_scanned"], info1["reads_scanned"])


# ---- 5. selections, lists, several sets, empties --------------------------------------------------------------------------------------
_SYNTH = {}


def _synth_pair(n, n_index):
    from commet_amd import synth
    if (n, n_index) not in _SYNTH:
        _SYNTH[(n, n_index)] = (synth.synth_set(0, n_index, 100), synth.synth_set(1, n, 100))
    return _SYNTH[(n, n_index)]


def test_selections_lists_sets_and_empty_calls():
    import commet_amd as commet
    n = 5000
    (ib, io), (sb, so) = _synth_pair(n, n)
    rng = np.random.default_rng(3)
    with commet.Context(k=32, t=2) as ctx:
        ctx.set_option("max_kmer", 90000)                     # 345 000 k-mers: four chunks
        irs = commet.ReadSet.from_files(ctx, [(ib, io)])
        srs = commet.ReadSet.from_files(ctx, [(sb, so)])
        srs2 = commet.ReadSet.from_files(ctx, [(sb[:257 * 100], so[:258])])
        tags0, _, jinfo = ctx.index_and_search(irs, [srs])
        ctx.set_option("chunk_group", 1)
        one, info1 = ctx.index_and_profile(irs, [srs], max_hits=5)
        ctx.set_option("chunk_group", 8)
        ctx.set_option("kernel_timing", 1)
        full, info = ctx.index_and_profile(irs, [srs], max_hits=5)
        assert "hits_group_kernel" in ctx.kernel_times()
        assert info["n_chunks"] == info1["n_chunks"] == jinfo["n_chunks"] >= 3 and info["search_launches"] == 1
        assert np.array_equal(full[0], one[0]) and int((full[0] > 0).sum()) > n // 10
        for frac, sparse in ((0.7, 0), (0.2, 0), (0.2, 1), (0.02, 2)):      # (less than half of the set: the pass walks a list)
            sel = rng.random(n) < frac
            ctx.set_option("sparse_search", sparse)
            hits, info = ctx.index_and_profile(irs, [srs, srs2], search_selects=[util.bits_from_bools(sel), None], max_hits=5)
            assert np.array_equal(hits[0], np.where(sel, full[0], 0)), (frac, sparse)
            assert np.array_equal(hits[1], full[0][:257])
            assert info["reads_scanned"] == int(sel.sum()) + 257 and info["search_launches"] == 2
        ctx.set_option("sparse_search", 0)
        # an all-zero selection of the search set, of the index set; no search set at all
        hits, info = ctx.index_and_profile(irs, [srs], search_selects=[util.bits_from_bools(np.zeros(n, bool))], max_hits=5)
        assert not hits[0].any() and info["reads_scanned"] == 0
        hits, info = ctx.index_and_profile(irs, [srs], index_select=util.bits_from_bools(np.zeros(n, bool)), max_hits=5)
        assert not hits[0].any() and info["n_chunks"] == 0 and info["reads_indexed"] == 0
        hits, info = ctx.index_and_profile(irs, [], max_hits=5)
        assert hits == [] and info["n_chunks"] >= 3 and info["search_launches"] == 0
        # the job is what it was: the slots and the current slot are left sane
        tags, stats, _ = ctx.index_and_search(irs, [srs])
        assert tags[0].tobytes() == tags0[0].tobytes() == commet.tags_at(full[0], 2).tobytes()


# ---- 6. workgroup and word edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_tags_equal_the_search_kernels_over_chunks(n):
    import commet_amd as commet
    (ib, io), (sb, so) = _synth_pair(n, 300)
    for t in (1, 2, 3):
        with commet.Context(k=25, t=t) as ctx:
            ctx.set_option("max_kmer", 8000)                  # 300 reads of 76 k-mers: three chunks
            ctx.set_option("kernel_timing", 1)
            irs = commet.ReadSet.from_files(ctx, [(ib, io)])
            srs = commet.ReadSet.from_files(ctx, [(sb, so)])
            hits, info = ctx.index_and_profile(irs, [srs], max_hits=t)
            assert "hits_group_kernel" in ctx.kernel_times()
            tags, stats, jinfo = ctx.index_and_search(irs, [srs])
            assert commet.tags_at(hits[0], t).tobytes() == tags[0].tobytes(), (n, t)
            assert int(hits[0].max()) <= t
            assert info["n_chunks"] == jinfo["n_chunks"] >= 2 and info["search_launches"] == 1 and info["reads_scanned"] == n


# ---- 7. randomised --------------------------------------------------------------------------------------------------------------------
def _load_set(commet, ctx, files, sdir):
    batches = [util.to_batch(util.parse_reads(os.path.join(sdir, fa))) for fa, _, _, _ in files]
    rs = commet.ReadSet.from_files(ctx, batches)
    sel = np.concatenate([s for _, _, _, s in files]) if files else np.zeros(0, bool)
    has_bv = any(bv for _, bv, _, _ in files)
    return rs, (util.bits_from_bools(sel) if has_bv else None)


@pytest.mark.parametrize("seed", gs.RANDOM_SEEDS)
def test_random_scenarios_match_checker(tmp_path, seed):
    import commet_amd as commet
    T = 6
    k, max_kmer, chunk_group = gs.random_case(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    names = sorted(scn.search_names)
    with commet.Context(k=k, t=2) as ctx:
        irs, isel = _load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
        loaded = [_load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
        ctx.set_option("max_kmer", max_kmer)
        ctx.set_option("chunk_group", chunk_group)
        ctx.set_option("long_search", 1 + seed % 2)
        hits, info = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T)
    assert info["n_chunks"] >= 2
    assert info["search_launches"] == gs.groups_of(info["n_chunks"], chunk_group)[0] * sum(1 for h in hits if h.size)
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


# ---- 8. a job and a profile build the same groups --------------------------------------------------------------------------------------
def test_job_and_profile_build_the_same_groups():
    """both go through run_slot_groups and run_wide_passes (capi/job.hpp): on one context the job and the profile build the same
    groups of chunk filters — equal build and interleave launches — and scan every non-empty set once per group or pass"""
    import commet_amd as commet
    import hit_profile_wide_sets as ws

    def both(ctx, irs, srs):
        ctx.set_option("kernel_timing", 1)                    # (the totals start again)
        _, _, jinfo = ctx.index_and_search(irs, srs)
        jtimes = ctx.kernel_times()
        ctx.set_option("kernel_timing", 1)
        _, pinfo = ctx.index_and_profile(irs, srs, max_hits=4)
        return jinfo, jtimes, pinfo, ctx.kernel_times()

    # the slot loop: 11 chunks in groups of 1 | 2 + a single chunk | 4, 4, 3 | 8, 3; the second search set is empty
    k, n_chunks = 25, 11
    index, search, max_kmer = gs.group_set(k, n_chunks)
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in (search, [], search[:70])]
        for name, value in (("max_kmer", max_kmer), ("tiled_search", 1), ("slice_mode", 1), ("long_search", 1)):
            ctx.set_option(name, value)
        for chunk_group in (1, 2, 4, 8):
            ctx.set_option("chunk_group", chunk_group)
            jinfo, jtimes, pinfo, ptimes = both(ctx, irs, srs)
            groups = gs.groups_of(n_chunks, chunk_group)[0]
            grouped = n_chunks // chunk_group + (n_chunks % chunk_group >= 2) if chunk_group > 1 else 0   # groups of two chunks or more
            print(chunk_group, jinfo["index_launches"], jinfo["search_launches"], jtimes.get("interleave_a_kernel"), ptimes.get("interleave_a_kernel"))
            assert jinfo["n_chunks"] == pinfo["n_chunks"] == n_chunks
            assert jinfo["index_launches"] == pinfo["index_launches"] == n_chunks
            assert jtimes.get("interleave_a_kernel", (0, 0))[0] == ptimes.get("interleave_a_kernel", (0, 0))[0] == grouped
            assert jinfo["search_launches"] == pinfo["search_launches"] == groups * 2, chunk_group

    # the wide rows: 300 chunks, rows capped at one group of 256: two passes
    k, L, n_chunks, _, _ = ws.ROWS[0]
    index, queries = ws.row_set(k, L, n_chunks)
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in (queries, queries[:70])]
        for name, value in (("max_kmer", 1), ("slice_wide", 2), ("profile_wide", 2), ("slice_wide_words", 8)):
            ctx.set_option(name, value)
        jinfo, jtimes, pinfo, ptimes = both(ctx, irs, srs)
        passes = ws.passes_of(jinfo["n_chunks"], 8)[0]
        print(jinfo["n_chunks"], passes, jtimes["slice_build_kernel"][0], ptimes["slice_build_kernel"][0])
        assert passes == 2 and jinfo["n_chunks"] == pinfo["n_chunks"]
        assert "search_wide_kernel" in jtimes and "hits_wide_kernel" in ptimes
        for name in ("slice_build_kernel", "slice_transpose_kernel"):
            assert jtimes[name][0] == ptimes[name][0] == passes, name
        assert jinfo["index_launches"] == pinfo["index_launches"] == 2 * passes
        assert jinfo["search_launches"] == pinfo["search_launches"] == passes * 2


# ---- 9. the sweep command ---------------------------------------------------------------------------------------------------------------
def test_sweep_chunk_group_writes_the_same_vectors(tmp_path):
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f in "ABC":
        open(d / "ABCDE_bench" / (f + ".fa"), "wb").write(gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read())
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("B:ABCDE_bench/B.fa\nC:ABCDE_bench/C.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    passes = {}
    for cg in (1, 8):                                         # k = 20: the index set makes several chunk filters
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "20", "--max-t", "3", "-o", f"sweep{cg}",
                            "--chunk-group", str(cg)], cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-800:]
        line = r.stdout.decode().strip().split("\n")[-1]
        passes[cg] = (int(line.split(" chunk filter(s)")[0].split()[-1]), int(line.split(" search pass(es)")[0].split()[-1]))
    chunks = passes[1][0]
    assert chunks >= 2 and passes[8][0] == chunks
    assert passes[1][1] == 2 * chunks and passes[8][1] == 2 * gs.groups_of(chunks, 8)[0]
    shared = []
    for t in range(1, 4):
        names = sorted(os.listdir(d / "sweep1" / f"t{t}"))
        assert names == ["B.fa_in_A.bv", "C.fa_in_A.bv"] and sorted(os.listdir(d / "sweep8" / f"t{t}")) == names
        for nme in names:
            assert open(d / "sweep1" / f"t{t}" / nme, "rb").read() == open(d / "sweep8" / f"t{t}" / nme, "rb").read(), (t, nme)
    assert open(d / "sweep1" / "sweep.csv", "rb").read() == open(d / "sweep8" / "sweep.csv", "rb").read()
    rows = [ln.split(";") for ln in open(d / "sweep1" / "sweep.csv").read().strip().split("\n")][1:]
    shared = [int(r[4]) for r in rows]
    assert len(set(shared)) > 2 and shared[0] > 0             # (the thresholds tell the reads apart)
