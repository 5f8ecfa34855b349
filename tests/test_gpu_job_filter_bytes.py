"""The chunk filters that JOBS build, byte for byte against the CPU checker (job_filters.py).

A job zeroes no filter slot in front of the bucketed build (`launch_index(fresh_filter = true, filter_zeroed = false)`: part_scan_kernel gives
every empty bucket a work item, part_zero_split_kernel clears the tiles several workgroups OR into, part_build_kernel stores its tile
over what was there), builds into slots 1 .. 7 as well, on two lanes for groups of two, and through the item paths of a selection.
A tag sees a stale bit only when a read happens to probe it; a fresh context's slots are zeroed memory anyway.  So every case here

1. runs the job with kernel_timing = 1 and asserts from kernel_times() that part_build_kernel ran once per chunk, that no filter_memset
   ran, that part_zero_split_kernel ran and which search kernels ran how often (a fall-back to smaller groups fails the case);
2. fills every bit array of the context with 0xFF (option "poison"; the slots stay allocated) and runs the same job with
   kernel_timing = 0 — the condition of the two index lanes (build_group: g == 2, index_lanes > 1, kernel_timing off);
3. compares tags, log numbers, chunk and k-mer counts with the checker's run, and EVERY slot's export with the checker's filter of the
   chunk that run_slots built into it last (job_filters.slot_chunks) — exact, no tolerance;
4. does 2 and 3 again with 0xA5.

The index sets hold, per chunk, buckets of all three kinds (job_filters.tile_census; asserted, and checked without a GPU in
test_job_filters_cpu.py): empty, of one build workgroup, and split over several (more than 2^17 equal keys: copies of A x 150)."""
import time

import numpy as np
import pytest

import job_filters as jf
import planted_sets as ps
import test_gpu_planted_search as tps
import util

pytestmark = pytest.mark.gpu

ALL = ("empty", "single", "split")
T = 2
BASE = dict(tps.DEFAULTS, index_mode=2, part_packed=1, index_lanes=2, multi_job=0)
INDEX_NOISE = ("filter_memset", "index_kernel")


# ---- sets ------------------------------------------------------------------------------------------------------------------------------
def search_reads(seed, index, n=150, L=100):
    """reads of one length (group8_ok): pieces of index reads, and random ones"""
    rng = np.random.default_rng(seed)
    long_enough = [r for r in index if len(r) >= L and b"N" not in r]
    out = []
    for i in range(n):
        if i % 2 == 0 and long_enough:
            r = long_enough[int(rng.integers(len(long_enough)))]
            a = int(rng.integers(0, len(r) - L + 1))
            out.append(r[a:a + L])
        else:
            out.append(util.random_reads(rng, 1, L, L, n_rate=0.0, lower_rate=0.0, other_rate=0.0)[0])
    return out


_SETS = {}


def tile_case_set(k, n_random):
    """-> (index reads, max_kmer, the one chunk's trace row as the planner will cut it)"""
    key = ("tile", k, n_random)
    if key not in _SETS:
        reads = jf.three_class_reads(1000 + k, k, n_random)
        mk, _ = jf.max_kmer_for(k, reads, 1)
        _SETS[key] = (reads, mk, (0, len(reads) - 1, len(reads), mk - 1))
    return _SETS[key]


def chunked_set(k, n_chunks, n_random):
    key = ("chunked", k, n_chunks, n_random)
    if key not in _SETS:
        reads = jf.three_class_reads(2000 + 10 * k + n_chunks, k, n_random, n_chunks)
        _SETS[key] = (reads, jf.max_kmer_for(k, reads, n_chunks)[0])
    return _SETS[key]


# ---- the common shape of a case ----------------------------------------------------------------------------------------------------------
def expected_search_launches(n_chunks, group):
    """one search set: a launch per group, of the kernel that takes groups of that size"""
    out = {}
    for c0 in range(0, n_chunks, group):
        g = min(group, n_chunks - c0)
        name = "search_kernel" if g == 1 else "search_group_kernel" if g <= 4 else "search_group8_kernel"
        out[name] = out.get(name, 0) + 1
    return out


def check_build_kernels(times, n_chunks, what):
    ran = {n: times[n][0] for n in times}
    print(what, ran)
    assert ran.get("part_build_kernel") == n_chunks, (what, ran)
    assert not [n for n in INDEX_NOISE if n in ran], (what, ran)
    assert ran.get("part_zero_split_kernel") == n_chunks, (what, ran)


def check_slots(ctx, what, want_by_slot):
    """every slot that holds a chunk filter against the checker's bytes of it"""
    for slot, want in enumerate(want_by_slot):
        if want is None:
            continue
        diff = jf.first_difference(ctx.export_filter_reference(slot), want)
        assert diff is None, f"{what}, slot {slot}: {diff}"


def check_job(what, got, truth, set_sizes):
    tags, stats, info = got
    assert info["n_chunks"] == truth["chunks"] and info["kmers_indexed"] == truth["kmers"], (what, info)
    for s, n in enumerate(set_sizes):
        mine = util.bools_from_bits(tags[s], n)
        assert np.array_equal(mine, truth["tags"][s]), (what, s, np.nonzero(mine != truth["tags"][s])[0][:10].tolist())
        assert [stats[s][f] for f in ("indexed", "searched", "shared")] == [truth["stats"][s][f] for f in ("indexed", "searched", "shared")], (what, s)


def run_case(tmp_path, what, k, index, max_kmer, opts, n_chunks, names=None, index_select=None, must_run=(), must_not_run=(),
             rounds=None, search=None):
    """the four steps above in one context.  names: the bucket classes of the chunks, together (asserted from the census); rounds:
    [(poison byte, index_lanes)] after the timed run"""
    import commet_amd as commet
    t0 = time.time()
    search = search if search is not None else search_reads(k, index)
    truth = jf.checker_run(tmp_path / "orc", k, T, index, [search], max_kmer=max_kmer, index_select=index_select)
    assert truth["chunks"] == n_chunks, (what, truth["trace"])
    census = [jf.tile_census(k, index, row, index_select) for row in truth["trace"]]
    print(what, "census per chunk:", census)
    if names is not None:
        assert set().union(*[jf.classes(c) for c in census]) == set(names), (what, census)
    group = jf.effective_group(n_chunks, opts.get("chunk_group", 1))
    in_slot = jf.slot_chunks(n_chunks, group)
    filters = {c: jf.chunk_filter(k, index, truth["trace"][c], index_select) for c in set(in_slot) if c is not None}
    want_by_slot = [None if c is None else filters[c] for c in in_slot]
    sel = None if index_select is None else util.bits_from_bools(index_select)
    with commet.Context(k=k, t=T) as ctx:
        for name, value in dict(BASE, max_kmer=max_kmer, **opts).items():
            ctx.set_option(name, value)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        ctx.set_option("kernel_timing", 1)
        got = ctx.index_and_search(irs, [qrs], index_select=sel)
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        check_build_kernels(times, n_chunks, what)
        ran = {n: times[n][0] for n in tps.SEARCH_KERNELS if n in times}
        assert ran == expected_search_launches(n_chunks, group), (what, ran)
        assert all(n in times for n in must_run) and not any(n in times for n in must_not_run), (what, sorted(times))
        check_job((what, "timed"), got, truth, [len(search)])
        for byte, lanes in rounds or [(b, 2) for b in jf.POISONS]:
            ctx.set_option("index_lanes", lanes)
            ctx.poison(byte)
            got = ctx.index_and_search(irs, [qrs], index_select=sel)
            check_job((what, hex(byte), lanes), got, truth, [len(search)])
            check_slots(ctx, f"{what}, poison 0x{byte:02x}, index_lanes {lanes}", want_by_slot)
        with pytest.raises(commet.CommetError):
            ctx.export_filter_reference(8)
        n_slots = 1 if group == 1 else 2 if group == 2 else 4 if group <= 4 else 8      # (ensure_slots: a whole group's worth at once)
        if n_slots < 8:
            with pytest.raises(commet.CommetError):                # no such slot in this context
                ctx.export_filter_reference(n_slots)
        irs.close()
        qrs.close()
    print(what, f"{time.time() - t0:.1f} s")
    return census


# ---- tile classes: one chunk, one slot -----------------------------------------------------------------------------------------------------
# (k, part_packed, random reads, bucket classes of the chunk).  Geometries (make_geom): k <= 25 a single level; 26, 28 two levels, plain
# and packed; 30 packed (7 + 6 bits); 33 packed with 64-bit keys.  k = 20 has 8 buckets, two per plane: the copies of A x 150 split
# bucket 0 of every plane, the random reads fill the other — hardly any bucket can be empty there, and none is.
# Few random reads at k <= 28: the planes' high key bits decide the bucket, and plane d = a | b reaches a bucket of few one bits only
# with probability (1/4)^zeros per k-mer — some hundred reads leave no bucket of 2^(k-17) empty below k = 30.
TILE_CASES = [(20, 1, 300, ("single", "split")), (24, 1, 2, ALL), (25, 1, 3, ALL), (26, 0, 12, ALL), (26, 1, 12, ALL), (28, 0, 40, ALL),
              (28, 1, 40, ALL), (30, 1, 300, ALL), (33, 1, 300, ALL)]


@pytest.mark.parametrize("k,packed,n_random,names", TILE_CASES)
def test_one_chunk_defines_every_tile_of_its_slot(tmp_path, k, packed, n_random, names):
    index, max_kmer, _ = tile_case_set(k, n_random)
    census = run_case(tmp_path, f"tiles k={k} packed={packed}", k, index, max_kmer, dict(chunk_group=1, part_packed=packed), 1, names)
    assert jf.classes(census[0]) == set(names)                    # all of them in the ONE chunk


def test_one_read_of_k_bases_leaves_every_other_bucket_empty(tmp_path):
    k = 26
    index = [util.random_reads(np.random.default_rng(26), 1, k, k, n_rate=0.0, lower_rate=0.0, other_rate=0.0)[0]]
    search = [index[0] + index[0], index[0] + b"ACGT" * 7, b"ACGT" * 16]
    import commet_amd as commet
    truth = jf.checker_run(tmp_path / "orc", k, T, index, [search], max_kmer=10)
    census = jf.tile_census(k, index, truth["trace"][0])
    assert census == dict(empty=(1 << (k - 17)) - 4, single=4, split=0, keys=4)
    want = jf.chunk_filter(k, index, truth["trace"][0])
    assert int(np.unpackbits(want).sum()) == 4
    with commet.Context(k=k, t=T) as ctx:
        for name, value in dict(BASE, max_kmer=10, chunk_group=1).items():
            ctx.set_option(name, value)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        ctx.set_option("kernel_timing", 1)
        got = ctx.index_and_search(irs, [qrs])
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        check_build_kernels(times, 1, "one read")
        check_job("one read", got, truth, [len(search)])
        assert truth["tags"][0].tolist() == [True, False, False]
        for byte in jf.POISONS:
            ctx.poison(byte)
            check_job(("one read", byte), ctx.index_and_search(irs, [qrs]), truth, [len(search)])
            check_slots(ctx, f"one read, poison 0x{byte:02x}", [want])
        irs.close()
        qrs.close()


# ---- slots 1 .. 7 ---------------------------------------------------------------------------------------------------------------------------
SLOT_SHAPES = [(2, 2), (3, 4), (4, 4), (6, 8), (8, 8), (3, 2), (9, 4)]      # (chunks, chunk_group); the last two leave older chunks in the higher slots


@pytest.mark.parametrize("k,n_random", [(21, 300), (26, 12)])
@pytest.mark.parametrize("n_chunks,chunk_group", SLOT_SHAPES)
def test_every_slot_of_a_group_holds_its_chunk(tmp_path, k, n_random, n_chunks, chunk_group):
    index, max_kmer = chunked_set(k, n_chunks, n_random)
    names = ("single", "split") if k == 21 else ALL               # (k = 21: four buckets per plane)
    run_case(tmp_path, f"slots k={k} chunks={n_chunks} group={chunk_group}", k, index, max_kmer, dict(chunk_group=chunk_group), n_chunks, names)


# ---- two lanes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n_random", [(26, 12), (32, 300)])
def test_two_chunks_built_on_two_lanes(tmp_path, k, n_random):
    """Nothing observable says that the second lane ran; its conditions are: a group of exactly two chunks that both take the bucketed
    build (index_mode = 2), index_lanes = 2, kernel_timing = 0 — the state of every poisoned run below but the last, which builds the
    same two chunks on one lane.  k = 32: the benchmark's configs[1] geometry (7 + 8 bits, packed, 2 GiB per slot)."""
    index, max_kmer = chunked_set(k, 2, n_random)
    run_case(tmp_path, f"lanes k={k}", k, index, max_kmer, dict(chunk_group=2), 2, ALL, rounds=[(0xFF, 2), (0xA5, 2), (0xFF, 1)])


# ---- the item paths of hist / scatter1 inside a job --------------------------------------------------------------------------------------------
def _item_case(path):
    k = 21
    rng = np.random.default_rng(77)
    if path == "fixed_selected":                                  # d_ids: UNI over the list of selected reads, pos_first of the second chunk != 0
        reads = util.random_reads(rng, 400, 100, 100, n_rate=0.005) + [b"A" * 100] * 11000 + [(b"ACG" * 34)[:100]] * 300
        reads = [reads[i] for i in rng.permutation(len(reads))]
        select = np.arange(len(reads)) % 3 == 0
    elif path == "ragged_selected":                               # LIST from the bitmap
        reads = jf.three_class_reads(78, k, 300, 2)
        reads = reads + reads
        select = np.arange(len(reads)) % 3 != 1
    else:                                                         # a read of more than 4096 k-mers: the list written by whole workgroups
        reads = jf.three_class_reads(79, k, 300, 2)
        reads.insert(len(reads) // 3, util.random_reads(rng, 1, 6000, 6000, n_rate=0.0, lower_rate=0.0, other_rate=0.0)[0])
        select = None
    return k, reads, select, jf.max_kmer_for(k, reads, 2, select)[0]


@pytest.mark.parametrize("path,names,must_run,must_not_run", [
    ("fixed_selected", ("single", "split"), (), ("part_items_kernels", "part_items_fill_kernel")),
    ("ragged_selected", ("single", "split"), ("part_items_kernels",), ("part_items_fill_kernel",)),
    ("long_read", ("single", "split"), ("part_items_kernels", "part_items_fill_kernel"), ())])
def test_item_paths_inside_a_job(tmp_path, path, names, must_run, must_not_run):
    k, index, select, max_kmer = _item_case(path)
    if path == "fixed_selected":
        assert len({len(r) for r in index}) == 1
    run_case(tmp_path, f"items {path}", k, index, max_kmer, dict(chunk_group=2), 2, names, index_select=select, must_run=must_run,
             must_not_run=must_not_run, search=search_reads(5, [r for r in index if len(r) < 1000]))


# ---- a dense job, then a sparse one: no poison ----------------------------------------------------------------------------------------------------
def test_sparse_job_after_a_dense_job(tmp_path):
    """the real-life form: the slot holds the filter of a job that filled every tile when a job of mostly empty buckets comes"""
    import commet_amd as commet
    k = 24
    rng = np.random.default_rng(24)
    dense = util.random_reads(rng, 40000, 100, 100, n_rate=0.0, lower_rate=0.0, other_rate=0.0)
    sparse, mk_sparse, _ = tile_case_set(k, 2)
    search = search_reads(k, sparse)
    assert int((jf.bucket_counts(k, dense[:4000]) == 0).sum()) == 0      # every tile of the slot holds bits of the dense job (a tenth of it already)
    truth = jf.checker_run(tmp_path / "orc", k, T, sparse, [search], max_kmer=mk_sparse)
    assert jf.classes(jf.tile_census(k, sparse, truth["trace"][0])) == set(ALL)
    want = jf.chunk_filter(k, sparse, truth["trace"][0])
    with commet.Context(k=k, t=T) as ctx:
        for name, value in dict(BASE, chunk_group=1).items():
            ctx.set_option(name, value)
        drs = commet.ReadSet.from_files(ctx, [util.to_batch(dense)])
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(sparse)])
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        ctx.set_option("max_kmer", 1 << 40)
        ctx.set_option("kernel_timing", 1)
        _, _, info = ctx.index_and_search(drs, [qrs])
        assert info["n_chunks"] == 1
        ctx.set_option("max_kmer", mk_sparse)
        got = ctx.index_and_search(srs, [qrs])
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        check_build_kernels(times, 2, "dense, sparse")
        check_job("sparse after dense", got, truth, [len(search)])
        check_slots(ctx, "sparse after dense", [want])
        for r in (drs, srs, qrs):
            r.close()


# ---- jobs that share passes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,k,n_chunks", [("pairs", 26, 1), ("group8", 25, 3)])
def test_slots_of_jobs_that_share_a_pass(tmp_path, how, k, n_chunks):
    """pairs: run_pair (capi/multi.hpp), the one chunk of each of two jobs in slots 0 and 1, on two lanes when kernel_timing is off;
    group8: run_shared_pass, the three chunks of each job in six slots"""
    import commet_amd as commet
    _, opts, kernel, launches = tps.JOB_RUNS[how]
    c = ps.ladder_jobs(k, n_chunks)
    truth = [jf.checker_run(tmp_path / f"j{j}", k, T, c["index_sets"][j], [c["search"]], max_kmer=c["max_kmer"]) for j in range(2)]
    assert [tr["chunks"] for tr in truth] == [n_chunks, n_chunks]
    want_by_slot = [jf.chunk_filter(k, c["index_sets"][j], truth[j]["trace"][ci]) for j in range(2) for ci in range(n_chunks)]
    with commet.Context(k=k, t=T) as ctx:
        for name, value in dict(BASE, max_kmer=c["max_kmer"], **opts).items():
            ctx.set_option(name, value)
        sets = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in c["index_sets"]]
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(c["search"])])

        def check(what, got):
            tags, stats, _ = got
            for j in range(2):
                mine = util.bools_from_bits(tags[j], len(c["search"]))
                want = c["counts"][j] >= T
                assert np.array_equal(mine, want) and np.array_equal(mine, truth[j]["tags"][0]), (what, j, np.nonzero(mine != want)[0][:10].tolist())
                assert [stats[j][f] for f in ("indexed", "searched", "shared")] == [truth[j]["stats"][0][f] for f in ("indexed", "searched", "shared")], (what, j)

        ctx.set_option("kernel_timing", 1)
        got = ctx.index_many_and_search(sets, qrs)
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        check_build_kernels(times, 2 * n_chunks, how)
        ran = {n: times[n][0] for n in tps.SEARCH_KERNELS if n in times}
        assert ran.pop("tq_probe_kernel", launches) == launches and ran == {kernel: launches}, (how, ran)
        check((how, "timed"), got)
        for byte in jf.POISONS:
            ctx.poison(byte)
            check((how, hex(byte)), ctx.index_many_and_search(sets, qrs))
            check_slots(ctx, f"{how}, poison 0x{byte:02x}", want_by_slot)
        for r in sets + [qrs]:
            r.close()


# ---- tables and interleaved planes: tags only (nothing exports them) ------------------------------------------------------------------------------
def _tags_after_poison(what, case, t, runs):
    """every option set of `runs`: the job, then poisoned with either byte and again — the tags equal the design and the first run.
    The search kernels count on zeros in what no build writes: the columns past the last chunk of the bit-sliced tables and rows
    (slice_transpose_kernel), the unused columns of the interleaved A planes (interleave_a_kernel: g = 3 of a stride of 4, 5 .. 7 of 8)"""
    import commet_amd as commet
    names = list(case["sets"])
    reads = [case["sets"][n][0] for n in names]
    with commet.Context(k=case["k"], t=t) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(case["index"])])
        qrs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in reads]
        for opts, must, may in runs:
            for name, value in dict(tps.DEFAULTS, **opts).items():
                ctx.set_option(name, value)
            ctx.set_option("kernel_timing", 1)
            first, _, info = ctx.index_and_search(irs, qrs)
            times = ctx.kernel_times()
            ctx.set_option("kernel_timing", 0)
            ran = {n for n in tps.SEARCH_KERNELS if n in times}
            assert must <= ran and (ran - must <= may if may is not None else ran == must), (what, opts, sorted(ran))
            assert info["n_chunks"] == case["n_chunks"]
            for byte in (None,) + jf.POISONS:
                if byte is not None:
                    ctx.poison(byte)
                    tags, _, _ = ctx.index_and_search(irs, qrs)
                else:
                    tags = first
                for s, n in enumerate(names):
                    mine = util.bools_from_bits(tags[s], len(reads[s]))
                    want = case["sets"][n][1] >= t
                    assert np.array_equal(mine, want), (what, opts, byte, n, np.nonzero(mine != want)[0][:10].tolist())
                    assert np.array_equal(tags[s], first[s]), (what, opts, byte, n)
        for r in qrs + [irs]:
            r.close()


@pytest.mark.parametrize("k", [16, 21])
def test_bit_sliced_tables_after_poison(k):
    """300 chunk filters: 44 columns of the last 32-chunk words and of the second 256-chunk group hold no chunk"""
    _tags_after_poison("sliced", ps.ladder_case(k, 300), T, tps.SLICED_RUNS + tps.WIDE_RUNS)


@pytest.mark.parametrize("k,n_chunks,opts,kernel", [(25, 3, dict(chunk_group=4), "search_group_kernel"),
                                                    (25, 5, dict(chunk_group=8), "search_group8_kernel"), (20, 5, dict(chunk_group=8), "search_group8_kernel")])
def test_unused_interleave_columns_after_poison(k, n_chunks, opts, kernel):
    _tags_after_poison("interleave", ps.ladder_case(k, n_chunks), T, [(dict(opts, index_mode=m), {kernel}, None) for m in (0, 2)])


def test_tiled_search_of_two_filters_after_poison():
    _tags_after_poison("tiled", ps.ladder_case(25, 6), T, [(dict(tiled_search=2, chunk_group=2, index_mode=m), {"tq_probe_kernel", "tq_replay_kernel"}, None)
                                                            for m in (0, 2)])


def test_hit_profile_after_poison():
    """commet_index_and_profile builds its chunk filters with the same launch_index calls: groups of four (4 + 2 chunks), k = 25"""
    import commet_amd as commet
    c = ps.ladder_case(25, 6)
    names = list(c["sets"])
    reads = [c["sets"][n][0] for n in names]
    with commet.Context(k=25, t=T) as ctx:
        for name, value in dict(BASE, max_kmer=c["max_kmer"], chunk_group=4).items():
            ctx.set_option(name, value)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(c["index"])])
        qrs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in reads]
        ctx.set_option("kernel_timing", 1)
        first, info = ctx.index_and_profile(irs, qrs, max_hits=4)
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        check_build_kernels(times, 6, "profile")
        assert info["n_chunks"] == 6 and times["hits_group_kernel"][0] == 2 * len(names)
        for byte in jf.POISONS:
            ctx.poison(byte)
            hits, _ = ctx.index_and_profile(irs, qrs, max_hits=4)
            for s, n in enumerate(names):
                assert np.array_equal(hits[s], first[s]) and np.array_equal(hits[s], np.minimum(c["sets"][n][1], 4)), (byte, n)
        for r in qrs + [irs]:
            r.close()
