"""The filter's bits, EXACTLY, at every k and on every build path, through the sparse export (Context.filter_set_bits; filter_bits.py).

The byte export needs 2^(k-1) bytes of host memory, so above k = 28 the suite compared bytes for a few shapes only and above k = 33
tags alone — which cannot see an extra bit, and see a missing one only when a query carries that k-mer.  The list of set bits is a
few MB at any k.  It is also independent of the device's psi_a: the device reports plane A at the stored address, the expectation goes
through the numpy mirror (filter_bits.expected_bits).

a. the hook against the byte export and the expectation (k <= 26), empty filters, the cap, missing slots, whole poisoned slots
b. the atomic index_kernel at every k = 1 .. 38 (64-bit keys, up to 128 GiB per slot)
c. the bucketed build at every k = 20 .. 34, every item path (UNI, LIST, round planner, LIST filled by whole workgroups), both packings
d. the chunk filters of jobs (no memset, two lanes, after poison) at k = 29, 31, 32, 34
Every comparison is exact and complete: filter_set_bits raises when the list does not fit its cap."""
import collections
import time

import numpy as np
import pytest

import filter_bits as fb
import job_filters as jf
import oracle_binding as ob
import test_gpu_job_filter_bytes as jb
import util

pytestmark = pytest.mark.gpu

CAP = 1 << 23


@pytest.fixture(scope="module")
def commet():
    import commet_amd
    return commet_amd


def assert_bits(ctx, want, k, what, slot=0):
    got = ctx.filter_set_bits(slot, CAP)                          # (raises when the slot holds more than CAP bits)
    assert got.size <= CAP and want.size <= CAP // 4, (what, got.size, want.size)
    diff = fb.difference(got, want, k)
    assert diff is None, f"{what}: {diff}"


def kmers_of(k, reads, select=None):
    counts = collections.Counter(r for i, r in enumerate(reads) if select is None or select[i])
    return sum(n * len(ob.keys_of_read(r, k)[1]) for r, n in counts.items())


def mixed_reads(seed, n=300):
    """reads of 1-170 bases with N, lower case and other letters; an empty one"""
    rng = np.random.default_rng(seed)
    reads = util.random_reads(rng, n, 1, 170, n_rate=0.01, lower_rate=0.2)
    reads[n // 3] = b""
    return reads


def three_calls(ctx, rs, k, reads, what, first, count, select, first2, count2):
    """the whole set on a reset filter; a range under a selection on a reset filter; an additive second call on a range without one"""
    n = len(reads)
    ctx.filter_reset()
    assert ctx.index_reads(rs) == kmers_of(k, reads), what
    assert_bits(ctx, fb.expected_bits(k, reads), k, f"{what}, whole set")
    in_range = (np.arange(n) >= first) & (np.arange(n) < first + count)
    sel1 = in_range & select
    ctx.filter_reset()
    assert ctx.index_reads(rs, first, count, util.bits_from_bools(select)) == kmers_of(k, reads, sel1), what
    assert_bits(ctx, fb.expected_bits(k, reads, sel1), k, f"{what}, reads {first} .. {first + count - 1} under a selection")
    sel2 = (np.arange(n) >= first2) & (np.arange(n) < first2 + count2)
    assert ctx.index_reads(rs, first2, count2) == kmers_of(k, reads, sel2), what
    assert_bits(ctx, fb.expected_bits(k, reads, sel1 | sel2), k, f"{what}, plus reads {first2} .. {first2 + count2 - 1}")


# ---- a. the hook itself ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5, 8, 13, 20, 21, 26])
def test_set_bits_equal_the_byte_export_and_the_expectation(commet, k):
    reads = mixed_reads(k)
    want = fb.expected_bits(k, reads)
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("index_mode", 1)
        rs = commet.ReadSet.from_files(ctx, [util.to_batch(reads)])
        assert ctx.filter_set_bits().size == 0                    # a context's first slot starts zeroed
        ctx.index_reads(rs)
        got = ctx.filter_set_bits()
        assert got.dtype == np.uint64 and got.size > 0
        from_bytes = fb.bits_of_reference_bytes(k, ctx.export_filter_reference())
        assert fb.difference(got, from_bytes, k) is None, fb.difference(got, from_bytes, k)
        assert fb.difference(got, want, k) is None, fb.difference(got, want, k)
        f = ob.Bloom(k)
        f.index(*util.to_batch(reads))
        assert fb.difference(got, fb.bits_of_reference_bytes(k, f.bytes()), k) is None
        f.close()
        # a cap below the count: an error that names the full count, whatever the cap
        for cap in (0, 1, got.size - 1):
            with pytest.raises(commet.CommetError, match=rf"\b{got.size} set bits"):
                ctx.filter_set_bits(0, cap)
        assert np.array_equal(ctx.filter_set_bits(0, got.size), got)
        # slots the context does not have
        for slot in (1, 7, 8):
            with pytest.raises(commet.CommetError):
                ctx.filter_set_bits(slot)
        ctx.filter_reset()
        assert ctx.filter_set_bits().size == 0
        rs.close()


@pytest.mark.parametrize("k,byte", [(1, 0xFF), (3, 0xFF), (4, 0xA5), (5, 0xFF), (8, 0xFF), (12, 0x80), (12, 0xA5)])
def test_the_scan_sees_the_whole_slot_and_nothing_beyond(commet, k, byte):
    """a slot filled with one byte: every bit of the four planes that the byte sets, and no address >= 2^k (k < 5: a plane is a
    part of one word)"""
    with commet.Context(k=k, t=1) as ctx:
        ctx.poison(byte)
        got = ctx.filter_set_bits()
    address = np.arange(1 << k, dtype=np.uint64)
    address = address[((byte >> (address & np.uint64(7)).astype(np.int64)) & 1) == 1]
    want = np.concatenate([fb.words_of(p, address) for p in range(4)])
    assert want.size == 4 * (1 << k) * bin(byte).count("1") // 8
    assert fb.difference(got, want, k) is None, fb.difference(got, want, k)
    if byte == 0x80:
        assert np.all((got & np.uint64(7)) == np.uint64(7)) and got.size == 4 << (k - 3)


# ---- b. the atomic kernel where no byte export reaches --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", list(range(1, 39)))
def test_atomic_index_kernel_sets_exactly_the_keys_bits(commet, k):
    """every k the library takes (a case costs a few hundredths of a second below k = 37): above k = 28 nothing else pins the atomic
    kernel's bits at k = 29, 31 and 34 .. 38"""
    t0 = time.time()
    reads = mixed_reads(1000 + k)
    select = np.random.default_rng(k).random(len(reads)) < 0.6
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("index_mode", 1)
        rs = commet.ReadSet.from_files(ctx, [util.to_batch(reads)])
        assert ctx.filter_set_bits().size == 0
        ctx.set_option("kernel_timing", 1)
        three_calls(ctx, rs, k, reads, f"atomic k={k}", 17, 200, select, 230, 60)
        times = ctx.kernel_times()
        assert times["index_kernel"][0] == 3 and "part_build_kernel" not in times, sorted(times)
        rs.close()
    print(f"atomic k={k}: {time.time() - t0:.1f} s")


# ---- c. the bucketed build, every k it takes -------------------------------------------------------------------------------------------------
# random reads per k so that buckets of all three kinds occur (jf.bucket_counts; test_gpu_job_filter_bytes.py says why so few below k = 30)
N_RANDOM = {20: 300, 21: 300, 22: 40, 23: 1, 24: 2, 25: 3, 26: 12, 27: 20, 28: 40, 29: 100}
UNI_L = 150


def bucketed_set(k, shape):
    """as job_filters.three_class_reads: random reads, BUILD_CAP // (L - k + 1) + 12 copies of poly-A (bucket 0 of every plane split over
    several build workgroups), (ACG) repeats — uni: all of one length; ragged: 40-160 bases; long: ragged plus one read of 6000 bases"""
    n_random = N_RANDOM.get(k, 300)
    rng = np.random.default_rng(7000 + k)
    if shape == "uni":
        L = UNI_L
        reads = util.random_reads(rng, n_random, L, L, n_rate=0.005) + [b"A" * L] * (jf.BUILD_CAP // (L - k + 1) + 12) + [(b"ACG" * L)[i % 3:][:L] for i in range(300)]
        return [reads[i] for i in rng.permutation(len(reads))]
    reads = jf.three_class_reads(7100 + k, k, n_random)
    if shape == "long":
        reads.insert(len(reads) // 3, util.random_reads(rng, 1, 6000, 6000, n_rate=0.0, lower_rate=0.0, other_rate=0.0)[0])
    return reads


def expected_classes(k, shape):
    """the classes a set must hold at least.  k = 20, 21, 22 have two, four and eight buckets per plane: one random read of 40 bases
    or more leaves none empty (19+ k-mers over 8 buckets of plane a; plane d = a | b reaches a bucket with z zeros among its 3 high bits
    with probability 4^-z per k-mer, and poly-A fills the one of z = 3), so k = 22 takes a few dozen random reads and no empty bucket,
    k = 23 .. 25 one to three reads.  The 5967+ k-mers of the long read fill nearly every bucket below k = 27"""
    if k <= 22 or (shape == "long" and k <= 26):
        return {"single", "split"}
    return {"empty", "single", "split"}


VARIANTS = {"uni": [dict(part_no_uni=0), dict(part_no_uni=1)], "ragged": [dict(part_list=0), dict(part_list=1)], "long": [dict()]}
ITEM_KERNELS = ("part_items_kernels", "part_items_fill_kernel")


def expected_item_kernels(shape, opts):
    if shape == "long":
        return set(ITEM_KERNELS)
    return {"part_items_kernels"} if shape == "ragged" and not opts["part_list"] else set()


def expected_scatter2(k, packed):
    """k <= 25: a single level, scatter1 writes the final buckets; k = 34: 2^9 final buckets per coarse one, beyond the packed kernel"""
    if k <= 25:
        return set()
    return {"part_scatter2_packed_kernel"} if packed and k <= 33 else {"part_scatter2_kernel"}


@pytest.mark.parametrize("shape", ["uni", "ragged", "long"])
@pytest.mark.parametrize("k", list(range(20, 35)))
def test_bucketed_build_sets_exactly_the_keys_bits(commet, k, shape):
    t0 = time.time()
    reads = bucketed_set(k, shape)
    n = len(reads)
    assert (len({len(r) for r in reads}) == 1) == (shape == "uni")
    counts = jf.bucket_counts(k, reads)
    classes = {name for name, some in (("empty", (counts == 0).any()), ("single", ((counts > 0) & (counts <= jf.BUILD_CAP)).any()),
                                        ("split", (counts > jf.BUILD_CAP).any())) if some}
    assert classes >= expected_classes(k, shape) and (k > 21 or "empty" not in classes), (k, shape, classes)
    select = np.random.default_rng(k).random(n) < 0.6
    select[[i for i, r in enumerate(reads) if len(r) > 1000]] = True      # (the long read is of the selection)
    ran = []
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("index_mode", 2)
        rs = commet.ReadSet.from_files(ctx, [util.to_batch(reads)])
        for opts in VARIANTS[shape]:
            for packed in ((0, 1) if 26 <= k <= 33 else (1,)):
                what = f"bucketed k={k} {shape} {opts} part_packed={packed}"
                for name, value in dict(opts, part_packed=packed).items():
                    ctx.set_option(name, value)
                ctx.set_option("kernel_timing", 1)
                three_calls(ctx, rs, k, reads, what, 5, n - 405, select, n - 399, 399)     # reads 0-4 and one more skipped
                times = ctx.kernel_times()
                ctx.set_option("kernel_timing", 0)
                names = set(times)
                assert times["part_build_kernel"][0] == 3 and "index_kernel" not in names, (what, sorted(names))
                assert names & set(ITEM_KERNELS) == expected_item_kernels(shape, opts), (what, sorted(names))
                assert {x for x in names if x.startswith("part_scatter2")} == expected_scatter2(k, packed), (what, sorted(names))
                ran.append(what)
        rs.close()
    print(f"{len(ran)} variants, {time.time() - t0:.1f} s:", *ran, sep="\n  ")


# ---- d. the chunk filters of jobs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [29, 31, 32, 34])
def test_job_slots_hold_exactly_their_chunks_bits(commet, tmp_path, k):
    """index_and_search on two chunks, chunk_group = 2: no slot is zeroed, the chunks are built into slots 0 and 1 on two lanes (and
    once on one); after either poison each slot holds exactly its chunk's bits, and the job gives the checker's tags and numbers"""
    t0 = time.time()
    index, max_kmer = jb.chunked_set(k, 2, N_RANDOM.get(k, 300))
    search = jb.search_reads(k, index)
    truth = jf.checker_run(tmp_path / "orc", k, jb.T, index, [search], max_kmer=max_kmer)
    assert truth["chunks"] == 2, truth["trace"]
    census = [jf.tile_census(k, index, row) for row in truth["trace"]]
    assert all(jf.classes(c) == set(jb.ALL) for c in census), census
    selects = [jf.chunk_select(len(index), row) for row in truth["trace"]]
    want = [fb.expected_bits(k, index, s) for s in selects]
    assert [kmers_of(k, index, s) for s in selects] == [row[3] for row in truth["trace"]]
    with commet.Context(k=k, t=jb.T) as ctx:
        for name, value in dict(jb.BASE, max_kmer=max_kmer, chunk_group=2).items():
            ctx.set_option(name, value)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        qrs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        ctx.set_option("kernel_timing", 1)
        got = ctx.index_and_search(irs, [qrs])
        times = ctx.kernel_times()
        ctx.set_option("kernel_timing", 0)
        jb.check_build_kernels(times, 2, f"job k={k}")
        jb.check_job((k, "timed"), got, truth, [len(search)])
        for slot in (0, 1):
            assert_bits(ctx, want[slot], k, f"job k={k}, timed run, slot {slot}", slot)
        for byte, lanes in [(0xFF, 2), (0xA5, 2), (0xFF, 1)]:
            ctx.set_option("index_lanes", lanes)
            ctx.poison(byte)
            jb.check_job((k, hex(byte), lanes), ctx.index_and_search(irs, [qrs]), truth, [len(search)])
            for slot in (0, 1):
                assert_bits(ctx, want[slot], k, f"job k={k}, poison 0x{byte:02x}, index_lanes {lanes}, slot {slot}", slot)
        with pytest.raises(commet.CommetError):
            ctx.filter_set_bits(2)
        irs.close()
        qrs.close()
    print(f"job k={k}: {time.time() - t0:.1f} s")
