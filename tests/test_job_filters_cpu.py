"""job_filters.py against itself and the checker, without a GPU: the per-chunk filters of a job, the tile census, the slot map, and
the census of every index set test_gpu_job_filter_bytes.py builds (checked here, before any GPU run)."""
import numpy as np
import pytest

import job_filters as jf
import oracle_binding as ob
import util


def test_chunk_filters_or_to_the_filter_of_all_indexed_reads(tmp_path):
    k = 20
    rng = np.random.default_rng(5)
    index = util.random_reads(rng, 400, 15, 120, n_rate=0.01)
    search = [util.random_reads(rng, 70, 60, 60)]
    select = rng.random(len(index)) < 0.7
    for sel in (None, select):
        run = jf.checker_run(tmp_path / ("sel" if sel is not None else "all"), k, 2, index, search, max_kmer=3000, index_select=sel)
        assert run["chunks"] == len(run["trace"]) >= 4 and sum(r[3] for r in run["trace"]) == run["kmers"]
        assert sum(r[2] for r in run["trace"]) == run["stats"][0]["indexed"]
        union = np.zeros(1 << (k - 1), dtype=np.uint8)
        indexed = np.zeros(len(index), dtype=bool)
        for a, b in zip(run["trace"], run["trace"][1:]):
            assert a[1] < b[0]                                   # chunks are disjoint read ranges (the look-ahead read lies between)
        for row in run["trace"]:
            union |= jf.chunk_filter(k, index, row, sel)
            indexed |= jf.chunk_select(len(index), row, sel)
        assert int(indexed.sum()) == run["stats"][0]["indexed"] < (len(index) if sel is None else int(select.sum()))   # reads were dropped
        f = ob.Bloom(k)
        bases, offs = util.to_batch(index)
        assert f.index(bases, offs, util.bits_from_bools(indexed)) == run["kmers"]
        assert np.array_equal(union, f.bytes())


def test_census_of_a_hand_made_set():
    """k = 20: two buckets per plane, bucket = plane * 2 + the key's top bit.  A: (a, b, c, d) = (0, 0, 0, 0); T: (1, 1, 0, 1);
    G: (1, 0, 1, 1); C: (0, 1, 1, 1) per base"""
    k = 20
    reads = [b"A" * 20, b"A" * 22, b"T" * 21, b"G" * 20, b"ACGTN", b"C" * 19]      # 1 + 3 + 2 + 1 k-mers
    want = np.zeros(8, dtype=np.int64)
    want[[0, 2, 4, 6]] += 4                                      # poly-A: key 0 in every plane
    want[[1, 3, 4, 7]] += 2                                      # poly-T
    want[[1, 2, 5, 7]] += 1                                      # poly-G
    assert jf.bucket_counts(k, reads).tolist() == want.tolist()
    row = (0, len(reads) - 1, len(reads), 7)
    assert jf.tile_census(k, reads, row) == dict(empty=0, single=8, split=0, keys=28)
    sel = np.array([1, 1, 0, 0, 1, 1], dtype=bool)
    assert jf.tile_census(k, reads, (0, 5, 4, 4), sel) == dict(empty=4, single=4, split=0, keys=16)
    # more than 2^17 keys in a bucket: 1200 copies of A x 130 give 1200 x 111 = 133 200 in bucket 0 of every plane
    many = [b"A" * 130] * 1200 + [b"T" * 20]
    census = jf.tile_census(k, many, (0, 1200, 1201, 133201))
    assert census == dict(empty=1, single=3, split=4, keys=4 * 133201) and jf.classes(census) == {"empty", "single", "split"}
    assert jf.BUILD_CAP == 131072 < 133200


def test_census_agrees_with_the_checkers_filter():
    """a bucket holds a key exactly when the checker's filter has a bit of that plane in the bucket's 2^18 bytes"""
    k = 24
    reads = jf.three_class_reads(3, k, 3, hot=20)[:400]
    counts = jf.bucket_counts(k, reads)
    bases, offs = util.to_batch(reads)
    f = ob.Bloom(k)
    f.index(bases, offs)
    by = f.bytes().reshape(-1, 1 << 18)
    for plane, mask in enumerate((0x88, 0x44, 0x22, 0x11)):
        used = (np.bitwise_or.reduce(by, axis=1) & mask) != 0
        assert np.array_equal(used, counts[plane << (k - 19):(plane + 1) << (k - 19)] > 0), plane


@pytest.mark.parametrize("n,g,want", [(1, 1, [0]), (2, 2, [0, 1]), (3, 2, [2, 1]), (6, 8, [0, 1, 2, 3, 4, 5, None, None]), (9, 4, [8, 5, 6, 7])])
def test_slot_map(n, g, want):
    assert jf.slot_chunks(n, g) == want


def test_effective_group():
    assert [jf.effective_group(n, g) for n, g in ((1, 8), (2, 2), (3, 4), (4, 8), (5, 8), (6, 8), (9, 4), (3, 2))] == [1, 2, 4, 4, 8, 8, 4, 2]


def test_first_difference_names_the_tile():
    want = np.zeros(1 << 19, dtype=np.uint8)
    assert jf.first_difference(want.copy(), want) is None
    got = want.copy()
    got[(3 << 16) + 5] = 0x80
    got[(3 << 16) + 9] = 0x03
    got[(6 << 16)] = 0x01
    msg = jf.first_difference(got, want)
    assert "tile 3 " in msg and "2 bytes differ there" in msg and "3 extra bits, 0 missing" in msg and "3 bytes in all" in msg and "planes acd" in msg
    assert "expected" in jf.first_difference(got[:100], want)


def test_every_gpu_case_has_the_buckets_it_names():
    """the census of the index sets of test_gpu_job_filter_bytes.py (the small k: the large ones are asserted in the GPU tests themselves)"""
    import test_gpu_job_filter_bytes as gj
    for k, packed, n_random, names in gj.TILE_CASES:
        if k > 28:
            continue
        reads, mk, row = gj.tile_case_set(k, n_random)
        census = jf.tile_census(k, reads, row)
        assert jf.classes(census) == set(names), (k, census)
