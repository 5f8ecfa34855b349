"""filter_bits.py against the CPU checker's filter, the numpy mirror of psi_a at the k no exhaustive test reaches, and the
comparison itself on planted differences: what test_gpu_filter_bits.py rests on, checked without a GPU."""
import numpy as np
import pytest

import filter_bits as fb
import oracle_binding as ob
import util
from test_psi_layout import brev, psi


def mixed_reads(seed, k, n=120):
    """N, lower case, IUPAC letters and other bytes (util.random_reads), reads shorter than k, a read of k bases, one of N only, an
    empty one, repeats"""
    rng = np.random.default_rng(seed)
    reads = util.random_reads(rng, n, 1, 170, n_rate=0.02, lower_rate=0.3, other_rate=0.01)
    reads += util.random_reads(rng, 10, 1, max(1, k - 1)) + util.random_reads(rng, 5, k, k, n_rate=0.0)
    reads += [b"N" * 50, b"", b"acgtRYKMacgtnACGT" * 6, b"A" * 90, b"A" * 90, (b"ACG" * 40)[:100]]
    return [reads[i] for i in rng.permutation(len(reads))]


@pytest.mark.parametrize("k", [1, 2, 5, 8, 12, 13, 16, 20, 21, 24])
def test_expected_bits_equal_the_bits_of_the_checkers_filter(k):
    reads = mixed_reads(k, k)
    bases, offs = util.to_batch(reads)
    select = np.random.default_rng(100 + k).random(len(reads)) < 0.6
    for sel in (None, select):
        f = ob.Bloom(k)
        fed = f.index(bases, offs, None if sel is None else util.bits_from_bools(sel))
        want = fb.bits_of_reference_bytes(k, f.bytes())
        assert int(np.unpackbits(f.bytes()).sum()) == want.size
        f.close()
        got = fb.expected_bits(k, reads, sel)
        assert fed > 0 and got.size > 0
        assert got.dtype == np.uint64 and np.all(got[1:] > got[:-1])
        assert fb.difference(got, want, k) is None, fb.difference(got, want, k)
    assert fb.expected_bits(k, [], None).size == 0 and fb.expected_bits(k, reads, np.zeros(len(reads), dtype=bool)).size == 0


@pytest.mark.parametrize("k", list(range(17, 39)))
def test_psi_mirror_is_injective_and_pairs_the_strands_on_samples(k):
    """beyond the exhaustive k <= 16 of test_psi_layout.py: 10^5 random keys, the plane's first and last key, self-paired keys"""
    rng = np.random.default_rng(k)
    mask = np.uint64((1 << k) - 1)
    h = k >> 1
    keys = [rng.integers(0, 1 << k, size=100000, dtype=np.uint64), np.array([0, (1 << k) - 1], dtype=np.uint64)]
    planted = 0
    if k % 2 == 0:                                               # T(key) == key: the upper half is the complemented reverse of the lower
        low = np.concatenate([rng.integers(0, 1 << h, size=2000, dtype=np.uint64), np.array([0, (1 << h) - 1], dtype=np.uint64)])
        keys.append((((~brev(low, h)) & np.uint64((1 << h) - 1)) << np.uint64(h)) | low)
        planted = np.unique(low).size
    keys = np.unique(np.concatenate(keys))
    T = (~brev(keys, k)) & mask
    a, selfp = psi(keys, k)
    a = a.astype(np.uint64)
    assert np.all(a <= mask)
    assert np.unique(a).size == keys.size                       # injective on the sample ...
    aT = psi(T, k)[0].astype(np.uint64)
    both = np.unique(np.concatenate([keys, T]))
    assert np.unique(psi(both, k)[0]).size == both.size         # ... and on the sample with its partners
    assert np.array_equal(selfp, T == keys)
    assert int(selfp.sum()) >= planted >= (450 if k % 2 == 0 else 0) and (k % 2 == 0 or not selfp.any())
    assert np.array_equal(aT[~selfp], a[~selfp] ^ np.uint64(1))


@pytest.mark.parametrize("k", [1, 4, 5, 20, 34, 38])
def test_difference_reports_planted_bits(k):
    last = (1 << k) - 1
    rng = np.random.default_rng(k)
    body = rng.integers(1, max(last, 2), size=300, dtype=np.uint64) if last > 2 else np.zeros(0, dtype=np.uint64)
    body = body[(body > 0) & (body < last)]
    want = np.unique(np.concatenate([fb.words_of(p, body) for p in range(4)]))
    assert fb.difference(want, want, k) is None
    assert fb.difference(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64), k) is None
    for plane in range(4):
        for address in (0, last):
            planted = fb.words_of(plane, [address])
            text = f"plane {'ABCD'[plane]} address {address:#x}"
            more = np.unique(np.concatenate([want, planted]))
            msg = fb.difference(more, want, k)                   # one extra bit
            assert msg is not None and "1 extra bits" in msg and "missing" not in msg and text in msg, msg
            msg = fb.difference(want, more, k)                   # one missing bit
            assert msg is not None and "1 missing bits" in msg and "extra" not in msg and text in msg, msg
            if plane:
                assert f"key {address:#x}" in msg
            if k >= 20:
                assert f"bucket {(plane << (k - 19)) | (address >> 19)}" in msg, msg
            other = fb.words_of((plane + 1) % 4, [last - address])
            msg = fb.difference(np.unique(np.concatenate([want, planted])), np.unique(np.concatenate([want, other])), k)
            assert "1 extra bits" in msg and "1 missing bits" in msg
    # what no filter of this k can hold, repeats, disorder
    assert "outside" in fb.difference(fb.words_of(1, [last + 1]), np.zeros(0, dtype=np.uint64), k)
    assert "outside" in fb.difference(fb.words_of(4, [0]), np.zeros(0, dtype=np.uint64), k)
    two = fb.words_of(2, [0, 0])
    assert "not sorted" in fb.difference(two, two[:1], k)
