"""The set bits a filter slot must hold, exactly, at every k (test_gpu_filter_bits.py on the GPU, test_filter_bits_cpu.py here):
no GPU, TEST INFRASTRUCTURE ONLY.

`Context.filter_set_bits` lists the set bits of a slot AS STORED, one np.uint64 word per bit: (plane << 56) | address within the
plane — plane 0 = A, whose bit of `key` sits at psi_a(key); planes 1..3 = B, C, D at the key itself.  The device applies no psi_a
to make that list; the side computed here goes through the numpy mirror `psi` (test_psi_layout.py, the one copy), so a psi_a that
is wrong on the device shows, which it does not where the device's own psi_a translates the export back.

expected_bits             the words of the forward keys of `reads` (ob.keys_of_read, as BloomFilter::feed), sorted, unique
bits_of_reference_bytes   the same form from a filter in the reference's byte layout (small k)
difference                None, or what differs: counts, the first extra and missing bit decoded, the build's bucket"""
import numpy as np

import oracle_binding as ob
from test_psi_layout import psi

PLANE_SHIFT = 56
ADDRESS_MASK = np.uint64((1 << PLANE_SHIFT) - 1)
TILE_BITS = 19                    # index_part.hpp: a bucket of the bucketed build is a tile of 2^19 bits of one plane


def address_a(keys, k):
    """where plane A holds lane a of `keys`: psi for k >= 2, the key itself at k = 1 (as export_reference_kernel reads it)"""
    keys = np.asarray(keys, dtype=np.uint64)
    return psi(keys, k)[0].astype(np.uint64) if k >= 2 and keys.size else keys


def words_of(plane, addresses):
    return (np.uint64(plane) << np.uint64(PLANE_SHIFT)) | np.asarray(addresses, dtype=np.uint64)


def expected_bits(k, reads, select=None):
    """sorted unique words of the bits that indexing `reads` (those of `select`, bools, when given) sets in a zeroed filter"""
    if select is not None:
        assert len(select) == len(reads)
        reads = [r for r, s in zip(reads, select) if s]
    keys = [ob.keys_of_read(r, k)[0] for r in set(reads)]
    keys = np.concatenate(keys) if keys else np.zeros((0, 4), dtype=np.uint64)
    if not len(keys):
        return np.zeros(0, dtype=np.uint64)
    planes = [np.unique(keys[:, p]) for p in range(4)]
    return np.unique(np.concatenate([words_of(0, address_a(planes[0], k))] + [words_of(p, planes[p]) for p in (1, 2, 3)]))


def bits_of_reference_bytes(k, data):
    """the same words from 2^(k-1) bytes of the reference's layout: byte key / 2, even keys 0x80/40/20/10, odd keys 0x08/04/02/01
    for lanes a/b/c/d (bloom_filter.h:63-70,114-117)"""
    data = np.asarray(data, dtype=np.uint8)
    assert data.size == int(2 ** (k - 1)), (k, data.size)
    at = np.flatnonzero(data)
    bit = np.flatnonzero(np.unpackbits(data[at]))                # bit j of a byte, most significant first: 0..3 even key, 4..7 odd key
    j = (bit & 7).astype(np.uint64)
    keys = (at[bit >> 3].astype(np.uint64) << np.uint64(1)) | (j >> np.uint64(2))
    plane = j & np.uint64(3)
    out = [words_of(0, address_a(keys[plane == 0], k))] + [words_of(p, keys[plane == p]) for p in (1, 2, 3)]
    return np.unique(np.concatenate(out))


def decode(word, k):
    """'plane B address 0x.. (key 0x.., bucket n)' of one word"""
    word = int(word)
    plane, address = word >> PLANE_SHIFT, word & int(ADDRESS_MASK)
    text = f"plane {'ABCD'[plane] if plane < 4 else plane} address {address:#x}"
    if 1 <= plane <= 3:
        text += f" = key {address:#x}"
    if k >= TILE_BITS + 1 and plane < 4 and address < (1 << k):
        text += f", bucket {(plane << (k - TILE_BITS)) | (address >> TILE_BITS)}"
    return text


def difference(got, want, k):
    """None when `got` holds exactly the words of `want`, else a message: how many bits are extra and how many missing, the first of
    each as (plane, address, key of B / C / D) and the build's bucket (plane << (k - 19)) | (address >> 19) for k >= 20"""
    got, want = np.asarray(got, dtype=np.uint64), np.asarray(want, dtype=np.uint64)
    problems = []
    if got.size and np.any(got[1:] <= got[:-1]):
        problems.append("the list is not sorted and free of repeats")
    bad = got[((got >> np.uint64(PLANE_SHIFT)) > np.uint64(3)) | ((got & ADDRESS_MASK) >= np.uint64(1 << k))]
    if bad.size:
        problems.append(f"{bad.size} words outside the four planes of 2^{k} bits, first {int(bad[0]):#x}")
    extra, missing = np.setdiff1d(got, want), np.setdiff1d(want, got)
    if extra.size:
        problems.append(f"{extra.size} extra bits, first {decode(extra[0], k)}")
    if missing.size:
        problems.append(f"{missing.size} missing bits, first {decode(missing[0], k)}")
    if not problems:
        return None
    return f"k = {k}: {got.size} bits set, {want.size} expected; " + "; ".join(problems)
