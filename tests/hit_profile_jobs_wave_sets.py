"""The read sets of the wave-per-read many-job hit profile's tests (test_gpu_hit_profile_jobs_wave.py on the GPU,
test_hit_profile_jobs_wave_cpu.py through the CPU checker alone): generators only, importable without a GPU, every case seeded and
cached so that both files see the same reads.

hits_jobs_wave_kernel (hit_profile_jobs.hpp) walks a read in BLOCKS of 64 consecutive window starts, the per-slot state carried from
block to block.  The block fixtures plant hits around the block bounds of a read of 200 bases (k = 20: 181 windows, blocks 0-63,
64-127, 128-180) so that a state not carried, a walk or a block loop that ends with the first decided job, a sum over a job's slots and a
block bound off by one each give another byte than the design's.  As in hit_profile_jobs_sets.py the bytes a test compares with are
never the design's: `checker_bytes` derives min(cap, count) per job and read from the CPU checker, one run per job and t; the CPU file
proves that the checker's bytes ARE the design's for the planted reads.

A read of 200 bases holds at most ten non-overlapping 20-mers, so the checker at t = 1..10 gives every count exactly."""
import os

import numpy as np

import hit_profile_group_sets as gs
import hit_profile_jobs_sets as js
import util

K = js.K
L = 200
T_TOP = L // K                                  # no read of L bases has more non-overlapping k-mers
BLOCK = 64                                      # window starts per block of the wave kernels

plant = js.plant

_FIXTURES = {}
NAMES = ("carry", "stop_far", "max_far", "edge")


def fixture(name, strand):
    """-> dict(jobs = [index reads], caps, search, max_kmer, chunks = [chunk filters per job], design = {job: bytes of the first reads
    of the search set}): one commet_index_many_and_profile call"""
    key = (name, strand)
    if key in _FIXTURES:
        return _FIXTURES[key]
    rng = np.random.default_rng(4000 + 10 * NAMES.index(name) + strand)
    r = gs.rand(rng, L)
    max_kmer = 0
    search = [r]
    if name == "carry":
        # job 0: hits at 50, 66, 86.  50 is taken in block 0 and forbids 66, the third window of block 1; 86 is taken: 2.  A next_free
        # that is not carried into block 1 takes 66 and then 86: 3.  job 1: hits at 64 .. 104, taken at 64, 84, 104: 3; one next_free
        # for all slots leaves it 70 and 90: 2
        jobs = [[plant(r[50:70], strand), plant(r[66:86], strand), plant(r[86:106], strand)], [plant(r[64:124], strand)]]
        caps, chunks, design = [255, 255], [1, 1], {0: [2], 1: [3]}
    elif name == "stop_far":
        # job 0 reaches its cap of 1 at window 0, in block 0; job 1's three hits (130, 150, 170) lie in block 2: a walk or a block
        # loop that ends when ANY job is decided gives 0
        jobs = [[plant(r[0:30], strand)], [plant(r[130:190], strand)]]
        caps, chunks, design = [1, 3], [1, 1], {0: [1], 1: [3]}
    elif name == "max_far":
        # ONE job of two chunks: two hits in the first chunk filter (block 0), three in the second (blocks 1 and 2): max 3, a sum over
        # the job's slots gives 5.  A second job (a piece of another read, one chunk) makes the call share a pass
        other = gs.rand(rng, L)
        index, max_kmer = gs.chunked(rng, K, [[plant(r[0:40], strand)], [plant(r[100:160], strand)]])
        jobs = [index, [plant(other[0:25], strand)]]
        caps, chunks, design = [255, 255], [2, 1], {0: [3], 1: [0]}
    else:
        # search reads of 63, 64 and 65 windows (the 65th alone in block 1); job 0 holds the last window of each, job 1 the first:
        # a block bound off by one loses a hit
        ends = [gs.rand(rng, K + n) for n in (BLOCK - 2, BLOCK - 1, BLOCK)]
        search = ends + [r]
        jobs = [[plant(e[-K:], strand) for e in ends], [plant(e[:K], strand) for e in ends]]
        caps, chunks, design = [255, 255], [1, 1], {0: [1, 1, 1], 1: [1, 1, 1]}
    f = dict(jobs=jobs, caps=caps, search=search + js.edge_reads(rng, r), max_kmer=max_kmer, chunks=chunks, design=design)
    assert all(len(x) <= L for x in f["search"])
    _FIXTURES[key] = f
    return f


FIXTURES = [(n, s) for n in NAMES for s in (0, 1)]
_BYTES = {}


def _bytes_of(d, tag, f, t_top):
    out, chunks = [], []
    for j, (index, cap) in enumerate(zip(f["jobs"], f["caps"])):
        counts, c = js.checker_counts(os.path.join(str(d), f"{tag}_j{j}"), K, index, f["search"], f["max_kmer"], t_top)
        out.append(np.minimum(counts, cap).astype(np.uint8))
        chunks.append(c)
    return out, chunks


def checker_bytes(d, name, strand):
    """-> ([min(cap, count) per read of the search set] per job, [chunks per job]) from the checker; made once per fixture"""
    key = (name, strand)
    if key not in _BYTES:
        _BYTES[key] = _bytes_of(d, f"w{name}{strand}", fixture(name, strand), T_TOP)
    return _BYTES[key]


# ---- the auto regime: a ragged set whose longest read has 5000 bases and more (LONG_MIN_MAX_LEN, search_dispatch.hpp) ------------------
AUTO_MIN_MAX_LEN = 5000
AUTO_AT = 76 * BLOCK                            # 4864: the plants start on a block bound beyond base 5000 - 200
AUTO_CAPS = [5, 3]
_AUTO = {}


def auto_fixture():
    """about 20 ragged reads of 200 to 6000 bases.  The longest, x, carries at AUTO_AT the plants of `carry` and one block pair behind
    them those of `stop_far`:
      job 0 (cap 5): carry's 50, 66, 86 -> 2 (3 without the carry), stop_far's near piece -> 1 more: 3
      job 1 (cap 3, reverse complements): carry's 64 .. 104 -> 3: decided there, in front of job 0's last hit; a walk that ends with
      the first decided job leaves job 0 at 2.  stop_far's far piece is job 1's as well and changes nothing
    -> the dict of `fixture`, design for x alone"""
    if _AUTO:
        return _AUTO
    rng = np.random.default_rng(4100)
    x = gs.rand(rng, 6000)
    a, b = AUTO_AT, AUTO_AT + 4 * BLOCK
    jobs = [[x[a + 50:a + 70], x[a + 66:a + 86], x[a + 86:a + 106], x[b:b + 30]],
            [util.revcomp(x[a + 64:a + 124]), util.revcomp(x[b + 130:b + 190])]]
    with_n = bytearray(x[a - 100:b + 300])
    with_n[100 + 90:100 + 91] = b"N"            # inside job 0's window 86 (an N in window 50 would free 66 instead)
    search = [x, gs.rand(rng, 200), x[a - 300:b + 250], util.revcomp(x[a:b + 200]), bytes(with_n), x[a + 40:a + 130].lower(), x[:K - 1], x[a:b]]
    search += [gs.rand(rng, int(n)) for n in rng.integers(200, 4001, size=12)]
    assert AUTO_AT > AUTO_MIN_MAX_LEN - 200 and max(len(s) for s in search) == len(x) >= AUTO_MIN_MAX_LEN
    assert sum(1 for s in search if len(s) >= AUTO_MIN_MAX_LEN) == 1
    _AUTO.update(jobs=jobs, caps=AUTO_CAPS, search=search, max_kmer=0, chunks=[1, 1], design={0: [3], 1: [3]})
    return _AUTO


def auto_bytes(d):
    """the checker at t = 1 .. max(caps): exact for bytes that stop at the caps"""
    if "auto" not in _BYTES:
        _BYTES["auto"] = _bytes_of(d, "wauto", auto_fixture(), max(AUTO_CAPS))
    return _BYTES["auto"]
