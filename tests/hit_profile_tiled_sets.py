"""The read sets of the tiled hit profile's tests (test_gpu_hit_profile_tiled.py on the GPU, test_hit_profile_tiled_cpu.py through the
CPU checker alone): generators only, importable without a GPU, every case seeded and cached so that both files and every
parametrised case see the same reads.

The tiled profile (option profile_tiled = 2; capi/profile.hpp, hit_profile_tiled.hpp) takes passes of one or two chunk filters over a
set with 25 <= k <= 34 and 1..255 windows per read; its replay keeps a mask bit per window, 32 to a word, 2 / 3 / 4 / 6 / 8 words by
the set's longest read.  The sets here put hits where that layout can go wrong."""
import numpy as np

import util
from hit_profile_group_sets import chunked, greedy, planted_slots, planted_states, rand  # noqa: F401  (the GPU file takes them from here)

# ---- 1. window sweep ---------------------------------------------------------------------------------------------------------------
WINDOWS = (1, 32, 33, 65, 97, 129, 193, 255)                   # windows per read: reads of k + W - 1 bases
MASK_WORDS = {1: 2, 32: 2, 33: 2, 65: 3, 97: 4, 129: 6, 193: 8, 255: 8}
SWEEP_KS = (25, 32)
WIDE_K = 33                                                      # 64-bit keys
_SWEEPS = {}


def mask_words(n_windows):
    """mask words of the replay for a set whose longest read has n_windows windows (mask_words_of, capi/search_dispatch.hpp)"""
    return 2 if n_windows <= 64 else 3 if n_windows <= 96 else 4 if n_windows <= 128 else 6 if n_windows <= 192 else 8


def window_plants(k, W):
    """window starts planted into one strand of one filter, for a read of W windows: the first and the last window, bits 31 / 32 and
    63 / 64 of the mask words, k - 1 apart (an overlap: one hit) and k apart (adjacent: two)"""
    pats = [(0,), (W - 1,), (31,), (32,), (31, 32), (63,), (64,), (63, 64), (5, 5 + k - 1), (5, 5 + k), (31, 31 + k), (32 - k, 32), (32 - k + 1, 32),
            (64 - k, 64), (W - 1 - k, W - 1), (W - k, W - 1), (0, k, 2 * k), (0, k - 1, 2 * k - 2), (31, 63, 95), (96 - k, 96, 127, 128), (160, 191, 192, 254),
            (W - 1 - 2 * k, W - 1 - k, W - 1)]
    out = []
    for p in pats:
        if all(0 <= s < W for s in p) and p not in out:
            out.append(p)
    return out


def window_sweep(k, n_chunks):
    """-> (index, max_kmer, {W: (reads, expected bytes)}): per W a set of reads of k + W - 1 bases; read by read the plants of one
    pattern on the forward strand in the first chunk filter, of one on the reverse strand in the last, of two patterns at once (the
    byte is the larger count), and reads with none"""
    key = (k, n_chunks)
    if key in _SWEEPS:
        return _SWEEPS[key]
    rng = np.random.default_rng(7000 + 10 * k + n_chunks)
    chunks = [[] for _ in range(n_chunks)]
    sets = {}
    for W in WINDOWS:
        reads, exp = [], []
        pats = window_plants(k, W)
        for i, p in enumerate(pats):
            q = pats[(i + 1) % len(pats)]
            for fw, rv in ((p, ()), ((), p), (p, q), (q, p)):
                x = rand(rng, k + W - 1)
                chunks[0] += [x[s:s + k] for s in fw]
                chunks[-1] += [util.revcomp(x[s:s + k]) for s in rv]
                reads.append(x)
                exp.append(max(greedy(fw, k), greedy(rv, k)))
        reads.append(rand(rng, k + W - 1))
        exp.append(0)
        sets[W] = (reads, exp)
    for c in chunks:                                             # (no chunk without a read)
        c.append(rand(rng, k + 2))
    index, max_kmer = chunked(rng, k, chunks)
    _SWEEPS[key] = (index, max_kmer, sets)
    return _SWEEPS[key]


CHECKED_SWEEPS = ((25, 2), (32, 1), (33, 2))                    # the sweeps whose bytes the GPU test also holds against the checker's tags


# ---- 2. filter and strand independence ------------------------------------------------------------------------------------------------
def independence_sets(k=25):
    """-> [(name, index, search, expected bytes, max_kmer, n_chunks)]: planted_states (among them the read with F = 1, R = 3 in filter
    0 and F = 2 in filter 1: 3) and planted_slots with two chunks"""
    return [("states",) + tuple(planted_states(k)), ("slots",) + tuple(planted_slots(k, n_chunks=2))]


# ---- 3. heavy scans ------------------------------------------------------------------------------------------------------------------
HEAVY_K = 26                                                     # reads of 280 bases have 255 windows
_HEAVY = {}


def heavy_sets(k=HEAVY_K):
    """-> (index, max_kmer, {L: (reads, expected bytes at max_hits = 255)}) for L = 100 and 280: search reads copied from index reads
    of two chunks — every window of a copy is a lane-a candidate on one strand (more than 20: a heavy scan), the other strand and
    the other filter hold a planted hit or nothing"""
    if k in _HEAVY:
        return _HEAVY[k]
    rng = np.random.default_rng(2600 + k)
    chunks, sets = [[], []], {}
    for L in (100, 280):
        full = (L - k) // k + 1                                  # greedy over every window of the read
        a, b, c = rand(rng, L), rand(rng, L), rand(rng, L)
        chunks[0] += [a, c[:L // 2]]
        chunks[1] += [b, util.revcomp(c[L // 2 - k + 1:])]       # c: its first half forward in filter 0, the rest reverse in filter 1
        half_f, half_r = (L // 2 - k) // k + 1, (L - (L // 2 - k + 1) - k) // k + 1
        x = rand(rng, L)                                         # a light read beside them: one planted hit on each strand
        chunks[0].append(x[3:3 + k])
        chunks[1].append(util.revcomp(x[L - k:]))
        reads = [a, util.revcomp(a), b, util.revcomp(b), c, util.revcomp(c), a[:L - 7] + rand(rng, 7), x, rand(rng, L)]
        exp = [full, full, full, full, max(half_f, half_r), max(half_f, half_r), (L - 7 - k) // k + 1, 1, 0]
        sets[L] = (reads, exp)
    index, max_kmer = chunked(rng, k, chunks)
    _HEAVY[k] = (index, max_kmer, sets)
    return _HEAVY[k]


# ---- 4. piece edges, unclean reads, folds ----------------------------------------------------------------------------------------------
PIECE_SIZES = (1, 255, 256, 257, 513)
_RELATED = {}


def related_case(k, n_chunks, n_search, seed=0, len_lo=20, len_hi=200):
    """-> (index, search, max_kmer): n_chunks chunks of four clean 110-base reads; n_search related reads of len_lo..len_hi bases with N
    runs and lower-case bases, some shorter than k; the first is a clean stretch of an index read"""
    key = (k, n_chunks, n_search, seed, len_lo, len_hi)
    if key not in _RELATED:
        rng = np.random.default_rng(90000 + 1000 * k + 10 * n_chunks + seed)
        L, per_chunk = 110, 4
        index = [rand(rng, L) for _ in range(n_chunks * (per_chunk + 1))]
        search = [r if len(r) else b"A" for r in util.related_reads(rng, index, n_search, len_lo, len_hi, share=0.6, n_rate=0.01, lower_rate=0.3)]
        search[0] = index[0][5:105]                               # (a set of one read has a k-mer, and a hit)
        _RELATED[key] = (index, search, per_chunk * (L - k + 1))
    return _RELATED[key]


def piece_selection(n):
    """a selection that crosses the piece boundaries at reads 256 and 512"""
    sel = np.zeros(n, dtype=bool)
    sel[::3] = True
    sel[250:262] = True
    sel[505:520] = True
    if n > 256:
        sel[255], sel[256] = True, False                         # the last read of piece 0 without the first of piece 1
    return sel


# ---- 5. randomised -------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(400, 410))
RANDOM_MAX_KMER = 20


def random_k(seed):
    return (25, 31, 32)[seed % 3]
