"""The read sets of the narrow-table hit profile's tests (test_gpu_hit_profile_slice.py on the GPU, test_hit_profile_slice_cpu.py through
the CPU checker alone): generators only, importable without a GPU, every case seeded and cached so that both files see the same reads.

The planted sets, the saturation set, the edge set and the hit model are hit_profile_wide_sets' own, the palindrome and `greedy`
hit_profile_group_sets'.  As there, max_kmer = 1 makes every chunk ONE read; here the index sets are laid out as [chunk read, dropped
read] * n with chunk reads of plain ACGT, so a set has EXACTLY n chunk filters and the tests assert the number."""
import numpy as np

import util
from hit_profile_group_sets import greedy, planted_palindrome, rand   # noqa: F401
from hit_profile_wide_sets import PLANTED_CHUNKS, PLANTED_KS, edge_set, hit_model, one_read_chunks, planted, random_case, saturation   # noqa: F401

# ---- 1. every instantiation, the word and pass edges: (k, L, chunks, slice_words, gw, passes) ---------------------------------------
ROWS = [
    (12, 40, 20, 0, 1, 1),
    (14, 60, 33, 0, 2, 1),               # one chunk in the second word
    (16, 80, 100, 0, 4, 1),
    (21, 150, 200, 0, 8, 1),
    (13, 50, 257, 0, 8, 2),              # the second pass holds one chunk
    (15, 90, 70, 1, 1, 3),               # the last pass holds 6 of 32
    (24, 60, 140, 8, 4, 2),              # slice_words = 8 clamped to 4 by the 1 GiB of tables; no checker: its filters are too large
]
ROW_T = 8
ROW_QUERIES = 1200
CHECKER_MAX_K = 21
_ROW_SETS = {}


def plan(n_chunks, k, slice_words=0):
    """(gw, passes) as the library plans its narrow tables: option slice_words or the chunk count, the four tables within 1 GiB"""
    gw = slice_words or (8 if n_chunks > 128 else 4 if n_chunks > 64 else 2 if n_chunks > 32 else 1)
    while gw > 1 and ((16 * gw) << k) > (1 << 30):
        gw //= 2
    return gw, -(-n_chunks // (32 * gw))


def table_bytes(k, gw):
    """the four tables of one table set; the staging planes of 32 * gw chunks are as large (ensure_slice_buffers)"""
    return ((4 * gw) << k) * 4


def row_set(k, L, n_chunks):
    """-> (index reads: n_chunks chunk reads without N, each followed by the read the planner drops; ROW_QUERIES related query reads)"""
    key = (k, L, n_chunks)
    if key not in _ROW_SETS:
        rng = np.random.default_rng(57 * k + n_chunks)
        idx = [rand(rng, L) for _ in range(2 * n_chunks)]
        _ROW_SETS[key] = (idx, util.related_reads(rng, idx[::2], ROW_QUERIES, L, L, share=0.5, n_rate=0.002))
    return _ROW_SETS[key]


# ---- 2. the two lower bounds --------------------------------------------------------------------------------------------------------
BOUNDS_K, BOUNDS_CHUNKS = 20, 70
_BOUNDS = {}


def bounds_set(k=BOUNDS_K):
    """-> (index, search, expected counts, names), max_kmer = 1, BOUNDS_CHUNKS chunks.  `ones_everywhere`: every chunk and strand that
    hits the read does so in ONE block of window ends (counter 1: the count is 1 and nothing is replayed); `blocks_i_and_i_plus_2`: one
    chunk hits in blocks 0 and 2 of the forward strand and nowhere between (counter 2, count 2); `adjacent_blocks_apart`: blocks 1 and 2
    with windows that do not overlap (counter 2, count 2, beside `overlap` of the planted set, counter 2 and count 1)"""
    if k not in _BOUNDS:
        rng = np.random.default_rng(4100 + k)
        L = 150
        chunks, search, exp, names = {}, [], [], []
        x = rand(rng, L)
        chunks[3] = [x[10:10 + k], x[12:12 + k]]                         # two windows of block 0: they overlap
        chunks[40] = [util.revcomp(x[70:70 + k])]
        chunks[41] = [x[100:100 + k]]
        search.append(x), exp.append(1), names.append("ones_everywhere")
        x = rand(rng, L)
        chunks[7] = [x[5:5 + k], x[2 * k + 3:3 * k + 3]]
        search.append(x), exp.append(2), names.append("blocks_i_and_i_plus_2")
        x = rand(rng, L)
        chunks[69] = [util.revcomp(x[k + 1:2 * k + 1]), util.revcomp(x[3 * k - 1:4 * k - 1])]
        search.append(x), exp.append(2), names.append("adjacent_blocks_apart")
        search.append(rand(rng, L)), exp.append(0), names.append("nothing")
        _BOUNDS[k] = (one_read_chunks(rng, k, chunks, BOUNDS_CHUNKS), search, exp, names)
    return _BOUNDS[k]


# ---- 3. selections and edges: the edge set cut to 200 chunks ---------------------------------------------------------------------------
EDGE_K, EDGE_CHUNKS = 14, 200


def edge_cut():
    """-> (index reads of about EDGE_CHUNKS chunks, 1 200 query reads of 60 bases, 600 ragged reads of 5..150 bases)"""
    index, fixed, ragged = edge_set()[:]
    return index[:2 * EDGE_CHUNKS], fixed, ragged


# ---- 6. randomised --------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(700, 720))         # (k, max_kmer) of a seed: random_case, hit_profile_wide_sets' own
