"""The read sets of the wide-row hit profile's tests (test_gpu_hit_profile_wide.py on the GPU, test_hit_profile_wide_cpu.py through the
CPU checker alone): generators only, importable without a GPU, every case seeded and cached so that both files see the same reads.

max_kmer = 1 (the library's test hook and the checker's twin of it) makes every chunk ONE read: a chunk is full with its first k-mer,
and the read fetched when it closes is dropped (index_reads.h:49-61).  An index set laid out as [chunk read, dropped read] * n has
exactly n chunk filters when every chunk read holds a k-mer; `one_read_chunks` writes a chunk's planted k-mers into one read, joined
by N, so that no k-mer spans two of them."""
import numpy as np

import util
from hit_profile_group_sets import rand

# ---- 1. every instantiation: (k, L, chunks, slice_wide_words, instantiation) ----------------------------------------------------
ROWS = [
    (12, 40, 300, 0, "8x1"),
    (14, 60, 1500, 0, "16x1"),
    (16, 80, 3000, 0, "32x1"),
    (15, 90, 6000, 0, "64x1"),
    (13, 50, 9000, 0, "64x2"),
    (16, 80, 2900, 48, "16x1"),          # 12 groups of 256 chunks in two passes of six
    (21, 150, 700, 8, "8x1"),            # configs[4]'s k and read length, three passes of one group
]
ROW_T = 8
ROW_QUERIES = 1200
CHECKER_MAX_CHUNKS = 1500                # rows of at most this many chunks also meet the CPU checker, t = 1..4
_ROW_SETS = {}


def row_set(k, L, n_chunks):
    """-> (index reads, query reads)"""
    key = (k, L, n_chunks)
    if key not in _ROW_SETS:
        rng = np.random.default_rng(91 * k + n_chunks)
        idx = util.random_reads(rng, 2 * n_chunks, L, L, n_rate=0.002)
        _ROW_SETS[key] = (idx, util.related_reads(rng, idx, ROW_QUERIES, L, L, share=0.5, n_rate=0.002))
    return _ROW_SETS[key]


def passes_of(n_chunks, cap_words):
    """(passes, words per row that hold chunks, instantiation) as the library plans its wide rows when the table budget is no limit"""
    groups = -(-n_chunks // 256)
    cap = min(512, cap_words) if cap_words else 512
    passes = -(-groups * 8 // cap)
    nw = -(-groups // passes) * 8
    pieces = nw // 4
    return passes, nw, f"{8 if pieces <= 8 else 16 if pieces <= 16 else 32 if pieces <= 32 else 64}x{1 if pieces <= 64 else 2}"


# ---- 2. planted reads --------------------------------------------------------------------------------------------------------------
PLANTED_CHUNKS = 700                     # with slice_wide_words = 8: three passes of 256 chunks
PLANTED_KS = [20, 21]
_PLANTED = {}


def one_read_chunks(rng, k, chunks, n_chunks):
    """chunks: {chunk number: [k-mers]} -> index reads for max_kmer = 1: chunk c's filter holds exactly its k-mers (the others a
    random read's)"""
    index = []
    for c in range(n_chunks):
        index.append(b"N".join(chunks[c]) if chunks.get(c) else rand(rng, k + 10))
        index.append(rand(rng, k + 3))                          # the look-ahead read the planner drops
    return index


def planted(k):
    """-> (index, search, expected hit counts, names): every search read has a designed count; max_kmer = 1, PLANTED_CHUNKS chunks"""
    if k in _PLANTED:
        return _PLANTED[k]
    rng = np.random.default_rng(700 + k)
    chunks, search, exp, names = {}, [], [], []
    L = 150

    def fw(x, s):
        return x[s:s + k]

    def rc(x, s):
        return util.revcomp(x[s:s + k])

    def case(name, read, count, plants):
        for c, kmers in plants.items():
            chunks.setdefault(c, []).extend(kmers)
        search.append(read), exp.append(count), names.append(name)

    # two full hits in adjacent blocks of window ends whose windows overlap (starts k - 3 and k + 2): the bound is 2, the count 1
    x = rand(rng, L)
    case("overlap_then_two", x, 2, {5: [fw(x, k - 3), fw(x, k + 2)], 9: [fw(x, 60), fw(x, 100)]})
    x = rand(rng, L)
    case("overlap_alone", x, 1, {6: [fw(x, k - 3), fw(x, k + 2)]})
    x = rand(rng, L)
    case("forward_1_reverse_3", x, 3, {7: [fw(x, 0), rc(x, 30), rc(x, 60), rc(x, 100)]})
    x = rand(rng, L)
    case("forward_2_reverse_2_apart", x, 2, {11: [fw(x, 3), fw(x, 70)], 13: [rc(x, 30), rc(x, 110)]})
    # a hit window cut by an N: the other plant alone counts
    x = rand(rng, L)
    cut = bytearray(x)
    cut[45] = ord("N")
    case("cut_by_n", bytes(cut), 1, {15: [fw(x, 40), fw(x, 90)]})
    case("not_cut", x, 2, {})
    # the first window, and the last one: it ends in the last, partial block of window ends
    x = rand(rng, L)
    assert (L - k + 1) % k != 0
    case("first_and_last_window", x, 2, {17: [fw(x, 0), fw(x, L - k)]})
    x = rand(rng, L)
    case("last_window_reverse", x, 1, {19: [rc(x, L - k)]})
    # the passes (256 chunks each at slice_wide_words = 8): the best chunk in the last pass, in the first, an equal count later
    x = rand(rng, L)
    case("best_in_last_pass", x, 3, {21: [fw(x, 10)], 600: [fw(x, 10), fw(x, 50), fw(x, 100)]})
    x = rand(rng, L)
    case("best_in_first_pass", x, 3, {23: [rc(x, 10), rc(x, 50), rc(x, 100)], 300: [rc(x, 50)], 601: [fw(x, 10)]})
    x = rand(rng, L)
    case("equal_in_later_passes", x, 2, {25: [fw(x, 10), fw(x, 50)], 301: [fw(x, 80), rc(x, 20)], 650: [rc(x, 20), rc(x, 100)]})
    # more blocks with a hit than the counter holds (saturation), overlapping so that the count stays below
    x = rand(rng, L)
    case("saturated_bound_count_2", x, 2, {27: [fw(x, k - 2), fw(x, k + 1), fw(x, 2 * k), fw(x, 3 * k - 5)]})
    case("nothing", rand(rng, L), 0, {})
    case("shorter_than_k", rand(rng, k - 1), 0, {})
    index = one_read_chunks(rng, k, chunks, PLANTED_CHUNKS)
    _PLANTED[k] = (index, search, exp, names)
    return _PLANTED[k]


def saturation(k):
    """-> (index, search, len // k): an index read is its own chunk; its copy and its reverse complement have len // k hits there"""
    rng = np.random.default_rng(900 + k)
    x = rand(rng, 150)
    index = []
    for c in range(12):
        index += [x if c == 4 else x[:2 * k + 1] if c == 2 else rand(rng, 60), rand(rng, k + 3)]
    return index, [x, util.revcomp(x), x[:100], rand(rng, 150)], 150 // k


# ---- 3. selections and edges ----------------------------------------------------------------------------------------------------
EDGE_K, EDGE_CHUNKS = 14, 400
_EDGE = {}


def edge_set():
    """-> (index reads, 1 200 query reads of 60 bases, 600 ragged reads of 5..150 bases)"""
    if not _EDGE:
        rng = np.random.default_rng(1414)
        idx = util.random_reads(rng, 2 * EDGE_CHUNKS, 60, 60, n_rate=0.002)
        fixed = util.related_reads(rng, idx, 1200, 60, 60, share=0.5, n_rate=0.002)
        ragged = util.related_reads(rng, idx, 600, 5, 150, share=0.6, n_rate=0.01)
        _EDGE["s"] = (idx, fixed, ragged)
    return _EDGE["s"]


# ---- 4. randomised -----------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(500, 520))


def random_case(seed):
    """-> (k, max_kmer) of scenarios.Scenario(seed, n_scale = 4); one read per chunk only where the checker's filters are small"""
    k = 12 + (seed * 7) % 13
    return k, ([1, 40, 150][seed % 3] if k <= 20 else [40, 150][seed % 2])


# ---- the hits of a window in a chunk filter, in numpy (the filter's four planes are exact key sets) ------------------------------------
def hit_model(k, chunk_reads):
    """-> f(read) = {(chunk, strand): ascending window end positions of `read` whose four keys are all in that chunk's filter}"""
    import oracle_binding as ob
    n_chunks = len(chunk_reads)
    planes = [[] for _ in range(4)]
    for c, r in enumerate(chunk_reads):
        keys, _ = ob.keys_of_read(r, k)
        for p in range(4):
            planes[p].append(keys[:, p].astype(np.int64) * n_chunks + c)
    planes = [np.unique(np.concatenate(p)) if p else np.zeros(0, np.int64) for p in planes]
    return lambda rd: _window_hits(k, n_chunks, planes, rd)


def _window_hits(k, n_chunks, planes, read):
    import oracle_binding as ob
    out = {}
    for strand in (0, 1):
        keys, pos = ob.keys_of_read(read, k, reverse=bool(strand))
        if not len(pos):
            continue
        # plane A decides the candidates (window, chunk): the chunks whose plane holds the window's key
        ka = keys[:, 0].astype(np.int64) * n_chunks
        lo, hi = np.searchsorted(planes[0], ka), np.searchsorted(planes[0], ka + n_chunks)
        for w in np.nonzero(hi > lo)[0]:
            for c in (planes[0][lo[w]:hi[w]] - ka[w]).tolist():
                if all(_has(planes[p], int(keys[w, p]) * n_chunks + c) for p in (1, 2, 3)):
                    out.setdefault((c, strand), []).append(int(pos[w]))
    return out


def _has(sorted_arr, v):
    i = int(np.searchsorted(sorted_arr, v))
    return i < len(sorted_arr) and int(sorted_arr[i]) == v
