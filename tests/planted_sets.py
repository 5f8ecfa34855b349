"""The read sets of the planted tests of the short-read search kernels and of the hit-profile kernels (test_gpu_planted_search.py and
test_gpu_planted_profile.py on the GPU, test_planted_sets_cpu.py through the CPU checker alone): generators only, importable without
a GPU, every case seeded and cached.

Every search read carries a DESIGNED count: the greedy non-overlapping full hits on its better strand in its best chunk filter (the
hit byte of commet_index_and_profile); the read is found at t exactly when count >= t.  test_planted_sets_cpu.py proves design ==
checker for every read of every case, so that the GPU tests may compare with either.

The filter's four keys of a window are plain bit strings of its bases: lane a the high bits (1 for G / T), lane b the low bits (1 for
C / T), c = a ^ b, d = a | b.  A DECOY of a k-mer y is y under a translation of the alphabet that keeps exactly one of the four:

    LO    A<->C, G<->T     keeps a
    HI    A<->G, C<->T     keeps b
    BOTH  A<->T, C<->G     keeps c
    ROT   C->G->T->C       keeps d

With all four decoys of y in one chunk filter, y is a full hit there although y itself was never indexed; with fewer, or with the
four in different filters, y is a candidate in some lanes and a hit in none."""
import itertools

import numpy as np

import util
from hit_profile_group_sets import chunked, greedy, rand

ORDER = ("LO", "HI", "BOTH", "ROT")
DECOY = {"LO": bytes.maketrans(b"ACGT", b"CATG"), "HI": bytes.maketrans(b"ACGT", b"GTAC"),
         "BOTH": bytes.maketrans(b"ACGT", b"TGCA"), "ROT": bytes.maketrans(b"ACGT", b"AGTC")}
KEEPS = {"LO": 0, "HI": 1, "BOTH": 2, "ROT": 3}
FHW = (1, 32, 33, 65, 97, 129, 193, 255)            # first-hit windows: mask words 2, 2, 2, 3, 4, 6, 8, 8
BAD = (ord("N"), ord("n"), ord("R"))
EDGE_P = (30, 31, 32, 33, 63, 64, 95, 96)


def mask_words(fhw):
    return 2 if fhw <= 64 else 3 if fhw <= 96 else 4 if fhw <= 128 else 6 if fhw <= 192 else 8


def lanes(kmer):
    """the four keys of a clean k-mer, forward strand"""
    a = b = 0
    for ch in kmer:
        v = b"ACGT".index(ch)
        a, b = a << 1 | v >> 1, b << 1 | v & 1
    return a, b, a ^ b, a | b


def decoys(kmer, names=ORDER):
    return [kmer.translate(DECOY[n]) for n in names]


def degenerate(kmer):
    """a decoy of it shares more than its one lane (poly-A under ROT, a k-mer of G and T alone under LO, ...)"""
    own = lanes(kmer)
    return any([j for j in range(4) if lanes(kmer.translate(DECOY[n]))[j] == own[j]] != [KEEPS[n]] for n in ORDER)


class _Builder:
    """chunks of index reads, and what was decoyed (the CPU file checks every such k-mer's decoys lane by lane)"""

    def __init__(self, seed, k):
        self.rng = np.random.default_rng(seed)
        self.k = k
        self.chunks = []
        self.decoyed = []

    def chunk(self, c):
        while len(self.chunks) <= c:
            self.chunks.append([])
        return self.chunks[c]

    def put(self, c, window, kind, names=ORDER):
        """kind 0: the window's k-mer, 1: its decoys, 2: its reverse complement, 3: the decoys of that"""
        w = window if kind < 2 else util.revcomp(window)
        if kind & 1:
            assert not degenerate(w), w
            self.chunk(c).extend(decoys(w, names))
            self.decoyed.append(w)
        else:
            self.chunk(c).append(w)

    def planted(self, L, starts, kind, c, bad=(), ghost=False):
        """a random read of L bases with its windows at `starts` planted in chunk c; bad: (position, byte) written over the read
        afterwards; ghost: the last start lies one window past the read's end (the read is cut there).  -> (read, count)"""
        k = self.k
        read = bytearray(rand(self.rng, L + (1 if ghost else 0)))
        own = (lambda w: w) if kind < 2 else util.revcomp      # (the k-mer that put() decoys)
        while kind & 1 and any(degenerate(own(bytes(read[s:s + k]))) for s in starts):      # (one window in a thousand at k = 12)
            read = bytearray(rand(self.rng, L + (1 if ghost else 0)))
        for s in starts:
            self.put(c, bytes(read[s:s + k]), kind)
        for pos, ch in bad:
            read[pos] = ch
        live = [s for s in starts if s + k <= L and not any(s <= pos < s + k for pos, _ in bad)]
        return bytes(read[:L]), greedy(live, k)

    def near_miss(self, L, p, c, i):
        """t = 1's twin: the k-mer at p is indexed with one base changed"""
        k = self.k
        read = rand(self.rng, L)
        w = bytearray(read[p:p + k])
        j = i % k
        w[j] = b"ACGT"[(b"ACGT".index(w[j]) + 1 + i % 3) % 4]
        self.put(c, bytes(w), 0)
        return read, 0

    def index(self, extra=0):
        return chunked(self.rng, self.k, self.chunks, extra=extra)


def _odd_size(b, reads, counts, L):
    """set sizes are no multiple of 64"""
    while len(reads) % 64 == 0:
        reads.append(rand(b.rng, L))
        counts.append(0)


# ---- B, C, D: positions -------------------------------------------------------------------------------------------------------------
def _sweep_reads(b, t, fhw, chunk_of, n0):
    """family B for one (t, fhw): reads of fhw + t k - 1 bases.  -> (reads, counts)"""
    k = b.k
    L = fhw + t * k - 1
    last, pe = L - k, fhw - 1
    reads, counts = [], []

    def add(rc):
        reads.append(rc[0])
        counts.append(rc[1])

    def n():
        return n0 + len(reads)

    for p in range(fhw):                                        # every first window: found; its twin: not
        i = n()
        starts = [p + j * k for j in range(t)]
        add(b.planted(L, starts, i % 4, chunk_of(i)))
        i = n()
        if t == 1:
            add(b.near_miss(L, p, chunk_of(i), i))
        else:
            add(b.planted(L, starts[:-1] + [starts[-1] - 1], i % 4, chunk_of(i)))
    if t >= 2:                                                  # the gap in front of the last hit, in tail requests of W windows
        seen = set()
        for p in sorted({0, max(pe - 1, 0), pe}):
            head = [p + j * k for j in range(t - 1)]
            free = head[-1] + k
            # (... and the read's last window, and the first two windows behind the first-hit ones: where the tail starts)
            for g in [g for W in (16, 32) for g in (0, 1, W - 1, W, W + 1, 2 * W - 1, 2 * W, 3 * W + 5)] + [last - free, fhw - free, fhw - free + 1]:
                if g < 0 or free + g > last or (p, g) in seen:
                    continue
                seen.add((p, g))
                i = n()
                add(b.planted(L, head + [free + g], i % 4, chunk_of(i)))
                i = n()
                add(b.planted(L, head + [free - 1], i % 4, chunk_of(i)))                 # overlaps by one base
                i = n()
                add(b.planted(L, head + [last + 1], i % 4, chunk_of(i), ghost=True))     # ends one base past the read
    return reads, counts


def _edge_reads(b, t, chunk_of, n0, validity=True):
    """families C (strands, palindromes) and D (non-ACGT bases at mask edges).  -> (reads, counts), ragged"""
    k = b.k
    reads, counts = [], []

    def add(rc):
        reads.append(rc[0])
        counts.append(rc[1])

    def n():
        return n0 + len(reads)

    def two_strands(L, fw, rv, c):
        read = rand(b.rng, L)
        for s in fw:
            b.put(c, read[s:s + k], 0)
        for s in rv:
            b.put(c, read[s:s + k], 2)
        return read, max(greedy(fw, k), greedy(rv, k))

    step = k + 2
    for rep in range(3):
        off = (0, 29, 61)[rep]
        L = off + 2 * t * step + k + 3
        fw = [off + j * step for j in range(t - 1)]
        add(two_strands(L, fw, [off + (t - 1) * step], chunk_of(n())))                                 # t - 1 forward + 1 reverse
        add(b.planted(L, [off + j * step for j in range(t)], 2, chunk_of(n())))                        # reverse only
        add(two_strands(L, fw, [off + (t - 1 + j) * step for j in range(t)], chunk_of(n())))           # too few forward, then t reverse
        add(two_strands(L, [off + (t - 1 + j) * step for j in range(t)], fw, chunk_of(n())))
        if k % 2 == 0:                                          # a k-mer that is its own reverse complement: plane A stores it once
            for where in ("alone", "first", "second"):
                c = chunk_of(n())
                half = rand(b.rng, k // 2)
                pal = half + util.revcomp(half)
                assert util.revcomp(pal) == pal
                read = bytearray(rand(b.rng, L))
                at = off + (step if where == "second" else 0)
                other = off + (0 if where == "second" else step)
                read[at:at + k] = pal
                b.put(c, pal, 0)
                starts = [at]
                if where != "alone":
                    b.put(c, bytes(read[other:other + k]), 0)
                    starts.append(other)
                reads.append(bytes(read))
                counts.append(greedy(starts, k))
    if validity:
        for j, p in enumerate(EDGE_P):
            ch = BAD[j % 3]
            L = p + t * (k + 1) + 5
            starts = [p + i * (k + 1) for i in range(t)]
            for bad in ([(p - 1, ch), (p + k, ch)], [(p, ch)], [(p + k - 1, ch)], [(p - 1, ch)], [(p + k, ch)]):
                i = n()
                add(b.planted(L, starts, (i + j) % 4, chunk_of(i), bad=bad))
    return reads, counts


_SWEEPS = {}


def sweep_case(k, t, n_chunks=1, fhws=FHW, per_chunk=0, validity=True):
    """families B, C, D at (k, t).  The plants of read i go to chunk i % n_chunks, or (per_chunk != 0: the small k, where one filter
    would be too dense) to chunk i // per_chunk.  -> dict(k, t, index, max_kmer, n_chunks, sets = {name: (reads, counts)}, decoyed):
    "f<fhw>" a fixed-length set per fhw, "edge" families C and D (ragged), "all" every read of them (ragged)"""
    key = (k, t, n_chunks, tuple(fhws), per_chunk, validity)
    if key in _SWEEPS:
        return _SWEEPS[key]
    b = _Builder(100000 * k + 1000 * t + 10 * n_chunks + per_chunk, k)
    chunk_of = (lambda i: i // per_chunk) if per_chunk else (lambda i: i % n_chunks)
    sets, n0 = {}, 0
    for fhw in fhws:
        reads, counts = _sweep_reads(b, t, fhw, chunk_of, n0)
        _odd_size(b, reads, counts, fhw + t * k - 1)
        sets[f"f{fhw}"] = (reads, np.array(counts))
        n0 += len(reads)
    reads, counts = _edge_reads(b, t, chunk_of, n0, validity)
    _odd_size(b, reads, counts, 3 * k)
    sets["edge"] = (reads, np.array(counts))
    every = [r for s in sets.values() for r in s[0]]
    every_counts = [int(c) for s in sets.values() for c in s[1]]
    _odd_size(b, every, every_counts, k + 1)
    sets["all"] = (every, np.array(every_counts))
    if not per_chunk:
        b.chunk(n_chunks - 1)
    index, max_kmer = b.index()
    _SWEEPS[key] = dict(k=k, t=t, index=index, max_kmer=max_kmer, n_chunks=len(b.chunks), sets=sets, decoyed=b.decoyed)
    return _SWEEPS[key]


# ---- A: the lane ladder ---------------------------------------------------------------------------------------------------------------
def ladder_patterns(n_chunks, light=False):
    """where the four decoys (LO, HI, BOTH, ROT) of a k-mer go: a chunk each, None = not indexed.  Full in one filter: a hit;
    everything else: none.  The anchors are the chunks at the edges of what one pass holds: groups of 2, 4 and 8 slots, the 32-chunk
    words of a bit-sliced row, the 256-chunk groups of the tables.  light (k < 20, where a filter takes a few dozen k-mers before
    it gives accidental hits): fewer splits and slot orders per anchor, spread over the chunks"""
    pats = []
    wanted = (0, 31, 32, 255, 256, n_chunks - 4) if light else \
        (0, 1, 2, 3, 4, 30, 31, 32, 62, 63, 64, 126, 127, 128, 254, 255, 256, n_chunks - 4, n_chunks - 2, n_chunks - 1)
    anchors = sorted({c for c in wanted if 0 <= c < n_chunks})
    for c in anchors[:6] + anchors[-2:]:
        pats.append((c, c, c, c))                               # all four in one filter: found
    for drop in range(4):                                       # the four triples
        c = (5 + 2 * drop) % n_chunks
        pats.append(tuple(None if j == drop else c for j in range(4)))
    c = [(13 + 2 * j) % n_chunks for j in range(3)]
    pats += [(c[0], None, None, None), (c[1], c[1], None, None), (c[2], c[2], c[2], None)]   # 2, 3 and 4 probes per window
    for c in anchors:                                           # two filters: every split, on both sides of every anchor
        if c + 1 < n_chunks:
            for bits in ((3, 5, 1, 8) if light else range(1, 15)):
                pats.append(tuple(c + (bits >> j & 1) for j in range(4)))
    for c in anchors:                                           # four filters: every slot order
        if c + 3 < n_chunks:
            for perm in list(itertools.permutations(range(4)))[::7 if light else 1]:
                pats.append(tuple(c + p for p in perm))
    return pats


_LADDERS = {}
# seeds moved on from an accidental hit (test_planted_sets_cpu.py): at k = 12 a window that is a candidate in lanes a, b and c is a
# hit in lane d of a filter of 33 k-mers with probability 0.11 (which is also why the ladder's longer reads start at k = 16)
LADDER_SEED = {(12, 300): 66, (16, 300): 1}


def _ladder_reads(b, pats, search, counts, place=None, light=False):
    """place(name, chunk, decoy): where a decoy goes (default: chunk `chunk` of b)"""
    k = b.k
    place = place or (lambda name, c, d: b.chunk(c).append(d))
    for pat in pats:
        y = rand(b.rng, k)
        while degenerate(y) or y == util.revcomp(y):
            y = rand(b.rng, k)
        for name, c in zip(ORDER, pat):
            if c is not None:
                place(name, c, y.translate(DECOY[name]))
        b.decoyed.append(y)
        hit = int(len(set(pat)) == 1 and pat[0] is not None)
        search += [y, util.revcomp(y), rand(b.rng, 7) + y + rand(b.rng, 11), y + y]
        counts += [hit, hit, hit, 2 * hit]
        if k >= 16:                                             # at both ends of a longer read (k = 12: see LADDER_SEED)
            search += [y + rand(b.rng, 40), rand(b.rng, 40) + y.lower()]
            counts += [hit, hit]


def ladder_case(k, n_chunks, whole=None, whole_reads=24):
    """family A.  -> dict(k, index, max_kmer, n_chunks, sets = {"ladder": ragged, "whole": fixed length}, decoyed, translated = the
    reads X of the whole-read ladders).  whole (default:
    k >= 25): whole-read ladders, reads X of 64 windows with X.translate(LO) indexed (every window a candidate in lane a and no
    hit), then HI (two lanes), BOTH (three) and ROT as well (every window a full false positive: count = len(X) // k).
    Three-lane reads only from k = 32 on, and few: lane d = a | b has 0.81 bits per base, so two random k-mers share it with
    probability (10/16)^k, and a window that is a candidate in a, b and c becomes an accidental hit against a few thousand
    indexed k-mers (k = 25: 8e-6 x 3 400 k-mers x 256 windows = 7 expected; k = 32: 0.25)"""
    whole = (k >= 25) if whole is None else whole
    whole_len = k + 63
    light = k < 20
    key = (k, n_chunks, whole, whole_reads)
    if key in _LADDERS:
        return _LADDERS[key]
    b = _Builder(7000 * k + n_chunks + 1000000 * LADDER_SEED.get((k, n_chunks), 0), k)
    b.chunk(n_chunks - 1)
    search, counts = [], []
    _ladder_reads(b, ladder_patterns(n_chunks, light), search, counts, light=light)
    _odd_size(b, search, counts, k + 5)
    sets = {"ladder": (search, np.array(counts))}
    if whole:
        reads, wc, translated = [], [], []
        for i in range(whole_reads):
            X = rand(b.rng, whole_len)
            rungs = (1, 2, 4, 1, 2, 3 if k >= 32 else 4)[i % 6]
            c = (i // 3) % n_chunks
            for name in ORDER[:rungs]:
                b.chunk(c).append(X.translate(DECOY[name]))
            translated.append(X)
            reads += [X, util.revcomp(X)]
            wc += [whole_len // k if rungs == 4 else 0] * 2
            if rungs == 4 and n_chunks > 1:                     # ... and the four translations in different filters: nothing
                X = rand(b.rng, whole_len)
                for j, name in enumerate(ORDER):
                    b.chunk((c + (j & 1)) % n_chunks).append(X.translate(DECOY[name]))
                translated.append(X)
                reads.append(X)
                wc.append(0)
        _odd_size(b, reads, wc, whole_len)
        sets["whole"] = (reads, np.array(wc))
    index, max_kmer = b.index()
    _LADDERS[key] = dict(k=k, index=index, max_kmer=max_kmer, n_chunks=n_chunks, sets=sets, decoyed=b.decoyed,
                         translated=translated if whole else [])
    return _LADDERS[key]


def ladder_jobs(k, n_chunks=3):
    """the decoys of every k-mer split between two index SETS (LO and BOTH in the first, HI and ROT in the second, the same chunk of
    each), and k-mers with all four in one set.  -> dict(k, index_sets, max_kmer, n_chunks, search, counts = [per job], decoyed)"""
    key = ("jobs", k, n_chunks)
    if key in _LADDERS:
        return _LADDERS[key]
    b = _Builder(9000 * k, k)
    other = _Builder(9000 * k + 1, k)
    for x in (b, other):
        x.chunk(n_chunks - 1)
    pats = [(c,) * 4 for c in range(n_chunks)] * 2
    search, scratch = [], []
    _ladder_reads(b, pats, search, scratch, place=lambda name, c, d: (b if name in ("LO", "BOTH") else other).chunk(c).append(d))
    counts = [[0] * len(search), [0] * len(search)]
    for j, x in enumerate((b, other)):                          # whole: found by job j alone
        mine = []
        _ladder_reads(b, pats, search, mine, place=lambda name, c, d: x.chunk(c).append(d))
        counts[j] += mine
        counts[1 - j] += [0] * len(mine)
    while len(search) % 64 == 0:
        search.append(rand(b.rng, k + 9))
        for c in counts:
            c.append(0)
    kmers = [max(sum(len(r) - k + 1 for r in c) for c in x.chunks) for x in (b, other)]
    out = [x.index(extra=max(kmers) - km) for x, km in zip((b, other), kmers)]
    assert out[0][1] == out[1][1]
    _LADDERS[key] = dict(k=k, index_sets=[o[0] for o in out], max_kmer=out[0][1], n_chunks=n_chunks, search=search,
                         counts=[np.array(c) for c in counts], decoyed=b.decoyed)
    return _LADDERS[key]


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
SLICED_FHW = (1, 32, 33, 65, 97, 129)
# (k, t, n_chunks, fhws, per_chunk): six chunk filters serve every slot regime (one by one; groups of 2 + 2 + 2, of 4 + 2, of 6)
SLOT_SWEEPS = [(k, t, 6, FHW, 0) for k in (25, 32, 33, 34) for t in (1, 2, 3)]
SMALL_SWEEPS = [(20, t, 6, FHW, 0) for t in (1, 2, 3)] + [(16, t, 0, FHW, 8) for t in (1, 2, 3)]                 # the plain kernel below the tiled search's k
# (k = 12, t = 1: one accidental hit anywhere flips a read, and a filter of 2^12 bits gives one in a thousand reads: three fhw only)
# (t >= 4: the wide row pass ends before the last window, at last - (t - 3) k; shorter fhw lists keep the reads within 255 first-hit windows)
SLICED_SWEEPS = [(12, 1, 0, (1, 32, 33), 4), (12, 2, 0, SLICED_FHW, 4), (16, 1, 0, SLICED_FHW, 16), (16, 2, 0, SLICED_FHW, 16),
                 (21, 3, 40, SLICED_FHW, 0), (24, 2, 40, SLICED_FHW, 0), (16, 5, 0, (1, 32, 33), 16), (21, 4, 40, (1, 32, 33, 65), 0)]
SLOT_LADDERS = [(k, 6) for k in (16, 20, 25, 32, 33, 34)]
SLICED_LADDERS = [(k, 300) for k in (12, 16, 21, 24)]
JOB_LADDERS = [(25, 3), (33, 3), (32, 1)]                      # (k, chunks per index set)
LARGEST_K = 36                                                  # family A alone, against the key-level checker

# ---- the cases of the hit-profile kernels (test_gpu_planted_profile.py), proved as BYTES by test_planted_sets_cpu.py -------------------
# the tiled profile takes sets of at most 255 complete windows per read: the t = 1 sweeps above (reads of fhw + k - 1 bases), and for
# counts above 1 sweeps at t = 3 over the shorter first-hit ranges (129 + 2 k windows in the longest fixed-length read: 197 at k = 34)
TILED_KS = (25, 32, 33, 34)
TILED_WINDOWS = 255
TILED_SWEEPS = [(k, 1, 6, FHW, 0) for k in TILED_KS] + [(k, 3, 6, SLICED_FHW, 0) for k in TILED_KS]
TILED_LADDERS = [(k, 6) for k in TILED_KS]
WIDE_PROFILE_KS = (12, 16, 21)                                  # (the k of the search file's wide rows)
# (profile_wide_ok takes every k the tables have, so the ladder also runs at their largest: rows of 128 bytes, tables of 8 GiB)
WIDE_PROFILE_LADDERS = [(k, 300) for k in WIDE_PROFILE_KS + (24,)]
# two index sets of 1, 2 and 3 chunks: passes of 2, 4 and 6 filter slots (hits_jobs_kernel<., 2 | 4 | 8>), 32-bit keys and 64-bit keys
PROFILE_JOB_LADDERS = [(32, 1), (25, 2), (25, 3), (33, 1), (33, 2), (33, 3)]


def tiled_sets(case):
    """the names of a case's sets that the tiled profile takes: no read of more than TILED_WINDOWS complete windows"""
    return [n for n, (reads, _) in case["sets"].items() if max(len(r) for r in reads) - case["k"] + 1 <= TILED_WINDOWS]
