"""The read sets of the grouped hit profile's tests (test_gpu_hit_profile_groups.py on the GPU, test_hit_profile_groups_cpu.py through
the CPU checker alone): generators only, importable without a GPU, every case seeded and cached so that both files and every
parametrised case see the same reads.

A job has several chunk filters when the index set holds more k-mers than `max_kmer` (the library's test hook, the checker's twin of
it).  The planner's rule (index_reads.h:49-61): reads are added while the chunk holds fewer than max_kmer k-mers, and the read that
was fetched when it closes is dropped.  `chunked` lays an index set out by that rule: every chunk but the last is filled to exactly
max_kmer k-mers and followed by one read to be dropped, so that a planted k-mer sits in the chunk it was meant for."""
import numpy as np

import util


def rand(rng, n):
    return util.ACGT[rng.integers(0, 4, size=n)].tobytes()


def greedy(starts, k):
    """non-overlapping windows of k bases taken from the left: the count one filter and strand gives"""
    cnt, free = 0, 0
    for s in sorted(starts):
        if s >= free:
            cnt, free = cnt + 1, s + k
    return cnt


def chunked(rng, k, chunks, extra=0):
    """chunks: per chunk, the index reads meant for it (clean ACGT reads of at least k bases).  -> (index reads, max_kmer): the reads
    of chunk c fall into chunk filter c"""
    kmers = [sum(len(r) - k + 1 for r in c) for c in chunks]
    max_kmer = max(kmers) + 1 + extra
    index = []
    for ci, (c, n) in enumerate(zip(chunks, kmers)):
        index += list(c)
        if ci + 1 < len(chunks):
            index.append(rand(rng, max_kmer - n + k - 1))     # fills the chunk to max_kmer k-mers exactly
            index.append(rand(rng, k + 3))                      # the look-ahead read the planner drops
    return index, max_kmer


# ---- 1. groups of every size and remainder ------------------------------------------------------------------------------------
GROUP_CASES = [(2, 8), (3, 8), (4, 8), (5, 8), (8, 8), (9, 8), (11, 8), (5, 4), (3, 2), (8, 3)]   # (n_chunks, chunk_group)
GROUP_KS = [20, 25]
WIDE_K = 33
WIDE_CHUNKS = [2, 3, 5]
_GROUP_SETS = {}


def group_set(k, n_chunks):
    """-> (index reads, search reads, max_kmer): fixed-length clean index reads, n_chunks chunks of them; related search reads with N
    runs and lower-case bases"""
    key = (k, n_chunks)
    if key not in _GROUP_SETS:
        rng = np.random.default_rng(1000 * k + n_chunks)
        L, per_chunk = 110, 4                                   # (a chunk: per_chunk reads, then the dropped one)
        index = [rand(rng, L) for _ in range(n_chunks * (per_chunk + 1))]
        search = [r if len(r) else b"A" for r in util.related_reads(rng, index, 260, 20, 200, share=0.6, n_rate=0.01, lower_rate=0.3)]
        for r in index[::per_chunk + 1]:                        # the first read of every chunk: stretches of it that hold 1, 2, 3 k-mers
            search += [r[:k + 3], util.revcomp(r[2:2 * k + 4]), r[:3 * k + 1].lower()]
        _GROUP_SETS[key] = (index, search, per_chunk * (L - k + 1))
    return _GROUP_SETS[key]


def groups_of(n_chunks, chunk_group):
    """(passes per search set, a group of >= 2 chunks exists, a group of one chunk exists) as the chunk loop forms its groups"""
    sizes = []
    left = n_chunks
    while left:
        sizes.append(min(chunk_group, left))
        left -= sizes[-1]
    return len(sizes), any(s >= 2 for s in sizes), any(s == 1 for s in sizes)


# ---- 2. state is per filter -----------------------------------------------------------------------------------------------------
def planted_states(k=25):
    """-> (index, search, expected bytes, max_kmer, n_chunks): reads whose hits lie in two chunk filters"""
    rng = np.random.default_rng(25)
    a, b, search, exp = [], [], [], []
    # (i) chunk A: window 10; chunk B: windows 10 + k - 1 and 10 + 2 k - 1.  A's hit must not close B's first window: B counts 2
    for strand in (0, 1):
        x = rand(rng, 200)
        f = (lambda s: x[s:s + k]) if strand == 0 else (lambda s: util.revcomp(x[s:s + k]))
        a += [f(10)]
        b += [f(10 + k - 1), f(10 + 2 * k - 1)]
        search.append(x)
        exp.append(2)
    # (ii) chunk A: F = 1, R = 3; chunk B: F = 2, R = 0
    x = rand(rng, 200)
    a += [x[0:k], util.revcomp(x[40:40 + k]), util.revcomp(x[80:80 + k]), util.revcomp(x[120:120 + k])]
    b += [x[30:30 + k], x[150:150 + k]]
    search.append(x)
    exp.append(3)
    # the same windows, each chunk's on both strands of the other: overlaps across filters and strands count separately
    x = rand(rng, 200)
    a += [x[5:5 + k], util.revcomp(x[5 + k - 1:5 + 2 * k - 1])]
    b += [util.revcomp(x[5:5 + k]), x[5 + k - 1:5 + 2 * k - 1]]
    search.append(x)
    exp.append(1)
    search.append(rand(rng, 200))
    exp.append(0)
    index, max_kmer = chunked(rng, k, [a, b])
    return index, search, exp, max_kmer, 2


def planted_slots(k=25, n_chunks=10):
    """(iii) read p has three hits in chunk p and one in chunk p + 1: the best chunk sits in every slot of the first group of eight
    in turn, and in the second group.  -> (index, search, expected bytes, max_kmer, n_chunks)"""
    rng = np.random.default_rng(77)
    chunks = [[] for _ in range(n_chunks)]
    search = []
    for p in range(n_chunks):
        x = rand(rng, 170)
        chunks[p] += [x[0:k], x[40:40 + k], util.revcomp(x[140:140 + k]), x[80:80 + k]]
        chunks[(p + 1) % n_chunks] += [x[120:120 + k]]
        search.append(x)
    index, max_kmer = chunked(rng, k, chunks, extra=10)
    return index, search, [3] * n_chunks, max_kmer, n_chunks


def planted_palindrome(k=20):
    """(iv) a k-mer that is its own reverse complement (even k): plane A stores it once, the `selfp` branch of the paired load"""
    rng = np.random.default_rng(20)
    pal = b"ACGT" * (k // 4)
    assert util.revcomp(pal) == pal and len(pal) == k
    z = rand(rng, 50) + pal + rand(rng, 50)
    z2 = rand(rng, 30) + pal + rand(rng, 7)
    z3 = rand(rng, 9) + pal + rand(rng, 40)
    a = [pal, z3[40:40 + k]]
    b = [z[0:k], util.revcomp(z[90:90 + k]), util.revcomp(z[5:5 + k])]
    index, max_kmer = chunked(rng, k, [a, b])
    # z: chunk A 1 (the palindrome, on either strand), chunk B F = 1, R = 2; z2: the palindrome alone; z3: it and a forward hit behind it
    return index, [z, z2, z3, rand(rng, 120)], [2, 1, 2, 0], max_kmer, 2


# ---- 3. the wave form at block edges: the plants of one read in DIFFERENT chunks --------------------------------------------------
def wave_plants(k):
    """(chunk 0 forward, chunk 0 reverse, chunk 1 forward, chunk 1 reverse) window starts"""
    one = [
        ((62, 62 + k), ()), ((62, 61 + k), ()), ((63, 64), ()), ((63, 63 + k, 63 + 2 * k), ()), ((40, 40 + k), ()), ((40, 39 + k), ()),
        ((0, k), ()), ((0, k - 1), ()), ((), (10, 50)), ((), (62, 61 + k)), ((), (62, 62 + k)), ((5,), (20, 60)), ((0, 33, 66), (90,)),
        ((5, 20), (60,)), ((127, 127 + k), ()), ((0,), ()), ((), ()),
    ]
    out = []
    for i, (fw, rv) in enumerate(one):                          # the plants of test_gpu_hit_profile, alternating between the chunks
        out.append((fw, rv, (), ()) if i % 2 == 0 else ((), (), fw, rv))
    for e in (63, 127, 191):
        # filter 0's hit in the last window of a block forbids filter 0's first window of the next block, not filter 1's
        out.append(((e, e + 1), (), (e + 1, e + 1 + k), ()))    # filter 0: 1, filter 1: 2
        out.append(((), (e, e + 1), (), (e + 1, e + 1 + k)))
        out.append(((e + 1, e + 1 + k), (), (e, e + 1), ()))    # ... and with the slots swapped
        out.append(((e, e + 1), (), (), (e + 1, e + 1 + k)))    # across strands as well
        out.append(((e - 1, e - 1 + k), (e,), (e, e + k, e + 2 * k), ()))   # carries of different lengths into the next block: 2 and 3
    return out


_WAVE_SETS = {}


def wave_sets(k):
    """-> (index, ragged search set, its expected bytes (None: the checker decides), fixed-length search set, its expected bytes,
    max_kmer)"""
    if k in _WAVE_SETS:
        return _WAVE_SETS[k]
    rng = np.random.default_rng(3000 + k)
    chunks = [[], []]
    ragged, exp_r, fixed, exp_f = [], [], [], []

    def plant(read, p):
        c0f, c0r, c1f, c1r = p
        chunks[0] += [read[s:s + k] for s in c0f] + [util.revcomp(read[s:s + k]) for s in c0r]
        chunks[1] += [read[s:s + k] for s in c1f] + [util.revcomp(read[s:s + k]) for s in c1r]
        return max(greedy(c0f, k), greedy(c0r, k), greedy(c1f, k), greedy(c1r, k))

    for n_win in (1, 63, 64, 65, 128, 129, 193, 257):
        for p in wave_plants(k):
            if any(s >= n_win for part in p for s in part):
                continue
            read = rand(rng, n_win + k - 1)
            exp_r.append(plant(read, p))
            ragged.append(read)
    n_win = max(257, 192 + 2 * k)                               # (every plant fits: the last one starts at 191 + 2 k; 257 up to k = 32)
    for p in wave_plants(k):
        read = rand(rng, n_win + k - 1)
        exp_f.append(plant(read, p))
        fixed.append(read)
    # N runs that split a block: every clean window of the read is a k-mer of the index set, on one strand or the other (these index
    # reads close chunks where they may: the checker and chunk_group = 1 decide)
    tail = []
    for L, runs in ((200, [(70, 71)]), (200, [(40, 41), (100, 130)]), (300, [(63 + k - 1, 63 + k), (64, 65)]), (257 + k, [(0, 150)]), (300, [(120, 121), (200, 202)])):
        read = rand(rng, L)
        s = bytearray(read)
        for a, b in runs:
            s[a:b] = b"N" * (b - a)
        tail.append(read)
        ragged += [bytes(s), util.revcomp(bytes(s)), bytes(s).lower()]
        exp_r += [None, None, None]
    index, max_kmer = chunked(rng, k, chunks + [tail])
    _WAVE_SETS[k] = (index, ragged, exp_r, fixed, exp_f, max_kmer)
    return _WAVE_SETS[k]


# ---- 4. saturation ----------------------------------------------------------------------------------------------------------------
def saturation_set(k=8, n_chunks=10):
    """-> (index, search, exact, max_kmer): chunk p holds the first 200 (p + 1) bases of `read`, the last chunk all of it: every
    window of `read` at 0, k, 2 k, ... is a hit there, `exact` of them"""
    rng = np.random.default_rng(11)
    read = rand(rng, 200 * n_chunks)
    index = []
    for p in range(n_chunks):
        index += [read[:200 * (p + 1)], rand(rng, k + 2)]       # (each piece closes its chunk; the read behind it is dropped)
    return index, [read, read[:1000], util.revcomp(read)], len(read) // k, 100


# ---- 7. randomised ------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = list(range(300, 320))


def random_case(seed):
    """-> (k, max_kmer, chunk_group) of scenarios.Scenario(seed, n_scale = 4)"""
    k = [12, 16, 20, 25, 32, 13][seed % 6]
    return k, (20 if k in (25, 32) else 300), 2 + seed % 7
