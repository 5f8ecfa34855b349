"""The read sets of the length-relative search's tests (test_gpu_relative.py on the GPU, test_relative_cpu.py through the CPU checker
alone): generators only, importable without a GPU, every case seeded and cached so that both files see the same reads.  TEST
INFRASTRUCTURE ONLY.

Every designed set is a dict(k, percent, min_hits, index, max_kmer, n_chunks, search, best): best = int[n_chunks, reads], the
designed max(F, R) of every read in every chunk filter — the plants decide it: the k-mers of the planted windows of a random read
(their reverse complements for the reverse strand) are index reads of exactly k bases in the chunk they were meant for
(hit_profile_group_sets.chunked), nothing else of the read is indexed.  designed_tags(case) follows from `best` and the rule;
test_relative_cpu.py proves both against the CPU checker."""
import functools

import numpy as np

import util
from commet_amd import relative
from hit_profile_group_sets import chunked, greedy, rand


def thresholds_of(case, search=None):
    reads = case["search"] if search is None else search
    return relative.thresholds([len(r) for r in reads], case["k"], case["percent"], case["min_hits"])


def designed_tags(case, select=None):
    """bool per search read: some chunk filter holds t_r of its non-overlapping k-mers on one strand (and the read is selected)"""
    thr = thresholds_of(case)
    found = (thr > 0) & (case["best"] >= np.maximum(thr, 1)[None, :]).any(axis=0)
    return found if select is None else found & np.asarray(select, dtype=bool)


def first_found_chunk(case):
    """per search read the first chunk filter that finds it; n_chunks where none does"""
    thr = thresholds_of(case)
    ok = (thr > 0)[None, :] & (case["best"] >= np.maximum(thr, 1)[None, :])
    return np.where(ok.any(axis=0), ok.argmax(axis=0), case["n_chunks"])


class _Planter:
    """collects search reads and, per chunk, the k-mers planted for them"""

    def __init__(self, rng, k, n_chunks):
        self.rng, self.k, self.chunks, self.search, self.best = rng, k, [[] for _ in range(n_chunks)], [], []

    def add(self, length, plants):
        """plants: [(chunk, reverse, window starts)] — several entries may name the same chunk and strand"""
        k = self.k
        read = rand(self.rng, length)
        per = {}
        for c, rev, starts in plants:
            assert all(0 <= s <= length - k for s in starts), (length, starts)
            self.chunks[c] += [util.revcomp(read[s:s + k]) if rev else read[s:s + k] for s in starts]
            per.setdefault((c, rev), []).extend(starts)
        col = [0] * len(self.chunks)
        for (c, rev), starts in per.items():
            col[c] = max(col[c], greedy(starts, k))
        self.search.append(read)
        self.best.append(col)

    def case(self, percent, min_hits):
        index, max_kmer = chunked(self.rng, self.k, self.chunks)
        return dict(k=self.k, percent=percent, min_hits=min_hits, index=index, max_kmer=max_kmer, n_chunks=len(self.chunks), search=self.search,
                    best=np.array(self.best, dtype=np.int64).T)


# ---- 1. ragged sets -------------------------------------------------------------------------------------------------------------
RAGGED_KS = (20, 31, 33)
RAGGED_W = (1, 2, 3, 5, 10, 20)                           # six length classes between k and 20 k: t_r = 1, 1, 2, 3, 5, 10 at 50 %
RAGGED_CHUNKS = 3


@functools.lru_cache(maxsize=None)
def ragged_set(k, min_hits=1):
    """reads of six length classes whose hits reach, miss by one, or are spread over chunks and strands; five distinct t_r.
    min_hits = 3: the same reads under a floor that the two shortest classes cannot reach (t_r > W_r: never found, never walked)"""
    if min_hits != 1:
        return dict(ragged_set(k), min_hits=min_hits)
    rng = np.random.default_rng(7100 + k)
    p = _Planter(rng, k, RAGGED_CHUNKS)
    for rep in range(4):
        for w in RAGGED_W:
            t = (50 * w + 99) // 100
            length = w * k + int(rng.integers(0, k))          # (every length of the class: W_r = w)
            off = int(rng.integers(0, length - w * k + 1))
            at = [off + i * k for i in range(w)]              # the w non-overlapping windows the read can hold
            for rev in (False, True):
                c = int(rng.integers(0, RAGGED_CHUNKS))
                c2 = (c + 1 + int(rng.integers(0, RAGGED_CHUNKS - 1))) % RAGGED_CHUNKS
                p.add(length, [(c, rev, at[:t])])                                       # exactly t_r hits in one chunk: found there
                p.add(length, [(c, rev, at[:t - 1])])                                   # one short
                p.add(length, [(c, rev, at[:t - 1]), (c2, rev, at[t - 1:t])])           # every hit indexed somewhere, no chunk holds t_r
                p.add(length, [(c, rev, at[:t - 1]), (c, not rev, at[t - 1:t])])        # ... nor one strand
                p.add(length, [(c, rev, at[:t - 1]), (c2, rev, at[:t])])                # short in an earlier or later chunk, enough in the other
                p.add(length, [(c, rev, at)])                                           # all the read can hold
                if t >= 2:
                    p.add(length, [(c, rev, at[:t - 1] + [at[t - 2] + k - 1])])         # the t_r-th window overlaps the one before: not taken
            p.add(length, [])
    # the shortest reads: fewer than k bases (never found), k and 2 k - 1 bases (one k-mer is all they can hold)
    p.add(k - 1, [])
    p.add(k, [(2, False, [0])])
    p.add(2 * k - 1, [(1, True, [k - 1])])
    case = p.case(percent=50, min_hits=1)
    assert len(set(thresholds_of(case).tolist())) <= 6
    return case


@functools.lru_cache(maxsize=None)
def ragged_selection(k, share=0.4):
    """a selection of about that share of ragged_set(k)'s search reads"""
    return np.random.default_rng(7200 + k).random(len(ragged_set(k)["search"])) < share


# ---- 2. block edges of the wave forms ---------------------------------------------------------------------------------------------
EDGE_KS = (31, 32, 33)


@functools.lru_cache(maxsize=None)
def edge_set(k):
    """percent = 25: reads of 5 k .. 9 k - 1 bases have t_r = 2, reads of 9 k .. 13 k - 1 bases t_r = 3.  The t_r-th accepted hit
    starts at window 63, 64, 65 (127, 128, 129) of the read — the last window of a 64-window block, the first and the second of the
    next — with the hit before it ending right in front of it (k windows back: in the block before), or one window later, so that
    the carry from the block before forbids the t_r-th hit and the read is NOT found"""
    rng = np.random.default_rng(7300 + k)
    p = _Planter(rng, k, 2)
    n = 0
    for e in (63, 64, 65, 127, 128, 129):
        for t in (2, 3):
            if e - (t - 1) * k < 0:
                continue
            lo, hi = ((5 * k, 9 * k - 1) if t == 2 else (9 * k, 13 * k - 1))
            length = min(max(e + 2 * k + int(rng.integers(0, 8)), lo), hi)
            assert e + 2 * k <= length
            chain = [e - i * k for i in range(t - 1, -1, -1)]              # t hits, each ending where the next starts, the last at e
            late = chain[:-2] + [chain[-2] + 1, e]                          # the hit before e one window later: it overlaps e
            for rev in (False, True):
                c = n % 2
                n += 1
                p.add(length, [(c, rev, chain)])                            # found
                p.add(length, [(c, rev, late)])                             # not found: t_r - 1 hits
                p.add(length, [(c, rev, late + [e + k])])                   # ... unless another hit follows: e + k >= (e - k + 1) + k
                p.add(length, [(c, rev, chain[:-1]), (1 - c, rev, chain[-1:])])   # the last hit in the other chunk's filter: not found
                p.add(length, [(c, rev, chain[:-1]), (c, not rev, chain[-1:])])   # ... on the other strand: not found
    for _ in range(4):
        p.add(6 * k, [])
    case = p.case(percent=25, min_hits=1)
    thr = thresholds_of(case)
    assert set(thr.tolist()) == {2, 3}
    return case


# ---- 3. uniform thresholds ---------------------------------------------------------------------------------------------------------
UNIFORM_KS = (32, 33)
UNIFORM_N, UNIFORM_LEN = 3000, 100
UNIFORM_CHUNKS = (1, 2, 3, 5, 8)


@functools.lru_cache(maxsize=None)
def uniform_set(k):
    """-> (index reads, search reads): 2 x 3 000 clean reads of 100 bases, a third of the search reads copies of index reads (or of
    their reverse complements) with a few substitutions.  W_r = 3 everywhere: 50 % is t_r = 2, 100 % is t_r = 3"""
    rng = np.random.default_rng(7400 + k)
    index = [rand(rng, UNIFORM_LEN) for _ in range(UNIFORM_N)]
    search = []
    for i in range(UNIFORM_N):
        if i % 3:
            search.append(rand(rng, UNIFORM_LEN))
            continue
        s = bytearray(index[int(rng.integers(0, UNIFORM_N))])
        for x in rng.integers(0, UNIFORM_LEN, size=int(rng.integers(0, 4))):
            s[x] = b"ACGT"[(b"ACGT".index(s[x]) + 1 + int(rng.integers(0, 3))) % 4]
        search.append(util.revcomp(bytes(s)) if rng.random() < 0.5 else bytes(s))
    return index, search


def uniform_max_kmer(k, n_chunks):
    """a max_kmer under which uniform_set(k)'s index set makes exactly n_chunks chunks: m reads each, one dropped behind each"""
    m = -(-(UNIFORM_N - n_chunks + 1) // n_chunks)
    return m * (UNIFORM_LEN - k + 1)


# ---- 4. thresholds beyond a byte --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_set(k=20, w=400):
    """-> dict(k, index, max_kmer, search, exp): two index reads of w k bases, a chunk each (the read between them is the dropped
    look-ahead read); the search set: the first of them (F = w), a copy with one base changed in the middle, and a read whose first
    half comes from the first index read and its second half from the second.  exp[percent] = the designed bits"""
    rng = np.random.default_rng(7500 + k)
    x1, x2 = rand(rng, w * k), rand(rng, w * k)
    mid = bytearray(x1)
    at = (w // 2) * k
    mid[at] = b"ACGT"[(b"ACGT".index(mid[at]) + 1) % 4]
    halves = x1[:at] + x2[at:]
    # the changed base breaks window w / 2; the next clean window starts one base later, and w / 2 - 1 more fit behind it: w - 1 hits
    return dict(k=k, index=[x1, rand(rng, k + 3), x2], max_kmer=w * k - k + 1, n_chunks=2, search=[x1, bytes(mid), halves],
                w=w, exp={100: [True, False, False], 99: [True, True, False]})


@functools.lru_cache(maxsize=None)
def widest_reads():
    """k = 1 against the index read ACGT (max_kmer 4): a read of 65 535 bases, every one a hit (t_r = 65 535 at 100 %, the largest
    16 bits hold), four bases that are none, and a read of 65 534"""
    rng = np.random.default_rng(7600)
    return [rand(rng, 65535), b"NNNN", rand(rng, 65534)]
