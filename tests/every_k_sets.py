"""Fixtures and a key-level job reference for EVERY k the library takes, 1 .. 38 (test_gpu_every_k.py on the GPU, test_every_k_sets_cpu.py
through the CPU checker alone): generators only, importable without a GPU, every case seeded and cached.  TEST INFRASTRUCTURE ONLY.

key_level_job is the whole job of the restated tool over the CPU checker's KEYS (oracle_binding.keys_of_read, good at every k up to
38), the four lanes of every chunk filter kept as sorted key arrays: no 2^(k-1)-byte filter is ever allocated, so it says what the
reference would say at k = 35 .. 38 too.  test_every_k_sets_cpu.py proves it equal to the checker's own run wherever the checker's
filter fits a test host (k <= 26).

case(k) is one job per k: an index set, a search set whose hit counts are mixed (reads found and not found at every t that is asked,
reads better on either strand, reads whose best chunk is a later one, reads whose only hits are broken by a non-ACGT base), reads of
200 .. 250 bases that cross word boundaries and several 64-window blocks, and from k = 34 on the THREE-WORD FAMILY: windows of whose
96 bits (words w-2, w-1, w of the read planes) the word w-2 gives k - 33 - j, for every j and both strands, each with a twin that
differs in the lowest base taken from word w-2."""
import functools

import numpy as np

import oracle_binding as ob
import oracle_pool as op
import util

KS = tuple(range(1, 39))
T_PROFILE = 255
ONE_CHUNK = 1 << 62                                   # a max_kmer no set reaches: every read in one filter, none dropped
NOT_ACGT = b"NnRYKM-.*"


def n_chunks_of(k):
    """six chunks; from k = 35 on as many as there are slots under the memory rule (test_gpu_every_k.py): 4, 2, 1, 1"""
    return {35: 4, 36: 2, 37: 1, 38: 1}.get(k, 6)


# ---- the reference's job over keys -----------------------------------------------------------------------------------------------------
class KeyLevelJob:
    """index_and_search.cpp:241-277 over keys.  chunks: [(a, e)] read ranges of the index set (read e, the look-ahead, is dropped);
    lanes[c]: the four sorted key arrays of chunk c; F[s], R[s]: int32[n_chunks, reads of set s], the greedy non-overlapping full hits
    of the whole forward / reverse strand in every chunk filter; hits[s]: the exact byte min(T, max over chunks of max(F, R))"""

    def __init__(self, k, index_reads, search_sets, max_kmer, T):
        self.k = k
        bases, offs = util.to_batch(index_reads)
        kc = ob.kmer_counts(bases, offs, k)
        self.chunks = op.chunks_from_counts(kc, max_kmer if max_kmer else ob.max_kmer(k))
        self.n_chunks = len(self.chunks)
        self.indexed = sum(e - a for a, e in self.chunks)
        self.kmers_indexed = int(sum(int(kc[a:e].sum()) for a, e in self.chunks))
        self.lanes = []
        for a, e in self.chunks:
            keys = [ob.keys_of_read(r, k)[0] for r in index_reads[a:e]]
            keys = np.concatenate(keys) if keys else np.zeros((0, 4), dtype=np.uint64)
            self.lanes.append([np.unique(keys[:, j]) for j in range(4)])
        self.F = [self._strand(s, False) for s in search_sets]
        self.R = [self._strand(s, True) for s in search_sets]
        self.best = [np.maximum(f, r) for f, r in zip(self.F, self.R)]
        self.hits = [np.minimum(T, b.max(axis=0, initial=0)).astype(np.uint8) for b in self.best]

    def full_hits(self, read, reverse):
        """-> (end positions of the read's complete windows on that strand, bool[n_chunks, windows]: a full hit in that chunk filter)"""
        keys, pos = ob.keys_of_read(read, self.k, reverse=reverse)
        return pos, self._full(keys)

    def _full(self, keys):
        out = np.zeros((self.n_chunks, len(keys)), dtype=bool)
        for c, lanes in enumerate(self.lanes):
            idx = np.arange(len(keys))
            for j in range(4):
                idx = idx[np.isin(keys[idx, j], lanes[j])]
            out[c, idx] = True
        return out

    def _strand(self, reads, reverse):
        got = [ob.keys_of_read(q, self.k, reverse=reverse) for q in reads]
        keys = np.concatenate([g[0] for g in got]) if got else np.zeros((0, 4), dtype=np.uint64)
        pos = np.concatenate([g[1] for g in got]).astype(np.int64) if got else np.zeros(0, dtype=np.int64)
        rid = np.repeat(np.arange(len(reads)), [len(g[1]) for g in got])
        out = np.zeros((self.n_chunks, len(reads)), dtype=np.int32)
        full = self._full(keys)
        for c in range(self.n_chunks):
            idx = np.flatnonzero(full[c])
            cur, next_end = -1, 0
            for r, p in zip(rid[idx].tolist(), pos[idx].tolist()):
                if r != cur:
                    cur, next_end = r, 0
                if p >= next_end:                      # hash.clear() after a hit: the next complete window ends k bases later
                    out[c, r] += 1
                    next_end = p + self.k
        return out

    def tags(self, t, selects=None):
        """per search set bool[reads]: found at t (under a selection: of the selected reads)"""
        out = [b.max(axis=0, initial=0) >= t for b in self.best]
        return out if selects is None else [o & np.asarray(s, dtype=bool) for o, s in zip(out, selects)]

    def stats(self, t, selects=None):
        """per search set [indexed, searched, shared] of the log line: `searched` is the LAST chunk's count, the reads that no earlier
        chunk tagged"""
        out = []
        for s, b in enumerate(self.best):
            sel = np.ones(b.shape[1], dtype=bool) if selects is None else np.asarray(selects[s], dtype=bool)
            before_last = b[:-1].max(axis=0, initial=0) >= t if self.n_chunks else np.zeros(b.shape[1], dtype=bool)
            out.append([self.indexed, int((sel & ~before_last).sum()) if self.n_chunks else 0, int(((b.max(axis=0, initial=0) >= t) & sel).sum())])
        return out


def key_level_job(k, index_reads, search_sets, max_kmer, T=T_PROFILE):
    """the job of index_reads (chunks of max_kmer k-mers; 0 = the reference's constant) against every set of search_sets -> KeyLevelJob:
    .hits (per set the exact byte at T), .n_chunks, .kmers_indexed, .tags(t), .stats(t)"""
    return KeyLevelJob(k, list(index_reads), [list(s) for s in search_sets], max_kmer, T)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def _clean(rng, n, lo, hi):
    return util.random_reads(rng, n, lo, hi, n_rate=0.0, lower_rate=0.0, other_rate=0.0)


def fit_max_kmer(k, index_reads, n_chunks):
    """a max_kmer under which the index set makes exactly n_chunks chunks (None: there is none)"""
    kc = ob.kmer_counts(*util.to_batch(index_reads), k)
    total = int(kc.sum())
    if n_chunks == 1:
        return total + 1
    for mk in sorted(range(1, total + 1), key=lambda m: abs(m - total // n_chunks)):
        if len(op.chunks_from_counts(kc, mk)) == n_chunks:
            return mk
    return None


def _patched(rng, k, pool, n, lo, hi, bad=False):
    """reads of lo .. hi random bases with one to three stretches of k .. 3 k bases copied from reads of the pool or their reverse
    complements; bad: a non-ACGT letter in the middle of the first stretch"""
    out = []
    for r in _clean(rng, n, lo, hi):
        s = bytearray(r)
        at = 0
        for i in range(int(rng.integers(1, 4))):
            src = pool[int(rng.integers(0, len(pool)))]
            if rng.random() < 0.5:
                src = util.revcomp(src)
            ln = min(int(rng.integers(k, 3 * k + 1)), len(src), len(s) - at)
            if ln < k:
                break
            a = int(rng.integers(0, len(src) - ln + 1))
            at += int(rng.integers(0, max(1, (len(s) - at - ln) // 2 + 1)))
            s[at:at + ln] = src[a:a + ln]
            if bad and i == 0:
                s[at + ln // 2] = NOT_ACGT[int(rng.integers(0, len(NOT_ACGT)))]
            at += ln + int(rng.integers(0, k))
        out.append(bytes(s))
    return out


# k-mers per chunk filter below k = 13, as a share of the 2^k bits of a lane: a lane is then about half full and a random window a
# full hit now and then — 0.2 x 4^k k-mers would fill every lane from k = 3 on and every read would count len / k
LANE_FILL = {2: 0.8, 3: 0.7, 4: 0.9, 5: 0.8, 6: 0.7, 7: 0.6, 8: 0.25, 9: 0.22, 10: 0.2, 11: 0.15, 12: 0.12}


def _small_case(rng, k, n_chunks):
    """k = 1 .. 7: index reads of exactly k bases; random search reads of 1 .. 6 k bases, a non-ACGT base in every fiftieth place"""
    if k == 1:
        # four keys: the chunks index A or C alone; only a read without A, C, G and T is found by none (hence so many N, so short reads)
        index = [b"A", b"G", b"C", b"T", b"A", b"A", b"A", b"C", b"C", b"G", b"A"][:2 * n_chunks - 1]
        search = util.random_reads(rng, 200, 1, 4, n_rate=0.4, lower_rate=0.1)
    else:
        per = max(1, round(LANE_FILL[k] * 2 ** k))
        index = _clean(rng, per * n_chunks + n_chunks - 1, k, k)
        search = util.random_reads(rng, 200, 1, 6 * k, n_rate=0.02, lower_rate=0.1)
    return index, search


def _sparse_case(rng, k, n_chunks):
    """k = 8 .. 12: a sparse index of reads of k + 15 bases, related search reads"""
    per = max(1, round(LANE_FILL[k] * 2 ** k / 16))
    index = _clean(rng, per * n_chunks + n_chunks - 1, k + 15, k + 15)
    search = util.related_reads(rng, index, 200, 1, 6 * k, share=0.6, n_rate=0.01)
    return index, search


def _three_word_family(rng, k):
    """-> (index reads, search reads, [dict(read, twins, end, reverse)] numbering the search reads from 0): for every j in 0 .. k - 34,
    end word w in {2, 3} and strand a random read R of 32 w + j + 1 + 40 bases whose window ending at base 32 w + j is indexed (its
    reverse complement for the reverse strand), and R with that window's first base substituted.  R's last k bases are indexed too: R
    then counts 2 and its twins 1, which a SEARCH at t = 2 tells apart (alone the planted window would show in the hit bytes only).
    The index reads come in groups of six, the two k-mers of an R three times in turn: where a chunk ends inside a group (its last
    read, the dropped look-ahead read, the next chunk's first), one side still holds both"""
    index, search, family = [], [], []
    for j in range(0, k - 34 + 1):
        for w in (2, 3):
            for reverse in (False, True):
                end = 32 * w + j
                R = _clean(rng, 1, end + 1 + 40, end + 1 + 40)[0]
                window = R[end - k + 1:end + 1]
                index += [util.revcomp(y) if reverse else y for y in (window, R[-k:])] * 3
                spots = [end - k + 1]                               # the window's first base: the lowest bit taken from word w-2
                if end - k + 1 <= 32 * (w - 2) + 10:                # bit 10 of word w-2 (no window reaches it below k = 55)
                    spots.append(32 * (w - 2) + 10)
                assert 32 * (w - 2) <= spots[0] <= 32 * (w - 2) + 31
                twins = []
                for x in spots:
                    s = bytearray(R)
                    s[x] = b"ACGT"[(b"ACGT".index(R[x]) + 1 + int(rng.integers(0, 3))) % 4]
                    twins.append(bytes(s))
                family.append(dict(read=len(search), twins=list(range(len(search) + 1, len(search) + 1 + len(twins))), end=end, reverse=reverse))
                search += [R] + twins
    return index, search, family


_JOBS = {}


@functools.lru_cache(maxsize=None)
def case(k):
    """-> dict(k, index, max_kmer, n_chunks, search, t_k, family, jobs, broken, max_kmer_small): one seeded job per k.  family: the
    three-word family's reads in `search` (k >= 34); broken: the reads of `search` made with a non-ACGT letter inside a copied stretch
    (k >= 8; below, random reads hold such letters and random windows hit); jobs: the index set split in two at a chunk boundary, or
    None (one chunk; k = 1); max_kmer_small: a chunk per index read for the bit-sliced kernels (12 <= k <= 24), else None"""
    rng = np.random.default_rng(52000 + k)
    n_chunks = n_chunks_of(k)
    if k <= 7:
        index, search = _small_case(rng, k, n_chunks)
    elif k <= 12:
        index, search = _sparse_case(rng, k, n_chunks)
    else:
        length = 60 if k <= 14 else 120                             # (k = 13, 14: a lane of 2^k bits stays sparse)
        index = util.random_reads(rng, 90 if k <= 24 else 40, length, length, n_rate=0.002, lower_rate=0.1)
        search = util.related_reads(rng, index, 200, 1, 250, share=0.6, n_rate=0.01)
    broken = None
    if k >= 8:
        search += _patched(rng, k, index, 24, 200, 250)
        broken = list(range(len(search), len(search) + 8))
        search += _patched(rng, k, index, 8, 3 * k, 250, bad=True)
    else:
        search += util.random_reads(rng, 24, 200, 250, n_rate=0.004, lower_rate=0.1)
    family = []
    if k >= 34:
        fi, fs, family = _three_word_family(rng, k)
        for i in range(0, len(fi), 6):                              # the groups of six among the index reads, wherever
            at = int(rng.integers(0, len(index) + 1))
            index[at:at] = fi[i:i + 6]
        for f in family:
            f["read"] += len(search)
            f["twins"] = [x + len(search) for x in f["twins"]]
        search += fs
    assert all(len(r) for r in index + search) and max(len(r) for r in search) <= 256
    max_kmer = fit_max_kmer(k, index, n_chunks)
    assert max_kmer is not None, k
    job = _JOBS[k] = key_level_job(k, index, [search], max_kmer)
    nonzero = job.hits[0][job.hits[0] > 0]
    t_k = int(np.median(nonzero)) if nonzero.size else 1
    assert max(len(r) for r in search) <= 254 + t_k * k or k == 1
    jobs = None
    if k >= 2 and n_chunks >= 2:
        mid = job.chunks[n_chunks // 2 - 1][1]                      # the first half's chunks end in front of read `mid`, which is dropped
        jobs = [index[:mid], index[mid + 1:]]
    return dict(k=k, index=index, max_kmer=max_kmer, n_chunks=n_chunks, search=search, t_k=t_k, family=family, jobs=jobs, broken=broken,
                max_kmer_small=1 if 12 <= k <= 24 else None)


@functools.lru_cache(maxsize=None)
def reference(k, which="job"):
    """key_level_job of case(k).  which: "job": the case's job; "small": the same sets in chunks of one index read (12 <= k <= 24);
    ("half", j): the job of the j-th half of the index set"""
    c = case(k)
    if which == "job":
        return _JOBS[k]
    if which == "small":
        return key_level_job(k, c["index"], [c["search"]], c["max_kmer_small"])
    return key_level_job(k, c["jobs"][which[1]], [c["search"]], c["max_kmer"])
