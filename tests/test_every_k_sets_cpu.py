"""What test_gpu_every_k.py presupposes of every_k_sets.py, proved through the CPU checker alone.

a. key_level_job == the checker's own run of the same job (checkers.checker_job, same max_kmer) at every k whose filter fits a test
   host (k <= 26: 32 MiB or less), at t in {1, 2, t_k}: tags, [indexed, searched, shared], chunk and k-mer counts — of the case's job, of
   the job in chunks of one read (the bit-sliced kernels' form) and of the two half jobs (the shared hits pass).
b. at every k = 1 .. 38 the case cannot be passed by saying the same thing for every read: the conditions of test_case_is_mixed.  They
   are requirements on the fixtures, not measurements: a recipe that misses one gets another seed or density, never a lower bar."""
import time

import numpy as np
import pytest

import every_k_sets as eks
from checkers import checker_job

CHECKER_MAX_K = 26
_T0 = time.time()
_SPENT = {"s": 0.0}


def _against_checker(tmp_path, k, job, index, search, max_kmer, ts):
    for t in ts:
        tags, stats, chunks, kmers = checker_job(tmp_path / "orc", k, t, index, [search], max_kmer=max_kmer)
        assert (chunks, kmers) == (job.n_chunks, job.kmers_indexed), (k, t)
        wrong = np.flatnonzero(tags[0] != job.tags(t)[0])
        assert wrong.size == 0, (k, t, wrong[:10].tolist(), job.hits[0][wrong[:10]].tolist())
        assert [stats[0][f] for f in ("indexed", "searched", "shared")] == job.stats(t)[0], (k, t)


@pytest.mark.parametrize("k", [k for k in eks.KS if k <= CHECKER_MAX_K])
def test_key_level_job_equals_the_checker(tmp_path, k):
    t0 = time.time()
    c = eks.case(k)
    ts = sorted({1, 2, c["t_k"]})
    _against_checker(tmp_path / "job", k, eks.reference(k), c["index"], c["search"], c["max_kmer"], ts)
    if c["max_kmer_small"]:
        small = eks.reference(k, "small")
        assert small.n_chunks >= 33                             # more than one 32-chunk word of the tables
        _against_checker(tmp_path / "small", k, small, c["index"], c["search"], c["max_kmer_small"], ts)
    if c["jobs"]:
        for j in range(2):
            _against_checker(tmp_path / f"half{j}", k, eks.reference(k, ("half", j)), c["jobs"][j], c["search"], c["max_kmer"], [c["t_k"]])
    _SPENT["s"] += time.time() - t0
    print(f"k={k}: {time.time() - t0:.1f} s; the file so far {_SPENT['s']:.1f} s of work, {time.time() - _T0:.1f} s since import")


def _broken_by_a_letter(job, read):
    """a non-ACGT base of the read lies inside a window that is a full hit, in some chunk filter on some strand, once the base is one of ACGT"""
    k = job.k
    for x in [i for i, ch in enumerate(read) if ch not in b"ACGTacgt"][:4]:
        for base in b"ACGT":
            mended = read[:x] + bytes([base]) + read[x + 1:]
            for reverse in (False, True):
                pos, full = job.full_hits(mended, reverse)
                covers = (pos >= x) & (pos < x + k)
                if full[:, covers].any():
                    return True
    return False


@pytest.mark.parametrize("k", eks.KS)
def test_case_is_mixed(k):
    t0 = time.time()
    c = eks.case(k)
    job = eks.reference(k)
    search, n = c["search"], len(c["search"])
    assert job.n_chunks == c["n_chunks"] == eks.n_chunks_of(k)
    assert max(len(r) for r in search) <= min(256, 254 + c["t_k"] * k if k > 1 else 256)
    assert sum(1 for r in search if len(r) >= 200) >= 20
    hits = job.hits[0]
    assert c["t_k"] == int(np.median(hits[hits > 0])) >= 1
    for t in sorted({1, c["t_k"]}):
        found = int(job.tags(t)[0].sum())
        assert 10 * found >= n and 10 * (n - found) >= n, (k, t, found, n)
    assert len(set(hits.tolist())) >= 4, (k, sorted(set(hits.tolist())))
    F, R = job.F[0].max(axis=0), job.R[0].max(axis=0)
    assert (R > F).sum() >= 3 and (F > R).sum() >= 3, (k, int((R > F).sum()), int((F > R).sum()))
    if job.n_chunks > 1:                                        # (k = 37, 38: one slot under the memory rule, hence one chunk)
        later = (job.best[0].argmax(axis=0) > 0) & (hits > 0)
        assert later.sum() >= 3, (k, int(later.sum()))
    broken = 0
    for r in (search if c["broken"] is None else [search[i] for i in c["broken"]]):
        if broken < 5 and any(ch not in b"ACGTacgt" for ch in r) and _broken_by_a_letter(job, r):
            broken += 1
    assert broken >= 5, (k, broken)
    # the three-word family: R counts its planted window, each twin exactly one less
    assert len(c["family"]) == (4 * (k - 33) if k >= 34 else 0)          # every j in 0 .. k - 34, end words 2 and 3, both strands
    for f in c["family"]:
        R_read = search[f["read"]]
        pos, full = job.full_hits(R_read, f["reverse"])
        assert full[:, pos == f["end"]].any(), (k, f)
        assert f["end"] % 32 <= k - 34 and f["end"] - k + 1 < 32 * (f["end"] // 32 - 1), (k, f)     # the window starts in word w-2
        assert hits[f["read"]] >= 1 and f["twins"], (k, f)
        # (the search at t_k sees the family too: R is found there, its twins are not)
        assert int(hits[f["read"]]) == c["t_k"], (k, f, int(hits[f["read"]]), c["t_k"])
        for x in f["twins"]:
            assert int(hits[x]) == int(hits[f["read"]]) - 1, (k, f, int(hits[x]), int(hits[f["read"]]))
    if c["jobs"]:
        halves = [eks.reference(k, ("half", j)) for j in range(2)]
        assert [h.n_chunks for h in halves] == [c["n_chunks"] // 2, c["n_chunks"] - c["n_chunks"] // 2], k
        assert all(len(set(h.hits[0].tolist())) >= 3 for h in halves) and not np.array_equal(halves[0].hits[0], halves[1].hits[0])
    else:
        assert k == 1 or c["n_chunks"] == 1
    _SPENT["s"] += time.time() - t0
    print(f"k={k}: {time.time() - t0:.1f} s; the file so far {_SPENT['s']:.1f} s of work, {time.time() - _T0:.1f} s since import")
