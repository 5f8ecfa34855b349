"""The length-relative threshold rule (commet_amd/relative.py: thresholds) against a plain loop, and the fixtures of
test_gpu_relative.py (relative_sets.py) against the CPU checker: their designed tags are what the reference gives when every read is
judged at its own t_r.  No GPU."""
import numpy as np
import pytest

import checkers
import every_k_sets as eks
import relative_sets as rs
from commet_amd import relative


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _rule(length, k, percent, min_hits):
    w = length // k
    t = max(max(min_hits, 1), (percent * w + 99) // 100)
    return 0 if t > w else t


@pytest.mark.parametrize("k", [1, 20, 33])
def test_thresholds_follow_the_rule(k):
    lengths = [0, k - 1, k, 2 * k - 1, 2 * k, 100 * k - 1, 100 * k, 65535 * k]
    seen = set()
    for percent in (1, 33, 50, 99, 100):
        for min_hits in (1, 3):
            got = relative.thresholds(lengths, k, percent, min_hits)
            exp = [_rule(n, k, percent, min_hits) for n in lengths]
            assert got.tolist() == exp, (k, percent, min_hits)
            seen.update(exp)
    assert {0, 1, 3, 50, 99, 100, 65535} <= seen
    # min_hits below 1 behaves as 1; the ceiling is exact where percent * W_r is a multiple of 100 and one above it
    assert relative.thresholds(lengths, k, 50, 0).tolist() == relative.thresholds(lengths, k, 50, 1).tolist()
    assert relative.thresholds([200 * k, 201 * k, 202 * k], k, 50, -4).tolist() == [100, 101, 101]


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
def _tags_by_checker(tmp_path, case):
    """every read's bit from the reference's run at that read's t_r: one checker run per distinct t_r; above k = 28, where the
    checker's filter is too large for a test host, one key-level job whose counts answer every t_r"""
    k, thr = case["k"], rs.thresholds_of(case)
    out = np.zeros(len(case["search"]), dtype=bool)
    distinct = sorted(set(thr.tolist()) - {0})
    assert len(distinct) <= 6
    if k > 28:
        job = eks.key_level_job(k, case["index"], [case["search"]], case["max_kmer"], T=max(distinct))
        assert job.n_chunks == case["n_chunks"]
        for t in distinct:
            out[thr == t] = job.tags(t)[0][thr == t]
        return out
    for t in distinct:
        tags, _, chunks, _ = checkers.checker_job(tmp_path / f"t{t}", k, t, case["index"], [case["search"]], max_kmer=case["max_kmer"])
        assert chunks == case["n_chunks"]
        out[thr == t] = tags[0][thr == t]
    return out


@pytest.mark.parametrize("k,min_hits", [(k, 1) for k in rs.RAGGED_KS] + [(20, 3)])
def test_ragged_fixture_is_what_the_checker_says(tmp_path, k, min_hits):
    case = rs.ragged_set(k, min_hits)
    thr = rs.thresholds_of(case)
    exp = rs.designed_tags(case)
    assert sorted(set(thr.tolist())) == ([0, 1, 2, 3, 5, 10] if min_hits == 1 else [0, 3, 5, 10])
    assert np.array_equal(_tags_by_checker(tmp_path, case), exp)
    # the plants decide the counts, chunk by chunk (the key-level job counts without a stop)
    job = eks.key_level_job(k, case["index"], [case["search"]], case["max_kmer"])
    assert np.array_equal(job.best[0], case["best"])
    # both answers at every threshold, reads found in a chunk that is not the first, reads that share but not enough in one filter
    first = rs.first_found_chunk(case)
    for t in set(thr.tolist()) - {0}:
        assert exp[thr == t].any() and not exp[thr == t].all(), t
    assert set(first.tolist()) == {0, 1, 2, 3}
    spread = (case["best"].sum(axis=0) >= thr) & (thr > 0) & ~exp
    assert spread.sum() >= 10
    # reads whose t_r exceeds what they can hold are not found whatever they share
    assert not exp[thr == 0].any() and ((case["best"][:, thr == 0] > 0).any() == (min_hits == 3))


@pytest.mark.parametrize("k", rs.EDGE_KS)
def test_edge_fixture_is_what_the_checker_says(tmp_path, k):
    case = rs.edge_set(k)
    exp = rs.designed_tags(case)
    assert np.array_equal(_tags_by_checker(tmp_path, case), exp)
    assert exp.any() and not exp.all()


@pytest.mark.parametrize("k,w", [(20, 400), (16, 300)])
def test_long_fixture_is_what_the_checker_says(tmp_path, k, w):
    case = rs.long_set(k, w)
    lengths = [len(r) for r in case["search"]]
    for percent, exp in case["exp"].items():
        thr = relative.thresholds(lengths, k, percent, 1)
        t = (percent * w + 99) // 100
        assert thr.tolist() == [t] * 3 and t > 255
        tags, _, chunks, _ = checkers.checker_job(tmp_path / f"p{percent}", k, t, case["index"], [case["search"]], max_kmer=case["max_kmer"])
        assert chunks == 2 and tags[0].tolist() == exp, (percent, tags[0].tolist())


@pytest.mark.parametrize("k", rs.UNIFORM_KS)
def test_uniform_fixture_has_one_threshold(k):
    index, search = rs.uniform_set(k)
    lengths = [len(r) for r in search]
    assert set(relative.thresholds(lengths, k, 50, 1).tolist()) == {2} and set(relative.thresholds(lengths, k, 100, 1).tolist()) == {3}
    counts = np.full(len(index), rs.UNIFORM_LEN - k + 1)
    import oracle_pool as op
    for n in rs.UNIFORM_CHUNKS:
        assert len(op.chunks_from_counts(counts, rs.uniform_max_kmer(k, n))) == n
    # the copies decide both answers at both thresholds: a quarter of the 1 000 copies is exact, and found unless its index read is
    # one of the few dropped ones; substitutions take k-mers away from the others, and some of them fall short
    job = eks.key_level_job(k, index, [search], rs.uniform_max_kmer(k, 3), T=3)
    for t in (2, 3):
        found = job.tags(t)[0]
        assert found[::3].sum() > 200 and not found[::3].all() and not found[1::3].any()


def test_widest_reads_are_what_the_checker_says(tmp_path):
    reads = rs.widest_reads()
    assert relative.thresholds([len(r) for r in reads], 1, 100, 1).tolist() == [65535, 4, 65534]
    at = {t: checkers.checker_job(tmp_path / f"t{t}", 1, t, [b"ACGT"], [reads], max_kmer=4)[0][0].tolist() for t in (65535, 4, 65534)}
    assert [at[65535][0], at[4][1], at[65534][2]] == [True, False, True] and at[65535][2] is False
