"""What the planted tests (test_gpu_planted_search.py, test_gpu_planted_profile.py) presuppose of their read sets, proved through the
CPU checker alone: for every read of every case the designed count says exactly what the checker finds, at every t; the chunk counts;
and that every decoy shares exactly its one lane key with its k-mer (oracle_binding.keys_of_read).

The search file compares tags at the case's own t.  The profile file compares the designed count itself, as a byte: for every case it
imports, the design is proved at every t in 1 .. max(count) + 1 (_byte_ts; the last t shows that no count is larger than designed)."""
import numpy as np
import pytest

import oracle_binding as ob
import planted_sets as ps
from checkers import checker_job, key_level_search


def _design_equals_checker(tmp_path, k, ts, index, sets, max_kmer, n_chunks):
    names = list(sets)
    for t in ts:
        tags, stats, chunks, _ = checker_job(tmp_path / "orc", k, t, index, [sets[n][0] for n in names], max_kmer=max_kmer)
        assert chunks == n_chunks
        for name, tg in zip(names, tags):
            want = sets[name][1] >= t
            wrong = np.nonzero(tg != want)[0]
            assert wrong.size == 0, (k, t, name, wrong[:10].tolist())


def _byte_ts(*counts):
    """every t at which a hit byte of these designed counts says something: 1 .. max + 1"""
    return tuple(range(1, max(int(c.max()) for c in counts) + 2))


def _decoys_share_one_lane(k, decoyed):
    assert decoyed
    for y in decoyed:
        own = ob.keys_of_read(y, k)[0]
        assert own.shape == (1, 4) and tuple(own[0].tolist()) == ps.lanes(y)
        for name in ps.ORDER:
            other = ob.keys_of_read(y.translate(ps.DECOY[name]), k)[0]
            assert [j for j in range(4) if own[0, j] == other[0, j]] == [ps.KEEPS[name]], (y, name)


def _translations_share_one_lane(k, reads):
    """the whole-read ladders: every window of X.translate(...) shares exactly its one lane key with the same window of X"""
    for X in reads:
        own = ob.keys_of_read(X, k)[0]
        assert own.shape == (len(X) - k + 1, 4)
        for name in ps.ORDER:
            same = own == ob.keys_of_read(X.translate(ps.DECOY[name]), k)[0]
            want = np.zeros(4, dtype=bool)
            want[ps.KEEPS[name]] = True
            assert (same == want).all(), (X, name)


PROFILE_SWEEPS = ps.SLICED_SWEEPS + ps.TILED_SWEEPS           # the sweeps whose counts the profile file compares as bytes


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLOT_SWEEPS + ps.SMALL_SWEEPS + ps.SLICED_SWEEPS + [s for s in ps.TILED_SWEEPS if s not in ps.SLOT_SWEEPS])
def test_position_sweeps(tmp_path, k, t, n_chunks, fhws, per_chunk):
    c = ps.sweep_case(k, t, n_chunks, fhws, per_chunk)
    assert c["n_chunks"] == n_chunks or per_chunk
    byte = (k, t, n_chunks, fhws, per_chunk) in PROFILE_SWEEPS
    ts = _byte_ts(*[counts for _, counts in c["sets"].values()]) if byte else (t,)
    assert ts[-1] >= t
    _design_equals_checker(tmp_path, k, ts, c["index"], c["sets"], c["max_kmer"], c["n_chunks"])
    if (k, t, n_chunks, fhws, per_chunk) in ps.TILED_SWEEPS:   # what the tiled profile takes: every fixed-length set; at t = 1 all of them
        took = ps.tiled_sets(c)
        assert set(took) >= {f"f{fhw}" for fhw in fhws} and (t > 1 or took == list(c["sets"]))
        assert max(int(c["sets"][n][1].max()) for n in took) >= t
    for fhw in fhws:                                            # the sets are what they are named for
        reads, counts = c["sets"][f"f{fhw}"]
        assert {len(r) for r in reads} == {fhw + t * k - 1} and len(reads) % 64 and len(reads) >= 2 * fhw
        assert (counts >= t).sum() >= fhw and (counts < t).sum() >= fhw
    assert len({len(r) for r in c["sets"]["all"][0]}) > len(fhws) and len(c["sets"]["all"][0]) % 64
    assert max(len(r) for r in c["sets"]["all"][0]) - t * k + 1 <= 255
    _decoys_share_one_lane(k, c["decoyed"])


@pytest.mark.parametrize("k,n_chunks", ps.SLOT_LADDERS + ps.SLICED_LADDERS)
def test_lane_ladders(tmp_path, k, n_chunks):
    c = ps.ladder_case(k, n_chunks)
    ts = _byte_ts(*[counts for _, counts in c["sets"].values()])
    assert ts[-1] >= 3
    _design_equals_checker(tmp_path, k, ts, c["index"], c["sets"], c["max_kmer"], n_chunks)
    if (k, n_chunks) in ps.TILED_LADDERS:
        assert ps.tiled_sets(c) == ["ladder", "whole"]
    counts = c["sets"]["ladder"][1]
    assert {0, 1, 2} == set(counts.tolist()) and (counts == 0).sum() > (counts > 0).sum()
    if "whole" in c["sets"]:
        assert {0, (k + 63) // k} == set(c["sets"]["whole"][1].tolist()) and len(c["translated"]) >= 24
        _translations_share_one_lane(k, c["translated"])
    _decoys_share_one_lane(k, c["decoyed"])


@pytest.mark.parametrize("k,n_chunks", ps.JOB_LADDERS + [j for j in ps.PROFILE_JOB_LADDERS if j not in ps.JOB_LADDERS])
def test_ladders_split_between_two_index_sets(tmp_path, k, n_chunks):
    c = ps.ladder_jobs(k, n_chunks)
    ts = _byte_ts(*c["counts"])
    assert ts == (1, 2, 3)
    for j in range(2):
        _design_equals_checker(tmp_path / f"j{j}", k, ts, c["index_sets"][j], {"s": (c["search"], c["counts"][j])}, c["max_kmer"], c["n_chunks"])
    both = (c["counts"][0] > 0) & (c["counts"][1] > 0)
    assert not both.any() and (c["counts"][0] > 0).any() and (c["counts"][1] > 0).any()
    _decoys_share_one_lane(k, c["decoyed"])


def test_ladder_at_the_largest_k_against_the_key_level_checker():
    k = ps.LARGEST_K
    c = ps.ladder_case(k, 1)
    for name, (reads, counts) in c["sets"].items():
        for t in (1, 2):
            assert np.array_equal(key_level_search(c["index"], reads, k, t), counts >= t), (name, t)
    _decoys_share_one_lane(k, c["decoyed"])
    _translations_share_one_lane(k, c["translated"])


def test_degenerate_kmers_are_refused():
    assert ps.degenerate(b"A" * 20) and ps.degenerate(b"GTTG" * 5) and ps.degenerate(b"ACCA" * 5) and not ps.degenerate(b"ACGT" * 5)
