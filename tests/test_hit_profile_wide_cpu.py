"""What the wide-row hit profile's GPU tests (test_gpu_hit_profile_wide.py) presuppose, proved without a GPU: the planted sets' chunk
counts and designed counts (through the CPU checker), the block bound the kernel prunes with (in numpy, tied to the checker), the
row plan the tests expect, and tags_at."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_wide_sets as ws
import oracle_pool
import oracle_binding as ob
import util
from conftest import ROOT
from hit_profile_group_sets import greedy, planted_palindrome
from test_hit_profile_groups_cpu import checker_counts, checker_tags


def test_row_plans():
    for k, L, n_chunks, cap, inst in ws.ROWS:
        assert ws.passes_of(n_chunks, cap)[2] == inst, (k, n_chunks)
    assert [ws.passes_of(n, c)[0] for _, _, n, c, _ in ws.ROWS] == [1, 1, 1, 1, 1, 2, 3]
    assert {r[4] for r in ws.ROWS} == {"8x1", "16x1", "32x1", "64x1", "64x2"}
    assert ws.passes_of(ws.PLANTED_CHUNKS, 8)[0] == 3 and ws.passes_of(ws.PLANTED_CHUNKS, 0)[:2] == (1, 24)
    assert {ws.random_case(s)[0] for s in ws.RANDOM_SEEDS} == set(range(12, 25))


@pytest.mark.parametrize("k", ws.PLANTED_KS)
def test_planted_reads_reach_their_counts(tmp_path, k):
    index, search, exp, names = ws.planted(k)
    counts, chunks = checker_counts(tmp_path, k, index, search, 1, 4)
    assert chunks == ws.PLANTED_CHUNKS
    assert counts.tolist() == exp, list(zip(names, counts.tolist(), exp))
    # the designs themselves: the overlapping pair has hits in two blocks, the saturated one in three, each with a lower count
    model = ws.hit_model(k, index[::2])
    for name, chunk, blocks, count in (("overlap_then_two", 5, 2, 1), ("overlap_alone", 6, 2, 1), ("saturated_bound_count_2", 27, 3, 2)):
        ends = model(search[names.index(name)])[(chunk, 0)]
        assert len({(e - (k - 1)) // k for e in ends}) == blocks and greedy([e - (k - 1) for e in ends], k) == count, name
    assert model(search[names.index("last_window_reverse")]) == {(19, 1): [149]}
    assert model(search[names.index("first_and_last_window")])[(17, 0)] == [k - 1, 149]


@pytest.mark.parametrize("k", ws.PLANTED_KS)
def test_saturation_set(tmp_path, k):
    index, search, exact = ws.saturation(k)
    for t, found in ((1, True), (exact, True), (exact + 1, False)):
        tags, chunks = checker_tags(tmp_path, k, t, index, [search], max_kmer=1)
        assert chunks == 12 and tags[0][0] == found and tags[0][1] == found and not tags[0][3], t


def test_palindrome_set_at_one_read_per_pass(tmp_path):
    index, search, exp, max_kmer, n_chunks = planted_palindrome(20)
    counts, chunks = checker_counts(tmp_path, 20, index, search, max_kmer, max(exp) + 1)
    assert chunks == n_chunks and counts.tolist() == exp


def _checker_counts_of_row(k, index, queries, t_max):
    ib, io = util.to_batch(index)
    qb, qo = util.to_batch(queries)
    chunks = oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, k), 1)
    counts = np.zeros(len(queries), dtype=int)
    for t in range(1, t_max + 1):
        found, _ = oracle_pool.chunk_loop_in_threads(k, t, ib, io, qb, qo, chunks, len(queries))
        counts[util.bools_from_bits(found, len(queries))] = t
    return counts, chunks


@pytest.mark.parametrize("k,L,n_chunks,cap,inst", ws.ROWS)
def test_block_bound_holds_on_the_random_rows(k, L, n_chunks, cap, inst):
    """the number of k-blocks of window ends that hold a full hit is at least the greedy count, per read, chunk and strand; on the rows
    the checker meets, the best greedy count over chunks and strands IS the checker's count (so the numpy hits are the filter's)"""
    index, queries = ws.row_set(k, L, n_chunks)
    ib, io = util.to_batch(index)
    chunks = oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, k), 1)
    assert abs(len(chunks) - n_chunks) <= n_chunks // 50
    model = ws.hit_model(k, [b"N".join(index[a:e]) for a, e in chunks])
    best = np.zeros(len(queries), dtype=int)
    pairs = strict = 0
    for r, q in enumerate(queries):
        for (c, strand), ends in model(q).items():
            cnt = greedy([e - (k - 1) for e in ends], k)
            blocks = len({(e - (k - 1)) // k for e in ends})
            assert blocks >= cnt >= 1, (r, c, strand, ends)
            best[r] = max(best[r], cnt)
            pairs += 1
            strict += blocks > cnt
    # half of the queries derive from an index read and half of the index reads are dropped look-ahead reads: ~300 pairs with a hit;
    # the bound is not always tight (pruning by it alone would be wrong)
    assert pairs > 100 and strict > 0
    if k == 21:
        assert set(range(5)) <= set(np.minimum(best, ws.ROW_T).tolist()), sorted(set(best.tolist()))
    if n_chunks <= ws.CHECKER_MAX_CHUNKS:
        counts, _ = _checker_counts_of_row(k, index, queries, 4)
        assert np.array_equal(np.minimum(best, 4), counts)


def test_tags_at_round_trips():
    import commet_amd
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 1000):
        hits = rng.integers(0, 9, size=n).astype(np.uint8)
        for t in (1, 2, 8):
            bits = commet_amd.tags_at(hits, t)
            assert bits.dtype == np.uint8 and bits.size == n // 8 + 1
            assert np.array_equal(util.bools_from_bits(bits, n), hits >= t)
            assert bits.tobytes() == util.bits_from_bools(hits >= t).tobytes()


def test_sweep_profile_wide_argument_errors(tmp_path):
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for bad in ("3", "-1", "x"):
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "21", "-o", "out", "--max-t", "4", "--profile-wide", bad],
                           cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--profile-wide" in r.stderr, (bad, r.stderr)
        assert not os.path.exists(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "--help"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"--profile-wide" in r.stdout
