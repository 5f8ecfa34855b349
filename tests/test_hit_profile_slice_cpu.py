"""What the narrow-table hit profile's GPU tests (test_gpu_hit_profile_slice.py) presuppose, proved without a GPU: the table plans the
tests expect, the sets' chunk counts and designed counts (through the CPU checker), and the two-sided block bounds hits_sliced_kernel
prunes with (in numpy, tied to the checker): with v = the number of k-blocks of window ends that hold a full hit of one chunk filter and
strand, saturated at 3, the greedy count is at most v unless v is saturated, exactly 1 when v = 1, and at least 2 when v = 3."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_slice_sets as ss
import oracle_binding as ob
import oracle_pool
import util
from conftest import ROOT
from test_hit_profile_groups_cpu import checker_counts


def test_plans():
    for k, L, n_chunks, words, gw, passes in ss.ROWS:
        assert ss.plan(n_chunks, k, words) == (gw, passes), (k, n_chunks)
    assert {r[4] for r in ss.ROWS} == {1, 2, 4, 8} and max(r[5] for r in ss.ROWS) == 3
    assert ss.plan(140, 24, 8) == (4, 2) and ss.plan(140, 23, 8) == (8, 1)        # the clamp bites at k = 24 only
    assert ss.plan(ss.PLANTED_CHUNKS, 21) == (8, 3) and ss.plan(ss.BOUNDS_CHUNKS, ss.BOUNDS_K) == (4, 1)
    assert ss.table_bytes(16, 4) == 4 << 20
    assert {ss.random_case(s)[0] for s in ss.RANDOM_SEEDS} == set(range(12, 25))


def _bounds(k, chunk_reads, queries):
    """-> (best greedy count per query, pairs with a hit by their v): every (read, chunk, strand) meets the three bounds"""
    model = ss.hit_model(k, chunk_reads)
    best = np.zeros(len(queries), dtype=int)
    by_v = {1: 0, 2: 0, 3: 0}
    loose = 0
    for r, q in enumerate(queries):
        for (c, strand), ends in model(q).items():
            cnt = ss.greedy([e - (k - 1) for e in ends], k)
            v = min(3, len({(e - (k - 1)) // k for e in ends}))
            assert cnt >= 1 and (v == 3 or cnt <= v), (r, c, strand, ends)
            assert v != 1 or cnt == 1, (r, c, strand, ends)
            assert v < 3 or cnt >= 2, (r, c, strand, ends)
            best[r] = max(best[r], cnt)
            by_v[v] += 1
            loose += v == 2 and cnt == 1
    return best, by_v, loose


@pytest.mark.parametrize("k,L,n_chunks,words,gw,passes", [r for r in ss.ROWS if r[0] <= 16])
def test_bounds_hold_on_the_rows(k, L, n_chunks, words, gw, passes):
    index, queries = ss.row_set(k, L, n_chunks)
    assert all(set(r) <= set(b"ACGT") for r in index[::2])
    ib, io = util.to_batch(index)
    qb, qo = util.to_batch(queries)
    chunks = oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, k), 1)
    assert len(chunks) == n_chunks and all(e - a == 1 for a, e in chunks)
    best, by_v, _ = _bounds(k, index[::2], queries)
    # half of the queries derive from a chunk read: hundreds of pairs with a hit.  How they spread over v depends on L / k (a whole copy
    # hits three blocks and more), so no floor per v here: v = 1 and v = 2 are pinned by the planted sets and bounds_set below
    assert sum(by_v.values()) > 100, by_v
    counts = np.zeros(len(queries), dtype=int)
    for t in range(1, 5):
        found, _ = oracle_pool.chunk_loop_in_threads(k, t, ib, io, qb, qo, chunks, len(queries))
        counts[util.bools_from_bits(found, len(queries))] = t
    assert np.array_equal(np.minimum(best, 4), counts)
    assert len(set(counts.tolist())) >= 3 and int((counts > 0).sum()) > 60


@pytest.mark.parametrize("k", ss.PLANTED_KS)
def test_bounds_hold_on_the_planted_reads(tmp_path, k):
    index, search, exp, names = ss.planted(k)
    best, by_v, loose = _bounds(k, index[::2], search)
    assert by_v[1] and by_v[2] and by_v[3] and loose >= 2                    # the overlapping pairs: two blocks, one hit
    assert best.tolist() == exp, list(zip(names, best.tolist(), exp))
    counts, chunks = checker_counts(tmp_path, k, index, search, 1, 4)
    assert chunks == ss.PLANTED_CHUNKS and counts.tolist() == [min(4, e) for e in exp]


def test_bounds_set_pins_the_lower_bounds(tmp_path):
    k = ss.BOUNDS_K
    index, search, exp, names = ss.bounds_set(k)
    model = ss.hit_model(k, index[::2])
    blocks = lambda ends: sorted({(e - (k - 1)) // k for e in ends})
    ones = model(search[names.index("ones_everywhere")])
    assert sorted(ones) == [(3, 0), (40, 1), (41, 0)] and all(len(blocks(e)) == 1 for e in ones.values()) and len(ones[(3, 0)]) == 2
    assert {kk: blocks(e) for kk, e in model(search[names.index("blocks_i_and_i_plus_2")]).items()} == {(7, 0): [0, 2]}
    assert {kk: blocks(e) for kk, e in model(search[names.index("adjacent_blocks_apart")]).items()} == {(69, 1): [1, 2]}
    best, by_v, loose = _bounds(k, index[::2], search)
    assert best.tolist() == exp and by_v == {1: 3, 2: 2, 3: 0} and loose == 0
    counts, chunks = checker_counts(tmp_path, k, index, search, 1, 3)
    assert chunks == ss.BOUNDS_CHUNKS and counts.tolist() == exp


def test_edge_cut_has_about_its_chunks():
    index, fixed, ragged = ss.edge_cut()
    ib, io = util.to_batch(index)
    n = len(oracle_pool.chunks_from_counts(ob.kmer_counts(ib, io, ss.EDGE_K), 1))
    assert abs(n - ss.EDGE_CHUNKS) <= 4 and ss.plan(n, ss.EDGE_K) == (8, 1) and ss.plan(n, ss.EDGE_K, 2) == (2, 4)


def test_sweep_profile_slice_argument_errors(tmp_path):
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for bad in ("3", "-1", "x"):
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "21", "-o", "out", "--max-t", "4", "--profile-slice", bad],
                           cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--profile-slice" in r.stderr, (bad, r.stderr)
        assert not os.path.exists(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "--help"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"--profile-slice" in r.stdout
