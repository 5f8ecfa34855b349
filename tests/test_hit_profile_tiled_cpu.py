"""What the tiled hit profile's GPU tests (test_gpu_hit_profile_tiled.py) presuppose of their read sets, proved through the CPU checker
alone: every designed byte of hit_profile_tiled_sets.py at every threshold t <= T (found at t = byte, not at t = byte + 1), the chunk
counts, the mask widths the window sweep is meant to reach, and the sweep command's --profile-tiled argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_tiled_sets as ts
from conftest import ROOT
from scenarios import Scenario, run_oracle
from test_hit_profile_groups_cpu import checker_tags


def checker_counts_of(d, k, index, search_sets, max_kmer, t_max):
    """min(t_max, hits) per read of every search set, from one checker run per t; -> ([counts per set], chunks)"""
    counts = [np.zeros(len(s), dtype=int) for s in search_sets]
    chunks = None
    for t in range(1, t_max + 1):
        tags, chunks = checker_tags(d, k, t, index, search_sets, max_kmer=max_kmer)
        for c, tg in zip(counts, tags):
            assert not (tg & (c < t - 1)).any()               # found at t: found at t - 1
            c[tg] = t
    return counts, chunks


def test_window_sweep_reaches_every_mask_width():
    assert [ts.mask_words(W) for W in ts.WINDOWS] == [2, 2, 2, 3, 4, 6, 8, 8] == [ts.MASK_WORDS[W] for W in ts.WINDOWS]
    for k in ts.SWEEP_KS + (ts.WIDE_K,):
        for W in ts.WINDOWS:
            pats = ts.window_plants(k, W)
            assert (0,) in pats and (W - 1,) in pats
            if W > 64:
                assert {(31, 32), (63, 64), (5, 5 + k - 1), (5, 5 + k)} <= set(pats)
        assert ts.greedy((5, 5 + k - 1), k) == 1 and ts.greedy((5, 5 + k), k) == 2


@pytest.mark.parametrize("n_chunks", [1, 2])
@pytest.mark.parametrize("k", ts.SWEEP_KS + (ts.WIDE_K,))
def test_window_sweep_bytes(tmp_path, k, n_chunks):
    index, max_kmer, sets = ts.window_sweep(k, n_chunks)
    T = max(max(exp) for _, exp in sets.values()) + 1
    assert T >= 4
    counts, chunks = checker_counts_of(tmp_path, k, index, [sets[W][0] for W in ts.WINDOWS], max_kmer, T)
    assert chunks == n_chunks
    for W, c in zip(ts.WINDOWS, counts):
        reads, exp = sets[W]
        assert all(len(r) == k + W - 1 for r in reads)
        assert c.tolist() == exp, (k, n_chunks, W)


def test_independence_bytes(tmp_path):
    for name, index, search, exp, max_kmer, n_chunks in ts.independence_sets():
        counts, chunks = checker_counts_of(tmp_path / name, 25, index, [search], max_kmer, max(exp) + 1)
        assert chunks == n_chunks == 2 and counts[0].tolist() == exp, name
    assert 3 in ts.independence_sets()[0][3]                     # the read with F = 1, R = 3 in filter 0 and F = 2 in filter 1


def test_heavy_bytes(tmp_path):
    k = ts.HEAVY_K
    index, max_kmer, sets = ts.heavy_sets()
    T = max(max(exp) for _, exp in sets.values()) + 1
    counts, chunks = checker_counts_of(tmp_path, k, index, [sets[L][0] for L in (100, 280)], max_kmer, T)
    assert chunks == 2
    for L, c in zip((100, 280), counts):
        reads, exp = sets[L]
        assert all(len(r) == L for r in reads) and L - k + 1 <= 255
        assert c.tolist() == exp, L
        assert L // 2 - k + 1 > 20                               # the windows of a copied half read: alone a heavy scan


def test_related_and_piece_sets():
    for n in ts.PIECE_SIZES:
        index, search, max_kmer = ts.related_case(25, 2, n)
        assert len(search) == n and max(len(r) for r in search) - 25 + 1 <= 255
        sel = ts.piece_selection(n)
        assert len(sel) == n and (n < 257 or (sel[255] and not sel[256])) and (n < 513 or (sel[511] and sel[512]))
    index, search, max_kmer = ts.related_case(25, 2, 513)
    assert any(len(r) < 25 for r in search) and any(b"N" in r for r in search) and any(r != r.upper() for r in search)
    assert len(set(len(r) for r in search)) > 20


@pytest.mark.parametrize("seed", ts.RANDOM_SEEDS)
def test_random_scenarios_have_chunks_and_a_set_with_a_kmer(tmp_path, seed):
    k = ts.random_k(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    scn.t = 1
    rc, res, chunks, kmers = run_oracle(scn, str(tmp_path / "out"), str(tmp_path / "log"), max_kmer=ts.RANDOM_MAX_KMER)
    assert rc == 0 and chunks >= 3                                # passes of two filters and of one at chunk_group = 2
    longest = [max(len(r) for _, _, reads, _ in scn.sets[nme] for r in reads) for nme in scn.search_names]
    assert max(longest) >= k and max(longest) - k + 1 <= 255


def test_random_scenarios_draw_every_k():
    assert {ts.random_k(s) for s in ts.RANDOM_SEEDS} == {25, 31, 32}


def test_sweep_profile_tiled_argument_errors(tmp_path):
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for bad in ("3", "-1", "x"):
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "32", "-o", "out", "--max-t", "4", "--profile-tiled", bad],
                           cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--profile-tiled" in r.stderr, (bad, r.stderr)
        assert not os.path.exists(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "--help"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"--profile-tiled" in r.stdout
