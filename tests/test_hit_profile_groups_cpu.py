"""What the grouped hit profile's GPU tests (test_gpu_hit_profile_groups.py) presuppose of their read sets, proved through the CPU
checker alone: the chunk count of every parametrised case, and that the planted reads reach the intended counts at the intended
thresholds (found at t = count, not at t = count + 1).  Also the sweep command's --chunk-group argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hit_profile_group_sets as gs
import oracle_binding as ob
import util
from conftest import ROOT
from scenarios import Scenario, run_oracle


def checker_tags(d, k, t, index_reads, search_sets, max_kmer=0):
    """-> ([found bools per search set], chunks)"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    util.write_fasta(os.path.join(d, "I.fa"), index_reads)
    open(os.path.join(d, "i.txt"), "w").write("I:I.fa\n")
    for q, rs in enumerate(search_sets):
        util.write_fasta(os.path.join(d, f"Q{q:02d}.fa"), rs)
    open(os.path.join(d, "s.txt"), "w").write("".join(f"Q{q:02d}:Q{q:02d}.fa\n" for q in range(len(search_sets))))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", f"out{t}", f"log{t}", k, t, max_kmer=max_kmer)
    finally:
        os.chdir(cwd)
    assert rc == 0
    tags = []
    for q, rs in enumerate(search_sets):
        _, n, bits = util.read_bv(os.path.join(d, f"out{t}", f"Q{q:02d}.fa_in_I.bv"))
        assert n == len(rs)
        tags.append(util.bools_from_bits(bits, n))
    return tags, chunks


def checker_counts(d, k, index, search, max_kmer, t_max):
    """min(t_max, hits) per read of one search set, from one checker run per t; -> (counts, chunks)"""
    counts = np.zeros(len(search), dtype=int)
    for t in range(1, t_max + 1):
        tags, chunks = checker_tags(d, k, t, index, [search], max_kmer=max_kmer)
        assert not (tags[0] & (counts < t - 1)).any()         # found at t: found at t - 1
        counts[tags[0]] = t
    return counts, chunks


@pytest.mark.parametrize("k", gs.GROUP_KS + [gs.WIDE_K])
def test_group_sets_have_their_chunks_and_counts(tmp_path, k):
    for n_chunks in sorted(set(n for n, _ in gs.GROUP_CASES)) if k != gs.WIDE_K else gs.WIDE_CHUNKS:
        index, search, max_kmer = gs.group_set(k, n_chunks)
        counts, chunks = checker_counts(tmp_path / f"c{n_chunks}", k, index, search, max_kmer, 4)
        assert chunks == n_chunks
        assert {0, 1, 2, 3} <= set(counts.tolist()), (k, n_chunks, sorted(set(counts.tolist())))
        assert any(b"N" in r for r in search) and any(r != r.upper() for r in search)


def test_groups_of():
    assert gs.groups_of(9, 8) == (2, True, True) and gs.groups_of(8, 3) == (3, True, False) and gs.groups_of(5, 1) == (5, False, True)
    assert gs.groups_of(11, 8) == (2, True, False) and gs.groups_of(2, 8) == (1, True, False) and gs.groups_of(5, 4) == (2, True, True)


@pytest.mark.parametrize("case", ["states", "slots", "palindrome"])
def test_planted_reads_reach_their_counts(tmp_path, case):
    k = 20 if case == "palindrome" else 25
    index, search, exp, max_kmer, n_chunks = {"states": gs.planted_states, "slots": gs.planted_slots, "palindrome": gs.planted_palindrome}[case](k)
    counts, chunks = checker_counts(tmp_path, k, index, search, max_kmer, max(exp) + 1)
    assert chunks == n_chunks
    assert counts.tolist() == exp
    if case == "slots":
        # the best chunk of read p is chunk p: without chunk p's plants the read has one hit
        for p in (0, 7, 9):
            x = search[p]
            without = [r for r in index if r not in (x[0:k], x[40:40 + k], x[80:80 + k], util.revcomp(x[140:140 + k]))]
            tags, _ = checker_tags(tmp_path / f"w{p}", k, 2, without, [[x]], max_kmer=0)
            assert tags[0].tolist() == [False]


@pytest.mark.parametrize("k", [31, 32, 33])
def test_wave_sets_reach_their_counts(tmp_path, k):
    index, ragged, exp_r, fixed, exp_f, max_kmer = gs.wave_sets(k)
    assert len(set(len(r) for r in ragged)) > 5 and len(set(len(r) for r in fixed)) == 1
    for name, search, exp in (("r", ragged, exp_r), ("f", fixed, exp_f)):
        counts, chunks = checker_counts(tmp_path / name, k, index, search, max_kmer, 4)
        assert chunks == 3
        for i, e in enumerate(exp):
            if e is not None:
                assert counts[i] == min(4, e), (k, name, i, e, counts[i])
        assert {1, 2, 3} <= set(counts.tolist())


def test_saturation_set(tmp_path):
    index, search, exact, max_kmer = gs.saturation_set()
    for t, found in ((1, True), (exact, True), (exact + 1, False)):
        tags, chunks = checker_tags(tmp_path, 8, t, index, [search], max_kmer=max_kmer)
        assert chunks >= 9
        assert tags[0][0] == found and tags[0][2] == found, t


@pytest.mark.parametrize("seed", gs.RANDOM_SEEDS)
def test_random_scenarios_have_several_chunks(tmp_path, seed):
    k, max_kmer, chunk_group = gs.random_case(seed)
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=4.0)
    scn.t = 1
    rc, res, chunks, kmers = run_oracle(scn, str(tmp_path / "out"), str(tmp_path / "log"), max_kmer=max_kmer)
    assert rc == 0 and chunks >= 2 and 2 <= chunk_group <= 8


def test_random_scenarios_draw_every_group_size():
    assert {gs.random_case(s)[2] for s in gs.RANDOM_SEEDS} == set(range(2, 9))


def test_sweep_chunk_group_argument_errors(tmp_path):
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for bad in ("0", "9", "-1", "x"):
        r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "32", "-o", "out", "--max-t", "4", "--chunk-group", bad],
                           cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and b"--chunk-group" in r.stderr, (bad, r.stderr)
        assert not os.path.exists(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "--help"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"--chunk-group" in r.stdout
