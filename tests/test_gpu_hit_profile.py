"""commet_index_and_profile (capi/profile.hpp; hits_kernel and hits_wave_kernel, hit_profile.hpp): one hit count per read,
min(max_hits, max over the chunks of max(F, R)), must reproduce the tags of a job at EVERY threshold t in 1..max_hits — against the
CPU checker run once per t on the same files, against the library's own search, at saturation, in the wave-per-read kernel at its
block edges, and through `python -m commet_amd.sweep`."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import util
from conftest import ROOT
from scenarios import Scenario, run_oracle

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "commet_amd", "bin", "index_and_search")
GOLD = os.path.join(ROOT, "tests", "golden")


def _load_set(commet, ctx, files, sdir):
    batches = [util.to_batch(util.parse_reads(os.path.join(sdir, fa))) for fa, _, _, _ in files]
    rs = commet.ReadSet.from_files(ctx, batches)
    sel = np.concatenate([s for _, _, _, s in files]) if files else np.zeros(0, bool)
    has_bv = any(bv for _, bv, _, _ in files)
    return rs, (util.bits_from_bools(sel) if has_bv else None)


# ---- 1. every threshold against the checker ------------------------------------------------------------------------------------
T_MAX = 6
# (seed, forced k or None, index_mode); k = 32 / 33: both key widths at k == BITS and beyond (k = 33: 4 GiB filters, two seeds only)
SCENARIOS = ([(s, None, 0) for s in range(26)] + [(s, [20, 21, 24, 25][s % 4], 2) for s in range(26, 34)] +
             [(34, 31, 0), (35, 32, 0), (36, 32, 2), (37, 31, 2), (38, 33, 0), (39, 33, 0)])


def _profile_against_checker(tmp_path, seed, k, index_mode, max_kmer=0, n_scale=1.0):
    import commet_amd as commet
    scn = Scenario(str(tmp_path / "scn"), seed, k=k, n_scale=n_scale)
    names = sorted(scn.search_names)                      # std::map order
    with commet.Context(k=scn.k, t=2) as ctx:
        irs, isel = _load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
        loaded = [_load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
        ctx.set_option("index_mode", index_mode)
        ctx.set_option("max_kmer", max_kmer)
        hits, info = ctx.index_and_profile(irs, [r for r, _ in loaded], isel, [s for _, s in loaded], max_hits=T_MAX)
        for r in [irs] + [r for r, _ in loaded]:
            r.close()
    assert info["probes"] == 0
    best = 0
    for t in range(1, T_MAX + 1):
        scn.t = t                                         # (the same files: only the threshold moves)
        out_o, log_o = str(tmp_path / f"out{t}"), str(tmp_path / f"log{t}")
        rc, res, chunks, kmers = run_oracle(scn, out_o, log_o, max_kmer=max_kmer)
        assert rc == 0
        assert info["n_chunks"] == chunks and info["kmers_indexed"] == kmers, (seed, t)
        by_name = {r["name"]: r for r in res}
        for nme, h in zip(names, hits):
            assert info["reads_indexed"] == by_name[nme]["indexed"], (seed, t, nme)
            pos = 0
            for fa, _, reads, _ in scn.sets[nme]:
                _, n, bits = util.read_bv(os.path.join(out_o, os.path.basename(fa) + "_in_" + scn.index_name + ".bv"))
                exp = util.bools_from_bits(bits, n)
                print(f"seed {seed} k {scn.k} t {t} {fa}: checker {int(exp.sum())} of {n}, profile {int((h[pos:pos + n] >= t).sum())}")
                assert np.array_equal(h[pos:pos + n] >= t, exp), (seed, scn.k, t, nme, fa)
                pos += n
            assert pos == h.size and (h.size == 0 or int(h.max()) <= T_MAX)
            best = max(best, int(h.max()) if h.size else 0)
    return info, best


@pytest.mark.parametrize("seed,k,index_mode", SCENARIOS)
def test_every_threshold_matches_checker(tmp_path, seed, k, index_mode):
    _profile_against_checker(tmp_path, seed, k, index_mode)


# (reads of 5..90 bases hold few k-mers at k = 25 and 32: chunks of 20 k-mers there)
@pytest.mark.parametrize("seed,k,max_kmer", [(100 + s, [12, 16, 20, 25, 32, 13][s % 6], 20 if s % 6 in (3, 4) else [300, 900, 3000][s % 3]) for s in range(12)])
def test_every_threshold_matches_checker_over_several_chunks(tmp_path, seed, k, max_kmer):
    """a small `max_kmer`: several chunk filters, the counts folded with max over them"""
    info, _ = _profile_against_checker(tmp_path, seed, k, 0, max_kmer=max_kmer, n_scale=4.0)
    assert info["n_chunks"] >= 2


# ---- the checker on lists of reads ----------------------------------------------------------------------------------------------
def _rand(rng, n):
    return util.ACGT[rng.integers(0, 4, size=n)].tobytes()


def _checker_tags(d, k, t, index_reads, search_sets, max_kmer=0):
    """-> ([found bools per search set], chunks)"""
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


def test_best_chunk_is_not_the_first(tmp_path):
    """a read with one hit in the first chunk's filter and three in the second's: the fold keeps the larger count, and the
    first chunk alone gives the smaller"""
    import commet_amd as commet
    k = 25
    rng = np.random.default_rng(7)
    x = _rand(rng, 200)
    first = [x[0:k]] + [_rand(rng, 60) for _ in range(8)]           # 1 + 8 * 36 k-mers: the first chunk at max_kmer = 250
    second = [x[40:40 + k], x[80:80 + k], x[120:120 + k]] + [_rand(rng, 60) for _ in range(3)]
    index, search = first + second, [x, _rand(rng, 150)]
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("max_kmer", 250)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        hits, info = ctx.index_and_profile(irs, [srs], max_hits=4)
        only_first = util.bits_from_bools(np.arange(len(index)) < len(first))
        hits1, info1 = ctx.index_and_profile(irs, [srs], index_select=only_first, max_hits=4)
    assert info["n_chunks"] >= 2
    assert hits[0].tolist() == [3, 0] and hits1[0].tolist() == [1, 0]
    for t in range(1, 5):
        tags, chunks = _checker_tags(str(tmp_path / "orc"), k, t, index, [search], max_kmer=250)
        assert chunks == info["n_chunks"]
        assert np.array_equal(hits[0] >= t, tags[0]), t


# ---- 2. against the library's own search: workgroup and word edges -------------------------------------------------------------------
_SYNTH = {}


def _synth_pair(n):
    from commet_amd import synth
    if n not in _SYNTH:
        _SYNTH[n] = (synth.synth_set(0, max(n, 300), 100), synth.synth_set(1, n, 100))
    return _SYNTH[n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 20000])
def test_tags_equal_the_search_kernels(n):
    import commet_amd as commet
    (ib, io), (sb, so) = _synth_pair(n)
    seen = set()
    for t in (1, 2, 3):
        with commet.Context(k=32, t=t) as ctx:
            irs = commet.ReadSet.from_files(ctx, [(ib, io)])
            srs = commet.ReadSet.from_files(ctx, [(sb, so)])
            hits, info = ctx.index_and_profile(irs, [srs], max_hits=t)
            tags, stats, jinfo = ctx.index_and_search(irs, [srs])
            got = commet.tags_at(hits[0], t)
            print(f"n {n} t {t}: search {stats[0]['shared']} shared, profile {int((hits[0] >= t).sum())}, walked {info['reads_scanned']}")
            assert got.tobytes() == tags[0].tobytes(), (n, t)
            assert int(hits[0].max()) <= t
            assert info["n_chunks"] == jinfo["n_chunks"] == 1 and info["kmers_indexed"] == jinfo["kmers_indexed"]
            assert info["reads_scanned"] == n and info["search_launches"] == 1 and info["probes"] == 0
            seen.update(hits[0].tolist())
    if n >= 255:
        assert {0, 3} <= seen                             # (the synthetic sets share a quarter of their reads)


def test_selections_and_empty_calls():
    import commet_amd as commet
    n = 5000
    (ib, io), (sb, so) = _synth_pair(20000)
    ib, io, sb, so = ib[:n * 100], io[:n + 1], sb[:n * 100], so[:n + 1]
    rng = np.random.default_rng(3)
    with commet.Context(k=32, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [(ib, io)])
        srs = commet.ReadSet.from_files(ctx, [(sb, so)])
        srs2 = commet.ReadSet.from_files(ctx, [(sb[:257 * 100], so[:258])])
        full, _ = ctx.index_and_profile(irs, [srs], max_hits=5)
        assert int((full[0] > 0).sum()) > n // 10
        for frac, sparse in ((0.7, 0), (0.2, 0), (0.2, 1), (0.02, 2)):      # (less than half of the set: the pass walks a list)
            sel = rng.random(n) < frac
            ctx.set_option("sparse_search", sparse)
            hits, info = ctx.index_and_profile(irs, [srs, srs2], search_selects=[util.bits_from_bools(sel), None], max_hits=5)
            assert np.array_equal(hits[0], np.where(sel, full[0], 0)), (frac, sparse)
            assert np.array_equal(hits[1], full[0][:257])
            assert info["reads_scanned"] == int(sel.sum()) + 257
        ctx.set_option("sparse_search", 0)
        # an all-zero selection of the search set, of the index set; no search set at all
        hits, info = ctx.index_and_profile(irs, [srs], search_selects=[util.bits_from_bools(np.zeros(n, bool))], max_hits=5)
        assert not hits[0].any() and info["reads_scanned"] == 0
        hits, info = ctx.index_and_profile(irs, [srs], index_select=util.bits_from_bools(np.zeros(n, bool)), max_hits=5)
        assert not hits[0].any() and info["n_chunks"] == 0 and info["reads_indexed"] == 0
        hits, info = ctx.index_and_profile(irs, [], max_hits=5)
        assert hits == [] and info["n_chunks"] == 1 and info["search_launches"] == 0
        # the job is what it was: same bits before and after a profile call on the same sets
        tags, stats, _ = ctx.index_and_search(irs, [srs])
        assert tags[0].tobytes() == commet.tags_at(full[0], 2).tobytes()


# ---- 3. saturation and range ------------------------------------------------------------------------------------------------------
def test_saturation_and_range(tmp_path):
    """(each read is a set of its own, index and search: at k = 8 a chunk holds 29 k-mers, and the read that follows a full chunk is
    the reference's dropped look-ahead read)"""
    import commet_amd as commet
    k = 8
    rng = np.random.default_rng(11)
    long_read, read = _rand(rng, 3000), _rand(rng, 2000)
    exact = len(read) // k                                   # every window of `read` is a k-mer of the index set: 0, k, 2 k, ...
    with commet.Context(k=k, t=2) as ctx:
        sets = {r: (commet.ReadSet.from_files(ctx, [util.to_batch([r])]), commet.ReadSet.from_files(ctx, [util.to_batch([r])])) for r in (long_read, read)}

        def profile(r, max_hits):
            hits, info = ctx.index_and_profile(sets[r][0], [sets[r][1]], max_hits=max_hits)
            assert info["n_chunks"] == 1 and hits[0].size == 1
            return int(hits[0][0])

        for long_search in (1, 2):
            ctx.set_option("long_search", long_search)
            assert profile(long_read, 255) == 255 and profile(long_read, 1) == 1
            assert profile(read, 255) == exact and profile(read, exact) == exact and profile(read, exact + 1) == exact and profile(read, 1) == 1
        for bad in (0, 256, -1):
            with pytest.raises(commet.CommetError, match="max_hits"):
                ctx.index_and_profile(sets[read][0], [sets[read][1]], max_hits=bad)
    # the checker brackets the count: found at t = len // k, not at t + 1
    at, _ = _checker_tags(str(tmp_path / "orc"), k, exact, [read], [[read]])
    above, _ = _checker_tags(str(tmp_path / "orc"), k, exact + 1, [read], [[read]])
    sat, _ = _checker_tags(str(tmp_path / "orc2"), k, 255, [long_read], [[long_read]])
    assert at[0].tolist() == [True] and above[0].tolist() == [False] and sat[0].tolist() == [True]


# ---- 4. the wave kernel -------------------------------------------------------------------------------------------------------------
# a plant = (forward window starts, reverse window starts): the k-mers of those windows of the read (the reverse complements of the
# latter) are reads of the index set, nothing else of the read is.  K stands for the test's k
def _plants(k):
    return [
        ((62, 62 + k), ()),                 # a hit in the last windows of a block; the next allowed window lies in the following block
        ((62, 61 + k), ()),                 # ... and one window earlier the carry still forbids it
        ((63, 64), ()),                     # the last window of a block forbids the first of the next
        ((63, 63 + k, 63 + 2 * k), ()),
        ((40, 40 + k), ()), ((40, 39 + k), ()),
        ((0, k), ()), ((0, k - 1), ()),
        ((), (10, 50)),                     # hits on the reverse strand only
        ((), (62, 61 + k)),
        ((), (62, 62 + k)),
        ((5,), (20, 60)),                   # the strands differ: F = 1, R = 2
        ((0, 33, 66), (90,)),               # F = 3, R = 1
        ((5, 20), (60,)),                   # (5 and 20 overlap) F = 1, R = 1
        ((127, 127 + k), ()),               # second block edge
        ((0,), ()),
        ((), ()),
    ]


def _greedy(starts, k):
    cnt, free = 0, 0
    for s in sorted(starts):
        if s >= free:
            cnt, free = cnt + 1, s + k
    return cnt


def _wave_sets(rng, k):
    """-> (index reads, ragged search set, its expected counts, fixed-length search set, its expected counts)"""
    index, ragged, exp_r, fixed, exp_f = [], [], [], [], []
    for n_win in (1, 63, 64, 65, 128, 129, 193):
        L = n_win + k - 1
        for fw, rv in _plants(k):
            if any(s >= n_win for s in fw + rv):
                continue
            read = _rand(rng, L)
            index += [read[s:s + k] for s in fw] + [util.revcomp(read[s:s + k]) for s in rv]
            ragged.append(read)
            exp_r.append(max(_greedy(fw, k), _greedy(rv, k)))
    L = 193 + k - 1                                     # (every plant fits: the last one starts at 127 + k)
    for fw, rv in _plants(k):
        read = _rand(rng, L)
        index += [read[s:s + k] for s in fw] + [util.revcomp(read[s:s + k]) for s in rv]
        fixed.append(read)
        exp_f.append(max(_greedy(fw, k), _greedy(rv, k)))
    # N runs that split a block: every clean window of the read is a k-mer of the index set, on one strand or the other
    for L, runs in ((200, [(70, 71)]), (200, [(40, 41), (100, 130)]), (300, [(63 + k - 1, 63 + k), (64, 65)]), (257 + k, [(0, 150)]), (300, [(120, 121), (200, 202)])):
        read = _rand(rng, L)
        s = bytearray(read)
        for a, b in runs:
            s[a:b] = b"N" * (b - a)
        index += [read, ]
        ragged += [bytes(s), util.revcomp(bytes(s)), bytes(s).lower()]
        exp_r += [None, None, None]
    return index, ragged, exp_r, fixed, exp_f


@pytest.mark.parametrize("k", [31, 32, 33])                   # (33: the loader's three-word path, 64-bit keys)
def test_wave_kernel_at_block_edges(tmp_path, k):
    import commet_amd as commet
    rng = np.random.default_rng(k)
    index, ragged, exp_r, fixed, exp_f = _wave_sets(rng, k)
    assert len(set(len(r) for r in ragged)) > 5 and len(set(len(r) for r in fixed)) == 1
    got = {}
    for long_search in (2, 1):
        with commet.Context(k=k, t=2) as ctx:
            irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
            srs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in (ragged, fixed)]
            ctx.set_option("long_search", long_search)
            ctx.set_option("kernel_timing", 1)
            got[long_search], info = ctx.index_and_profile(irs, srs, max_hits=4)
            kt = ctx.kernel_times()
            assert ("hits_wave_kernel" in kt) == (long_search == 2) and ("hits_kernel" in kt) == (long_search == 1), kt
            assert info["search_launches"] == 2 and info["reads_scanned"] == len(ragged) + len(fixed)
    for q in range(2):
        assert np.array_equal(got[2][q], got[1][q]), q
    for h, exp in ((got[2][0], exp_r), (got[2][1], exp_f)):
        for i, e in enumerate(exp):
            if e is not None:
                assert int(h[i]) == min(4, e), (i, e, int(h[i]))     # the plants decide the count
    assert {1, 2, 3} <= set(got[2][0].tolist()) and 4 in set(got[2][0].tolist())   # (the N-run reads saturate)
    for t in range(1, 5):
        tags, _ = _checker_tags(str(tmp_path / "orc"), k, t, index, [ragged, fixed])
        for q in range(2):
            assert np.array_equal(got[2][q] >= t, tags[q]), (t, q)


@pytest.mark.parametrize("k", [33, 20])
def test_wave_kernel_wide_keys_and_chunks(tmp_path, k):
    """the wave kernel's 64-bit instantiation (k = 33), and its fold over several chunks (max_kmer)"""
    import commet_amd as commet
    rng = np.random.default_rng(k)
    pool = [_rand(rng, int(rng.integers(40, 400))) for _ in range(40)]
    search = util.related_reads(rng, pool, 120, 30, 500, share=0.7, n_rate=0.01)
    max_kmer = 0 if k == 33 else 2000
    got = {}
    for long_search in (2, 1):
        with commet.Context(k=k, t=2) as ctx:
            irs = commet.ReadSet.from_files(ctx, [util.to_batch(pool)])
            srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
            ctx.set_option("long_search", long_search)
            ctx.set_option("max_kmer", max_kmer)
            got[long_search], info = ctx.index_and_profile(irs, [srs], max_hits=4)
    assert np.array_equal(got[2][0], got[1][0])
    assert (info["n_chunks"] >= 2) == (k == 20)
    for t in range(1, 5):
        tags, chunks = _checker_tags(str(tmp_path / "orc"), k, t, pool, [search], max_kmer=max_kmer)
        assert chunks == info["n_chunks"]
        assert np.array_equal(got[2][0] >= t, tags[0]), t


# ---- 5. the sweep command ---------------------------------------------------------------------------------------------------------
def test_sweep_command_writes_the_tools_vectors(tmp_path):
    if not os.path.exists(TOOL):
        from commet_amd import build
        build.build_lib()
        build.build_tools()
    d = tmp_path
    os.makedirs(d / "ABCDE_bench")
    for f, copies in (("A", "A"), ("B", "BD"), ("C", "CE")):
        data = gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read()
        for c in copies:
            open(d / "ABCDE_bench" / (c + ".fa"), "wb").write(data)
    open(d / "i.txt", "w").write("A:ABCDE_bench/A.fa\n")
    open(d / "s.txt", "w").write("B:ABCDE_bench/B.fa\nCE:ABCDE_bench/C.fa;ABCDE_bench/E.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "commet_amd.sweep", "-i", "i.txt", "-s", "s.txt", "-k", "32", "--max-t", "4", "-o", "sweep"],
                       cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    rows = [ln.split(";") for ln in open(d / "sweep" / "sweep.csv").read().strip().split("\n")]
    assert rows[0] == ["t", "set", "file", "reads", "shared"] and len(rows) == 1 + 4 * 3
    shared = {(int(t), f): (int(n), int(s)) for t, _, f, n, s in rows[1:]}
    assert not [p for p in os.listdir(d / "sweep") if p.endswith(".log")]
    counts = []
    for t in range(1, 5):
        r = subprocess.run([TOOL, "-i", "i.txt", "-s", "s.txt", "-o", f"tool{t}", "-l", f"tool{t}", "-k", "32", "-t", str(t)], cwd=str(d),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()[-500:]
        names = sorted(p for p in os.listdir(d / f"tool{t}") if p.endswith(".bv"))
        assert names == ["B.fa_in_A.bv", "C.fa_in_A.bv", "E.fa_in_A.bv"]
        assert sorted(os.listdir(d / "sweep" / f"t{t}")) == names
        for nme in names:
            exp = open(d / f"tool{t}" / nme, "rb").read()
            assert open(d / "sweep" / f"t{t}" / nme, "rb").read() == exp, (t, nme)
            _, n, bits = util.read_bv(str(d / f"tool{t}" / nme))
            f = "ABCDE_bench/" + nme.split("_in_")[0]
            assert shared[(t, f)] == (n, int(util.bools_from_bits(bits, n).sum())), (t, nme)
            counts.append(shared[(t, f)][1])
    assert len(set(counts)) > 2 and counts[0] > 0          # (the thresholds tell the reads apart)
