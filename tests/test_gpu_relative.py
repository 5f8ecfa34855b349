"""commet_index_and_search_relative and commet_readset_relative_thresholds (capi/relative.hpp; relative_search.hpp): a threshold per
read, t_r = max(min_hits, ceil(percent / 100 x len // k)).  The thresholds kernel against the rule in numpy; sets on which the rule
gives one t against the library's own search at that t, through every group size and both mappings; ragged sets against the tags their
plants decide (relative_sets.py; test_relative_cpu.py proves those against the CPU checker) and against the hit profile; thresholds
beyond a byte; the wave forms at their block edges; the refusals; and `python -m commet_amd.relative`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import checkers
import relative_sets as rs
import util
from commet_amd import relative
from conftest import ROOT

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "commet_amd", "bin", "index_and_search")


def _commet():
    import commet_amd
    return commet_amd


def _set(ctx, reads):
    return _commet().ReadSet.from_files(ctx, [util.to_batch(reads)])


def _bools(bits, n):
    return util.bools_from_bits(bits, n)


# ---- 1. the thresholds kernel -------------------------------------------------------------------------------------------------------
RULES = [(50, 1), (100, 1), (1, 1), (33, 3), (99, 7), (10, 0)]


@pytest.mark.parametrize("k", [20, 33])
def test_thresholds_kernel_equals_the_rule(k):
    commet = _commet()
    rng = np.random.default_rng(800 + k)
    # 4 097 reads: one read past a multiple of every block size; every length from 1 to 20 k + 40, k - 1, k and 2 k - 1 in front
    lengths = [k - 1, k, 2 * k - 1, 2 * k, 1] + rng.integers(1, 20 * k + 41, size=4092).tolist()
    ragged = [rs.rand(rng, n) for n in lengths]
    fixed = [rs.rand(rng, 100) for _ in range(4097)]
    with commet.Context(k=k, t=2) as ctx:
        for reads in (ragged, fixed):
            srs = _set(ctx, reads)
            for percent, min_hits in RULES:
                got = srs.relative_thresholds(percent, min_hits)
                exp = relative.thresholds([len(r) for r in reads], k, percent, min_hits)
                assert got.dtype == np.uint16 and np.array_equal(got, exp), (k, percent, min_hits)
            srs.close()
    assert {0, 1, 2, 10} <= set(relative.thresholds(lengths, k, 50, 1).tolist())


# ---- 2. one threshold for every read: the library's own search at that t ---------------------------------------------------------
@pytest.mark.parametrize("n_chunks", rs.UNIFORM_CHUNKS)
@pytest.mark.parametrize("k", rs.UNIFORM_KS)
def test_uniform_thresholds_equal_the_search(k, n_chunks):
    commet = _commet()
    index, search = rs.uniform_set(k)
    max_kmer = rs.uniform_max_kmer(k, n_chunks)
    exp = {}
    for t in (2, 3):
        with commet.Context(k=k, t=t) as ctx:
            ctx.set_option("max_kmer", max_kmer)
            irs, srs = _set(ctx, index), _set(ctx, search)
            tags, stats, info = ctx.index_and_search(irs, [srs])
            assert info["n_chunks"] == n_chunks
            exp[t] = (tags[0].tobytes(), stats[0]["shared"])
            if t == 3:
                break
            # the same context serves the relative calls: its own t plays no part
            seen = set()
            for long_search in (0, 2):
                ctx.set_option("long_search", long_search)
                ctx.set_option("kernel_timing", 1)
                for chunk_group in (8, 4, 2, 1):
                    ctx.set_option("chunk_group", chunk_group)
                    for percent in (50, 100):
                        got, shared, rinfo = ctx.index_and_search_relative(irs, [srs], percent=percent, min_hits=1)
                        exp.setdefault(("rel", percent), []).append((long_search, chunk_group, got[0].tobytes(), int(shared[0][0]), rinfo))
                seen |= set(ctx.kernel_times())
            ctx.set_option("long_search", 0)
            assert "rel_thresholds_kernel" in seen
            assert ("rel_kernel" in seen and "rel_wave_kernel" in seen) and (("rel_group_kernel" in seen and "rel_group_wave_kernel" in seen) == (n_chunks > 1))
    assert exp[2][1] > exp[3][1] > 200                                          # (the copies: found at 2, fewer at 3)
    for percent, t in ((50, 2), (100, 3)):
        for long_search, chunk_group, bits, shared, rinfo in exp[("rel", percent)]:
            print(f"k {k} chunks {n_chunks} long_search {long_search} chunk_group {chunk_group} percent {percent}: shared {shared}, search {exp[t][1]}, "
                  f"passes {rinfo['search_launches']}, walked {rinfo['reads_scanned']}")
            assert bits == exp[t][0] and shared == exp[t][1], (long_search, chunk_group, percent)
            assert rinfo["n_chunks"] == n_chunks and rinfo["probes"] == 0
            assert rinfo["search_launches"] == -(-n_chunks // chunk_group)
            # a pass walks the reads no earlier pass has found: all of them once, the unfound ones in every pass
            assert len(search) <= rinfo["reads_scanned"] <= len(search) * rinfo["search_launches"]
            if rinfo["search_launches"] > 1:
                assert rinfo["reads_scanned"] < len(search) * rinfo["search_launches"]


# ---- 3. ragged sets -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", rs.RAGGED_KS)
def test_ragged_sets_equal_their_design_and_the_profile(k):
    commet = _commet()
    case = rs.ragged_set(k)
    n, nc = len(case["search"]), case["n_chunks"]
    thr = rs.thresholds_of(case)
    first = rs.first_found_chunk(case)
    sel = rs.ragged_selection(k)
    with commet.Context(k=k, t=7) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        irs, srs = _set(ctx, case["index"]), _set(ctx, case["search"])
        assert np.array_equal(srs.relative_thresholds(50, 1), thr)
        hits, pinfo = ctx.index_and_profile(irs, [srs], max_hits=255)
        assert pinfo["n_chunks"] == nc and np.array_equal(hits[0], case["best"].max(axis=0))
        for long_search in (1, 2):                                              # lane forms, wave forms
            ctx.set_option("long_search", long_search)
            for chunk_group in (8, 1):
                ctx.set_option("chunk_group", chunk_group)
                for min_hits in (1, 3):
                    c = rs.ragged_set(k, min_hits)
                    t_c = rs.thresholds_of(c)
                    exp = rs.designed_tags(c)
                    tags, shared, info = ctx.index_and_search_relative(irs, [srs], percent=50, min_hits=min_hits)
                    got = _bools(tags[0], n)
                    print(f"k {k} long_search {long_search} chunk_group {chunk_group} min_hits {min_hits}: found {int(got.sum())} of {n}, "
                          f"designed {int(exp.sum())}, walked {info['reads_scanned']} in {info['search_launches']} passes")
                    assert np.array_equal(got, exp), np.flatnonzero(got != exp)
                    assert np.array_equal(got, (t_c > 0) & (hits[0] >= np.maximum(t_c, 1)))      # the profile's bytes, thresholded per read
                    assert tags[0].tobytes() == util.bits_from_bools(exp).tobytes() and int(shared[0][0]) == int(exp.sum())
                    # a read is walked by every pass up to the one that finds it; never when t_r > W_r
                    f_c = rs.first_found_chunk(c)
                    walked = sum(int(((t_c > 0) & (f_c >= p)).sum()) for p in range(nc)) if chunk_group == 1 else int((t_c > 0).sum())
                    assert info["search_launches"] == (nc if chunk_group == 1 else 1) and info["reads_scanned"] == walked
                    if chunk_group == 1:
                        assert walked < nc * int((t_c > 0).sum())               # (found reads are not walked again)
                # a selection on the search set; again as a list of the selected reads
                for sparse in (1, 2):
                    ctx.set_option("sparse_search", sparse)
                    tags, shared, info = ctx.index_and_search_relative(irs, [srs], search_selects=[util.bits_from_bools(sel)], percent=50)
                    exp = rs.designed_tags(case, sel)
                    assert np.array_equal(_bools(tags[0], n), exp) and int(shared[0][0]) == int(exp.sum()), (long_search, chunk_group, sparse)
                    walked = sum(int((sel & (thr > 0) & (first >= p)).sum()) for p in range(nc)) if chunk_group == 1 else int((sel & (thr > 0)).sum())
                    assert info["reads_scanned"] == walked
                ctx.set_option("sparse_search", 0)
        assert (rs.designed_tags(case) & ~sel).any()                            # (the selection takes found reads away)


# ---- 4. thresholds beyond a byte ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,w", [(20, 400), (16, 300)])
def test_thresholds_beyond_255(tmp_path, k, w):
    """(k = 16, reads of 4 800 bases: below the length at which a set takes the wave forms by itself, so t_r > 255 alone sends it there)"""
    commet = _commet()
    case = rs.long_set(k, w)
    exp = {}
    for percent in (100, 99):
        t = (percent * w + 99) // 100
        tags, _, chunks, _ = checkers.checker_job(tmp_path / f"p{percent}", k, t, case["index"], [case["search"]], max_kmer=case["max_kmer"])
        assert chunks == 2 and t > 255
        exp[percent] = tags[0]
        assert exp[percent].tolist() == case["exp"][percent]
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        irs, srs = _set(ctx, case["index"]), _set(ctx, case["search"])
        for long_search, chunk_group, kernel, passes in ((0, 8, "rel_group_wave_kernel", 1), (0, 1, "rel_wave_kernel", 2), (1, 8, "rel_kernel", 2),
                                                        (1, 1, "rel_kernel", 2)):
            ctx.set_option("long_search", long_search)
            ctx.set_option("chunk_group", chunk_group)
            ctx.set_option("kernel_timing", 1)
            for percent in (100, 99):
                tags, shared, info = ctx.index_and_search_relative(irs, [srs], percent=percent)
                assert _bools(tags[0], 3).tolist() == exp[percent].tolist(), (long_search, chunk_group, percent)
                assert int(shared[0][0]) == int(exp[percent].sum()) and info["n_chunks"] == 2 and info["search_launches"] == passes
            kt = set(ctx.kernel_times())
            assert kernel in kt and len(kt & {"rel_kernel", "rel_wave_kernel", "rel_group_kernel", "rel_group_wave_kernel"}) == 1, kt


# ---- 5. the wave forms at their block edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", rs.EDGE_KS)
def test_wave_forms_at_block_edges(k):
    commet = _commet()
    case = rs.edge_set(k)
    n = len(case["search"])
    exp = rs.designed_tags(case)
    got = {}
    with commet.Context(k=k, t=2) as ctx:
        ctx.set_option("max_kmer", case["max_kmer"])
        irs, srs = _set(ctx, case["index"]), _set(ctx, case["search"])
        for long_search in (2, 1):
            ctx.set_option("long_search", long_search)
            for chunk_group in (8, 1):
                ctx.set_option("chunk_group", chunk_group)
                tags, shared, info = ctx.index_and_search_relative(irs, [srs], percent=case["percent"], min_hits=case["min_hits"])
                assert info["n_chunks"] == 2
                got[(long_search, chunk_group)] = _bools(tags[0], n)
    for key, g in got.items():
        assert np.array_equal(g, exp), (key, np.flatnonzero(g != exp))


# ---- 6. what is refused -------------------------------------------------------------------------------------------------------------
def test_refusals():
    commet = _commet()
    rng = np.random.default_rng(5)
    with commet.Context(k=20, t=2) as ctx:
        irs, srs = _set(ctx, [rs.rand(rng, 60) for _ in range(20)]), _set(ctx, [rs.rand(rng, 60) for _ in range(30)])
        for bad in (0, 101, -3):
            with pytest.raises(commet.CommetError, match="percent"):
                ctx.index_and_search_relative(irs, [srs], percent=bad)
            with pytest.raises(commet.CommetError, match="percent"):
                srs.relative_thresholds(bad)
        srs.offload()
        with pytest.raises(commet.CommetError, match="offloaded"):
            ctx.index_and_search_relative(irs, [srs], percent=50)
        with pytest.raises(commet.CommetError, match="offloaded"):
            srs.relative_thresholds(50)
        srs.restore()
        tags, shared, info = ctx.index_and_search_relative(irs, [srs], percent=50)
        assert not tags[0].any() and info["reads_scanned"] == 30
        tags, shared, info = ctx.index_and_search_relative(irs, [], percent=50)
        assert tags == [] and info["search_launches"] == 0
    with commet.Context(k=1, t=1) as ctx:                                       # W_r = 70 000: above what 16 bits hold
        irs, srs = _set(ctx, [b"ACGT"]), _set(ctx, [rs.rand(rng, 70000)])
        with pytest.raises(commet.CommetError, match="16 bits"):
            ctx.index_and_search_relative(irs, [srs], percent=50)
        with pytest.raises(commet.CommetError, match="16 bits"):
            srs.relative_thresholds(50)
        # the largest threshold there is: every base of the first read is a 1-mer of ACGT (the reference's max_kmer is 0 at k = 1 and
        # indexes nothing: the hook's 4 takes the read); the checker at t = 65 535 says the same (test_relative_cpu.py)
        reads = rs.widest_reads()
        ok = _set(ctx, reads)
        ctx.set_option("max_kmer", 4)
        assert ok.relative_thresholds(100).tolist() == [65535, 4, 65534]
        tags, _, info = ctx.index_and_search_relative(irs, [ok], percent=100)
        assert _bools(tags[0], 3).tolist() == [True, False, True] and info["kmers_indexed"] == 4


@pytest.mark.parametrize("which", ["found", "thr"])
def test_refused_allocation_fails_the_call_and_no_more(which):
    """the search set's bytes: n found flags, then 2 n bytes of thresholds, both larger than anything else the call asks for"""
    commet = _commet()
    rng = np.random.default_rng(6)
    k, n = 20, 200 * 1024
    index = [rs.rand(rng, k) for _ in range(50)]
    search = [index[int(rng.integers(0, 50))] if i % 5 == 0 else rs.rand(rng, k) for i in range(n)]
    exp = np.arange(n) % 5 == 0
    with commet.Context(k=k, t=2) as ctx:
        irs, small, srs = _set(ctx, index), _set(ctx, search[:100]), _set(ctx, search)
        tags, _, _ = ctx.index_and_search_relative(irs, [small], percent=100)   # everything else the job needs is in place
        assert np.array_equal(_bools(tags[0], 100), exp[:100])
        with commet.refusing_device_allocs(at_least=n if which == "found" else 2 * n) as r:
            with pytest.raises(commet.CommetError, match="cannot allocate"):
                ctx.index_and_search_relative(irs, [srs], percent=100)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == (n if which == "found" else 2 * n), r.seen
        tags, shared, _ = ctx.index_and_search_relative(irs, [srs], percent=100)
        assert np.array_equal(_bools(tags[0], n), exp) and int(shared[0][0]) == int(exp.sum())


# ---- 7. the command -------------------------------------------------------------------------------------------------------------------
def test_relative_command_writes_the_tools_vectors(tmp_path):
    if not os.path.exists(TOOL):
        from commet_amd import build
        build.build_lib()
        build.build_tools()
    k = 32
    index, search = rs.uniform_set(k)
    d = tmp_path
    util.write_fasta(str(d / "I.fa"), index[:400])
    util.write_fasta(str(d / "Q1.fa"), search[:300])
    util.write_fasta(str(d / "Q2.fa"), index[100:160] + search[300:400])
    open(d / "i.txt", "w").write("I:I.fa\n")
    open(d / "s.txt", "w").write("Q:Q1.fa;Q2.fa\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "commet_amd.relative", "-i", "i.txt", "-s", "s.txt", "-k", str(k), "--percent", "50", "-o", "rel"],
                       cwd=str(d), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    r = subprocess.run([TOOL, "-i", "i.txt", "-s", "s.txt", "-o", "tool", "-l", "tool", "-k", str(k), "-t", "2"], cwd=str(d), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    names = sorted(p for p in os.listdir(d / "tool") if p.endswith(".bv"))
    assert names == ["Q1.fa_in_I.bv", "Q2.fa_in_I.bv"]
    assert sorted(p for p in os.listdir(d / "rel") if p.endswith(".bv")) == names
    rows = [ln.split(";") for ln in open(d / "rel" / "relative.csv").read().strip().split("\n")]
    assert rows[0] == ["set", "file", "reads", "shared", "min_t", "max_t"] and len(rows) == 3
    total = 0
    for nme, row in zip(names, rows[1:]):
        assert open(d / "rel" / nme, "rb").read() == open(d / "tool" / nme, "rb").read(), nme
        _, n, bits = util.read_bv(str(d / "tool" / nme))
        shared = int(_bools(bits, n).sum())
        assert row == ["Q", nme.split("_in_")[0], str(n), str(shared), "2", "2"], row
        total += shared
    assert total >= 60                                                          # (Q2 opens with sixty index reads)
