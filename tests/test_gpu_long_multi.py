"""commet_index_many_and_search on a search set of LONG reads: the chunk filters of several jobs side by side in one pass of
search_long_kernel (long_search.hpp, job_mask) — every job's tags and numbers must be what commet_index_and_search gives for that
job alone, and what the CPU checker gives.  The shared pass is not auto's choice (MEASUREMENTS.md, "Long reads"): every case asks
for it with multi_job = 2 and forces the kernels with long_search = 2 / index_mode, as test_gpu_multi.py and
test_gpu_long_search.py do."""
import os

import numpy as np
import pytest

import oracle_binding as ob
import util

pytestmark = pytest.mark.gpu

INDEX_LEN = 600          # bases per index read
PER_CHUNK = 20           # index reads per chunk under _max_kmer (a chunk also swallows the read it has fetched when it closes, index_reads.h:51)


def _rand(rng, n):
    return util.ACGT[rng.integers(0, 4, size=n)].tobytes()


def _max_kmer(k):
    return PER_CHUNK * (INDEX_LEN - k + 1)


def _index_set(rng, n_chunks):
    """reads that plan as n_chunks chunks under _max_kmer"""
    return [_rand(rng, INDEX_LEN) for _ in range(n_chunks * (PER_CHUNK + 1) - 5)]


def _search_set(rng, pools, n, lo, hi):
    return [r if len(r) else b"A" for r in util.related_reads(rng, sum(pools, []), n, lo, hi, share=0.4, n_rate=0.002)]


def _passes(chunks):
    """consecutive jobs while their chunks fit eight slots"""
    passes, g = 1, 0
    for c_ in chunks:
        if g + c_ > 8:
            passes, g = passes + 1, 0
        g += c_
    return passes


def _context(commet, k, t, max_kmer, index_mode=2, long_search=2, multi_job=2):
    ctx = commet.Context(k=k, t=t)
    ctx.set_option("long_search", long_search)
    ctx.set_option("index_mode", index_mode)
    ctx.set_option("max_kmer", max_kmer)
    ctx.set_option("multi_job", multi_job)           # (unknown value before long-read sets shared passes)
    return ctx


def _numbers(st):
    return {f: st[f] for f in ("indexed", "searched", "shared")}


def _together(ctx, irs, srs, sels=None, search_select=None):
    ctx.set_option("kernel_timing", 1)
    tags, stats, info = ctx.index_many_and_search(irs, srs, index_selects=sels, search_select=search_select)
    times = ctx.kernel_times()
    ctx.set_option("kernel_timing", 0)
    return tags, stats, info, times


def _check_against_alone(ctx, irs, srs, sels=None, expect_chunks=None, shared=True):
    """the jobs alone, then together: the same tags and numbers; the launches of a shared run.  Returns the shared run"""
    sels = sels or [None] * len(irs)
    alone = [ctx.index_and_search(rs, [srs], index_select=sel) for rs, sel in zip(irs, sels)]
    chunks = [a[2]["n_chunks"] for a in alone]
    if expect_chunks is not None:
        assert chunks == list(expect_chunks)
    tags, stats, info, times = _together(ctx, irs, srs, sels)
    for j, a in enumerate(alone):
        assert np.array_equal(tags[j], a[0][0]), j
        assert _numbers(stats[j]) == _numbers(a[1][0]), j
    assert info["n_chunks"] == sum(chunks) and info["kmers_indexed"] == sum(a[2]["kmers_indexed"] for a in alone)
    if shared:
        passes = _passes(chunks)
        assert info["search_launches"] == passes
        assert times["search_long_kernel"][0] == passes
    return tags, stats, info, times, alone


# ---- 1. jobs of 1 / 2 / 3 / 1 / 4 chunks: two passes ------------------------------------------------------------------------------
def test_five_jobs_share_two_passes():
    import commet_amd as commet
    k, t = 26, 2
    rng = np.random.default_rng(1)
    layout = (1, 2, 3, 1, 4)
    pools = [_index_set(rng, c_) for c_ in layout]
    search = _search_set(rng, pools, 3000, 300, 6000)
    with _context(commet, k, t, _max_kmer(k)) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
        tags, stats, info, times, alone = _check_against_alone(ctx, irs, srs, expect_chunks=layout)
        assert info["search_launches"] == 2 and times["search_long_kernel"][0] == 2
        assert "search_group8_kernel" not in times and "search_kernel" not in times
        assert all(a[1][0]["shared"] > 50 for a in alone)              # (the jobs do find reads)


# ---- 2. per-job separation at block edges, against the CPU checker ----------------------------------------------------------------
K, T = 32, 2
FHW = [63, 64, 65, 127, 128, 129, 256, 257, 1000]     # first-hit windows of the search reads


def _oracle(d, k, t, index_reads, search, max_kmer):
    """the CPU checker on one job -> (tags, (indexed, searched, shared), chunks)"""
    os.makedirs(d, exist_ok=True)
    util.write_fasta(os.path.join(d, "I.fa"), index_reads)
    util.write_fasta(os.path.join(d, "Q.fa"), search)
    open(os.path.join(d, "i.txt"), "w").write("I:I.fa\n")
    open(os.path.join(d, "s.txt"), "w").write("Q:Q.fa\n")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", "out", "log", k, t, max_kmer=max_kmer)
    finally:
        os.chdir(cwd)
    assert rc == 0
    _, n, bits = util.read_bv(os.path.join(d, "out", "Q.fa_in_I.bv"))
    assert n == len(search)
    r = res[0]
    return util.bits_from_bools(util.bools_from_bits(bits, n)), (r["indexed"], r["searched"], r["shared"]), chunks


def _plants(n_win, k):
    """per search read: the window starts whose k-mers go into (job A's second chunk, job B's first chunk, job B's second chunk, job
    C's only chunk as reverse complements), and whether A / B / C find the read (test_gpu_long_search.py, PLANTS: the same edges)"""
    last = n_win - 1
    out = [
        ((62, 94), (40, 72), (0, 32), (10, 50), (True, True, True)),          # next_free carried over the first block edge (A), exactly k apart across it (B)
        ((62, 93), (63, 95), (63, 95), (62, 93), (False, True, False)),       # one window too close (A, C); last window of a block (B)
        ((last - k, last), (0, last), (last - k, last), (last - k, last), (True, True, True)),   # the read's last two windows that hold t hits
        ((40, 71), (5, 20), (0, 32), (5,), (False, True, False)),             # B's first chunk misses (its two hits overlap): its second one counts
    ]
    if n_win > 250:
        out.append(((127, 159), (100, 191), (5, 40), (192, 250), (True, True, True)))            # second block edge, fourth block
    return [v for v in out if all(0 <= s < n_win for p in v[:4] for s in p)]


def test_jobs_stay_apart_at_block_edges(tmp_path):
    """Job A is found only in its second chunk; job B in its first, and its second chunk would hit too (it must neither count nor
    scan); job C only on the reverse strand; job D never.  All four in one pass, on reads whose window counts straddle the block of
    64.  Tags and stats of every job against the CPU checker: `searched` is the scanned counter of a job's last chunk, and the call
    itself fails when a chunk's scanned counter is not the host plan's."""
    import commet_amd as commet
    rng = np.random.default_rng(2)
    M = 100                                            # max_kmer: index reads are single k-mers, a chunk holds M of them
    search, a2, b1, b2, c1, expect = [], [], [], [], [], []
    for f in FHW:
        L = f + T * K - 1
        for pa, pb1, pb2, pc, found in _plants(L - K + 1, K):
            read = _rand(rng, L)
            a2 += [read[s:s + K] for s in pa]
            b1 += [read[s:s + K] for s in pb1]
            b2 += [read[s:s + K] for s in pb2]
            c1 += [util.revcomp(read[s:s + K]) for s in pc]
            search.append(read)
            expect.append(found)
    assert max(len(a2), len(b1), len(b2)) <= M - 10 and len(c1) + 10 < M
    fill = lambda n: [_rand(rng, K) for _ in range(n)]
    # (a closing chunk swallows one more read: fillers on both sides of every chunk edge)
    jobs = [fill(M + 8) + a2,                          # A: chunk 1 holds fillers only
            b1 + fill(M + 8 - len(b1)) + b2,           # B
            c1 + fill(10),                             # C: one chunk
            fill(50)]                                  # D
    orc = [_oracle(os.path.join(str(tmp_path), f"j{j}"), K, T, reads, search, M) for j, reads in enumerate(jobs)]
    assert [o[2] for o in orc] == [2, 2, 1, 1]
    for j in range(3):                                 # the plants decide what the checker finds
        assert util.bools_from_bits(orc[j][0], len(search)).tolist() == [e[j] for e in expect], j
    assert orc[3][1][2] == 0
    assert orc[1][1][1] < len(search)                  # B's second chunk is not reached by the reads its first one tagged
    with _context(commet, K, T, M) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(reads)]) for reads in jobs]
        tags, stats, info, times = _together(ctx, irs, srs)
        assert times["search_long_kernel"][0] == 1 and info["search_launches"] == 1 and info["n_chunks"] == 6
        for j, o in enumerate(orc):
            assert tags[j].tobytes() == o[0].tobytes(), j
            assert (stats[j]["indexed"], stats[j]["searched"], stats[j]["shared"]) == o[1], j


# ---- 3. slot layouts ------------------------------------------------------------------------------------------------------------
def _layout_sets(rng, name, k):
    """-> (index sets, selections, chunks expected of each job or None)"""
    plain = {"8x1": [1] * 8, "3_5": [3, 5], "8_1_1": [8, 1, 1], "9x1": [1] * 9}
    if name in plain:
        return [_index_set(rng, c_) for c_ in plain[name]], None, plain[name]
    if name == "selection":
        pools = [_index_set(rng, c_) for c_ in (3, 1, 2)]
        sels = [util.bits_from_bools(rng.random(len(pools[0])) < 0.6), None, util.bits_from_bools(rng.random(len(pools[2])) < 0.3)]
        return pools, sels, None
    if name == "shorter_than_k":
        short = _index_set(rng, 2)
        for i in range(0, len(short), 3):
            short[i] = short[i][:int(rng.integers(1, k))]
        return [_index_set(rng, 1), short, _index_set(rng, 2)], None, None
    assert name == "all_N"
    return [_index_set(rng, 2), [b"N" * INDEX_LEN for _ in range(30)], _index_set(rng, 1)], None, None


@pytest.mark.parametrize("name,k", [("8x1", 26), ("3_5", 26), ("8_1_1", 26), ("9x1", 26), ("selection", 26), ("shorter_than_k", 26),
                                    ("all_N", 26), ("3_5", 33)])
def test_slot_layouts(name, k):
    import commet_amd as commet
    rng = np.random.default_rng(30 + k)
    pools, sels, expect = _layout_sets(rng, name, k)
    search = _search_set(rng, [p for p in pools if p[0][:1] != b"N"], 500, 300, 3000)
    with _context(commet, k, 2, _max_kmer(k)) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
        # (a set without a k-mer has no chunk: such a call runs job by job — same bits)
        _check_against_alone(ctx, irs, srs, sels, expect_chunks=expect, shared=name != "all_N")


# ---- 4. chunks built by index_kernel in a shared pass -------------------------------------------------------------------------------
def test_atomic_build_chunks_share_a_pass_of_long_reads():
    import commet_amd as commet
    k = 26
    rng = np.random.default_rng(4)
    layout = (2, 3, 1, 4)
    pools = [_index_set(rng, c_) for c_ in layout]
    search = _search_set(rng, pools, 500, 300, 3000)
    with _context(commet, k, 2, _max_kmer(k), index_mode=1) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
        sels = [None, util.bits_from_bools(rng.random(len(pools[1])) < 0.7), None, None]
        tags, stats, info, times, _ = _check_against_alone(ctx, irs, srs, sels)
        assert info["search_launches"] == 2 and times["index_kernel"][0] == info["n_chunks"]
        assert not any(name.startswith("part_") for name in times)


def test_atomic_build_chunks_keep_short_read_sets_job_by_job():
    """a search set of 100-base reads (the register-mask kernel) takes only chunks of the bucketed build into a shared pass"""
    import commet_amd as commet
    k = 26
    rng = np.random.default_rng(5)
    pools = [_index_set(rng, c_) for c_ in (2, 1, 2)]
    search = _search_set(rng, pools, 2000, 100, 100)
    with _context(commet, k, 2, _max_kmer(k), index_mode=1, long_search=0) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
        tags, stats, info, times, _ = _check_against_alone(ctx, irs, srs, shared=False)
        assert info["search_launches"] >= len(irs) and "search_long_kernel" not in times


# ---- 5. fallbacks: the same bits ----------------------------------------------------------------------------------------------------
def test_fallbacks_give_the_same_bits():
    import commet_amd as commet
    k = 26
    rng = np.random.default_rng(6)
    pools = [_index_set(rng, c_) for c_ in (2, 1, 3)]
    search = _search_set(rng, pools, 500, 300, 3000)
    with _context(commet, k, 2, _max_kmer(k)) as ctx:
        srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
        irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
        tags, stats, info, times = _together(ctx, irs, srs)
        assert info["search_launches"] == 1 and times["search_long_kernel"][0] == 1

        def same(other):
            t2, s2, _, _ = other
            for j in range(len(t2)):
                assert np.array_equal(t2[j], tags[j]) and _numbers(s2[j]) == _numbers(stats[j]), j

        for multi_job in (1, 0):                       # job by job on request, and auto (the shared pass of long reads is an option)
            ctx.set_option("multi_job", multi_job)
            other = _together(ctx, irs, srs)
            same(other)
            assert other[2]["search_launches"] >= len(irs)
        ctx.set_option("multi_job", 2)
        ctx.set_option("count_probes", 1)
        other = _together(ctx, irs, srs)
        ctx.set_option("count_probes", 0)
        same(other)
        assert other[2]["search_launches"] >= len(irs)
        one = _together(ctx, irs[:1], srs)             # a single job
        same(one)
        # a selection on the search set: against the jobs alone under the same selection
        ssel = util.bits_from_bools(rng.random(len(search)) < 0.4)
        t3, s3, i3, _ = _together(ctx, irs, srs, search_select=ssel)
        assert i3["search_launches"] >= len(irs)
        for j, rs in enumerate(irs):
            a = ctx.index_and_search(rs, [srs], search_selects=[ssel])
            assert np.array_equal(t3[j], a[0][0]) and _numbers(s3[j]) == _numbers(a[1][0]), j
            full, part = util.bools_from_bits(tags[j], len(search)), util.bools_from_bits(t3[j], len(search))
            assert np.array_equal(part, full & util.bools_from_bits(ssel, len(search))), j


# ---- 6. the N x N driver ------------------------------------------------------------------------------------------------------------
def test_matrix_of_long_read_sets_shares_passes(tmp_path, monkeypatch):
    from commet_amd import build, matrix
    build.build_lib()
    build.build_tools()
    rng = np.random.default_rng(7)
    base = [_rand(rng, 4000) for _ in range(60)]
    monkeypatch.chdir(tmp_path)
    lines = []
    for s in range(4):
        reads = _search_set(rng, [base], 300, 1000, 8000)
        util.write_fasta(f"s{s}.fa", reads)
        lines.append(f"s{s}: s{s}.fa\n")
    open("sets.txt", "w").write("".join(lines))
    monkeypatch.setenv("COMMET_MATRIX_KERNEL_TIMES", "1")
    launches = {}
    for multi_job in (2, 1):
        monkeypatch.setenv("COMMET_MULTI_JOB", str(multi_job))
        res = matrix.run("sets.txt", f"out{multi_job}/", k=26, t=2, verbose=False)
        launches[multi_job] = res["rank0_profile"]["kernel_ms"]["search_long_kernel"][0]
        assert all(res["matrix"][a][b] > 0 for a in range(4) for b in range(4))
    files = sorted(os.listdir("out1"))
    assert sorted(os.listdir("out2")) == files
    compared = [f for f in files if f.endswith((".bv", ".csv"))]
    assert sum(f.endswith(".csv") for f in compared) == 3 and sum(f.endswith(".bv") for f in compared) >= 12
    for f in compared:
        assert open(os.path.join("out1", f), "rb").read() == open(os.path.join("out2", f), "rb").read(), f
    assert launches[2] < launches[1]
