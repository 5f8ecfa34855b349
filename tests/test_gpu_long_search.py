"""search_long_kernel (long_search.hpp): one wave per read, 64 consecutive windows per block, the reference's greedy rule on the
ballots.  Every case runs the job with `long_search` = 2 (probe-counting build and plain build) and = 1 (the lane-per-read
kernels) and compares tags, [indexed, searched, shared] and — counting — the probe count with the CPU checker run on the same
reads written as FASTA."""
import os
import shutil
import tempfile

import numpy as np
import pytest

import oracle_binding as ob
import util

pytestmark = pytest.mark.gpu

K, T = 32, 2
BLOCK = 64


# ---- the CPU checker on lists of reads ----------------------------------------------------------------------------------------
def _oracle(d, k, t, index_reads, search_sets, isel=None, ssels=None, max_kmer=0):
    """-> (tags [bits per search set], stats [(indexed, searched, shared)], probes, chunks, kmers)"""
    os.makedirs(d, exist_ok=True)

    def put(name, reads, sel):
        util.write_fasta(os.path.join(d, name + ".fa"), reads)
        if sel is None:
            return f"{name}:{name}.fa"
        util.write_bv(os.path.join(d, name + ".bv"), "sel", sel)
        return f"{name}:{name}.fa,{name}.bv"

    ssels = ssels or [None] * len(search_sets)
    open(os.path.join(d, "i.txt"), "w").write(put("I", index_reads, isel) + "\n")
    open(os.path.join(d, "s.txt"), "w").write("".join(put(f"Q{q:02d}", rs, ssels[q]) + "\n" for q, rs in enumerate(search_sets)))
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", "out", "log", k, t, max_kmer=max_kmer)
    finally:
        os.chdir(cwd)
    assert rc == 0
    by = {r["name"]: r for r in res}
    tags, stats = [], []
    for q, rs in enumerate(search_sets):
        _, n, bits = util.read_bv(os.path.join(d, "out", f"Q{q:02d}.fa_in_I.bv"))
        assert n == len(rs)
        tags.append(util.bits_from_bools(util.bools_from_bits(bits, n)))
        r = by[f"Q{q:02d}"]
        stats.append((r["indexed"], r["searched"], r["shared"]))
    return tags, stats, sum(r["probes"] for r in res), chunks, kmers


def _bits(sel):
    return None if sel is None else util.bits_from_bools(sel)


RUNS = ((2, 1), (2, 0), (1, 0))     # (long_search, count_probes)


def _check(tmp, k, t, index_reads, search_sets, isel=None, ssels=None, max_kmer=0, opts=(), runs=RUNS, expect_chunks=None,
           between=None):
    """the job under every (long_search, count_probes) of `runs` against the CPU checker; returns the checker's tags"""
    import commet_amd as commet
    exp_tags, exp_stats, exp_probes, chunks, kmers = _oracle(os.path.join(str(tmp), "orc"), k, t, index_reads, search_sets, isel, ssels, max_kmer)
    if expect_chunks is not None:
        assert chunks == expect_chunks
    for long_search, counting in runs:
        with commet.Context(k=k, t=t) as ctx:
            irs = commet.ReadSet.from_files(ctx, [util.to_batch(index_reads)])
            srs = [commet.ReadSet.from_files(ctx, [util.to_batch(r)]) for r in search_sets]
            ctx.set_option("long_search", long_search)
            ctx.set_option("count_probes", counting)
            ctx.set_option("max_kmer", max_kmer)
            ctx.set_option("kernel_timing", 1)
            for name, value in opts:
                ctx.set_option(name, value)
            if between:
                between(irs, srs)
            tags, stats, info = ctx.index_and_search(irs, srs, _bits(isel), None if ssels is None else [_bits(s) for s in ssels])
            what = f"long_search={long_search} count_probes={counting} k={k} t={t}"
            assert info["n_chunks"] == chunks and info["kmers_indexed"] == kmers, what
            if counting:
                assert info["probes"] == exp_probes, what
            for q in range(len(search_sets)):
                assert (stats[q]["indexed"], stats[q]["searched"], stats[q]["shared"]) == exp_stats[q], (what, q)
                assert tags[q].tobytes() == exp_tags[q].tobytes(), (what, q)
            kt = ctx.kernel_times()
            searched = any(len(r) for r in search_sets) and chunks > 0
            if long_search == 2 and searched:
                assert kt.get("search_long_kernel", (0, 0.0))[0] > 0, what
            if long_search == 1:
                assert "search_long_kernel" not in kt, what
            for r in [irs] + srs:
                r.close()
    return exp_tags


def _rand(rng, n):
    return util.ACGT[rng.integers(0, 4, size=n)].tobytes()


# ---- 1. block boundaries ---------------------------------------------------------------------------------------------------------
# a plant = (forward window starts, reverse window starts, found?): the k-mers of those windows of the read (or their reverse
# complements) are the index set's reads, nothing else of the read is
PLANTS = [
    ((62, 94), (), True),            # a hit in windows 60..63, the next allowed window (62 + k) in the following block: next_free is carried
    ((62, 93), (), False),           # ... and one window earlier is still forbidden there
    ((61, 70, 92), (), False),       # (both later ones overlap the first)
    ((40, 72), (), True),            # exactly k apart across the block edge
    ((40, 71), (), False),           # k - 1 apart across the edge: the second is rejected
    ((63, 95), (), True),            # last window of a block, first allowed one k later
    ((0, 32), (), True),
    ((0, 31), (), False),
    ((), (10, 50), True),            # the only hits are on the reverse strand
    ((), (62, 93), False),
    ((5,), (20, 60), True),          # fewer than t forward hits, then reverse hits: found on the reverse strand alone
    ((5,), (60,), False),            # one hit per strand is not two: the reverse scan starts afresh
    ((5, 20), (60,), False),         # (5 and 20 overlap)
    ((120, 127), (), False),
    ((127, 159), (), True),          # second block edge
    ((100, 191), (192, 250), True),
    ((0,), (), False),
    ((), (), False),
]
FHW = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]


def _boundary_sets(rng, k=K, t=T):
    lens = [f + t * k - 1 for f in FHW] + [k - 1, k, t * k - 1, t * k]
    index, search, expect = [], [], []
    for L in lens:
        for fw, rv, found in PLANTS:
            n_win = L - k + 1
            if any(s >= n_win for s in fw + rv):
                if fw or rv:
                    continue
            read = _rand(rng, L)
            for s in fw:
                index.append(read[s:s + k])
            for s in rv:
                index.append(util.revcomp(read[s:s + k]))
            search.append(read)
            expect.append(found)
        # the read's last two windows that can hold t hits, and one base too close to the end
        if L >= t * k:
            read = _rand(rng, L)
            index += [read[L - 2 * k:L - k], read[L - k:]]
            search.append(read)
            expect.append(True)
        if L > t * k:
            read = _rand(rng, L)
            index += [read[L - 2 * k + 1:L - k + 1], read[L - k:]]
            search.append(read)
            expect.append(False)
    return index, search, expect


def test_block_boundaries(tmp_path):
    rng = np.random.default_rng(1)
    index, search, expect = _boundary_sets(rng)
    assert len(search) > 150
    exp = _check(tmp_path, K, T, index, [search])
    assert util.bools_from_bits(exp[0], len(search)).tolist() == expect     # the plants decide what the checker finds


# ---- 2. validity -----------------------------------------------------------------------------------------------------------------
def _with(read, edits):
    s = bytearray(read)
    for a, b, ch in edits:
        s[a:b] = ch * (b - a)
    return bytes(s)


def test_validity_bits_at_block_edges(tmp_path):
    rng = np.random.default_rng(2)
    index, search = [], []
    for L in (200, 400, 1000):
        for t_edits in (
            [(63 + K - 1, 63 + K, b"N")],                    # the last base of a block's last window
            [(64, 65, b"N")],                                 # the first base of the next block
            [(63 + K - 1, 63 + K, b"N"), (64, 65, b"N")],
            [(70, 170, b"N")],                                # no complete window in more than 64 starts
            [(0, 150, b"N")],
            [(30, 31, b"N"), (130, 131, b"n"), (190, 191, b"R")],
            [(L - 1, L, b"N")],
            [(0, 1, b"N")],
        ):
            read = _rand(rng, L)
            index.append(read)                                # every clean window of the search read is a k-mer of the index set
            search.append(_with(read, t_edits))
            search.append(_with(read, t_edits).lower())
            search.append(util.revcomp(_with(read, t_edits)))
            mixed = bytearray(_with(read, t_edits))
            mixed[50:120] = bytes(mixed[50:120]).lower()
            search.append(bytes(mixed))
    for t in (2, 5):
        _check(tmp_path / f"t{t}", K, t, index, [search])


# ---- 3. parameters ---------------------------------------------------------------------------------------------------------------
def _related(seed, n_index=40, index_len=600, n_search=160, lo=40, hi=1500):
    rng = np.random.default_rng(seed)
    index = [_rand(rng, index_len) for _ in range(n_index)]
    search = util.related_reads(rng, index, n_search, lo, hi, share=0.6, n_rate=0.004)
    search = [r if len(r) else b"A" for r in search]
    return index, search


@pytest.mark.parametrize("k", [12, 20, 25, 32, 33, 36])
@pytest.mark.parametrize("t", [1, 2, 5, 60])
def test_k_and_t(tmp_path, k, t):
    """t = 60: more hits than a read of 1500 bases holds at k >= 25 (t_eff), and than most hold at smaller k"""
    index, search = _related(100 + k)
    if k == 12:                      # 2^12 keys: a filter of random 600-base reads answers yes to everything; keep it sparse
        index = index[:2]
    _check(tmp_path, k, t, index, [search], opts=(("slice_mode", 1),))


@pytest.mark.parametrize("k", [32, 33])
@pytest.mark.parametrize("n_chunks,chunk_group", [(1, 8), (2, 8), (3, 8), (5, 8), (8, 8), (5, 4), (3, 2), (8, 3), (3, 1)])
def test_chunk_filters_per_pass(tmp_path, k, n_chunks, chunk_group):
    """1, 2, 3, 5 and 8 chunk filters in a pass (NF = 1, 2, 4, 8, 8), and the remainder groups of smaller chunk_group values"""
    index, search = _related(200 + n_chunks)
    # reads per chunk: a chunk closes at max_kmer k-mers, and the reference drops the read it has fetched by then (index_reads.h:51)
    per_chunk = -(-len(index) // n_chunks) - 1
    max_kmer = 0 if n_chunks == 1 else per_chunk * (len(index[0]) - k + 1)
    _check(tmp_path, k, T, index, [search], max_kmer=max_kmer, opts=(("chunk_group", chunk_group),), expect_chunks=n_chunks)


# ---- 4. shapes of sets -----------------------------------------------------------------------------------------------------------
def test_one_read(tmp_path):
    rng = np.random.default_rng(4)
    read = _rand(rng, 700)
    _check(tmp_path / "a", K, T, [read], [[read]])
    _check(tmp_path / "b", K, T, [read], [[_rand(rng, 700)]])
    _check(tmp_path / "c", K, T, [read], [[b"ACGT"]])


def test_ragged_3000(tmp_path):
    rng = np.random.default_rng(5)
    index = [_rand(rng, 2000) for _ in range(100)]
    search = [r if len(r) else b"A" for r in util.related_reads(rng, index, 3000, 50, 5000, share=0.3, n_rate=0.002)]
    _check(tmp_path, K, T, index, [search], max_kmer=70000)            # three chunks


def test_one_long_read_among_short(tmp_path):
    rng = np.random.default_rng(6)
    index = [_rand(rng, 100) for _ in range(300)] + [_rand(rng, 3000)]
    search = [r if len(r) else b"A" for r in util.related_reads(rng, index[:300], 2000, 100, 100, share=0.3)]
    long_read = bytearray(_rand(rng, 20000))
    long_read[15000:15100] = index[300][500:600]                        # its only shared stretch, far into the read
    search.insert(1234, bytes(long_read))
    search.insert(77, _rand(rng, 20000))
    _check(tmp_path, K, T, index, [search])


@pytest.mark.parametrize("sparse", [1, 2])
def test_selection(tmp_path, sparse):
    """search_select leaving a third of the reads: as a bitmap (sparse_search = 1) and as the list of the pass (= 2)"""
    rng = np.random.default_rng(7)
    index, search = _related(7, n_search=900)
    ssel = rng.random(len(search)) < 0.33
    isel = rng.random(len(index)) < 0.8
    per = 6 * (len(index[0]) - K + 1)
    _check(tmp_path, K, T, index, [search, search[::-1]], isel=isel, ssels=[ssel, None], max_kmer=per,
           opts=(("sparse_search", sparse),), runs=((2, 0), (1, 0)) + (((2, 1),) if sparse == 1 else ()))


def test_offloaded_and_restored_set(tmp_path):
    index, search = _related(8, n_search=500)

    def away_and_back(irs, srs):
        for r in srs + [irs]:
            r.offload()
            assert not r.resident
        for r in [irs] + srs:
            r.restore()

    _check(tmp_path, K, T, index, [search], between=away_and_back)


def test_index_many_and_search(tmp_path):
    """three index sets against one search set in one call: the same tags as job by job, which the checker pins"""
    import commet_amd as commet
    rng = np.random.default_rng(9)
    pools = [[_rand(rng, 500) for _ in range(20)] for _ in range(3)]
    search = [r if len(r) else b"A" for r in util.related_reads(rng, sum(pools, []), 800, 40, 1200, share=0.5, n_rate=0.003)]
    exp = [_oracle(os.path.join(str(tmp_path), f"j{j}"), K, T, pools[j], [search]) for j in range(3)]
    for long_search in (2, 1):
        with commet.Context(k=K, t=T) as ctx:
            ctx.set_option("long_search", long_search)
            ctx.set_option("kernel_timing", 1)
            srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
            irs = [commet.ReadSet.from_files(ctx, [util.to_batch(p)]) for p in pools]
            tags, stats, info = ctx.index_many_and_search(irs, srs)
            for j in range(3):
                assert tags[j].tobytes() == exp[j][0][0].tobytes(), (long_search, j)
                assert (stats[j]["indexed"], stats[j]["searched"], stats[j]["shared"]) == exp[j][1][0], (long_search, j)
            assert ("search_long_kernel" in ctx.kernel_times()) == (long_search == 2)


# ---- 5. the feature is taken, and only where it should be -------------------------------------------------------------------------
def test_option_and_kernel_times(tmp_path):
    import commet_amd as commet
    index, search = _related(10, n_search=300)
    for long_search in (2, 1):
        with commet.Context(k=K, t=T) as ctx:
            ctx.set_option("long_search", long_search)             # (unknown option before search_long_kernel existed)
            ctx.set_option("kernel_timing", 1)
            irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
            srs = commet.ReadSet.from_files(ctx, [util.to_batch(search)])
            ctx.index_and_search(irs, [srs])
            kt = ctx.kernel_times()
            if long_search == 2:
                assert kt["search_long_kernel"][0] > 0
            else:
                assert "search_long_kernel" not in kt and ("search_kernel" in kt or "search_group_kernel" in kt)
    with commet.Context(k=K, t=T) as ctx:
        with pytest.raises(commet.CommetError):
            ctx.set_option("long_search", 3)


def test_auto_keeps_the_fast_paths_of_short_reads():
    """long_search = 0: a 2^20-read set of 100-base reads still takes the tiled search, a small one no wave-per-read kernel"""
    import commet_amd as commet
    rng = np.random.default_rng(11)
    with commet.Context(k=K, t=T) as ctx:
        ctx.set_option("long_search", 0)
        ctx.set_option("kernel_timing", 1)
        n = 1 << 20
        bases = util.ACGT[rng.integers(0, 4, size=n * 100)]
        offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(100)
        big = commet.ReadSet.from_files(ctx, [(bases, offs)])
        irs = commet.ReadSet.from_files(ctx, [(bases[:100 * 4096].copy(), offs[:4097].copy())])
        tags, stats, _ = ctx.index_and_search(irs, [big])
        kt = ctx.kernel_times()
        assert kt["tq_probe_kernel"][0] > 0 and "search_long_kernel" not in kt
        assert stats[0]["shared"] >= 4096
        ctx.set_option("kernel_timing", 1)                         # (resets the totals)
        small = commet.ReadSet.from_files(ctx, [(bases[:100 * 3000].copy(), offs[:3001].copy())])
        ctx.index_and_search(irs, [small])
        assert "search_long_kernel" not in ctx.kernel_times()


# ---- 6. randomised ---------------------------------------------------------------------------------------------------------------
def _stretched_scenario(d, seed, k):
    """a scenario of the suite's generator (tests/scenarios.py) with its read lengths stretched to 30..3000"""
    import scenarios
    real = util.related_reads

    def stretched(rng, pool, n, len_lo, len_hi, **kw):
        return real(rng, pool, n, 30, 3000, **kw)

    util.related_reads = stretched
    try:
        return scenarios.Scenario(d, seed, k=k)
    finally:
        util.related_reads = real


@pytest.mark.parametrize("seed", range(100))
def test_randomised_scenarios(seed):
    import commet_amd as commet
    from fuzz_cases import load_set
    from scenarios import run_oracle
    d = tempfile.mkdtemp(prefix="longfuzz")
    try:
        k = [12, 16, 20, 25, 28, 31, 32, 33, 34, 13][seed % 10]
        scn = _stretched_scenario(os.path.join(d, "s"), 3000 + seed, k)
        max_kmer = [0, 4000, 20000][seed % 3]
        rc, res, chunks, kmers = run_oracle(scn, os.path.join(d, "o"), os.path.join(d, "l"), max_kmer=max_kmer)
        assert rc == 0
        with commet.Context(k=scn.k, t=scn.t) as ctx:
            counting = seed % 2 == 0
            ctx.set_option("long_search", 2)
            ctx.set_option("slice_mode", 1)
            ctx.set_option("count_probes", int(counting))
            ctx.set_option("max_kmer", max_kmer)
            ctx.set_option("chunk_group", 1 + (seed // 2) % 8)
            if not counting and seed % 3 == 1:
                ctx.set_option("sparse_search", 2)
            irs, isel = load_set(commet, ctx, scn.sets[scn.index_name], scn.dir)
            names = sorted(scn.search_names)
            loaded = [load_set(commet, ctx, scn.sets[nme], scn.dir) for nme in names]
            tags, stats, info = ctx.index_and_search(irs, [x[0] for x in loaded], isel, [x[1] for x in loaded])
            assert info["n_chunks"] == chunks and info["kmers_indexed"] == kmers
            if counting:
                assert info["probes"] == sum(r["probes"] for r in res)
            by = {r["name"]: r for r in res}
            for nme, tg, st in zip(names, tags, stats):
                o = by[nme]
                assert (st["indexed"], st["searched"], st["shared"]) == (o["indexed"], o["searched"], o["shared"]), nme
                pos = 0
                for fa, _, reads, _ in scn.sets[nme]:
                    _, n, bits = util.read_bv(os.path.join(d, "o", os.path.basename(fa) + "_in_" + scn.index_name + ".bv"))
                    assert np.array_equal(util.bools_from_bits(tg, pos + n)[pos:pos + n], util.bools_from_bits(bits, n)), (nme, fa)
                    pos += n
    finally:
        shutil.rmtree(d, ignore_errors=True)
