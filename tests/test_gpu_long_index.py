"""The bucketed index construction (index_part.hpp) on sets with LONG reads: a read of more than 4096 k-mers or 4096 bases no longer
sends every chunk of its set to index_kernel.  Such launches walk the chunk's item list (LIST), written by part_items_fill_kernel and
cut into hist / scatter1 pieces by ITEMS.  Filter bytes are compared with the CPU checker's (ob.Bloom) and the atomic kernel's, jobs
with the checker's tags and counts; `kernel_times()` says which kernels ran."""
import numpy as np
import pytest

import oracle_binding as ob
import test_gpu_long_search as tls
import util

pytestmark = pytest.mark.gpu

NEW_NAMES = ("part_items_fill_kernel", "part_scatter1_pieces")


def _ctx(k, t=2, **opts):
    import commet_amd as commet
    ctx = commet.Context(k=k, t=t)
    for name, value in opts.items():
        ctx.set_option(name, value)
    return ctx


def _read_set(ctx, reads):
    import commet_amd as commet
    return commet.ReadSet.from_files(ctx, [util.to_batch(reads)])


def _filter_bytes(k, reads, calls, **opts):
    """the filter after index_reads(first, count, bits) for every call of `calls` -> (bytes, k-mers fed, kernel_times())"""
    with _ctx(k, kernel_timing=1, **opts) as ctx:
        rs = _read_set(ctx, reads)
        ctx.filter_reset()
        fed = sum(ctx.index_reads(rs, first, count, bits) for first, count, bits in calls)
        out = ctx.export_filter_reference()
        kt = ctx.kernel_times()
        rs.close()
    return out, fed, kt


def _checker_bytes(k, reads, sel=None):
    f = ob.Bloom(k)
    bases, offs = util.to_batch(reads)
    fed = f.index(bases, offs, None if sel is None else util.bits_from_bools(sel))
    out = f.bytes()
    f.close()
    return out, fed


def _queries(rng, index, n):
    """reads cut from the index set: plain, reverse complements, mutated, with a random head; and unrelated ones"""
    out = []
    for i in range(n):
        r = index[int(rng.integers(0, len(index)))]
        a = int(rng.integers(0, max(1, len(r) - 30)))
        piece = r[a:a + int(rng.integers(30, 2500))]
        if i % 3 == 0:
            piece = util.revcomp(piece)
        if i % 5 == 0:
            piece = util.mutate(rng, piece, 0.01)
        out.append(util.random_reads(rng, 1, 5, 400)[0] + piece if i % 2 else piece)
    return out + util.random_reads(rng, n // 4, 20, 700)


# ---- 1, 2. filter bytes at the old limit's edges ----------------------------------------------------------------------------------
def _edge_set(k):
    rng = np.random.default_rng(50 + k)
    lens = [19, 20, 40, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 4096 + k, 5000, 8191, 8192, 8200, 40000]
    reads = [util.random_reads(rng, 1, L, L, n_rate=0.002)[0] for L in lens[:-1] * 3 + lens[-1:]]
    # an N in each of the three words before a word boundary beyond word 3 (a window looks back three words at the most): one read
    # per word, and one read with all three
    for words in ((5,), (6,), (7,), (5, 6, 7), (130, 131, 132)):
        s = bytearray(util.random_reads(rng, 1, 5000, 5000, n_rate=0.0, other_rate=0.0, lower_rate=0.0)[0])
        for w in words:
            s[32 * w + (7, 0, 31)[w % 3]] = ord("N")
        reads.append(bytes(s))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


@pytest.fixture(scope="module")
def edge20():
    reads = _edge_set(20)
    return reads, _checker_bytes(20, reads)


def test_forced_bucketed_build_takes_long_reads(edge20):
    """index_mode = 2 on a set with reads of more than 4096 k-mers: "bucketed index construction needs ..." before this feature"""
    reads, (want, want_fed) = edge20
    got, fed, _ = _filter_bytes(20, reads, [(0, None, None)], index_mode=2)
    assert fed == want_fed
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [20, 25])
def test_filter_bytes_at_the_old_limit(k, edge20):
    if k == 20:
        reads, (want, want_fed) = edge20
    else:
        reads = _edge_set(k)
        want, want_fed = _checker_bytes(k, reads)
    assert 38 <= len(reads) <= 50
    got, fed, kt = _filter_bytes(k, reads, [(0, None, None)], index_mode=2)
    atomic, fed1, kt1 = _filter_bytes(k, reads, [(0, None, None)], index_mode=1)
    assert fed == want_fed == fed1
    assert np.array_equal(got, want)
    assert np.array_equal(atomic, want)
    assert kt["part_scatter1_kernel"][0] == 1 and kt["part_items_fill_kernel"][0] == 1 and "index_kernel" not in kt
    assert kt1["index_kernel"][0] == 1 and "part_scatter1_kernel" not in kt1


# ---- 3. few huge reads ------------------------------------------------------------------------------------------------------------
def test_few_huge_reads():
    rng = np.random.default_rng(3)
    huge = util.random_reads(rng, 3, 300000, 300000, n_rate=0.0005)
    short = util.random_reads(rng, 2, 60, 60, n_rate=0.0)
    for reads in ([short[0]] + huge + [short[1]], huge[:1]):
        want, want_fed = _checker_bytes(20, reads)
        got, fed, kt = _filter_bytes(20, reads, [(0, None, None)], index_mode=2)
        assert fed == want_fed
        assert np.array_equal(got, want)
        # the cut follows the items: 37 500 octets per read, at most 2048 to a piece (by the read count this chunk was ONE piece)
        assert kt["part_scatter1_pieces"][0] >= len(reads[len(reads) // 2]) // 8 // 2048 > 1
        assert kt["part_scatter1_kernel"][0] == 1 and "index_kernel" not in kt


# ---- 4. fixed-length long reads ---------------------------------------------------------------------------------------------------
def test_fixed_length_long_reads(tmp_path):
    k = 24
    rng = np.random.default_rng(4)
    reads = util.random_reads(rng, 40, 6000, 6000, n_rate=0.002)
    sel = rng.random(40) < 0.6
    sel[[3, 32]] = True
    bits = util.bits_from_bools(sel)
    opts = dict(index_mode=2)
    # unselected
    got, fed, kt = _filter_bytes(k, reads, [(0, None, None)], **opts)
    want, want_fed = _checker_bytes(k, reads)
    assert fed == want_fed and np.array_equal(got, want)
    assert kt["part_items_fill_kernel"][0] == 1 and "index_kernel" not in kt
    # a range with a selection bitmap and no list of the selected reads (the round planner's before)
    in_range = np.zeros(40, dtype=bool)
    in_range[3:33] = True
    got, fed, kt = _filter_bytes(k, reads, [(3, 30, bits)], **opts)
    want, want_fed = _checker_bytes(k, reads, sel & in_range)
    assert fed == want_fed and np.array_equal(got, want)
    assert kt["part_items_fill_kernel"][0] == 1 and "index_kernel" not in kt
    # two additive calls over disjoint ranges
    got, fed, kt = _filter_bytes(k, reads, [(0, 11, None), (17, 23, bits)], **opts)
    two = sel.copy()
    two[:11] = True
    two[11:17] = False
    want, want_fed = _checker_bytes(k, reads, two)
    assert fed == want_fed and np.array_equal(got, want)
    assert kt["part_scatter1_kernel"][0] == 2 and "index_kernel" not in kt
    # through a job with index_select (the job makes the list of the selected reads of a fixed-length set)
    search = _queries(rng, reads, 200)
    tls._check(tmp_path, k, 2, reads, [search], isel=sel, opts=(("index_mode", 2),), runs=((0, 0),))


# ---- 5. wide keys and large k, through the job ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [32, 33, 34])
def test_large_k_through_the_job(tmp_path, k):
    rng = np.random.default_rng(500 + k)
    index = [util.random_reads(rng, 1, L, L, n_rate=0.002)[0] for L in rng.integers(3000, 9001, size=30)]
    search = _queries(rng, index, 300)
    for mode in (2, 1):
        tags = tls._check(tmp_path / f"m{mode}", k, 2, index, [search], opts=(("index_mode", mode),), runs=((0, 0),))
    assert util.bools_from_bits(tags[0], len(search)).sum() > 100


# ---- 6. chunk edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_chunk_edges(tmp_path, lanes):
    """k = 20, max_kmer = 5000.  Ten short reads and a read of 6000 bases close the first chunk right behind the long read; the
    read the reference has fetched by then and drops is a long one; the next chunk is one read of 9000 bases, more than a whole
    chunk; then short and long reads under a selection bitmap.  Chunks are built in groups of two (both lanes when index_lanes = 2)"""
    k = 20
    rng = np.random.default_rng(6)

    def rd(L):
        return util.random_reads(rng, 1, L, L, n_rate=0.002)[0]

    index = [rd(100) for _ in range(10)] + [rd(6000), rd(7000), rd(9000), rd(100)]
    index += [rd(int(L)) for L in rng.choice([60, 100, 150, 300, 4100, 5000, 6500, 12000], size=60)]
    sel = rng.random(len(index)) < 0.8
    sel[:14] = True
    search = _queries(rng, index, 300)
    for mode, min_kmers in ((2, 1), (0, 1), (0, 7000)):      # forced; auto with two thresholds (whichever construction auto takes for a chunk, its slot must be zeroed or fully written)
        tls._check(tmp_path / f"m{mode}_{min_kmers}", k, 2, index, [search], isel=sel, max_kmer=5000, runs=((0, 0),),
                   opts=(("index_mode", mode), ("part_min_kmers", min_kmers), ("index_lanes", lanes), ("chunk_group", 2), ("kernel_timing", 0)))
    exp = tls._oracle(str(tmp_path / "first"), k, 2, index[:13], [search], max_kmer=5000)
    # (the plan the docstring describes is the checker's: two chunks from the first thirteen reads, the twelfth in neither)
    assert exp[3] == 2 and exp[4] == _checker_bytes(k, index[:13], [True] * 11 + [False, True])[1]


# ---- 7. fallbacks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform,option", [(False, "part_list"), (True, "part_no_uni")])
def test_fallbacks(tmp_path, uniform, option):
    """no item path (the list switched off): auto takes index_kernel on a zeroed filter, a forced bucketed build says so"""
    import commet_amd as commet
    k = 24
    rng = np.random.default_rng(7 + uniform)
    index = util.random_reads(rng, 30, 6000, 6000 if uniform else 9000, n_rate=0.002)
    search = _queries(rng, index, 200)
    exp_tags, exp_stats, _, chunks, kmers = tls._oracle(str(tmp_path / "orc"), k, 2, index, [search], max_kmer=50000)
    with _ctx(k, index_mode=0, part_min_kmers=1, max_kmer=50000, kernel_timing=1, **{option: 1}) as ctx:
        irs, srs = _read_set(ctx, index), _read_set(ctx, search)
        tags, stats, info = ctx.index_and_search(irs, [srs])
        assert info["n_chunks"] == chunks > 1 and info["kmers_indexed"] == kmers
        assert (stats[0]["indexed"], stats[0]["searched"], stats[0]["shared"]) == exp_stats[0]
        assert tags[0].tobytes() == exp_tags[0].tobytes()
        kt = ctx.kernel_times()
        assert kt["index_kernel"][0] == chunks and "part_scatter1_kernel" not in kt
        ctx.set_option("index_mode", 2)
        with pytest.raises(commet.CommetError, match="bucketed index construction needs"):
            ctx.index_and_search(irs, [srs])
        ctx.set_option(option, 0)                       # ... and with the list back, the same context builds the chunks in buckets
        tags, stats, info = ctx.index_and_search(irs, [srs])
        assert tags[0].tobytes() == exp_tags[0].tobytes() and info["kmers_indexed"] == kmers
        assert ctx.kernel_times()["part_scatter1_kernel"][0] == chunks


# ---- 8. several jobs in one call --------------------------------------------------------------------------------------------------
def test_index_many_and_search(tmp_path):
    k = 25
    rng = np.random.default_rng(8)
    pools = [[util.random_reads(rng, 1, int(L), int(L), n_rate=0.002)[0] for L in rng.integers(200, 9001, size=25)] for _ in range(2)]
    search = _queries(rng, pools[0] + pools[1], 400)
    exp = [tls._oracle(str(tmp_path / f"j{j}"), k, 2, pools[j], [search]) for j in range(2)]
    with _ctx(k, index_mode=2) as ctx:
        srs = _read_set(ctx, search)
        irs = [_read_set(ctx, p) for p in pools]
        many = ctx.index_many_and_search(irs, srs)
        for j in range(2):
            one = ctx.index_and_search(irs[j], [srs])
            assert many[0][j].tobytes() == one[0][0].tobytes() == exp[j][0][0].tobytes()
            assert all(many[1][j][f] == one[1][0][f] for f in ("indexed", "searched", "shared"))
            assert (one[1][0]["indexed"], one[1][0]["searched"], one[1][0]["shared"]) == exp[j][1][0]


# ---- 9. unchanged ground ----------------------------------------------------------------------------------------------------------
def test_short_reads_take_the_launches_they_took():
    rng = np.random.default_rng(9)
    reads = util.random_reads(rng, 5000, 100, 300, n_rate=0.002)
    got, fed, kt = _filter_bytes(20, reads, [(0, None, None)], index_mode=2)
    want, want_fed = _checker_bytes(20, reads)
    assert fed == want_fed and np.array_equal(got, want)
    assert set(kt) == {"filter_memset", "part_items_kernels", "part_hist_kernel", "part_scan_kernel", "part_blockoff_kernel",
                       "part_scatter1_kernel", "part_build_kernel"}
    assert all(kt[name][0] == 1 for name in kt) and not any(name in kt for name in NEW_NAMES)
