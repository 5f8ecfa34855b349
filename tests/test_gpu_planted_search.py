"""The short-read search kernels on planted windows and lane decoys (planted_sets.py): search_kernel, search_group_kernel<2 | 4>,
search_group8_kernel at its five mask widths, tq_probe_kernel / tq_replay_kernel, search_sliced_kernel, search_wide_kernel, their
list forms, and family A through search_long_kernel and the slot loop's hit-profile kernels.  The profile kernels of the wide rows, the
narrow tables, the tiled probe and the shared jobs pass run on the same fixtures in test_gpu_planted_profile.py, count for count.

Every read has a designed count (found at t exactly when count >= t) that test_planted_sets_cpu.py proves equal to the CPU checker;
here the tags are compared with the design, the log numbers, chunk and k-mer counts (and in counting builds the probe count) with the
checker's run of the same job, and kernel_times() says that the intended kernel ran and the excluded ones did not."""
import numpy as np
import pytest

import planted_sets as ps
import util
from checkers import checker_job

pytestmark = pytest.mark.gpu

SEARCH_KERNELS = ("search_kernel", "search_group_kernel", "search_group8_kernel", "tq_probe_kernel", "tq_replay_kernel", "search_sliced_kernel",
                  "search_wide_kernel", "search_long_kernel")
DEFAULTS = dict(chunk_group=8, tiled_search=1, slice_mode=1, slice_words=0, slice_wide=0, slice_wide_words=0, count_probes=0, sparse_search=0,
                long_search=1, ordered_scan=0, mask_split=0, tq_hit_cap=1024, index_mode=0)
PLAIN = dict(chunk_group=1)
SLOT_RUNS = {
    "plain": [(dict(PLAIN, count_probes=c), {"search_kernel"}, None) for c in (0, 1)],
    # (sets of more than 256 bases are beyond four filters' LDS masks: such a set goes filter by filter)
    "group": [(dict(chunk_group=g, count_probes=c), {"search_group_kernel"}, {"search_kernel"} if g == 4 else set()) for g in (2, 4) for c in (0, 1)],
    "group8": [(dict(chunk_group=8), {"search_group8_kernel"}, None), (dict(chunk_group=8, ordered_scan=2), {"search_group8_kernel"}, None),
               (dict(chunk_group=8, ordered_scan=2, mask_split=1), {"search_group8_kernel"}, None)],
    "tiled": [(dict(tiled_search=2, chunk_group=g, tq_hit_cap=cap), {"tq_probe_kernel", "tq_replay_kernel"}, None)
              for g, cap in ((2, 1024), (1, 1024), (2, 0), (1, 2), (2, 2), (1, 0))],
    "long": [(dict(long_search=2, chunk_group=g), {"search_long_kernel"}, None) for g in (1, 2, 4, 8)],
}
SLICED_RUNS = [(dict(slice_mode=2, slice_wide=1, slice_words=w), {"search_sliced_kernel"}, None) for w in (1, 2, 4, 8)]
WIDE_RUNS = [(dict(slice_mode=2, slice_wide=2, slice_wide_words=w), {"search_wide_kernel"}, None) for w in (0, 8)]

_TRUTH = {}


def _truth(tmp_path, key, k, t, index, set_reads, max_kmer):
    """the checker's run of the job, once per case: (tags, stats, chunks, k-mers)"""
    if key not in _TRUTH:
        _TRUTH[key] = checker_job(tmp_path / "orc", k, t, index, set_reads, max_kmer=max_kmer)
    return _TRUTH[key]


def _jobs(k, t, index, set_reads, max_kmer, runs, selects=None):
    """the job under every option set of `runs` in one context -> [(tags as bools, stats, info, kernel names, kernel times)]"""
    import commet_amd as commet
    out = []
    with commet.Context(k=k, t=t) as ctx:
        ctx.set_option("max_kmer", max_kmer)
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(index)])
        qrs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in set_reads]
        sel = None if selects is None else [util.bits_from_bools(s) for s in selects]
        for opts, _, _ in runs:
            for name, value in dict(DEFAULTS, **opts).items():
                ctx.set_option(name, value)
            ctx.set_option("kernel_timing", 1)
            tags, stats, info = ctx.index_and_search(irs, qrs, search_selects=sel)
            times = ctx.kernel_times()
            ctx.set_option("kernel_timing", 0)
            out.append(([util.bools_from_bits(tg, len(s)) for tg, s in zip(tags, set_reads)], stats, info, times))
        for r in qrs + [irs]:
            r.close()
    return out


def _check(what, runs, results, designs, truth, t):
    """designs: per search set the designed counts; truth: the checker's (tags, stats, chunks, kmers)"""
    exp_tags, exp_stats, chunks, kmers = truth
    for (opts, must, may), (tags, stats, info, times) in zip(runs, results):
        ran = {n for n in SEARCH_KERNELS if n in times}
        print(what, opts, sorted(ran), {n: times[n][0] for n in ran})
        assert must <= ran and (ran - must <= may if may is not None else ran == must), (what, opts, sorted(ran))
        assert info["n_chunks"] == chunks and info["kmers_indexed"] == kmers, (what, opts)
        for s, counts in enumerate(designs):
            wrong = np.nonzero(tags[s] != (counts >= t))[0]
            assert wrong.size == 0, (what, opts, s, wrong[:10].tolist(), counts[wrong[:10]].tolist())
            assert np.array_equal(tags[s], exp_tags[s]), (what, opts, s)
            assert [stats[s][f] for f in ("indexed", "searched", "shared")] == [exp_stats[s][f] for f in ("indexed", "searched", "shared")], (what, opts, s)
        if opts.get("count_probes"):
            assert info["probes"] == sum(r["probes"] for r in exp_stats), (what, opts)
        else:
            assert info["probes"] == 0


def _sweep(tmp_path, row, runs, k, t, n_chunks, fhws, per_chunk):
    c = ps.sweep_case(k, t, n_chunks, fhws, per_chunk)
    names = list(c["sets"])
    reads = [c["sets"][n][0] for n in names]
    designs = [c["sets"][n][1] for n in names]
    truth = _truth(tmp_path, ("sweep", k, t, n_chunks, per_chunk), k, t, c["index"], reads, c["max_kmer"])
    results = _jobs(k, t, c["index"], reads, c["max_kmer"], runs)
    _check((row, k, t), runs, results, designs, truth, t)
    return c, names, results


def _mask_classes(k, t, fhws):
    """the mask widths the fixed-length sets instantiate: the dispatch's rule on (longest read) - t k + 1 first-hit windows"""
    return {ps.mask_words(max(len(r) for r in ps.sweep_case(k, t, 6, fhws, 0)["sets"][f"f{fhw}"][0]) - t * k + 1) for fhw in fhws}


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLOT_SWEEPS + ps.SMALL_SWEEPS)
def test_plain_kernel_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    _sweep(tmp_path, "plain", SLOT_RUNS["plain"], k, t, n_chunks, fhws, per_chunk)


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLOT_SWEEPS)
def test_group_kernels_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    c, names, _ = _sweep(tmp_path, "group", SLOT_RUNS["group"], k, t, n_chunks, fhws, per_chunk)
    lens = [max(len(r) for r in c["sets"][n][0]) for n in names]
    assert min(lens) <= 256 < max(lens)                         # reads staged in LDS, and a set past the staging


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLOT_SWEEPS)
def test_group8_kernel_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    assert _mask_classes(k, t, fhws) == {2, 3, 4, 6, 8}
    runs = SLOT_RUNS["group8"]
    c, names, results = _sweep(tmp_path, "group8", runs, k, t, n_chunks, fhws, per_chunk)
    launches = [r[3]["search_group8_kernel"][0] for r in results]
    ragged = sum(1 for n in names if len({len(r) for r in c["sets"][n][0]}) > 1)
    assert launches[0] == launches[2] == len(names)             # six chunks: one pass per set
    assert launches[1] >= launches[0] + 2 * ragged - 2, launches    # the ragged sets' first pass in segments by mask width


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLOT_SWEEPS)
def test_tiled_search_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    assert _mask_classes(k, t, fhws) == {2, 3, 4, 6, 8}
    _sweep(tmp_path, "tiled", SLOT_RUNS["tiled"], k, t, n_chunks, fhws, per_chunk)


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", ps.SLICED_SWEEPS)
def test_sliced_kernel_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    _sweep(tmp_path, "sliced", SLICED_RUNS, k, t, n_chunks, fhws, per_chunk)


@pytest.mark.parametrize("k,t,n_chunks,fhws,per_chunk", [s for s in ps.SLICED_SWEEPS if s[0] <= 21])
def test_wide_kernel_positions(tmp_path, k, t, n_chunks, fhws, per_chunk):
    _sweep(tmp_path, "wide", WIDE_RUNS, k, t, n_chunks, fhws, per_chunk)


# ---- the list form: a selection of every third read -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,t", [(25, 2), (33, 1), (34, 3)])
def test_list_form_of_the_slot_kernels(tmp_path, k, t):
    """family B (one fhw, and the ragged set of all of them) and family A.  The tags against the design under the selection; the
    chunk and k-mer counts, `indexed` and (masked by the selection) `shared` against the checker's run of the whole sets"""
    c = ps.sweep_case(k, t, 6, ps.FHW, 0)
    lad = ps.ladder_case(k, 6)
    runs = [(dict(PLAIN, sparse_search=2), {"search_kernel"}, None), (dict(chunk_group=4, sparse_search=2), {"search_group_kernel"}, {"search_kernel"}),
            (dict(chunk_group=8, sparse_search=2), {"search_group8_kernel"}, None)]
    for what, case, names in (("B", c, ["f97", "all"]), ("A", lad, ["ladder"])):
        reads = [case["sets"][n][0] for n in names]
        designs = [case["sets"][n][1] for n in names]
        sels = [np.arange(len(r)) % 3 == 0 for r in reads]
        assert min(s.sum() for s in sels) > 20
        exp_tags, exp_stats, chunks, kmers = _truth(tmp_path, ("list", what, k, t), k, t, case["index"], reads, case["max_kmer"])
        for (opts, must, may), (tags, stats, info, times) in zip(runs, _jobs(k, t, case["index"], reads, case["max_kmer"], runs, selects=sels)):
            ran = {n for n in SEARCH_KERNELS if n in times}
            assert "active_list_kernels" in times and must <= ran and ran - must <= (may or set()), (what, opts, sorted(ran))
            assert info["n_chunks"] == chunks and info["kmers_indexed"] == kmers, (what, opts)
            for s, counts in enumerate(designs):
                want = (counts >= t) & sels[s]
                assert np.array_equal(tags[s], want), (what, opts, s, np.nonzero(tags[s] != want)[0][:10].tolist())
                assert stats[s]["shared"] == int((exp_tags[s] & sels[s]).sum()) == int(want.sum()) and stats[s]["indexed"] == exp_stats[s]["indexed"]


# ---- A: the lane ladder ------------------------------------------------------------------------------------------------------------------
def _ladder(tmp_path, row, runs, k, t, n_chunks):
    c = ps.ladder_case(k, n_chunks)
    names = list(c["sets"])
    reads = [c["sets"][n][0] for n in names]
    truth = _truth(tmp_path, ("ladder", k, t, n_chunks), k, t, c["index"], reads, c["max_kmer"])
    results = _jobs(k, t, c["index"], reads, c["max_kmer"], runs)
    _check((row, k, t), runs, results, [c["sets"][n][1] for n in names], truth, t)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("k,n_chunks", ps.SLOT_LADDERS)
def test_lane_ladder_in_the_slot_kernels(tmp_path, k, n_chunks, t):
    """plain, groups of 2 and 4 (both with the reference's probe count: 2, 3 and 4 probes per window of a k-mer with LO, LO + HI,
    LO + HI + BOTH indexed), groups of 8, the tiled search where k allows it, and a wave per read"""
    runs = SLOT_RUNS["plain"] + SLOT_RUNS["group"] + SLOT_RUNS["group8"][:1] + (SLOT_RUNS["tiled"] if k >= 25 else []) + SLOT_RUNS["long"]
    _ladder(tmp_path, "ladder", runs, k, t, n_chunks)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("k,n_chunks", ps.SLICED_LADDERS)
def test_lane_ladder_in_the_sliced_kernels(tmp_path, k, n_chunks, t):
    """300 chunk filters: the decoys of a k-mer in neighbouring columns of every 32-chunk word, and on both sides of the 256-chunk
    group boundary of the tables and of a wide row"""
    _ladder(tmp_path, "ladder", SLICED_RUNS + (WIDE_RUNS if k <= 21 else []), k, t, n_chunks)


def test_lane_ladder_at_the_largest_k():
    """k = 36: no checker filter fits a test host; the design (equal to the key-level checker, test_planted_sets_cpu.py) alone"""
    k = ps.LARGEST_K
    c = ps.ladder_case(k, 1)
    names = list(c["sets"])
    reads = [c["sets"][n][0] for n in names]
    for t in (1, 2):
        runs = [(dict(PLAIN, count_probes=p), {"search_kernel"}, None) for p in (0, 1)]
        for (opts, must, _), (tags, stats, info, times) in zip(runs, _jobs(k, t, c["index"], reads, c["max_kmer"], runs)):
            assert {n for n in SEARCH_KERNELS if n in times} == must and info["n_chunks"] == 1
            for s, n in enumerate(names):
                want = c["sets"][n][1] >= t
                assert np.array_equal(tags[s], want) and stats[s]["shared"] == int(want.sum()), (t, opts, n)


# (how the jobs of one call share passes, the job's options, the one search kernel and its launches for two jobs)
JOB_RUNS = {
    "group8": (3, dict(chunk_group=8, index_mode=2), "search_group8_kernel", 1),              # six filters of two jobs in one pass: job_mask
    "alone": (3, dict(chunk_group=8, index_mode=2, multi_job=1), "search_group_kernel", 2),   # job by job: three filters each, in four slots
    "tiled": (3, dict(chunk_group=2, tiled_search=2), "tq_replay_kernel", 4),
    "pairs": (1, dict(chunk_group=8, index_mode=2, tiled_search=2), "tq_replay_kernel", 1),   # one filter per job, two jobs per tiled scan: job_tag_words
    "long": (3, dict(chunk_group=8, long_search=2, multi_job=2), "search_long_kernel", 1),
}


@pytest.mark.parametrize("k,n_chunks,how", [(k, n, how) for k, n in ps.JOB_LADDERS for how in JOB_RUNS if JOB_RUNS[how][0] == n])
def test_lane_ladder_split_between_two_index_sets(tmp_path, k, n_chunks, how):
    """the four decoys of a k-mer in two index SETS of one commet_index_many_and_search call, whose jobs share passes: found in neither"""
    import commet_amd as commet
    _, opts, kernel, launches = JOB_RUNS[how]
    c = ps.ladder_jobs(k, n_chunks)
    for t in (1, 2):
        truth = [_truth(tmp_path / f"j{j}", ("jobs", k, n_chunks, t, j), k, t, c["index_sets"][j], [c["search"]], c["max_kmer"]) for j in range(2)]
        with commet.Context(k=k, t=t) as ctx:
            ctx.set_option("max_kmer", c["max_kmer"])
            for name, value in dict(DEFAULTS, **dict(dict(multi_job=0), **opts)).items():
                ctx.set_option(name, value)
            sets = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in c["index_sets"]]
            qrs = commet.ReadSet.from_files(ctx, [util.to_batch(c["search"])])
            ctx.set_option("kernel_timing", 1)
            tags, stats, info = ctx.index_many_and_search(sets, qrs)
            times = ctx.kernel_times()
        ran = {n: times[n][0] for n in SEARCH_KERNELS if n in times}
        print(k, t, how, ran)
        assert ran.pop("tq_probe_kernel", launches) == launches and ran == {kernel: launches}, (k, t, how, ran)
        for j in range(2):
            got = util.bools_from_bits(tags[j], len(c["search"]))
            want = c["counts"][j] >= t
            assert np.array_equal(got, want), (k, t, how, j, np.nonzero(got != want)[0][:10].tolist())
            assert np.array_equal(got, truth[j][0][0])
            assert [stats[j][f] for f in ("indexed", "searched", "shared")] == [truth[j][1][0][f] for f in ("indexed", "searched", "shared")], (k, t, how, j)


# ---- A through the hit profile ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_search", [1, 2])
@pytest.mark.parametrize("k,n_chunks", [(25, 6), (33, 6), (20, 6)])
def test_lane_ladder_hit_bytes(k, n_chunks, long_search):
    """the hit byte counts decoy-made full hits per filter and strand; a triple, or four decoys in four filters, counts 0"""
    import commet_amd as commet
    c = ps.ladder_case(k, n_chunks)
    names = list(c["sets"])
    reads = [c["sets"][n][0] for n in names]
    group = {1: "hits_group_kernel", 2: "hits_group_wave_kernel"}[long_search]
    one = {1: "hits_kernel", 2: "hits_wave_kernel"}[long_search]
    with commet.Context(k=k, t=2) as ctx:
        irs = commet.ReadSet.from_files(ctx, [util.to_batch(c["index"])])
        qrs = [commet.ReadSet.from_files(ctx, [util.to_batch(s)]) for s in reads]
        ctx.set_option("max_kmer", c["max_kmer"])
        ctx.set_option("long_search", long_search)
        for chunk_group in (1, 2, 4, 8):
            ctx.set_option("chunk_group", chunk_group)
            ctx.set_option("kernel_timing", 1)
            hits, info = ctx.index_and_profile(irs, qrs, max_hits=4)
            times = ctx.kernel_times()
            assert info["n_chunks"] == n_chunks and ((group if chunk_group > 1 else one) in times) and ((one if chunk_group > 1 else group) not in times)
            for s, n in enumerate(names):
                want = np.minimum(c["sets"][n][1], 4)
                assert np.array_equal(hits[s], want), (k, long_search, chunk_group, n, np.nonzero(hits[s] != want)[0][:10].tolist())
