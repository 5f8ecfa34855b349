"""Every search and hit-profile kernel at EVERY k it takes, k = 1 .. 38, against the key-level job reference (every_k_sets.py; proved
equal to the CPU checker at k <= 26 and mixed at every k by test_every_k_sets_cpu.py).

The filter-bits tests pin the index side at every k; the read side — windows cut from the read planes (ItemWords<W>::window: from
k = 34 on the 64-bit window takes bits of THREE plane words), psi_a at every h, the probe — ran at a hand-picked set of k only.  Here
one context per k runs the k's job under every option set that reaches another kernel, and after every run kernel_times() must name
the intended kernel and none of its rivals:

  search    search_kernel; search_group_kernel (groups of 2 and 4); search_group8_kernel; search_long_kernel on 1, 2, 4 and 8
            filters; the list form (a selection of every third read) of the widest group the k allows
  profile   hits_kernel, hits_wave_kernel; hits_group_kernel and hits_group_wave_kernel on 2, 4 and 8 filters; two jobs in one pass,
            hits_jobs_kernel and hits_jobs_wave_kernel (the index set split at a chunk boundary, each half against key_level_job of
            its own) — the bytes at max_hits = 255 and 3
  12 <= k <= 24   search_sliced_kernel / hits_sliced_kernel at 1 and 8 words per entry, search_wide_kernel / hits_wide_kernel, on the
            same sets in chunks of one index read (45 chunk filters)
  25 <= k <= 34   tq_probe_kernel + tq_replay_kernel on one and two filters, tq_probe_kernel + tq_hits_replay_kernel (over the reads of
            at most 254 + k bases, a set of their own where that is not every read)

Searches: tags bit for bit at the case's t_k, [indexed, searched, shared], chunk and k-mer counts.  Profiles: the bytes exactly.
(t_k is 2 from k = 34 on, and every read R of the three-word family counts exactly 2, its twin 1: the searches tell them apart, not
the hit bytes alone.  With word w-2 cut to its top bit in ItemWords<uint64_t>::load / load_with, search_group_kernel loses exactly
those R from k = 35 on; the planted files do not notice.)

MEMORY RULE above k = 34.  No case asks the device for more than the suite's largest case did before: one slot at k = 38, 128 GiB.  A
group of gs slots costs gs x 2^(k-1) bytes plus gs x 2^(k-3) for the interleaved A planes, which allows chunk_group <= 4 at k = 35,
<= 2 at k = 36 and 1 at k = 37 and 38; chunk_group is set to that cap before the first job (ensure_slots asks for a whole group's
worth) and the case has that many chunks.  search_group8_kernel and the eight-filter instantiations of the wave and hits kernels are
therefore NOT run above k = 34: their 64-bit builds get k = 33 and 34, the latter with the three-word family."""
import time

import numpy as np
import pytest

import every_k_sets as eks
import util

pytestmark = pytest.mark.gpu

SEARCH_KERNELS = ("search_kernel", "search_group_kernel", "search_group8_kernel", "tq_probe_kernel", "tq_replay_kernel", "search_sliced_kernel",
                  "search_wide_kernel", "search_long_kernel")
HITS_KERNELS = ("hits_kernel", "hits_group_kernel", "hits_wave_kernel", "hits_group_wave_kernel", "hits_wide_kernel", "hits_sliced_kernel",
                "tq_probe_kernel", "tq_hits_replay_kernel", "hits_jobs_kernel", "hits_jobs_wave_kernel")
DEFAULTS = dict(tiled_search=1, slice_mode=1, slice_words=0, slice_wide=1, slice_wide_words=0, count_probes=0, sparse_search=0, long_search=1,
                ordered_scan=0, mask_split=0, tq_hit_cap=1024, index_mode=0, profile_wide=1, profile_slice=1, profile_tiled=1, multi_job=0)
CAPS = (255, 3)
LARGEST_CASE = 1 << 37                                          # one slot at k = 38


def group_cap(k):
    """the memory rule: the widest group (8, 4 or 2 slots and their interleaved A planes) within the suite's largest case, else 1"""
    for gs in (8, 4, 2):
        if gs * ((1 << (k - 1)) + (1 << max(k - 3, 0))) <= LARGEST_CASE:
            return gs
    return 1


@pytest.fixture(scope="module")
def commet():
    import commet_amd
    return commet_amd


class _Runs:
    """the jobs of one context, each under DEFAULTS + its options, timed; what ran is held to `must` exactly"""

    def __init__(self, ctx, k, cap):
        self.ctx, self.k, self.cap, self.n = ctx, k, cap, 0

    def _timed(self, opts, names, call):
        for name, value in dict(dict(DEFAULTS, chunk_group=self.cap), **opts).items():
            self.ctx.set_option(name, value)
        self.ctx.set_option("kernel_timing", 1)                 # (the totals start again)
        try:
            out = call()
            times = self.ctx.kernel_times()
        finally:
            self.ctx.set_option("kernel_timing", 0)
        self.n += 1
        return out, {n: times[n][0] for n in names if n in times}, times

    def search(self, what, opts, must, irs, qrs, job, t, select=None):
        sel = None if select is None else [util.bits_from_bools(select)]
        (tags, stats, info), ran, times = self._timed(opts, SEARCH_KERNELS, lambda: self.ctx.index_and_search(irs, [qrs], search_selects=sel))
        assert set(ran) == must and (select is None or "active_list_kernels" in times), (self.k, what, opts, ran)
        assert info["n_chunks"] == job.n_chunks and info["kmers_indexed"] == job.kmers_indexed, (self.k, what, opts, info["n_chunks"], info["kmers_indexed"])
        selects = None if select is None else [select]
        want = job.tags(t, selects)[0]
        got = util.bools_from_bits(tags[0], len(want))
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (self.k, what, opts, "reads", wrong[:10].tolist(), "found", got[wrong[:10]].tolist(), "their counts", job.hits[0][wrong[:10]].tolist())
        assert [stats[0][f] for f in ("indexed", "searched", "shared")] == job.stats(t, selects)[0], (self.k, what, opts)

    def profile(self, what, opts, must, irs, qrs, want_bytes, n_chunks):
        for cap in CAPS:
            (hits, info), ran, _ = self._timed(opts, HITS_KERNELS, lambda: self.ctx.index_and_profile(irs, [qrs], max_hits=cap))
            assert set(ran) == must, (self.k, what, opts, cap, ran)
            assert info["n_chunks"] == n_chunks, (self.k, what, opts, info["n_chunks"])
            _same_bytes((self.k, what, opts, cap), hits[0], np.minimum(want_bytes, cap))


def _same_bytes(what, got, want):
    wrong = np.flatnonzero(got != want)
    assert got.dtype == np.uint8 and len(got) == len(want) and wrong.size == 0, (what, "reads", wrong[:10].tolist(), got[wrong[:10]].tolist(), want[wrong[:10]].tolist())


@pytest.mark.parametrize("k", eks.KS)
def test_every_kernel_at_this_k(commet, k):
    t0 = time.time()
    c, job, cap = eks.case(k), eks.reference(k), group_cap(k)
    t, n_chunks = c["t_k"], c["n_chunks"]
    assert n_chunks == job.n_chunks == (6 if cap == 8 else cap)
    groups = [g for g in (8, 4, 2) if g <= cap] if k >= 2 else []          # (k = 1: the one-filter kernels alone)
    group_kernel = {8: "search_group8_kernel", 4: "search_group_kernel", 2: "search_group_kernel"}
    with commet.Context(k=k, t=t) as ctx:
        ctx.set_option("chunk_group", cap)                      # before the first job: the slots are asked for once, a whole group's worth
        ctx.set_option("max_kmer", c["max_kmer"])
        load = lambda reads: commet.ReadSet.from_files(ctx, [util.to_batch(reads)])
        irs, qrs = load(c["index"]), load(c["search"])
        sets = [irs, qrs]
        run = _Runs(ctx, k, cap)
        # ---- the slot loop: searches (the widest group first) ------------------------------------------------------------------
        for g in groups:
            run.search("group", dict(chunk_group=g), {group_kernel[g]}, irs, qrs, job, t)
        run.search("plain", dict(chunk_group=1), {"search_kernel"}, irs, qrs, job, t)
        for g in ([1] + groups[::-1] if k >= 2 else []):
            run.search("long", dict(long_search=2, chunk_group=g), {"search_long_kernel"}, irs, qrs, job, t)
        third = np.arange(len(c["search"])) % 3 == 0
        run.search("list", dict(sparse_search=2), {group_kernel[cap] if groups else "search_kernel"}, irs, qrs, job, t, select=third)
        # ---- the slot loop: profiles ----------------------------------------------------------------------------------------------------
        want = job.hits[0]
        run.profile("one", dict(chunk_group=1), {"hits_kernel"}, irs, qrs, want, n_chunks)
        if k >= 2:
            run.profile("one wave", dict(chunk_group=1, long_search=2), {"hits_wave_kernel"}, irs, qrs, want, n_chunks)
        for g in groups:
            run.profile("group", dict(chunk_group=g), {"hits_group_kernel"}, irs, qrs, want, n_chunks)
            run.profile("group wave", dict(chunk_group=g, long_search=2), {"hits_group_wave_kernel"}, irs, qrs, want, n_chunks)
        # ---- two jobs in one hits pass ----------------------------------------------------------------------------------------------------
        if c["jobs"] and cap >= 2:
            halves = [eks.reference(k, ("half", j)) for j in range(2)]
            assert sum(h.n_chunks for h in halves) == n_chunks <= cap
            parts = [load(r) for r in c["jobs"]]
            sets += parts
            for opts, kernel in ((dict(), "hits_jobs_kernel"), (dict(multi_job=2, long_search=2), "hits_jobs_wave_kernel")):
                for caps in (CAPS, CAPS[::-1]):
                    (hits, info), ran, _ = run._timed(opts, HITS_KERNELS, lambda: ctx.index_many_and_profile(parts, qrs, max_hits=list(caps)))
                    assert ran == {kernel: 1} and info["n_chunks"] == n_chunks, (k, opts, caps, ran, info["n_chunks"])
                    for j in range(2):
                        _same_bytes((k, "jobs", opts, caps, j), hits[j], np.minimum(halves[j].hits[0], caps[j]))
        else:
            assert k == 1 or cap == 1
        # ---- the bit-sliced tables and the wide rows: many small chunks --------------------------------------------------------------
        if c["max_kmer_small"]:
            small = eks.reference(k, "small")
            assert 12 <= k <= 24 and small.n_chunks >= 33
            ctx.set_option("max_kmer", c["max_kmer_small"])
            for w in (1, 8):
                run.search("sliced", dict(slice_mode=2, slice_words=w), {"search_sliced_kernel"}, irs, qrs, small, t)
                run.profile("sliced", dict(profile_slice=2, slice_words=w), {"hits_sliced_kernel"}, irs, qrs, small.hits[0], small.n_chunks)
            run.search("wide", dict(slice_mode=2, slice_wide=2), {"search_wide_kernel"}, irs, qrs, small, t)
            run.profile("wide", dict(profile_wide=2), {"hits_wide_kernel"}, irs, qrs, small.hits[0], small.n_chunks)
            ctx.set_option("max_kmer", c["max_kmer"])
        else:
            assert not 12 <= k <= 24
        # ---- the tiled probe --------------------------------------------------------------------------------------------------------------
        if 25 <= k <= 34:
            short = np.array([len(r) <= 254 + k for r in c["search"]])          # at most 255 complete windows per read
            assert short.sum() >= 200
            srs = qrs if short.all() else load([r for r, s in zip(c["search"], short) if s])
            sets += [] if srs is qrs else [srs]
            for g in (2, 1):
                run.search("tiled", dict(tiled_search=2, chunk_group=g), {"tq_probe_kernel", "tq_replay_kernel"}, irs, qrs, job, t)
                run.profile("tiled", dict(profile_tiled=2, chunk_group=g), {"tq_probe_kernel", "tq_hits_replay_kernel"}, irs, srs, want[short], n_chunks)
        for rs in sets:
            rs.close()
    print(f"k={k}: t_k={t}, {n_chunks} chunks, group cap {cap}, {run.n} jobs, {time.time() - t0:.1f} s")
