"""Every no-room fallback of the library, run: device allocations refused on request (commet_device_alloc_refuse, the hook at the top
of dm_malloc: DevMemCache::malloc, host/devmem.hpp) on small shapes, every result against the CPU checker on the same reads.

"Out of device memory costs speed, never correctness" is promised at more than a dozen sites (the slot ladder 8 -> 4 -> 1 of
run_slot_groups, ensure_slots' "only the g needed now", wide rows -> narrow tables -> slot loop, rerun_alone_no_room of
the many-job calls, the list of a job's selected reads, query lists, length order, sparse lists, item lists, dev_alloc's retry, restore, create).  A refusal at
the top of dm_malloc is, for every caller, the driver saying no.

Two modes.  By size: every request of at least `at_least` bytes is refused.  By count: the nth request from arming on is refused once
(the retry of dev_alloc is request n + 1 and goes through).

Sizes of the slot cases (k = 26; filter_bytes = 4 planes x 2^26 bits = 32 MiB, plane_bytes = 8 MiB):

    one slot 32 MiB | groups of 2 / 4 / 8 slots 64 / 128 / 256 MiB | interleaved A planes at stride 2 / 4 / 8: 16 / 32 / 64 MiB

The read sets hold a few hundred short reads: every other buffer of a job stays far below 16 MiB (the scatter workspaces ~4 MiB each,
blockoff 2 MiB), so "refuse >= 2 slots" selects exactly the slot-group requests.  Thresholds are derived from filter_bytes(k).

Every armed run must give the checker's tags, indexed / searched / shared, n_chunks and kmers_indexed; where slots are concerned
also the checker's bytes in every slot (export_filter_reference, after disarming: the export allocates); kernel_times() and info say
which path ran — a fallback test that took the fast path fails — and refused > 0.  Disarming is in a `finally` (the context manager).

The sweep (test_sweep_*): every request of one API call refused in turn, a fresh context and fresh sets for every n; the call
returns the unarmed outputs, or raises an allocation error (never "internal error") and then, disarmed, succeeds on the same objects;
refused == 1 for every n; the sites that promise a fallback must return.  A line per n is printed: n, last_refused_bytes, outcome.

Two cases differ from the issue's table, by reading the code.  (g) Index sets of 3 + 5 chunks fit ONE pass of eight slots, so the
refusal sends the call to rerun_alone_no_room before any pass has run; the described course — pass one on three granted slots, pass two without
room, after pass one has written its stats — needs 3 + 6, which runs as well.  (p) An oversize read under index_mode = 2 is a clean
error ("needs memory for the item list"); the atomic fallback behind it is reached only with LONG_INDEX_AUTO, which is false."""
import re

import numpy as np
import pytest

import hit_profile_group_sets as hg
import job_filters as jf
import planted_sets as ps
import test_gpu_job_filter_bytes as fb
import test_gpu_long_search as tls
import test_gpu_planted_search as tps
import util

pytestmark = pytest.mark.gpu

T = 2
SLOT_K = 26
STAT = ("indexed", "searched", "shared")
ALLOC_MESSAGE = re.compile(r"memory|allocat", re.I)


def filter_bytes(k):
    """commet_create: filter_bytes = 4 * plane_words * 4, plane_words = 2^k / 32"""
    return 4 * max(1, (1 << k) // 32) * 4


def plane_bytes(k):
    return filter_bytes(k) // 4


def _commet():
    import commet_amd
    return commet_amd


def refusing(at_least=0, nth=0):
    return _commet().refusing_device_allocs(at_least=at_least, nth=nth)


# ---- sets and their checker runs, made once ----------------------------------------------------------------------------------------------
_JOBS, _TRUTH = {}, {}


def slot_job(k, n_chunks, seed=0, per_chunk=5, L=120, n_search=150, ragged_search=False):
    """an index set of n_chunks chunks (hit_profile_group_sets.chunked: per_chunk clean reads each; max_kmer depends on k, per_chunk and L
    alone, so sets of different chunk counts share it) and a search set of reads cut from them, two in three, and random ones"""
    key = (k, n_chunks, seed, per_chunk, L, n_search, ragged_search)
    if key not in _JOBS:
        rng = np.random.default_rng(100000 * k + 100 * n_chunks + seed)
        chunks = [[hg.rand(rng, L) for _ in range(per_chunk)] for _ in range(n_chunks)]
        index, max_kmer = hg.chunked(rng, k, chunks)
        search = []
        for i in range(n_search):
            n = int(rng.integers(k + 4, L + 1)) if ragged_search else 100
            if i % 3 == 2:
                search.append(hg.rand(rng, n))
            else:
                r = chunks[i % n_chunks][int(rng.integers(per_chunk))]
                a = int(rng.integers(0, L - n + 1))
                search.append(r[a:a + n])
        _JOBS[key] = dict(k=k, index=index, max_kmer=max_kmer, search=search, n_chunks=n_chunks)
    return _JOBS[key]


def truth_of(tmp_path, key, k, t, index, search_sets, max_kmer, index_select=None):
    """jf.checker_run, once per key"""
    key = (key, k, t)
    if key not in _TRUTH:
        _TRUTH[key] = jf.checker_run(tmp_path / ("orc_" + re.sub(r"\W+", "_", str(key))), k, t, index, search_sets, max_kmer=max_kmer, index_select=index_select)
    return _TRUTH[key]


def context(k, max_kmer, **opts):
    ctx = _commet().Context(k=k, t=T)
    for name, value in dict(fb.BASE, max_kmer=max_kmer, **opts).items():
        ctx.set_option(name, value)
    return ctx


def load(ctx, reads):
    return _commet().ReadSet.from_files(ctx, [util.to_batch(reads)])


def timed(ctx, call):
    """-> (the call's result, {kernel: launches})"""
    ctx.set_option("kernel_timing", 1)
    try:
        out = call()
        times = ctx.kernel_times()
    finally:
        ctx.set_option("kernel_timing", 0)
    return out, {n: times[n][0] for n in times}


def only(ran, names):
    return {n: ran[n] for n in names if n in ran}


HITS_KERNELS = ("hits_kernel", "hits_group_kernel", "hits_wave_kernel", "hits_group_wave_kernel", "hits_wide_kernel")


def slots_hold(ctx, what, k, index, truth, in_slot, n_slots):
    """every slot against the checker's bytes of the chunk built into it last; the context has n_slots slots and no more"""
    filters = {c: jf.chunk_filter(k, index, truth["trace"][c]) for c in set(in_slot) if c is not None}
    fb.check_slots(ctx, what, [None if c is None else filters[c] for c in in_slot])
    if n_slots < 8:
        with pytest.raises(_commet().CommetError):
            ctx.export_filter_reference(n_slots)


# ---- (a) - (e): the slot ladder, through jobs and through profiles ----------------------------------------------------------------------------
# (chunks, chunk_group, slots refused from, search kernels unarmed, armed, refusals, chunk per slot afterwards, slots afterwards)
LADDER = {
    "a_eight_to_fours": (8, 8, 8, {"search_group8_kernel": 1}, {"search_group_kernel": 2}, 1, [4, 5, 6, 7], 4),
    "b_eight_to_ones": (8, 8, 4, {"search_group8_kernel": 1}, {"search_kernel": 8}, 2, [7], 1),
    "c_three_on_three_slots": (3, 4, 4, {"search_group_kernel": 1}, {"search_group_kernel": 1}, 1, [0, 1, 2], 3),
    "d_two_to_ones": (2, 8, 2, {"search_group_kernel": 1}, {"search_kernel": 2}, 1, [1], 1),
}
HITS_OF = {"search_group8_kernel": "hits_group_kernel", "search_group_kernel": "hits_group_kernel", "search_kernel": "hits_kernel"}


@pytest.mark.parametrize("case", sorted(LADDER))
def test_slot_ladder_of_a_job(tmp_path, case):
    n_chunks, group, refuse_slots, unarmed, armed, refusals, in_slot, n_slots = LADDER[case]
    k = SLOT_K
    job = slot_job(k, n_chunks)
    truth = truth_of(tmp_path, ("slots", n_chunks), k, T, job["index"], [job["search"]], job["max_kmer"])
    assert truth["chunks"] == n_chunks
    sizes = [len(job["search"])]
    with context(k, job["max_kmer"], chunk_group=group) as ctx:                 # unarmed, fresh: the fast path, and the checker's result
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        assert only(ran, tps.SEARCH_KERNELS) == unarmed, (case, ran)
        fb.check_job((case, "unarmed"), got, truth, sizes)
    with context(k, job["max_kmer"], chunk_group=group) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        with refusing(at_least=refuse_slots * filter_bytes(k)) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        print(case, ran, r.seen)
        assert r.seen["refused"] == refusals and r.seen["last_refused_bytes"] % filter_bytes(k) == 0, (case, r.seen)
        assert only(ran, tps.SEARCH_KERNELS) == armed, (case, ran)
        fb.check_build_kernels(ran_as_times(ran), n_chunks, case)
        fb.check_job((case, "armed"), got, truth, sizes)
        slots_hold(ctx, case, k, job["index"], truth, in_slot, n_slots)
        # the next call asks again: disarmed, the fast path and its slots
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        assert only(ran, tps.SEARCH_KERNELS) == unarmed, (case, "disarmed", ran)
        fb.check_job((case, "disarmed"), got, truth, sizes)


def ran_as_times(ran):
    return {n: (c, 0.0) for n, c in ran.items()}


@pytest.mark.parametrize("case", sorted(LADDER))
def test_slot_ladder_of_a_profile(tmp_path, case):
    n_chunks, group, refuse_slots, unarmed, armed, refusals, in_slot, n_slots = LADDER[case]
    k, commet = SLOT_K, _commet()
    job = slot_job(k, n_chunks)
    truths = {t: truth_of(tmp_path, ("slots", n_chunks), k, t, job["index"], [job["search"]], job["max_kmer"]) for t in (1, 2)}
    n = len(job["search"])
    with context(k, job["max_kmer"], chunk_group=group) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        (first, info), ran = timed(ctx, lambda: ctx.index_and_profile(irs, [qrs], max_hits=4))
        assert only(ran, HITS_KERNELS) == {HITS_OF[n_]: c for n_, c in unarmed.items()}, (case, ran)
        assert info["n_chunks"] == n_chunks and info["kmers_indexed"] == truths[2]["kmers"]
    with context(k, job["max_kmer"], chunk_group=group) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        with refusing(at_least=refuse_slots * filter_bytes(k)) as r:
            (hits, info), ran = timed(ctx, lambda: ctx.index_and_profile(irs, [qrs], max_hits=4))
        print(case, ran, r.seen)
        assert r.seen["refused"] == refusals, (case, r.seen)
        assert only(ran, HITS_KERNELS) == {HITS_OF[n_]: c for n_, c in armed.items()}, (case, ran)
        assert info["n_chunks"] == n_chunks and info["kmers_indexed"] == truths[2]["kmers"]
        assert np.array_equal(hits[0], first[0])
        for t in (1, 2):
            assert np.array_equal(util.bools_from_bits(commet.tags_at(hits[0], t), n), truths[t]["tags"][0]), (case, t)
        slots_hold(ctx, case, k, job["index"], truths[2], in_slot, n_slots)


# ---- (f) the slots fit, the interleaved planes do not ---------------------------------------------------------------------------------------------
def test_interleaved_planes_refused_with_the_slots_granted(tmp_path):
    """No size threshold separates the planes (smaller) from the slot block, so by count: the context has run the job chunk by chunk
    (every kept buffer but slots and planes exists), then the job in groups of eight asks for the eight slots (request 1) and the
    planes at stride 8 (request 2, refused): ensure_slots fails WITH its eight slots, the ladder goes to groups of four"""
    k = SLOT_K
    job = slot_job(k, 8)
    truth = truth_of(tmp_path, ("slots", 8), k, T, job["index"], [job["search"]], job["max_kmer"])
    sizes = [len(job["search"])]
    with context(k, job["max_kmer"], chunk_group=1) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        fb.check_job("f warm", ctx.index_and_search(irs, [qrs]), truth, sizes)
        ctx.set_option("chunk_group", 8)
        with refusing(nth=2) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        print("f", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 8 * plane_bytes(k), r.seen
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group_kernel": 2}, ran
        fb.check_job("f armed", got, truth, sizes)
        slots_hold(ctx, "f", k, job["index"], truth, [4, 5, 6, 7, None, None, None, None], 8)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))          # the next job asks for the planes again
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": 1}, ran
        fb.check_job("f disarmed", got, truth, sizes)


# ---- (g), (h) shared passes ---------------------------------------------------------------------------------------------------------------------
def many_case(tmp_path, k, chunk_counts, **kw):
    jobs = [slot_job(k, c, seed=10 + j, **kw) for j, c in enumerate(chunk_counts)]
    assert len({j["max_kmer"] for j in jobs}) == 1
    search = [jobs[i // 3 % len(jobs)]["search"][i] for i in range(len(jobs[0]["search"]))]      # every job finds some of them (a job's every third read is random)
    truths = [truth_of(tmp_path, ("many", tuple(chunk_counts), j, len(search)), k, T, job["index"], [search], job["max_kmer"]) for j, job in enumerate(jobs)]
    assert [tr["chunks"] for tr in truths] == list(chunk_counts)
    assert all(tr["stats"][0]["shared"] > 0 for tr in truths)
    return jobs, search, truths


def check_many(what, got, truths, n):
    tags, stats, info = got
    for j, tr in enumerate(truths):
        mine = util.bools_from_bits(tags[j], n)
        assert np.array_equal(mine, tr["tags"][0]), (what, j, np.nonzero(mine != tr["tags"][0])[0][:10].tolist())
        assert [stats[j][f] for f in STAT] == [tr["stats"][0][f] for f in STAT], (what, j)
    assert info["n_chunks"] == sum(tr["chunks"] for tr in truths) and info["kmers_indexed"] == sum(tr["kmers"] for tr in truths), (what, info)


@pytest.mark.parametrize("chunk_counts", [(3, 5), (3, 6)])
def test_shared_passes_without_room(tmp_path, chunk_counts):
    """3 + 5 chunks are ONE pass of eight slots: refused at once, rerun_alone_no_room before anything ran.  3 + 6: pass one (job 0) runs on three
    granted slots and writes its stats, pass two finds no room, rerun_alone_no_room runs every job again alone and the account starts over"""
    k = SLOT_K
    jobs, search, truths = many_case(tmp_path, k, chunk_counts)
    n, total = len(search), sum(chunk_counts)
    with context(k, jobs[0]["max_kmer"]) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        alone = [ctx.index_and_search(rs, [qrs])[2] for rs in sets]
        got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        passes = 1 if total <= 8 else 2
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": passes} and got[2]["search_launches"] == passes, ran
        check_many("unarmed", got, truths, n)
    with context(k, jobs[0]["max_kmer"]) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        with refusing(at_least=4 * filter_bytes(k)) as r:
            got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        print(chunk_counts, ran, r.seen, got[2])
        assert r.seen["refused"] > 0
        # alone: the job of three chunks on its three granted slots in one group pass, the other chunk by chunk
        shared_first = 1 if total > 8 else 0
        assert only(ran, tps.SEARCH_KERNELS) == dict({"search_group_kernel": 1, "search_kernel": chunk_counts[1]},
                                                    **({"search_group8_kernel": 1} if shared_first else {})), ran
        check_many("armed", got, truths, n)
        info = got[2]
        for f in ("n_chunks", "kmers_indexed", "reads_indexed", "reads_scanned"):
            assert info[f] == sum(a[f] for a in alone), (f, info[f], [a[f] for a in alone])      # the jobs alone, not doubled
        assert info["index_launches"] == total and info["search_launches"] == 1 + chunk_counts[1], info
        got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))      # disarmed: the same call shares passes again
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": passes} and got[2]["search_launches"] == passes, ran
        check_many("disarmed", got, truths, n)


def test_shared_passes_without_their_tag_buffer(tmp_path):
    """ensure_pass_buffers: the jobs' found flags (8 * tag_words * 8 bytes) refused, by count — the context has run the call job by
    job, so the flags are the first thing a sharing call asks for"""
    k = SLOT_K
    jobs, search, truths = many_case(tmp_path, k, (3, 5))
    n = len(search)
    with context(k, jobs[0]["max_kmer"], multi_job=1) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        check_many("job by job", ctx.index_many_and_search(sets, qrs), truths, n)
        ctx.set_option("multi_job", 0)
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        print("h", ran, r.seen, got[2])
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 8 * (n // 64 + 1) * 8, r.seen
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group_kernel": 1, "search_group8_kernel": 1} and got[2]["search_launches"] == 2, ran
        check_many("armed", got, truths, n)
        got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": 1} and got[2]["search_launches"] == 1, ran
        check_many("disarmed", got, truths, n)


# ---- (i) pairs --------------------------------------------------------------------------------------------------------------------------------
def test_pairs_without_room(tmp_path):
    k = SLOT_K
    jobs, search, truths = many_case(tmp_path, k, (1, 1, 1, 1, 1))
    n = len(search)
    tq = ("tq_probe_kernel", "tq_replay_kernel", "search_kernel", "search_group_kernel", "search_group8_kernel")
    with context(k, jobs[0]["max_kmer"], tiled_search=2) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        assert only(ran, tq) == {"tq_probe_kernel": 3, "tq_replay_kernel": 3} and got[2]["search_launches"] == 3, ran
        check_many("unarmed", got, truths, n)
    with context(k, jobs[0]["max_kmer"], tiled_search=2) as ctx:                # no two slots: every job alone, through the tiled search of one
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        with refusing(at_least=2 * filter_bytes(k)) as r:
            got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        print("i slots", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 2 * filter_bytes(k), r.seen
        assert only(ran, tq) == {"tq_probe_kernel": 5, "tq_replay_kernel": 5} and got[2]["search_launches"] == 5, ran
        check_many("no two slots", got, truths, n)
    with context(k, jobs[0]["max_kmer"], tiled_search=1) as ctx:                # the list refused AFTER run_pair has built its two filters
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        check_many("warm", ctx.index_many_and_search(sets, qrs), truths, n)     # (a shared pass: every buffer but the list exists now)
        ctx.set_option("tiled_search", 2)
        n_slices, n_pieces = 1 << (k - 24), (n + 255) // 256
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        print("i list", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == (n_slices * n_pieces + 1) * 8, r.seen
        assert only(ran, tq) == {"search_kernel": 5} and got[2]["search_launches"] == 5, (ran, got[2])
        check_many("no list", got, truths, n)


# ---- (i') the list of a job's selected reads, refused inside a call of several jobs ------------------------------------------------------------------
# The list (sel_ids; job_parts.hpp, prepare_job_selection) is an optimisation of the bucketed build of a set of one read length: without
# room for it the build walks the selection bitmap.  That must hold inside a shared pass and a pair as it does for a job alone: the
# call goes on sharing, and every output is the checker's.
_SELECTED = {}


def selected_case(tmp_path, k, chunk_counts, n0=60, L=100, n_search=150):
    """many_case for index sets of ONE read length under a real selection (every third read dropped: plans neither dense nor all-ones).
    Job 0 fixes max_kmer for its chunk count, the others get the fewest reads that make theirs at that max_kmer; jobs of one chunk
    are one chunk without the selection too.  -> (jobs [dict(index, select, max_kmer)], search, truths)"""
    import oracle_pool
    key = (k, tuple(chunk_counts), n0, L, n_search)
    if key not in _SELECTED:
        rng = np.random.default_rng(7000 + 100 * k + sum(chunk_counts))
        w = L - k + 1
        select = lambda n: np.arange(n) % 3 != 0
        first = [hg.rand(rng, L) for _ in range(n0)]
        max_kmer = n0 * w + 1 if chunk_counts[0] == 1 else jf.max_kmer_for(k, first, chunk_counts[0], select(n0))[0]
        jobs = [dict(index=first, select=select(n0), max_kmer=max_kmer)]
        for c in chunk_counts[1:]:
            for n in range(n0, 8 * n0):
                cut = oracle_pool.chunks_from_counts(np.full(int(select(n).sum()), w), max_kmer)
                if len(cut) == c and cut[-1][1] - cut[-1][0] >= 3:
                    break
            jobs.append(dict(index=[hg.rand(rng, L) for _ in range(n)], select=select(n), max_kmer=max_kmer))
        search = []
        for i in range(n_search):                                               # every job finds some of them
            job = jobs[i // 3 % len(jobs)]
            if i % 3 == 2:
                search.append(hg.rand(rng, 80))
            else:
                r = job["index"][int(rng.choice(np.nonzero(job["select"])[0]))]
                a = int(rng.integers(0, L - 80 + 1))
                search.append(r[a:a + 80])
        _SELECTED[key] = jobs, search
    jobs, search = _SELECTED[key]
    truths = [truth_of(tmp_path, ("selected", key, j), k, T, job["index"], [search], job["max_kmer"], index_select=job["select"]) for j, job in enumerate(jobs)]
    assert [tr["chunks"] for tr in truths] == list(chunk_counts)
    assert all(tr["stats"][0]["shared"] > 0 for tr in truths)
    return jobs, search, truths


def ids_bytes(n_reads, indexed):
    """build_selection_list -> build_id_list: max(the plan's indexed reads, half the set) ids of four bytes"""
    return max(indexed, n_reads // 2) * 4


def test_selection_list_refused_in_a_shared_pass(tmp_path):
    """by count: the context has run the call on the whole sets (dense plans: every buffer of a shared pass, no list), so job 0's list is
    the first thing the call under selections asks for.  Job 0 is built from the bitmap, job 1 from its list, in ONE pass"""
    k = SLOT_K
    jobs, search, truths = selected_case(tmp_path, k, (2, 3))
    n = len(search)
    sels = [util.bits_from_bools(j["select"]) for j in jobs]
    with context(k, jobs[0]["max_kmer"]) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        _, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        assert "search_group8_kernel" in ran and "sel_ids_kernels" not in ran, ran
        call = lambda: ctx.index_many_and_search(sets, qrs, index_selects=sels)
        with refusing(nth=1) as r:
            got, ran = timed(ctx, call)
        print("list, shared pass", ran, r.seen, got[2])
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == ids_bytes(len(jobs[0]["index"]), truths[0]["stats"][0]["indexed"]), r.seen
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": 1} and got[2]["search_launches"] == 1, ran
        assert ran.get("sel_ids_kernels") == 1, ran
        check_many("armed", got, truths, n)
        again, ran = timed(ctx, call)                                            # disarmed: both lists, the same result
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group8_kernel": 1} and ran.get("sel_ids_kernels") == 2, ran
        check_many("disarmed", again, truths, n)
        assert same_job(again, got)


def test_selection_list_refused_in_a_pair(tmp_path):
    """the same for two jobs of one chunk each that go through one tiled scan (run_pair)"""
    k = 25                                                                       # (the tiled search: k > 24)
    jobs, search, truths = selected_case(tmp_path, k, (1, 1))
    n = len(search)
    sels = [util.bits_from_bools(j["select"]) for j in jobs]
    tq = ("tq_probe_kernel", "tq_replay_kernel", "search_kernel", "search_group_kernel", "search_group8_kernel")
    with context(k, jobs[0]["max_kmer"], tiled_search=2) as ctx:
        sets, qrs = [load(ctx, j["index"]) for j in jobs], load(ctx, search)
        _, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs))
        assert only(ran, tq) == {"tq_probe_kernel": 1, "tq_replay_kernel": 1} and "sel_ids_kernels" not in ran, ran
        qrs.drop_cache()                                                         # (else dev_alloc gives the set's query list back and asks again: granted)
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_many_and_search(sets, qrs, index_selects=sels))
        print("list, pair", ran, r.seen, got[2])
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == ids_bytes(len(jobs[0]["index"]), truths[0]["stats"][0]["indexed"]), r.seen
        assert only(ran, tq) == {"tq_probe_kernel": 1, "tq_replay_kernel": 1} and got[2]["search_launches"] == 1, ran
        assert ran.get("sel_ids_kernels") == 1, ran
        check_many("armed", got, truths, n)


def test_selection_list_refused_in_a_shared_profile_pass(tmp_path):
    """the threshold sweep's shape: two jobs on ONE set under two selections, caps 2 and 4; bytes as each job gives alone"""
    k = SLOT_K
    jobs, search, _ = selected_case(tmp_path, k, (2, 3))
    index = jobs[0]["index"]
    sels = [util.bits_from_bools(np.arange(len(index)) % 3 != m) for m in (0, 1)]
    caps = [2, 4]
    with context(k, jobs[0]["max_kmer"]) as ctx:
        irs, qrs = load(ctx, index), load(ctx, search)
        _, ran = timed(ctx, lambda: ctx.index_many_and_profile([irs, irs], qrs, max_hits=caps))
        assert ran.get("hits_jobs_kernel") == 1 and "sel_ids_kernels" not in ran, ran
        with refusing(nth=1) as r:
            (hits, info), ran = timed(ctx, lambda: ctx.index_many_and_profile([irs, irs], qrs, index_selects=sels, max_hits=caps))
        print("list, shared hits pass", ran, r.seen, info)
        assert ran.get("hits_jobs_kernel") == 1 and not only(ran, HITS_KERNELS) and info["search_launches"] == 1, ran
        assert ran.get("sel_ids_kernels") == 1, ran
        alone = [ctx.index_and_profile(irs, [qrs], index_select=sels[j], max_hits=caps[j]) for j in range(2)]
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == ids_bytes(len(index), alone[0][1]["reads_indexed"]), r.seen
        for j in range(2):
            assert np.array_equal(hits[j], alone[j][0][0]) and hits[j].any(), j
        for f in ("n_chunks", "kmers_indexed", "reads_indexed"):
            assert info[f] == sum(a[1][f] for a in alone), (f, info)


# ---- (j) the query list of one job ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nth", [1, 2, 3, 4, 5, 6, 7])
def test_query_list_refused(tmp_path, nth):
    """the list's allocations in build_query_list's order — tile offsets, the scan's totals, addresses, owners, tile starts, tile lengths —
    and the result bytes (ensure_query_results): the set keeps the gather kernels, a second job does not ask again, drop_cache() does"""
    k, n_chunks = SLOT_K, 3
    job = slot_job(k, n_chunks)
    truth = truth_of(tmp_path, ("slots", n_chunks), k, T, job["index"], [job["search"]], job["max_kmer"])
    sizes = [len(job["search"])]
    entries = (1 << (k - 24)) * ((sizes[0] + 255) // 256)
    known = {1: (entries + 1) * 8, 2: (entries // 4096 + 1 + 1) * 8, 5: entries * 4, 6: entries * 2}
    with context(k, job["max_kmer"], chunk_group=1, tiled_search=1) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        fb.check_job("j warm", ctx.index_and_search(irs, [qrs]), truth, sizes)
        ctx.set_option("tiled_search", 2)
        with refusing(nth=nth) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        print("j", nth, ran, r.seen)
        assert r.seen["refused"] == 1 and (nth not in known or r.seen["last_refused_bytes"] == known[nth]), (r.seen, known)
        assert "tq_probe_kernel" not in ran and ran.get("search_kernel") == n_chunks, ran
        fb.check_job("j armed", got, truth, sizes)
        with refusing() as r:                                                    # (counting only) the second job does not ask for the list again
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        assert "tq_probe_kernel" not in ran and "tq_count_kernel" not in ran and ran.get("search_kernel") == n_chunks, ran
        assert r.seen["refused"] == 0, r.seen
        fb.check_job("j second", got, truth, sizes)
        qrs.drop_cache()
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        assert ran.get("tq_probe_kernel") == n_chunks and "search_kernel" not in ran, ran
        fb.check_job("j after drop_cache", got, truth, sizes)


# ---- (k) dev_alloc gives cached lists back and asks again ----------------------------------------------------------------------------------------------
def test_refused_slot_group_is_granted_after_the_lists_went(tmp_path):
    k = SLOT_K
    job = slot_job(k, 2)
    other = job["search"][::-1][:130]                                           # a second search set with hits of its own
    one, two = sum(len(r) - k + 1 for r in job["index"]) + 1, job["max_kmer"]      # max_kmer of one chunk, of two
    truth_x = truth_of(tmp_path, ("k", "x"), k, T, job["index"], [other], one)
    truth_q = truth_of(tmp_path, ("slots", 2), k, T, job["index"], [job["search"]], two)
    assert truth_x["chunks"] == 1 and truth_q["chunks"] == 2
    with context(k, one, chunk_group=1, tiled_search=2) as ctx:
        irs, qrs, xrs = load(ctx, job["index"]), load(ctx, job["search"]), load(ctx, other)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [xrs]))         # a tiled job on X: its list is built and cached
        assert ran.get("tq_probe_kernel") == 1 and xrs.cache_bytes > 0
        fb.check_job("k x", got, truth_x, [len(other)])
        ctx.set_option("tiled_search", 1)
        ctx.set_option("max_kmer", two)
        fb.check_job("k warm", ctx.index_and_search(irs, [qrs]), truth_q, [len(job["search"])])      # two chunks, one at a time: one slot
        ctx.set_option("chunk_group", 2)
        before = ctx.cache_stats()["evictions"]
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        print("k", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == 2 * filter_bytes(k) and r.seen["requests"] >= 2, r.seen
        assert only(ran, tps.SEARCH_KERNELS) == {"search_group_kernel": 1}, ran   # the group of two DID get its slots, on the retry
        assert ctx.cache_stats()["evictions"] == before + 1 and xrs.cache_bytes == 0
        fb.check_job("k armed", got, truth_q, [len(job["search"])])
        slots_hold(ctx, "k", k, job["index"], truth_q, [0, 1], 2)
        ctx.set_option("tiled_search", 2)
        ctx.set_option("max_kmer", one)
        ctx.set_option("chunk_group", 1)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [xrs]))         # the evicted set's next tiled job builds its list again
        assert "tq_count_kernel" in ran and ran.get("tq_probe_kernel") == 1 and xrs.cache_bytes > 0, ran
        fb.check_job("k x again", got, truth_x, [len(other)])


# ---- (l), (m) the table regimes ---------------------------------------------------------------------------------------------------------------------
TABLE_K, TABLE_CHUNKS = 16, 300


def table_sizes(k, n_chunks):
    """bytes of the wide rows (ensure_wide_tables: 4 tables of 2^k rows of rw words, rw = 8 words per 256 chunks rounded up to 32) and of
    the staging planes of 256 chunks (ensure_slice_buffers, gw = 8)"""
    nw = (n_chunks + 255) // 256 * 8
    rw = (nw + 31) // 32 * 32
    return dict(wide=((4 * rw) << k) * 4, stage=((32 * 8 * 4) << (k - 5)) * 4, narrow=((4 * 8) << k) * 4)


def test_table_regimes_without_room(tmp_path):
    commet = _commet()
    case = ps.ladder_case(TABLE_K, TABLE_CHUNKS)
    reads, counts = case["sets"]["ladder"]
    truth = truth_of(tmp_path, ("ladder", TABLE_K, TABLE_CHUNKS), TABLE_K, T, case["index"], [reads], case["max_kmer"])
    assert truth["chunks"] == TABLE_CHUNKS and np.array_equal(truth["tags"][0], counts >= T)
    size = table_sizes(TABLE_K, TABLE_CHUNKS)
    assert size["wide"] > size["stage"] == size["narrow"]
    tables = ("search_wide_kernel", "search_sliced_kernel")
    opts = dict(tps.DEFAULTS, slice_mode=2, slice_wide=2, max_kmer=case["max_kmer"])

    def fresh():
        ctx = commet.Context(k=TABLE_K, t=T)
        for name, value in opts.items():
            ctx.set_option(name, value)
        return ctx, load(ctx, case["index"]), load(ctx, reads)

    for what, at_least, refused_bytes, must, must_not in (
            ("unarmed", 0, 0, {"search_wide_kernel"}, {"search_sliced_kernel"}),
            ("wide rows refused", size["wide"], size["wide"], {"search_sliced_kernel"}, {"search_wide_kernel"}),
            ("staging planes refused", size["stage"], size["stage"], set(), set(tables))):
        ctx, irs, qrs = fresh()
        with ctx:
            with refusing(at_least=at_least) as r:
                got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
            print("l", what, only(ran, tps.SEARCH_KERNELS), r.seen)
            assert (r.seen["refused"] > 0) == (at_least > 0) and r.seen["last_refused_bytes"] == refused_bytes, (what, r.seen)
            assert must <= set(ran) and not (must_not & set(ran)), (what, sorted(ran))
            if not must:
                assert set(only(ran, tps.SEARCH_KERNELS)) <= {"search_kernel", "search_group_kernel", "search_group8_kernel"} and only(ran, tps.SEARCH_KERNELS), ran
            fb.check_job(what, got, truth, [len(reads)])
            if at_least:                                                         # the next job asks again
                got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
                assert "search_wide_kernel" in ran, (what, "disarmed", sorted(ran))
                fb.check_job((what, "disarmed"), got, truth, [len(reads)])


def test_profile_wide_rows_without_room():
    commet = _commet()
    case = ps.ladder_case(TABLE_K, TABLE_CHUNKS)
    reads, counts = case["sets"]["ladder"]
    size = table_sizes(TABLE_K, TABLE_CHUNKS)
    results = []
    for at_least in (0, size["wide"]):
        with commet.Context(k=TABLE_K, t=T) as ctx:
            for name, value in dict(tps.DEFAULTS, profile_wide=2, max_kmer=case["max_kmer"]).items():
                ctx.set_option(name, value)
            irs, qrs = load(ctx, case["index"]), load(ctx, reads)
            with refusing(at_least=at_least) as r:
                (hits, info), ran = timed(ctx, lambda: ctx.index_and_profile(irs, [qrs], max_hits=4))
            print("m", at_least, only(ran, HITS_KERNELS), r.seen)
            assert info["n_chunks"] == TABLE_CHUNKS
            if at_least:
                assert r.seen["refused"] > 0 and r.seen["last_refused_bytes"] == size["wide"], r.seen
                assert "hits_wide_kernel" not in ran and "hits_group_kernel" in ran, ran
            else:
                assert "hits_wide_kernel" in ran and "hits_group_kernel" not in ran and "hits_kernel" not in ran, ran
            assert np.array_equal(hits[0], np.minimum(counts, 4))
            results.append(hits[0])
    assert np.array_equal(results[0], results[1])


# ---- (n) the length order, (o) the sparse list ----------------------------------------------------------------------------------------------------
def test_length_order_refused(tmp_path):
    k, n_chunks = SLOT_K, 2
    job = slot_job(k, n_chunks, ragged_search=True)
    assert len({len(r) for r in job["search"]}) > 1
    truth = truth_of(tmp_path, ("ragged", n_chunks), k, T, job["index"], [job["search"]], job["max_kmer"])
    sizes = [len(job["search"])]
    with context(k, job["max_kmer"], chunk_group=1, ordered_scan=1) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        fb.check_job("n warm", ctx.index_and_search(irs, [qrs]), truth, sizes)
        ctx.set_option("ordered_scan", 2)
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        print("n", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == (sizes[0] + 8) * 4, r.seen
        assert "len_order_kernels" not in ran, ran
        fb.check_job("n armed", got, truth, sizes)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))          # the set keeps its natural order
        assert "len_order_kernels" not in ran, ran
        fb.check_job("n next", got, truth, sizes)
        qrs.offload()
        qrs.restore()
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))          # ... until it has left the device and come back
        assert "len_order_kernels" in ran, ran
        fb.check_job("n restored", got, truth, sizes)


def test_sparse_list_refused(tmp_path):
    k, n_chunks = SLOT_K, 2
    job = slot_job(k, n_chunks)
    n = len(job["search"])
    select = np.arange(n) % 2 == 0
    tags, stats, _, chunks, kmers = tls._oracle(str(tmp_path / "orc_sparse"), k, T, job["index"], [job["search"]], None, [select], job["max_kmer"])
    assert chunks == n_chunks

    def check(what, got):
        assert got[0][0].tobytes() == tags[0].tobytes(), what
        assert tuple(got[1][0][f] for f in STAT) == stats[0] and got[2]["n_chunks"] == chunks and got[2]["kmers_indexed"] == kmers, (what, got[1], stats)

    bits = util.bits_from_bools(select)
    with context(k, job["max_kmer"], chunk_group=1, sparse_search=1) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        check("o warm", ctx.index_and_search(irs, [qrs], search_selects=[bits]))
        ctx.set_option("sparse_search", 2)
        with refusing(nth=1) as r:
            got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs], search_selects=[bits]))
        print("o", ran, r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == max(int(select.sum()), 1024) * 4, r.seen
        assert ran.get("search_kernel") == n_chunks and ran.get("active_list_kernels", 0) == n_chunks - 1, ran      # the first pass only: the bitmap form
        check("o armed", got)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs], search_selects=[bits]))
        assert ran.get("active_list_kernels") == n_chunks, ran
        check("o disarmed", got)


# ---- (p) the item list of an oversize read ---------------------------------------------------------------------------------------------------------
def long_job(k, seed=3):
    rng = np.random.default_rng(seed)
    index = [hg.rand(rng, 110) for _ in range(20)] + [hg.rand(rng, 6000)] + [hg.rand(rng, 110) for _ in range(20)]
    search = [index[20][a:a + 300] for a in range(0, 5700, 400)] + [index[3][:80], hg.rand(rng, 500)] + [hg.rand(rng, 90) for _ in range(30)]
    return index, search, sum(len(r) - k + 1 for r in index) + 1              # (max_kmer: one chunk)


def test_item_list_of_an_oversize_read_refused(tmp_path):
    """launch_index under index_mode = 2: no room for the item list is an error that says so (a fallback to the atomic kernel exists for
    auto mode only, and auto mode does not take the bucketed build for such sets: LONG_INDEX_AUTO); the same call, disarmed, is right"""
    commet = _commet()
    k = 20
    index, search, max_kmer = long_job(k)
    truth = truth_of(tmp_path, ("long", k), k, T, index, [search], max_kmer)
    assert truth["chunks"] == 1
    n_bases = sum(len(r) for r in index)
    need = min(len(index) * ((6000 + 7) // 8), n_bases // 8 + len(index)) + 1
    items_bytes = (need + need // 8) * 4
    with context(k, max_kmer, long_search=2) as ctx:
        irs, qrs = load(ctx, index), load(ctx, search)
        with refusing(at_least=items_bytes) as r:
            with pytest.raises(commet.CommetError, match="memory for the item list"):
                ctx.index_and_search(irs, [qrs])
        print("p", r.seen)
        assert r.seen["refused"] == 1 and r.seen["last_refused_bytes"] == items_bytes, (r.seen, items_bytes)
        got, ran = timed(ctx, lambda: ctx.index_and_search(irs, [qrs]))
        assert "part_items_fill_kernel" in ran and "search_long_kernel" in ran, ran
        fb.check_job("p after", got, truth, [len(search)])


# ---- (q) hard failures ------------------------------------------------------------------------------------------------------------------------------
def test_context_and_read_set_creation_refused(tmp_path):
    commet = _commet()
    k = 20
    job = slot_job(k, 2)
    truth = truth_of(tmp_path, ("slots", 2), k, T, job["index"], [job["search"]], job["max_kmer"])
    for nth in (1, 2):                                                           # the filter, the counters
        with refusing(nth=nth) as r:
            with pytest.raises(commet.CommetError, match=ALLOC_MESSAGE):
                commet.Context(k=k, t=T)
        assert r.seen["refused"] == 1 and r.seen["requests"] == nth, r.seen
    with context(k, job["max_kmer"], chunk_group=2) as ctx:
        for nth in range(1, 8):                                                  # commet_readset_create's seven
            with refusing(nth=nth) as r:
                with pytest.raises(commet.CommetError, match=ALLOC_MESSAGE):
                    commet.ReadSet(ctx, 1000, 100000)
            assert r.seen["refused"] == 1 and r.seen["requests"] == nth, r.seen
        with refusing(nth=8) as r:                                               # (there is no eighth)
            commet.ReadSet(ctx, 1000, 100000).close()
        assert r.seen["refused"] == 0 and r.seen["requests"] == 7, r.seen
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])             # the same process, disarmed: all is well
        fb.check_job("q after", ctx.index_and_search(irs, [qrs]), truth, [len(job["search"])])


def test_restore_refused(tmp_path):
    commet = _commet()
    k = 20
    job = slot_job(k, 2)
    truth = truth_of(tmp_path, ("slots", 2), k, T, job["index"], [job["search"]], job["max_kmer"])
    with context(k, job["max_kmer"], chunk_group=2) as ctx:
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        for rs in (irs, qrs):
            rs.offload()
            for nth in range(1, 8):
                with refusing(nth=nth) as r:
                    with pytest.raises(commet.CommetError, match=ALLOC_MESSAGE):
                        rs.restore()
                assert r.seen["refused"] == 1 and r.seen["requests"] == nth and not rs.resident and rs.device_bytes == 0, (nth, r.seen)
                with pytest.raises(commet.CommetError, match="offloaded"):
                    ctx.index_and_search(irs, [qrs])
            rs.restore()                                                         # its host copy was intact
            assert rs.resident
        fb.check_job("q restored", ctx.index_and_search(irs, [qrs]), truth, [len(job["search"])])


@pytest.mark.parametrize("name", ["uniform_100", "long_mixed_e1.5"])
def test_read_filter_refused(tmp_path, name):
    """the Shannon table (request 1) and the set's scratch (request 2); lane kernel and wave kernel; the filter_reads tool is the reference"""
    import test_gpu_read_filter as trf
    from read_filter_cases import CASES
    commet = _commet()
    case = next(c for c in CASES if c.name == name)
    paths = case.build(str(tmp_path / "in"))
    want_bools, want_stats, _ = trf._tool(case, paths, str(tmp_path / "tool"))
    with commet.Context(k=20, t=T) as ctx:
        rs = commet.ReadSet.from_fasta(ctx, paths)
        for nth in (1, 2):
            with refusing(nth=nth) as r:
                with pytest.raises(commet.CommetError, match=ALLOC_MESSAGE):
                    rs.filter(**case.api_kwargs())
            assert r.seen["refused"] == 1 and r.seen["requests"] == nth, r.seen
        with refusing() as r:
            trf._check(rs, case, want_bools, want_stats)
        assert r.seen["requests"] == 1 and r.seen["refused"] == 0, r.seen        # the scratch is asked for again (the table came with request 1 of the run before)
        trf._check(rs, case, want_bools, want_stats)


def test_staging_buffers_refused():
    """commet_readset_stage_acquire: a refused device staging buffer used to leave a stage with its pinned half only, which the next
    acquire took for complete (found by reading the call sites of dm_malloc); now the next acquire makes what is missing"""
    commet = _commet()
    rng = np.random.default_rng(9)
    reads = util.random_reads(rng, 300, 30, 150)
    bases, offs = util.to_batch(reads)
    with commet.Context(k=20, t=T) as ctx:
        want = load(ctx, reads).kmer_counts()
        rs = commet.ReadSet(ctx, len(reads), int(offs[-1]))
        for nth in (1, 2):
            with refusing(nth=nth) as r:
                with pytest.raises(commet.CommetError, match=ALLOC_MESSAGE):
                    rs.add_file_staged(bases, offs)
            assert r.seen["refused"] == 1, r.seen
            rs.close()
            rs = commet.ReadSet(ctx, len(reads), int(offs[-1]))
        # a stage that failed half-way, asked again on the SAME set
        rs._check(rs._lib.commet_readset_begin_file(rs._h))
        import ctypes as C
        from commet_amd import lib as _l
        hb, ho, bcap, rcap = _l.u8p(), _l.u64p(), C.c_uint64(0), C.c_uint64(0)
        with refusing(nth=2) as r:
            assert rs._lib.commet_readset_stage_acquire(rs._h, C.byref(hb), C.byref(bcap), C.byref(ho), C.byref(rcap)) != 0
        assert r.seen["refused"] == 1
        with refusing() as r:
            assert rs._lib.commet_readset_stage_acquire(rs._h, C.byref(hb), C.byref(bcap), C.byref(ho), C.byref(rcap)) == 0
        assert r.seen["requests"] == 1, r.seen                                   # only the buffer that was missing
        rs._check(rs._lib.commet_readset_stage_commit(rs._h, 0))
        rs.close()
        rs = commet.ReadSet(ctx, len(reads), int(offs[-1]))
        rs.add_file_staged(bases, offs)
        rs.finalize()
        assert np.array_equal(rs.kmer_counts(), want)


# ---- the sweep: every request of a call, one at a time -------------------------------------------------------------------------------------------------
def sweep(what, make, call, same, promised=()):
    """make() -> state (a fresh context and fresh sets; state[0] is the context); call(state) -> outputs; same(a, b): outputs equal.
    promised: byte counts whose refusal must be survived (a site that promises a fallback); each must occur.  -> (N, returned, raised)"""
    commet = _commet()
    state = make()
    try:
        with refusing() as r:
            base = call(state)
        n_requests = r.seen["requests"]
    finally:
        state[0].close()
    assert n_requests >= 1, what
    returned = raised = 0
    survived = set()
    for n in range(1, n_requests + 1):
        state = make()
        try:
            outcome = "returned"
            with refusing(nth=n) as r:
                try:
                    out = call(state)
                except commet.CommetError as e:
                    outcome, out = "raised: " + str(e), None
            print(f"{what}: n = {n}, last_refused_bytes = {r.seen['last_refused_bytes']}, {outcome}")
            assert r.seen["refused"] == 1, (what, n, r.seen)                     # else the run diverged before request n
            if out is None:
                raised += 1
                assert ALLOC_MESSAGE.search(outcome) and "internal error" not in outcome, (what, n, outcome)
                # (a scatter workspace buffer — launch_index_partitioned's HIP_OK run, which promises nothing — may have a promised site's size)
                assert r.seen["last_refused_bytes"] not in promised or "&ws." in outcome, (what, n, outcome)
                out = call(state)                                                # disarmed, the same call on the same context and sets
            else:
                returned += 1
                survived.add(r.seen["last_refused_bytes"])
            assert same(out, base), (what, n, outcome)
        finally:
            state[0].close()
    assert set(promised) <= survived, (what, sorted(promised), sorted(survived))
    print(f"{what}: N = {n_requests}, returned {returned}, raised {raised}")
    return base, n_requests, returned, raised


def same_job(a, b):
    return (all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and [[s[f] for f in STAT] for s in a[1]] == [[s[f] for f in STAT] for s in b[1]] and
            all(a[2][f] == b[2][f] for f in ("n_chunks", "kmers_indexed", "reads_indexed", "reads_scanned")))


def same_profile(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(a[1][f] == b[1][f] for f in ("n_chunks", "kmers_indexed", "reads_indexed"))


SWEEP_K = 20


def test_sweep_slot_loop(tmp_path):
    """3 chunks in a group of four (three granted slots when four are refused), a ragged index set under a selection (item list), two
    search sets, one under a selection that sparse_search = 2 walks as a list"""
    k = SWEEP_K
    rng = np.random.default_rng(41)
    index = [hg.rand(rng, int(rng.integers(60, 140))) for _ in range(90)]
    isel = np.arange(len(index)) % 4 != 1
    max_kmer = jf.max_kmer_for(k, index, 3, isel)[0]
    searches = [[index[i][:55] if i % 2 else hg.rand(rng, 70) for i in range(80)], [index[i][5:70] if i % 3 else hg.rand(rng, 64) for i in range(70)]]
    ssels = [None, np.arange(70) % 2 == 0]
    tags, stats, _, chunks, kmers = tls._oracle(str(tmp_path / "orc"), k, T, index, searches, isel, ssels, max_kmer)
    assert chunks == 3

    def make():
        ctx = context(k, max_kmer, chunk_group=4, sparse_search=2)
        return ctx, load(ctx, index), [load(ctx, s) for s in searches]

    def call(state):
        ctx, irs, qrs = state
        return ctx.index_and_search(irs, qrs, util.bits_from_bools(isel), [None, util.bits_from_bools(ssels[1])])

    promised = {4 * filter_bytes(k), 4 * plane_bytes(k), max(int(ssels[1].sum()), 1024) * 4}
    base, *_ = sweep("slot loop", make, call, same_job, promised)
    for q in range(2):
        assert base[0][q].tobytes() == tags[q].tobytes() and tuple(base[1][q][f] for f in STAT) == stats[q], q
    assert base[2]["n_chunks"] == chunks and base[2]["kmers_indexed"] == kmers


def test_sweep_uniform_selection_two_lanes(tmp_path):
    """an index set of one read length under a selection (the list of selected reads, sel_ids), two chunks on two lanes"""
    k = SWEEP_K
    rng = np.random.default_rng(42)
    index = [hg.rand(rng, 100) for _ in range(120)]
    isel = np.arange(len(index)) % 3 != 0
    max_kmer = jf.max_kmer_for(k, index, 2, isel)[0]
    search = [index[i][10:90] if i % 2 else hg.rand(rng, 80) for i in range(100)]
    truth = truth_of(tmp_path, "sweep uniform", k, T, index, [search], max_kmer, index_select=isel)
    assert truth["chunks"] == 2

    def make():
        ctx = context(k, max_kmer, chunk_group=2, index_lanes=2)
        return ctx, load(ctx, index), load(ctx, search)

    def call(state):
        ctx, irs, qrs = state
        return ctx.index_and_search(irs, [qrs], util.bits_from_bools(isel))

    promised = {2 * filter_bytes(k), 2 * plane_bytes(k)}
    base, *_ = sweep("uniform selection, two lanes", make, call, same_job, promised)
    fb.check_job("sweep uniform", base, truth, [len(search)])


@pytest.mark.parametrize("regime", ["narrow", "wide", "profile_wide"])
def test_sweep_tables(tmp_path, regime):
    commet = _commet()
    case = ps.ladder_case(TABLE_K, TABLE_CHUNKS)
    reads, counts = case["sets"]["ladder"]
    size = table_sizes(TABLE_K, TABLE_CHUNKS)
    opts = dict(narrow=dict(slice_mode=2, slice_wide=1), wide=dict(slice_mode=2, slice_wide=2), profile_wide=dict(profile_wide=2))[regime]

    def make():
        ctx = commet.Context(k=TABLE_K, t=T)
        for name, value in dict(tps.DEFAULTS, max_kmer=case["max_kmer"], **opts).items():
            ctx.set_option(name, value)
        return ctx, load(ctx, case["index"]), load(ctx, reads)

    if regime == "profile_wide":
        base, *_ = sweep(regime, make, lambda s: s[0].index_and_profile(s[1], [s[2]], max_hits=4), same_profile, {size["wide"], size["stage"]})
        assert np.array_equal(base[0][0], np.minimum(counts, 4)) and base[1]["n_chunks"] == TABLE_CHUNKS
    else:
        promised = {size["stage"]} | ({size["wide"]} if regime == "wide" else set())
        base, *_ = sweep(regime, make, lambda s: s[0].index_and_search(s[1], [s[2]]), same_job, promised)
        assert np.array_equal(util.bools_from_bits(base[0][0], len(reads)), counts >= T) and base[2]["n_chunks"] == TABLE_CHUNKS


def test_sweep_profile_through_slots(tmp_path):
    commet = _commet()
    k = SWEEP_K
    job = slot_job(k, 3)
    truth = truth_of(tmp_path, ("slots", 3), k, T, job["index"], [job["search"]], job["max_kmer"])

    def make():
        ctx = context(k, job["max_kmer"], chunk_group=4)
        return ctx, load(ctx, job["index"]), load(ctx, job["search"])

    base, *_ = sweep("profile through slots", make, lambda s: s[0].index_and_profile(s[1], [s[2]], max_hits=4), same_profile,
                     {4 * filter_bytes(k), 4 * plane_bytes(k)})
    assert np.array_equal(util.bools_from_bits(commet.tags_at(base[0][0], T), len(job["search"])), truth["tags"][0])
    assert base[1]["n_chunks"] == 3 and base[1]["kmers_indexed"] == truth["kmers"]


def test_sweep_shared_passes(tmp_path):
    k = SWEEP_K
    jobs, search, truths = many_case(tmp_path, k, (2, 3))

    def make():
        ctx = context(k, jobs[0]["max_kmer"])
        return ctx, [load(ctx, j["index"]) for j in jobs], load(ctx, search)

    same = lambda a, b: same_job(a, b) and a[2]["index_launches"] == b[2]["index_launches"]
    base, *_ = sweep("shared passes", make, lambda s: s[0].index_many_and_search(s[1], s[2]), same,
                     {8 * filter_bytes(k), 8 * plane_bytes(k), 8 * (len(search) // 64 + 1) * 8})
    check_many("sweep shared", base, truths, len(search))
    assert base[2]["search_launches"] == 1


def test_sweep_pairs(tmp_path):
    k = 25                                                                       # (the tiled search: k > 24)
    jobs, search, truths = many_case(tmp_path, k, (1, 1, 1))

    def make():
        ctx = context(k, jobs[0]["max_kmer"], tiled_search=2)
        return ctx, [load(ctx, j["index"]) for j in jobs], load(ctx, search)

    entries = (1 << (k - 24)) * ((len(search) + 255) // 256)
    base, *_ = sweep("pairs", make, lambda s: s[0].index_many_and_search(s[1], s[2]), same_job,
                     {2 * filter_bytes(k), 2 * plane_bytes(k), (entries + 1) * 8})
    check_many("sweep pairs", base, truths, len(search))
    assert base[2]["search_launches"] == 2


def test_sweep_shared_profile_passes(tmp_path):
    """commet_index_many_and_profile: the slot group, the interleaved planes and the jobs' byte arrays promise a fallback.  (More than
    256 search reads: two lines of bytes per job, so that the byte arrays are not the 512 bytes of the walked-reads counter, whose
    refusal is an error)"""
    commet = _commet()
    k, caps = SWEEP_K, [2, 4]
    jobs, search, truths = many_case(tmp_path, k, (2, 3), n_search=300)
    lines = (len(search) + 255) // 256
    assert lines == 2

    def make():
        ctx = context(k, jobs[0]["max_kmer"])
        return ctx, [load(ctx, j["index"]) for j in jobs], load(ctx, search)

    base, *_ = sweep("shared profile passes", make, lambda s: s[0].index_many_and_profile(s[1], s[2], max_hits=caps), same_profile,
                     {8 * filter_bytes(k), 8 * plane_bytes(k), len(jobs) * 256 * lines})
    for j, tr in enumerate(truths):
        assert np.array_equal(util.bools_from_bits(commet.tags_at(base[0][j], T), len(search)), tr["tags"][0]), j
    assert base[1]["search_launches"] == 1 and base[1]["n_chunks"] == 5 and base[1]["kmers_indexed"] == sum(tr["kmers"] for tr in truths)


def test_sweep_long_reads(tmp_path):
    k = SWEEP_K
    index, search, max_kmer = long_job(k)
    truth = truth_of(tmp_path, ("long", k), k, T, index, [search], max_kmer)
    assert truth["chunks"] == 1

    def make():
        ctx = context(k, max_kmer, long_search=2)
        return ctx, load(ctx, index), load(ctx, search)

    base, n, returned, raised = sweep("long reads", make, lambda s: s[0].index_and_search(s[1], [s[2]]), same_job)
    fb.check_job("sweep long", base, truth, [len(search)])
    assert raised >= 1                                                           # (the item list is one of them)


def test_sweep_read_filter(tmp_path):
    import test_gpu_read_filter as trf
    from read_filter_cases import CASES
    commet = _commet()
    cases = [next(c for c in CASES if c.name == n) for n in ("uniform_100", "long_mixed_e1.5")]
    paths = [c.build(str(tmp_path / c.name)) for c in cases]
    wants = [trf._tool(c, p, str(tmp_path / (c.name + "_tool"))) for c, p in zip(cases, paths)]

    def make():
        ctx = commet.Context(k=20, t=T)
        return ctx, [commet.ReadSet.from_fasta(ctx, p) for p in paths]

    def call(state):
        return [rs.filter(**c.api_kwargs()) for rs, c in zip(state[1], cases)]

    same = lambda a, b: all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(a, b))
    base, n, returned, raised = sweep("read filter", make, call, same)
    assert raised == n                                                           # the table and the scratch are needed: no fallback
    for (bits, stats), (want_bools, want_stats, _), c in zip(base, wants, cases):
        assert np.array_equal(np.unpackbits(bits, bitorder="little")[:want_bools.size].astype(bool), want_bools) and stats == want_stats, c.name


def test_sweep_restore(tmp_path):
    k = SWEEP_K
    job = slot_job(k, 2, ragged_search=True)
    truth = truth_of(tmp_path, ("ragged", 2), k, T, job["index"], [job["search"]], job["max_kmer"])

    def make():
        ctx = context(k, job["max_kmer"], chunk_group=2)
        irs, qrs = load(ctx, job["index"]), load(ctx, job["search"])
        qrs.offload()
        return ctx, irs, qrs

    def call(state):
        ctx, irs, qrs = state
        if not qrs.resident:                                                     # (a failed restore leaves it offloaded; a job that failed behind a good one does not)
            qrs.restore()
        return ctx.index_and_search(irs, [qrs])

    base, n, returned, raised = sweep("restore", make, call, same_job)
    fb.check_job("sweep restore", base, truth, [len(job["search"])])
    assert n >= 7 and raised >= 7
