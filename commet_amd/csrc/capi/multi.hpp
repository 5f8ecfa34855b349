// capi/multi.hpp — commet_index_many_and_search: several index_and_search jobs that search the SAME read set, their chunk filters side by side in one pass
// (a part of the one translation unit capi.hip: included there, in order, after job.hpp)
//
// Commet.py runs, for a reference set S_ref and every other set S_i, J2 = "S_ref in (S_i restricted to J1's result)" and
// J3 = "S_i in (S_ref restricted to J2's result)" (Commet.py:220, 233): index sets of a few chunk filters each, and the search set
// of all J2 jobs of a reference set is that reference set (of all J3 jobs of a target, that target).  A job on its own costs ~55
// L2-missing requests per searched read of which 37 are the lane-a gathers of the read's first-hit windows — addresses that depend on
// the read alone.  With the filters of up to eight chunks of several such jobs in the slots of one pass (their A planes interleaved:
// one 32-byte gather serves them all) the set is scanned once per pass instead of once per job; behind the gather
// search_group8_kernel runs job by job (kernels.hpp, job_mask).  Every job's result is what commet_index_and_search gives for it
// alone — tested against exactly that, and against the CPU checker through the N x N driver.
//
// The fast path takes what the N x N driver's jobs are: index sets whose chunks (at most eight per job) take the bucketed
// construction, a search set that is visited whole and qualifies for the register-mask kernel.  Anything else — and n_jobs = 1 — is
// run job by job through commet_index_and_search itself.
//
// Long reads: a search set that takes the wave-per-read kernel (long_ok) shares passes the same way — search_long_kernel with a
// job_mask, one interleaved plane-A load per window for the filters of every job of the pass (long_search.hpp) — under option
// multi_job = 2 only: whether such a pass beats the jobs alone has not been measured (MEASUREMENTS.md, "Long reads"), so auto runs
// them job by job.  For such a search set a chunk may take index_kernel (auto keeps it for sets with reads of more than 4096
// k-mers): its slot is zeroed first, as in build_group.
//
// Here: which calls take a fast path (plan_many), the pass itself — found flags, the scan, tags and statistics of every job — and two
// single-chunk jobs per tiled scan (run_pair).  In many.hpp, with commet_index_many_and_profile: the call's record (ManyCall), the
// argument checks, a job's plan, jobs run alone, the packing of jobs into passes, the build of a pass's filters, the account.
#pragma once

namespace {

// one commet_index_many_and_search call (the record both many-job calls keep: ManyCall, many.hpp)
struct ManyRun : ManyCall {
    uint8_t *const *tags_out;
    commet_pair_stats *stats;
    bool lng = false;                           // the search set takes the wave-per-read kernel (long_ok)
    ManyRun(commet_ctx *c_, int n, const commet_readset *const *irs, const uint8_t *const *isel, const commet_readset *srs, const uint8_t *ssel,
            uint8_t *const *tags, commet_pair_stats *st)
        : ManyCall(c_, n, irs, isel, srs, ssel), tags_out(tags), stats(st)
    {
    }
    uint64_t tag_words() const { return bitmap_words(search_rs->n_reads); }
};

// found flags of the jobs of a pass (`need` bitmaps over the search set; eight are taken) and their counters: 0 = there, 1 = no room
// for the flags, 2 = error
int ensure_pass_buffers(ManyRun &m, int need)
{
    commet_ctx *c = m.c;
    if (grow_kept(c, c->d_mtags, c->mtags_cap, (uint64_t) need * m.tag_words(), 8 * m.tag_words())) return 1;
    return grow_kept(c, c->d_jobcnt, c->jobcnt_cap, 16, 64) ? 2 : 0;
}

// Does a fast path take the call?  What the N x N driver's jobs are: index sets whose chunks (at most eight per job) take the bucketed
// construction, a search set that is visited whole and qualifies for the register-mask kernel — or, under multi_job = 2, for the
// wave-per-read kernel, whose passes also take chunks built by index_kernel.  Plans every job on the way (the plan from per-block
// k-mer sums made on the device, as commet_index_and_search does)
int plan_many(ManyRun &m, bool *fast)
{
    commet_ctx *c = m.c;
    const commet_readset *srs = m.search_rs;
    const uint8_t *ssel = m.search_select;
    if (ssel && all_ones(ssel, srs->n_reads)) ssel = nullptr;
    const uint64_t max_kmer = commet_max_kmer(c);
    m.lng = long_ok(c, srs);
    *fast = m.n_jobs >= 2 && c->k >= 2 && !c->count_probes && c->chunk_group >= 8 && c->multi_job != 1 && !c->part_no_uni && srs->n_reads > 0 &&
            slice_words(c, 8) == 0 && (m.lng ? c->multi_job == 2 : group8_ok(c, srs)) && plan_fast_ok(srs->files, ssel, srs->empty_reads, 1) &&
            (srs->n_reads + 255) / 256 < (1ull << 24);
    m.jobs.resize(*fast ? (size_t) m.n_jobs : 0);
    for (int j = 0; j < m.n_jobs && *fast; ++j) {
        const commet_readset *rs = m.index_rs[j];
        ManyRun::Job &job = m.jobs[(size_t) j];
        if (plan_many_job(m, j, max_kmer, fast)) return 1;
        if (job.plan.chunks.empty() || job.plan.chunks.size() > 8) *fast = false;
        for (const Chunk &ch : job.plan.chunks)
            if (!ch.n_reads || (!m.lng && !would_partition(c, rs, ch.kmers, ch.last - ch.first + 1))) *fast = false;    // (the bucketed build writes every tile of its slot itself; a pass of long reads zeroes the slots of the others)
        job.shares = *fast;
    }
    return 0;
}

// counters and the tags of jobs j0 .. j1 - 1 of a pass to the host; waits for the pass
int download_pass(ManyRun &m, int j0, int j1, unsigned long long *h_cnt, size_t n_cnt)
{
    commet_ctx *c = m.c;
    HIP_OK(hipMemcpyAsync(h_cnt, c->d_jobcnt, n_cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    for (int j = j0; j < j1; ++j)
        if (m.tags_out && m.tags_out[j])
            HIP_OK(hipMemcpyAsync(m.tags_out[j], c->d_mtags + (uint64_t) (j - j0) * m.tag_words(), bitmap_bytes_host(m.search_rs->n_reads), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    c->kclock.collect();
    m.clk.lap(m.ph_wait);
    return 0;
}

// ---- two single-chunk jobs per tiled scan ------------------------------------------------------------------------------------
// The J2 / J3 jobs of a matrix of 10 M-read sets index a fifth of a set (one chunk filter) and search a whole one through the
// tiled search: probe 2.2 ms + replay 3 ms per job.  The probe's gather of a query record's plane-A word serves two interleaved
// filters as cheaply as one, so consecutive jobs go through the scan in twos: their filters in slots 0 and 1, one probe, one
// replay that keeps the two jobs apart (tq_replay_kernel, job_tag_words).  An odd job out, and everything when the list cannot
// be had, runs through commet_index_and_search.
// Jobs j0, j0 + 1: 0 = done, 1 = error, 2 = not this way (no room for two slots, or the list could not be had after all): these two
// and the rest through the jobs' own path
int run_pair(ManyRun &m, int j0)
{
    commet_ctx *c = m.c;
    const commet_readset *srs = m.search_rs;
    if (ensure_slots(c, 2, 2)) {
        (void) hipGetLastError();
        return 2;
    }
    if (m.tm.begin_index()) return 1;
    // the two chunks are built side by side on the context's two index lanes (as the two chunks of one job are): first, on the main
    // stream, what each build reads — the selection bitmap and, for sets of one read length, the list of the selected reads, the
    // second job's in a buffer of its own — then the fork
    const uint32_t *ids_of[2] = {nullptr, nullptr};
    const bool same_set = m.index_rs[j0] == m.index_rs[j0 + 1];    // (one set in both jobs: ONE selection bitmap on the device — the second job's goes up behind the first build)
    auto prepare = [&](int j) { return prepare_job_selection(c, m.index_rs[j], m.jobs[(size_t) j].plan, j == j0 ? c->sel_ids : c->sel_ids2, &ids_of[j - j0]); };
    if (prepare(j0) || (!same_set && prepare(j0 + 1))) return 1;
    const bool lanes = c->index_lanes > 1 && !c->kclock.on && !same_set;
    if (lanes) {
        HIP_OK(hipEventRecord(c->ev_fork, c->stream));
        HIP_OK(hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
    }
    for (int j = j0; j < j0 + 2; ++j) {
        const commet_readset *rs = m.index_rs[j];
        const IndexPlan &plan = m.jobs[(size_t) j].plan;
        const Chunk &ch = plan.chunks[0];
        if (same_set && j == j0 + 1 && prepare(j)) return 1;
        c->cur_slot = j - j0;
        if (launch_index(c, rs, ch.first, ch.last - ch.first + 1, plan.dense ? nullptr : rs->d_sel, nullptr, ch.kmers, true, false, lanes ? j - j0 : 0,
                         ids_of[j - j0], 0, ch.n_reads))
            return 1;
        ++m.sum.index_launches;
    }
    if (lanes) {
        HIP_OK(hipEventRecord(c->ev_join, c->aux_stream));
        HIP_OK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    c->cur_slot = 0;
    if (launch_interleave(c, 2, 2) || m.tm.end_index()) return 1;
    HIP_OK(hipMemsetAsync(c->d_mtags, 0, 2 * m.tag_words() * sizeof(uint64_t), c->stream));
    HIP_OK(hipMemsetAsync(c->d_jobcnt, 0, 16 * sizeof(unsigned long long), c->stream));
    const int tiled = try_tiled(c, srs, 2, 0, nullptr, c->d_mtags, c->d_jobcnt, 2, m.tag_words());
    if (tiled == 2) return 1;
    if (tiled == 1) {
        HIP_OK(hipStreamSynchronize(c->stream));
        return 2;
    }
    ++m.sum.search_launches;
    if (m.tm.end_set(0)) return 1;
    m.clk.lap(m.ph_launch);
    unsigned long long h_cnt[4];
    if (download_pass(m, j0, j0 + 2, h_cnt, 4)) return 1;
    const float ms_s = account_pass_times(m);
    for (int j = j0; j < j0 + 2; ++j) {
        const IndexPlan &plan = m.jobs[(size_t) j].plan;
        const unsigned long long sc = h_cnt[2 * (j - j0)], fd = h_cnt[2 * (j - j0) + 1];
        if (sc != srs->n_reads)
            return fail("internal error: device scanned %llu reads, host plan says %llu (job %d)", sc, (unsigned long long) srs->n_reads, j);
        if (m.stats) {
            m.stats[j].indexed = plan.indexed_reads;
            m.stats[j].searched = srs->n_reads;
            m.stats[j].shared = fd;
            m.stats[j].search_ms = ms_s / 2.0;
        }
        m.sum.n_chunks += 1, m.sum.kmers_indexed += plan.kmers, m.sum.reads_indexed += plan.indexed_reads, m.sum.reads_scanned += srs->n_reads;
    }
    return 0;
}

// ---- a shared pass: the consecutive jobs `in_pass`, whose chunks fit the eight slots -----------------------------------------------------
// 0 = done, 1 = error, 2 = no room
int run_shared_pass(ManyRun &m, const std::vector<int> &in_pass)
{
    commet_ctx *c = m.c;
    const commet_readset *srs = m.search_rs;
    const int j0 = in_pass.front(), j1 = in_pass.back() + 1, g = pass_chunks(m, in_pass);
    if (const int rc = build_pass_filters(m, in_pass, g, 8)) return rc;
    uint32_t job_mask = 0;                          // the first slot of every job
    int slot = 0;
    for (int j : in_pass) job_mask |= 1u << slot, slot += m.n_chunks(j);
    if (hipMemsetAsync(c->d_mtags, 0, (size_t) (j1 - j0) * m.tag_words() * sizeof(uint64_t), c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_jobcnt, 0, 16 * sizeof(unsigned long long), c->stream) != hipSuccess)
        return fail("memset failed");
    // (a ragged search set: its reads in order of their window counts — every job's tags start empty; long reads: a wave per read, in the set's order)
    if (m.lng ? launch_search_long(c, srs, g, 8, nullptr, c->d_mtags, c->d_jobcnt, 2, nullptr, ActiveList{nullptr, nullptr}, 0, job_mask, m.tag_words())
              : launch_group_pass(c, srs, g, 8, nullptr, c->d_mtags, c->d_jobcnt, 2, nullptr, ActiveList{nullptr, nullptr}, true, 0, job_mask, m.tag_words()))
        return 1;
    ++m.sum.search_launches;
    if (m.tm.end_set(0)) return 1;
    m.clk.lap(m.ph_launch);
    unsigned long long h_cnt[16];
    if (download_pass(m, j0, j1, h_cnt, 16)) return 1;
    const float ms_s = account_pass_times(m);
    int rc = 0;
    slot = 0;
    for (int j : in_pass) {
        const ManyRun::Job &job = m.jobs[(size_t) j];
        uint64_t shared = 0, last_scanned = 0;
        for (size_t ci = 0; ci < job.plan.chunks.size(); ++ci, ++slot) {
            last_scanned = srs->n_reads - shared;          // (the set is visited whole)
            if (h_cnt[2 * slot] != last_scanned)
                rc = fail("internal error: device scanned %llu reads, host plan says %llu (job %d, chunk %zu)", h_cnt[2 * slot],
                          (unsigned long long) last_scanned, j, ci);
            shared += h_cnt[2 * slot + 1];
            m.sum.reads_scanned += last_scanned;
        }
        if (m.stats) {
            m.stats[j].indexed = job.plan.indexed_reads;
            m.stats[j].searched = last_scanned;
            m.stats[j].shared = shared;
            m.stats[j].search_ms = ms_s / (double) (j1 - j0);      // (the pass is shared: an equal part each)
        }
        m.sum.n_chunks += job.plan.chunks.size(), m.sum.kmers_indexed += job.plan.kmers, m.sum.reads_indexed += job.plan.indexed_reads;
    }
    return rc;
}

}  // namespace

extern "C" {

int commet_index_many_and_search(commet_ctx *c, int n_jobs, const commet_readset *const *index_rs, const uint8_t *const *index_select,
                                 const commet_readset *search_rs, const uint8_t *search_select, uint8_t *const *tags_out,
                                 commet_pair_stats *stats, commet_job_info *info)
{
    if (validate_many(c, n_jobs, index_rs, search_rs)) return 1;
    HIP_OK(hipSetDevice(c->device));
    // the sets of this call keep their cached query lists, and are neither exported nor offloaded, while it runs (as in
    // commet_index_and_search; the jobs that run one by one count their own sets again: in_job is a depth)
    SetUse in_jobs(c, search_rs);
    for (int j = 0; j < n_jobs; ++j) in_jobs.add(index_rs[j]);
    if (in_jobs.enter()) return 1;
    ManyRun m(c, n_jobs, index_rs, index_select, search_rs, search_select, tags_out, stats);
    const OneJob one = [&](int j, commet_job_info *ji) {
        uint8_t *to = tags_out ? tags_out[j] : nullptr;
        return commet_index_and_search(c, index_rs[j], index_select ? index_select[j] : nullptr, 1, &search_rs, search_select ? &search_select : nullptr,
                                       tags_out ? &to : nullptr, stats ? &stats[j] : nullptr, ji);
    };
    auto finish = [&](const char *what) {
        return finish_many(m, info, what, [&](const char *w) {
            fprintf(stderr, "[jobs x%d%s] plans %.2f ms, launches %.2f ms, wait + download %.2f ms; device: index %.2f ms, search %.2f ms\n", n_jobs, w,
                    m.ph_plan, m.ph_launch, m.ph_wait, m.sum.index_ms, m.sum.search_ms);
        });
    };
    bool fast = false, pairs = false;              // pairs: jobs of ONE chunk each on a search set that takes the tiled search, two jobs per scan
    if (plan_many(m, &fast)) return 1;
    if (fast) {
        // A search set that takes the tiled search (a query list within the cap: sets of up to ~15 M reads) loses little on its own — its
        // lane-a gathers come out of L2 — and jobs of one or two chunks each need no eight filter slots there (20 GiB more at k = 32, which a
        // fresh box hands out at 15-30 ms per GiB): such jobs stay out of the eight-slot passes (configs[2]'s leg: 1.5 s either way on a
        // used box, 2.0 s against 1.5 s on a fresh one).
        size_t most = 0;
        for (const ManyRun::Job &job : m.jobs) most = std::max(most, job.plan.chunks.size());
        std::lock_guard<std::mutex> qlk(c->ql_mu);
        if (most <= 2 && tiled_ok(c, search_rs, 2)) {
            fast = false;
            pairs = most == 1;
        }
    }
    if (!fast && !pairs) return run_jobs_alone(m, 0, n_jobs, one) || finish(nullptr);
    m.clk.lap(m.ph_plan);
    const int pb = ensure_pass_buffers(m, pairs ? 2 : 8);
    if (pb) return pb == 2 ? 1 : rerun_alone_no_room(m, one) || finish(nullptr);
    if (pairs) {
        int j0 = 0;
        for (; j0 + 1 < n_jobs; j0 += 2) {
            const int rc = run_pair(m, j0);
            if (rc == 1) return 1;
            if (rc == 2) break;
        }
        return run_jobs_alone(m, j0, n_jobs, one) || finish(", two per tiled scan");
    }
    for (const std::vector<int> &in_pass : pack_passes(m, 8)) {      // (every job shares: the passes are runs of consecutive jobs)
        const int rc = run_shared_pass(m, in_pass);
        if (rc == 1) return 1;
        if (rc == 2) return rerun_alone_no_room(m, one) || finish(nullptr);
    }
    return finish("");
}

}  // extern "C"
