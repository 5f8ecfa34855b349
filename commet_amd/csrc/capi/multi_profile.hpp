// capi/multi_profile.hpp — commet_index_many_and_profile: several commet_index_and_profile jobs that search the SAME read set, their chunk filters
// side by side in one hits pass (a part of the one translation unit capi.hip: included there, in order, after many.hpp, multi.hpp and profile.hpp)
// Here: which jobs a pass admits, the visited reads of the search set, the hits pass and its byte arrays.  The call's record, the argument
// checks, a job's plan, jobs run alone, the packing and the build of a pass's filters are many.hpp's, shared with commet_index_many_and_search.
//
// The threshold sweep of the symmetric comparison (commet_amd/sweep.py --full) runs, for every t, "A in (B restricted to the reads
// found at t)": T jobs that index selections of ONE set and all search A.  Alone each job walks A and makes its plane-A gathers,
// which depend on the read alone; with the chunk filters of up to eight slots of several such jobs in one pass (A planes
// interleaved, hits_jobs_kernel, hit_profile_jobs.hpp) the set is walked once per pass.  Every job's bytes are what
// commet_index_and_profile gives for it alone — tested against exactly that, and against the CPU checker.
// A search set of long reads (hits_wave_ok, profile.hpp) takes hits_jobs_wave_kernel, a wave per read on a persistent grid, under
// multi_job = 2: the same slots, builds and byte arrays, one other launch.
//
// A pass: the jobs in their order while their chunks fit min(8, chunk_group) slots (a job that runs alone does not close a pass);
// a job is never split, so its byte array is written by one pass.  The jobs are planned on the device (plan_index_on_device) and
// built one after the other on the context's one stream — jobs may index the same set under different selections: the selection
// bitmap, and the list made of it, go up in front of each job's build (build_pass_filters, many.hpp) — a chunk that does not take the
// bucketed build into a zeroed slot.  The search selection is the same for all jobs and reaches the kernel as the visited bitmap of plan_search: no list form.
//
// Through commet_index_and_profile itself, same bytes: the whole call when n_jobs < 2, k < 2, count_probes, multi_job = 1,
// chunk_group = 1, the search set is empty or takes the wave-per-read hits kernel and multi_job is not 2, or the device has no room
// for the slots or the byte arrays; a single job that the device planner does not take (an empty read in the set, a file without a selected read, an
// empty selection), that has no chunk or more chunks than a pass holds, or that is left alone in its pass — it picks its own regime
// (wide, narrow, tiled), its neighbours still share.
// Auto (multi_job = 0) shares where the search set takes a lane per read: measured against the jobs one by one in MEASUREMENTS.md,
// "Jobs that share a hits pass".  A search set of long reads stays job by job in auto, as on the search side (multi.hpp).
// Not built: the tiled probe or the bit-sliced tables for shared passes, passes shared between jobs whose search selections differ.
// commet_index_many_and_thresholds is the same call (profile_many below) with max_hits[j] = t[j] and another last step: per job the
// tags at t[j] and the per-file counts come down, not the bytes (HitsLeave, thresholds.hpp) — the many-job search with a threshold per job.
#pragma once

namespace {

// one commet_index_many_and_profile call (the record both many-job calls keep: ManyCall, many.hpp)
struct ProfileManyRun : ManyCall {
    const int *max_hits;
    uint8_t *const *hits_out;                   // job j's bytes; or, tags (commet_index_many_and_thresholds): job j's tags at max_hits[j] and its
    bool tags = false;                          // per-file counts, tags_out[j] and shared_out[j] (HitsLeave, thresholds.hpp)
    uint8_t *const *tags_out = nullptr;
    uint64_t *const *shared_out = nullptr;
    int cap = 8;                                // slots of a pass
    std::vector<uint8_t> vis;                   // the reads the passes visit (plan_search), unless all of them
    bool all_visited = false;
    uint64_t stride = 256;                      // bytes between the arrays of two jobs of a pass
    int shared_passes = 0;
    ProfileManyRun(commet_ctx *c_, int n, const commet_readset *const *irs, const uint8_t *const *isel, const commet_readset *srs, const uint8_t *ssel,
                   const int *caps, uint8_t *const *hits)
        : ManyCall(c_, n, irs, isel, srs, ssel), max_hits(caps), hits_out(hits)
    {
    }
    const uint64_t *d_sel() const { return all_visited ? nullptr : search_rs->d_sel; }
};

// does the call share passes at all?  A search set of long reads (hits_wave_ok, profile.hpp) under multi_job = 2 only: auto keeps
// such a set job by job, as multi.hpp does on the search side
bool profile_many_ok(const ProfileManyRun &m)
{
    const commet_ctx *c = m.c;
    const commet_readset *srs = m.search_rs;
    return m.n_jobs >= 2 && c->k >= 2 && !c->count_probes && c->multi_job != 1 && m.cap >= 2 && srs->n_reads > 0 &&
           (c->multi_job == 2 || !hits_wave_ok(c, srs)) && (srs->n_reads + 255) / 256 < (1ull << 24);
}

// the plan of every job the device planner takes, and the reads the passes visit (as plan_job makes them), on the device on return
int plan_profile_many(ProfileManyRun &m)
{
    commet_ctx *c = m.c;
    const uint64_t max_kmer = commet_max_kmer(c);
    m.jobs.resize((size_t) m.n_jobs);
    for (int j = 0; j < m.n_jobs; ++j) {
        ProfileManyRun::Job &job = m.jobs[(size_t) j];
        if (plan_many_job(m, j, max_kmer, &job.shares)) return 1;
        // a pass takes a planned job of 1 .. cap chunks, each with a read
        if (job.plan.chunks.empty() || job.plan.chunks.size() > (size_t) m.cap) job.shares = false;
        for (const Chunk &ch : job.plan.chunks)
            if (!ch.n_reads) job.shares = false;
    }
    const commet_readset *srs = m.search_rs;
    const uint8_t *ssel = m.search_select;
    if (ssel && all_ones(ssel, srs->n_reads)) ssel = nullptr;
    m.all_visited = plan_fast_ok(srs->files, ssel, srs->empty_reads, 1);
    if (!m.all_visited) {
        uint64_t visited = 0;
        m.vis = (ssel && srs->empty_reads.empty()) ? plan_search_select(srs->files, ssel, srs->n_reads, &visited)
                                                    : plan_search(srs->files, ssel, srs->empty_reads, srs->n_reads, &visited);
    }
    return 0;
}

// the visited reads of the search set to the device (a job that ran alone in between has put the same bits there)
int upload_visited(ProfileManyRun &m)
{
    if (m.all_visited) return 0;
    if (upload_bits(m.c, m.search_rs->d_sel, m.vis.data(), m.search_rs->n_reads)) return 1;
    HIP_OK(hipStreamSynchronize(m.c->stream));
    return 0;
}

int launch_hits_jobs(commet_ctx *c, const commet_readset *rs, int g, int gs, const JobSlots &js, const uint64_t *d_sel, uint8_t *d_hits, uint64_t stride,
                     unsigned long long *d_walked)
{
    const bool wave = hits_wave_ok(c, rs);          // a wave per read on a persistent grid, else a lane per read
    if (!wave && launch_size_ok(rs->n_reads)) return 1;
    const dim3 lanes((unsigned) ((rs->n_reads + 255) / 256));
    const FilterGroupView fg = filter_group(c, g, 0, true);
    KScope ks(c, wave ? "hits_jobs_wave_kernel" : "hits_jobs_kernel", c->stream);
    with_key(c->k, [&](auto key) {
        using W = decltype(key);
        with_value<2, 4, 8>(gs, [&](auto NF) {
            if (wave)
                COMMET_LAUNCH((hits_jobs_wave_kernel<W, NF>), dim3((unsigned) resident_blocks<hits_jobs_wave_kernel<W, NF>>(c, rs->n_reads)), dim3(LONG_WG), 0,
                              c->stream, rs->view(), fg, c->k, js, d_sel, d_hits, (uint32_t) (stride / 256), d_walked);
            else
                COMMET_LAUNCH((hits_jobs_kernel<W, NF>), lanes, dim3(256), 0, c->stream, rs->view(), fg, c->k, js, d_sel, d_hits, (uint32_t) (stride / 256),
                              d_walked);
        });
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- a shared pass: the jobs `in_pass`, whose chunks fit the pass's slots ---------------------------------------------------------------
// 0 = done, 1 = error, 2 = no room
int run_shared_hits_pass(ProfileManyRun &m, const std::vector<int> &in_pass)
{
    commet_ctx *c = m.c;
    const commet_readset *srs = m.search_rs;
    const int g = pass_chunks(m, in_pass), gs = g <= 2 ? 2 : g <= 4 ? 4 : 8;
    if (const int rc = build_pass_filters(m, in_pass, g, gs)) return rc;
    JobSlots js{0, 0};                              // per slot: the slots of its job, and the job's cap
    int slot = 0;
    for (int j : in_pass) {
        const ProfileManyRun::Job &job = m.jobs[(size_t) j];
        const int nc = m.n_chunks(j);
        const uint64_t mates = ((1ull << nc) - 1ull) << slot;
        for (int i = slot; i < slot + nc; ++i) js.mates |= mates << (8 * i), js.caps |= (uint64_t) m.max_hits[j] << (8 * i);
        slot += nc;
        m.sum.n_chunks += (uint64_t) nc, m.sum.kmers_indexed += job.plan.kmers, m.sum.reads_indexed += job.plan.indexed_reads;
    }
    if (hipMemsetAsync(c->d_hits, 0, in_pass.size() * m.stride, c->stream) != hipSuccess ||
        hipMemsetAsync(c->d_jobcnt, 0, sizeof(unsigned long long), c->stream) != hipSuccess)
        return fail("memset failed");
    if (launch_hits_jobs(c, srs, g, gs, js, m.d_sel(), c->d_hits, m.stride, c->d_jobcnt)) return 1;
    ++m.sum.search_launches, ++m.shared_passes;
    if (m.tm.end_set(0)) return 1;
    m.clk.lap(m.ph_launch);
    HIP_OK(hipMemcpyAsync(&c->h_counters[0], c->d_jobcnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HitsLeave leave;
    for (size_t q = 0; q < in_pass.size(); ++q) {
        const int j = in_pass[q];
        const uint8_t *d = c->d_hits + (uint64_t) q * m.stride;
        if (m.tags) leave.tags_of(d, srs, m.max_hits[j], 1, m.tags_out ? m.tags_out + j : nullptr, m.shared_out ? m.shared_out + j : nullptr);
        else if (m.hits_out && m.hits_out[j]) leave.bytes_of(d, srs->n_reads, m.hits_out[j]);
    }
    if (leave.queue(c)) return 1;
    HIP_OK(hipStreamSynchronize(c->stream));
    c->kclock.collect();
    leave.finish();
    m.sum.reads_scanned += c->h_counters[0];
    (void) account_pass_times(m);
    m.clk.lap(m.ph_wait);
    return 0;
}

// the call behind commet_index_many_and_profile (hits_out: the bytes) and commet_index_many_and_thresholds (hits_out == nullptr: job
// j's tags at max_hits[j] and its per-file counts): everything up to the download is the same
int profile_many(commet_ctx *c, int n_jobs, const commet_readset *const *index_rs, const uint8_t *const *index_select, const commet_readset *search_rs,
                 const uint8_t *search_select, const int *max_hits, uint8_t *const *hits_out, bool tags, uint8_t *const *tags_out,
                 uint64_t *const *shared_out, commet_job_info *info)
{
    if (validate_many(c, n_jobs, index_rs, search_rs)) return 1;
    for (int j = 0; j < n_jobs; ++j)
        if (max_hits[j] < 1 || max_hits[j] > 255) return fail("%s must be in 1..255 (got %d for job %d)", tags ? "t" : "max_hits", max_hits[j], j);
    HIP_OK(hipSetDevice(c->device));
    // the sets of this call are neither exported nor offloaded while it runs (the jobs that run alone count their own sets again: in_job is a depth)
    SetUse in_jobs(c, search_rs);
    for (int j = 0; j < n_jobs; ++j) in_jobs.add(index_rs[j]);
    if (in_jobs.enter()) return 1;
    ProfileManyRun m(c, n_jobs, index_rs, index_select, search_rs, search_select, max_hits, hits_out);
    m.cap = std::max(1, std::min(8, c->chunk_group));
    m.tags = tags, m.tags_out = tags_out, m.shared_out = shared_out;
    const OneJob one = [&](int j, commet_job_info *ji) {
        uint8_t *to = hits_out ? hits_out[j] : nullptr;
        ProfileWant want;
        if (tags) want.t_first = max_hits[j], want.n_t = 1, want.tags_out = tags_out ? tags_out + j : nullptr, want.shared_out = shared_out ? shared_out + j : nullptr;
        else want.hits_out = hits_out ? &to : nullptr;
        return profile_job(c, index_rs[j], index_select ? index_select[j] : nullptr, 1, &search_rs, search_select ? &search_select : nullptr, max_hits[j],
                           want, ji);
    };
    auto finish = [&](const char *what) {
        m.sum.probes = 0;
        return finish_many(m, info, what, [&](const char *w) {
            fprintf(stderr, "[profiles x%d%s] %d shared pass(es); plans %.2f ms, launches %.2f ms, wait + download %.2f ms\n", n_jobs, w, m.shared_passes,
                    m.ph_plan, m.ph_launch, m.ph_wait);
        });
    };
    // no room for the slots or the byte arrays of a shared pass: the single calls write every byte of every job again
    auto no_room = [&]() {
        m.shared_passes = 0;
        return rerun_alone_no_room(m, one) || finish(nullptr);
    };
    if (!profile_many_ok(m)) return run_jobs_alone(m, 0, n_jobs, one) || finish(nullptr);
    if (plan_profile_many(m)) return 1;
    m.clk.lap(m.ph_plan);
    // a pass of one job runs alone too, as the jobs that do not share; fewer than two jobs in every pass: the whole call job by job
    const std::vector<std::vector<int>> passes = pack_passes(m, m.cap);
    std::vector<int> alone;
    for (int j = 0; j < n_jobs; ++j)
        if (!m.jobs[(size_t) j].shares) alone.push_back(j);
    size_t most = 0;
    for (const std::vector<int> &ps : passes) {
        most = std::max(most, ps.size());
        if (ps.size() == 1) alone.push_back(ps[0]);
    }
    if (most < 2) return run_jobs_alone(m, 0, n_jobs, one) || finish(nullptr);
    // a byte per read and job of a pass (each job's bytes start on a 256-byte line), and the count of walked reads
    m.stride = (search_rs->n_reads + 255) & ~255ull;
    const uint64_t n_bytes = (uint64_t) most * m.stride;
    if (grow_kept(c, c->d_hits, c->hits_cap, n_bytes, n_bytes)) return no_room();
    if (grow_kept(c, c->d_jobcnt, c->jobcnt_cap, 1, 64)) return 1;
    for (int j : alone)
        if (run_jobs_alone(m, j, j + 1, one)) return 1;
    if (upload_visited(m)) return 1;                // (behind the jobs that ran alone: they plan the search set on their own)
    for (const std::vector<int> &ps : passes) {
        if (ps.size() < 2) continue;
        const int rc = run_shared_hits_pass(m, ps);
        c->cur_slot = 0;
        if (rc == 1) {
            (void) hipStreamSynchronize(c->stream);     // (host bit arrays of the call may be on their way up)
            return 1;
        }
        if (rc == 2) return no_room();
    }
    return finish("");
}

}  // namespace

extern "C" {

int commet_index_many_and_profile(commet_ctx *c, int n_jobs, const commet_readset *const *index_rs, const uint8_t *const *index_select,
                                  const commet_readset *search_rs, const uint8_t *search_select, const int *max_hits, uint8_t *const *hits_out,
                                  commet_job_info *info)
{
    return profile_many(c, n_jobs, index_rs, index_select, search_rs, search_select, max_hits, hits_out, false, nullptr, nullptr, info);
}

int commet_index_many_and_thresholds(commet_ctx *c, int n_jobs, const commet_readset *const *index_rs, const uint8_t *const *index_select,
                                     const commet_readset *search_rs, const uint8_t *search_select, const int *t, uint8_t *const *tags_out,
                                     uint64_t *const *shared_out, commet_job_info *info)
{
    return profile_many(c, n_jobs, index_rs, index_select, search_rs, search_select, t, nullptr, true, tags_out, shared_out, info);
}

}  // extern "C"
