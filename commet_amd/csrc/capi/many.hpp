// capi/many.hpp — what commet_index_many_and_search (multi.hpp) and commet_index_many_and_profile (multi_profile.hpp) share: the call's
// record, the argument checks, a job's plan, jobs run alone, the packing of jobs into passes, the build of a pass's filters, the account
// (a part of the one translation unit capi.hip: included there, in order, after job.hpp and before multi.hpp)
//
// Both calls run several jobs that search the SAME read set: each job indexes a set of its own (or a selection of one) into a few
// chunk filters, and the filters of consecutive jobs stand side by side in the slots of one pass over the search set.  What differs
// is the pass itself — tags and statistics there, a byte of hits per read here — and which jobs each call admits to a pass; those
// stay in the two files.  (The step "selection bitmap up, list of the selected reads made" is prepare_job_selection, job_parts.hpp:
// the single job takes it too.)
#pragma once

namespace {

// one many-job call
struct ManyCall {
    commet_ctx *c;
    int n_jobs;
    const commet_readset *const *index_rs;
    const uint8_t *const *index_select;
    const commet_readset *search_rs;
    const uint8_t *search_select;
    struct Job {
        IndexPlan plan;
        const uint8_t *sel = nullptr;
        std::vector<uint64_t> chunk_pos;        // first position of every chunk in the job's list of selected reads
        bool shares = false;                    // planned on the device and admitted to a pass by the caller's rules
    };
    std::vector<Job> jobs;                      // the fast paths' plans
    commet_job_info sum = commet_job_info();
    PhaseClock clk;
    double ph_plan = 0, ph_launch = 0, ph_wait = 0;
    JobTimer tm;                                // one bracket per pass: its builds, then its one scan
    ManyCall(commet_ctx *c_, int n, const commet_readset *const *irs, const uint8_t *const *isel, const commet_readset *srs, const uint8_t *ssel)
        : c(c_), n_jobs(n), index_rs(irs), index_select(isel), search_rs(srs), search_select(ssel), tm(c_, true, 1)
    {
    }
    int n_chunks(int j) const { return (int) jobs[(size_t) j].plan.chunks.size(); }
};

// job j alone through the call's single-job entry point, its account into *ji
using OneJob = std::function<int(int j, commet_job_info *ji)>;

int validate_many(const commet_ctx *c, int n_jobs, const commet_readset *const *index_rs, const commet_readset *search_rs)
{
    if (n_jobs < 0) return fail("n_jobs must be >= 0");
    if (!search_rs->finalized) return fail("search read set not finalized");
    if (search_rs->ctx != c) return fail("search read set belongs to another context");
    for (int j = 0; j < n_jobs; ++j) {
        if (!index_rs[j]->finalized) return fail("index read set %d not finalized", j);
        if (index_rs[j]->ctx != c) return fail("index read set %d belongs to another context", j);
        if (index_rs[j] == search_rs) return fail("a set cannot be searched against itself in one call");
    }
    return 0;
}

// Job j's plan from per-block k-mer sums made on the device, as commet_index_and_search makes it (a selection of every read is no
// selection).  *planned = false, and nothing else done: the device planner does not take the set (an empty read in it, a file
// without a selected read, an empty selection)
int plan_many_job(ManyCall &m, int j, uint64_t max_kmer, bool *planned)
{
    const commet_readset *rs = m.index_rs[j];
    ManyCall::Job &job = m.jobs[(size_t) j];
    job.sel = m.index_select ? m.index_select[j] : nullptr;
    if (job.sel && all_ones(job.sel, rs->n_reads)) job.sel = nullptr;
    *planned = rs->n_reads && plan_blocks_ok(rs->files, job.sel, rs->empty_reads, max_kmer);
    if (!*planned) return 0;
    if (plan_index_on_device(m.c, rs, job.sel, max_kmer, &job.plan)) return 1;
    job.chunk_pos = chunk_positions(job.plan);
    return 0;
}

// jobs j0 .. j1 - 1 alone, one after the other, summed into the call's account
int run_jobs_alone(ManyCall &m, int j0, int j1, const OneJob &one)
{
    for (int j = j0; j < j1; ++j) {
        commet_job_info ji = commet_job_info();
        if (one(j, &ji)) return 1;
        add_info(m.sum, ji);
    }
    return 0;
}

// No room for what a shared pass needs (eight filter slots + their interleaved A planes are 20 GiB at k = 32; the found flags or the
// byte arrays of its jobs): every job alone, as the headers promise — the single-job entry points degrade on their own
// (run_slot_groups).  Nothing a caller depends on has been written by then that the jobs do not write again; the account starts over
int rerun_alone_no_room(ManyCall &m, const OneJob &one)
{
    (void) hipGetLastError();
    m.c->cur_slot = 0;
    m.sum = commet_job_info();
    return run_jobs_alone(m, 0, m.n_jobs, one);
}

// The passes: the sharing jobs in their order while their chunks fit `cap` slots (a job that does not share closes no pass); a job
// is never split
std::vector<std::vector<int>> pack_passes(const ManyCall &m, int cap)
{
    std::vector<std::vector<int>> passes;
    int g = 0;
    for (int j = 0; j < m.n_jobs; ++j) {
        if (!m.jobs[(size_t) j].shares) continue;
        if (passes.empty() || g + m.n_chunks(j) > cap) passes.emplace_back(), g = 0;
        passes.back().push_back(j);
        g += m.n_chunks(j);
    }
    return passes;
}

int pass_chunks(const ManyCall &m, const std::vector<int> &in_pass)
{
    int g = 0;
    for (int j : in_pass) g += m.n_chunks(j);
    return g;
}

// The filters of a pass: the g chunks of the jobs `in_pass` into slots 0 .. g - 1, job after job, then their A planes interleaved
// with stride gs; the pass's index bracket around it.  0 = queued, 1 = error, 2 = no room for the slots.
// Uploads, lists and builds are ordered on the context's one stream, so a set's selection bitmap and the context's list buffer serve
// job after job — two jobs on one set under two selections included.  A chunk that does not take the bucketed build (which writes
// every tile of its slot itself) meets a zeroed slot, as in build_group: a chunk that takes index_kernel, in a pass of long reads
int build_pass_filters(ManyCall &m, const std::vector<int> &in_pass, int g, int gs)
{
    commet_ctx *c = m.c;
    if (ensure_slots(c, g, gs)) return 2;
    if (m.tm.begin_index()) return 1;
    int slot = 0;
    for (int j : in_pass) {
        const commet_readset *rs = m.index_rs[j];
        const ManyCall::Job &job = m.jobs[(size_t) j];
        const uint32_t *d_ids = nullptr;
        if (prepare_job_selection(c, rs, job.plan, c->sel_ids, &d_ids)) return 1;
        for (size_t ci = 0; ci < job.plan.chunks.size(); ++ci, ++slot) {
            const Chunk &ch = job.plan.chunks[ci];
            c->cur_slot = slot;
            const bool self_zeroing = would_partition(c, rs, ch.kmers, ch.last - ch.first + 1);
            if (!self_zeroing && commet_filter_reset(c)) return 1;
            if (launch_index(c, rs, ch.first, ch.last - ch.first + 1, job.plan.dense ? nullptr : rs->d_sel, nullptr, ch.kmers, true, !self_zeroing, 0, d_ids,
                             d_ids ? job.chunk_pos[ci] : 0, ch.n_reads))
                return 1;
            ++m.sum.index_launches;
        }
    }
    c->cur_slot = 0;
    return launch_interleave(c, g, gs) || m.tm.end_index() ? 1 : 0;
}

// the device times of the pass that just ended (the last bracket) into the account; returns the scan's
float account_pass_times(ManyCall &m)
{
    float ms_i = 0, ms_s = 0;
    (void) m.tm.index_ms(m.tm.brackets() - 1, &ms_i);
    (void) m.tm.set_ms(m.tm.brackets() - 1, 0, &ms_s);
    m.sum.index_ms += ms_i, m.sum.index_kernel_ms += ms_i, m.sum.search_ms += ms_s;
    return ms_s;
}

// The call's account to the caller, and one line on stderr under COMMET_JOB_VERBOSE: `line(what)` prints the caller's, whose words
// and numbers are its own (`what`: which path ran; nullptr = job by job, whose calls print their own)
int finish_many(ManyCall &m, commet_job_info *info, const char *what, const std::function<void(const char *)> &line)
{
    m.sum.total_ms = m.clk.total_ms();
    if (what && m.c->job_verbose) line(what);
    if (info) *info = m.sum;
    return 0;
}

}  // namespace
