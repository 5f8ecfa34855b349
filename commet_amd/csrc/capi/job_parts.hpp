// capi/job_parts.hpp — what commet_index_and_search and commet_index_many_and_search share: the phase clock, the timing recorder, the
// device planner, job accounting, and the steps of a search pass that both take
// (a part of the one translation unit capi.hip: included there, in order, after search_dispatch.hpp and before job.hpp)
#pragma once

namespace {

// host-side phase times of a call (COMMET_JOB_VERBOSE: one line per call on stderr)
struct PhaseClock {
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::chrono::steady_clock::time_point last = t0;
    void lap(double &acc)                          // the time since the last lap goes to acc
    {
        const auto now = std::chrono::steady_clock::now();
        acc += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
    double total_ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Device times of a job.  One event pair around all index work and one around all search work would overlap; instead the job is
// cut into brackets on the (in-order) job stream — the index work of a group of chunks, then one event behind each search set's
// pass over it — and the phases are summed from those.  Owns every event it makes; on every way out they are destroyed and the
// context's slot cursor is back at 0.
struct JobTimer {
    commet_ctx *c;
    bool timed;
    std::vector<hipEvent_t> evs, idx0, idx1, zero0, zero1;
    std::vector<std::vector<hipEvent_t>> set;      // end of set s's pass, per bracket
    JobTimer(commet_ctx *c_, bool timed_, int n_sets) : c(c_), timed(timed_), set((size_t) n_sets) {}
    JobTimer(const JobTimer &) = delete;
    JobTimer &operator=(const JobTimer &) = delete;
    ~JobTimer()
    {
        c->cur_slot = 0;
        for (hipEvent_t e : evs) (void) hipEventDestroy(e);
    }
    int mark(std::vector<hipEvent_t> &into)         // a new event, recorded on the job stream now
    {
        if (!timed) return 0;
        hipEvent_t e = nullptr;
        HIP_OK(hipEventCreate(&e));
        evs.push_back(e);
        (void) hipEventRecord(e, c->stream);
        into.push_back(e);
        return 0;
    }
    int begin_index() { return mark(idx0); }
    int end_index() { return mark(idx1); }
    int end_set(int s) { return mark(set[(size_t) s]); }
    int begin_zero() { return mark(zero0); }
    int end_zero() { return mark(zero1); }
    // after the stream has been synchronised
    size_t brackets() const { return idx1.size(); }
    static bool between(hipEvent_t a, hipEvent_t b, float *ms) { return hipEventElapsedTime(ms, a, b) == hipSuccess; }
    bool index_ms(size_t i, float *ms) const { return between(idx0[i], idx1[i], ms); }
    // set s is measured from set s - 1's event, the first set from the index end
    bool set_ms(size_t i, int s, float *ms) const
    {
        if (i >= set[(size_t) s].size()) return false;
        return between(s == 0 ? idx1[i] : set[(size_t) s - 1][i], set[(size_t) s][i], ms);
    }
    double zero_ms() const
    {
        double sum = 0;
        float ms = 0;
        for (size_t i = 0; i < zero1.size(); ++i)
            if (between(zero0[i], zero1[i], &ms)) sum += ms;
        return sum;
    }
};

// The index plan from per-block k-mer sums computed on the device, where kcnt lives; the host walks only the blocks in which a chunk
// starts or ends and fetches just those blocks' counts: no per-read loop over the set and no host copy of its counts (a selection
// bitmap, when there is one, is uploaded first for the kernel to use).  For sets that plan_blocks_ok admits.
int plan_index_on_device(commet_ctx *c, const commet_readset *rs, const uint8_t *sel, uint64_t max_kmer, IndexPlan *out)
{
    const uint64_t nblk = (rs->n_reads + PLAN_BLOCK_READS - 1) / PLAN_BLOCK_READS;
    if (grow_kept(c, c->d_plansum, c->plansum_cap, nblk, nblk)) return 1;
    if (sel && upload_bits(c, rs->d_sel, sel, rs->n_reads)) return 1;
    {
        KScope ks(c, "block_kmer_sums_kernel", c->stream);
        COMMET_LAUNCH(block_kmer_sums_kernel, dim3((unsigned) nblk), dim3(256), 0, c->stream, rs->d_kcnt, sel ? rs->d_sel : nullptr, rs->n_reads,
                      c->d_plansum);
    }
    HIP_OK(hipGetLastError());
    std::vector<uint64_t> blk_sums(nblk);
    HIP_OK(hipMemcpyAsync(blk_sums.data(), c->d_plansum, nblk * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    // counts of one block of reads, fetched on demand (or taken from the host copy when somebody made one)
    std::vector<uint32_t> kblock(PLAN_BLOCK_READS);
    uint64_t kblock_no = ~0ull;
    bool kfetch_failed = false;
    auto kcnt_of = [&](uint64_t q) -> uint32_t {
        if (rs->have_host_counts) return rs->h_kcnt[q];
        const uint64_t blk = q / PLAN_BLOCK_READS;
        if (blk != kblock_no) {
            const uint64_t lo = blk * PLAN_BLOCK_READS, cnt = std::min<uint64_t>(PLAN_BLOCK_READS, rs->n_reads - lo);
            if (hipMemcpy(kblock.data(), rs->d_kcnt + lo, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) kfetch_failed = true;
            kblock_no = blk;
        }
        return kblock[q % PLAN_BLOCK_READS];
    };
    *out = plan_index_blocks(sel, kcnt_of, rs->n_reads, max_kmer, blk_sums.data(), PLAN_BLOCK_READS);
    if (kfetch_failed) return fail("k-mer count fetch failed: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

// The reads a plan indexes as a list, for the bucketed build of a set of one read length to walk arithmetically (index_part.hpp,
// sel_ids_kernel; the plan's bitmap is in rs->d_sel by now).  0 = built, 1 = no room
int build_selection_list(commet_ctx *c, commet_ctx::IdList &l, const commet_readset *rs, const IndexPlan &plan, const uint32_t **d_ids, const uint32_t **d_len = nullptr)
{
    ActiveList al{nullptr, nullptr};
    if (build_id_list(c, l, "sel_ids_kernels", rs, rs->d_sel, nullptr, plan.indexed_reads, std::max<uint64_t>(plan.indexed_reads, rs->n_reads / 2), &al)) return 1;
    *d_ids = al.ids;
    if (d_len) *d_len = al.n;
    return 0;
}

// What the builds of a planned job read of its selection, queued on the context's stream: the plan's bitmap into rs->d_sel and, for a
// set of one read length (Commet.py's J2 / J3 jobs), the selected reads' numbers as a list in `buf`, which the bucketed build walks
// arithmetically.  A dense plan indexes whole read ranges and needs neither.  The list is an optimisation: without room for it
// *d_ids = nullptr and the build walks the bitmap, so only a failed upload is an error (1).  Every job entry point takes this step
int prepare_job_selection(commet_ctx *c, const commet_readset *rs, const IndexPlan &plan, commet_ctx::IdList &buf, const uint32_t **d_ids,
                          const uint32_t **d_len = nullptr)
{
    *d_ids = nullptr;
    if (plan.dense) return 0;
    if (upload_bits(c, rs->d_sel, plan.indexed_bits.data(), rs->n_reads)) return 1;
    if (rs->uniform_len == 0 || c->part_no_uni || !plan.indexed_reads || c->index_mode == 1) return 0;
    if (build_selection_list(c, buf, rs, plan, d_ids, d_len)) {
        (void) hipGetLastError();
        *d_ids = nullptr;
    }
    return 0;
}

// first position of every chunk of a plan in the list of its indexed reads
std::vector<uint64_t> chunk_positions(const IndexPlan &plan)
{
    std::vector<uint64_t> pos;
    uint64_t at = 0;
    for (const Chunk &ch : plan.chunks) pos.push_back(at), at += ch.n_reads;
    return pos;
}

// what one job did, added to the account of a call that ran several (total_ms is the call's own)
void add_info(commet_job_info &sum, const commet_job_info &ji)
{
    sum.n_chunks += ji.n_chunks, sum.kmers_indexed += ji.kmers_indexed, sum.reads_scanned += ji.reads_scanned;
    sum.reads_indexed += ji.reads_indexed, sum.index_launches += ji.index_launches, sum.search_launches += ji.search_launches;
    sum.probes += ji.probes, sum.zero_ms += ji.zero_ms, sum.index_ms += ji.index_ms, sum.index_kernel_ms += ji.index_kernel_ms;
    sum.search_ms += ji.search_ms;
}

// ---- steps of a search pass --------------------------------------------------------------------------------------------------
// The tiled search (tile_search.hpp) of one pass of rs over g <= 2 filters from slot0 on: 0 = launched, 1 = not for this set / group,
// 2 = error.  The set's query list is made or found, and its kernels queued, under ql_mu: no other thread gives the list back in between
int try_tiled(commet_ctx *c, const commet_readset *rs, int g, int slot0, const uint64_t *d_sel, uint64_t *d_tags, unsigned long long *d_counters,
              uint32_t cstride, uint64_t job_tag_words = 0)
{
    std::lock_guard<std::mutex> qlk(c->ql_mu);
    if (!tiled_ok(c, rs, g) || build_query_list(c, rs, t_eff(c, rs), rs->ql) != 0 || ensure_query_results(c, rs->ql) != 0) return 1;
    return launch_search_tiled(c, rs, g, slot0, d_sel, d_tags, d_counters, cstride, job_tag_words) ? 2 : 0;
}

// One pass of the group kernels over g filters (stride gs).  A ragged set visited whole by the job's first pass (no tags yet) and
// with no list of its own goes in order of its reads' window counts (ordered_pass); otherwise `al`, the pass's sparse list of at
// most `visited` reads, or the bitmap form
int launch_group_pass(commet_ctx *c, const commet_readset *rs, int g, int gs, const uint64_t *d_sel, uint64_t *d_tags, unsigned long long *d_counters,
                      uint32_t cstride, unsigned long long *d_probes, ActiveList al, bool first_pass, uint64_t visited, uint32_t job_mask = 0,
                      uint64_t job_tag_words = 0)
{
    const uint64_t n_listed = ordered_pass(c, rs, d_sel, first_pass, &al) ? rs->n_reads : visited;
    return launch_search_group(c, rs, g, gs, d_sel, d_tags, d_counters, cstride, d_probes, al, n_listed, job_mask, job_tag_words);
}

}  // namespace
