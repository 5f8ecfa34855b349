// capi/job.hpp — commet_index_reads, commet_search_reads and the chunk loop of the tool on resident sets, commet_index_and_search (index_and_search.cpp:241-277)
// (a part of the one translation unit capi.hip: included there, in order, after the kernels and state.hpp)
#pragma once

extern "C" {

int commet_index_reads(commet_ctx *c, const commet_readset *rs, uint64_t first, uint64_t count,
                       const uint8_t *select_bits, uint64_t *kmers_fed)
{
    if (!rs->finalized) return fail("read set not finalized");
    if (rs->ctx != c) return fail("read set belongs to another context");
    if (first > rs->n_reads || count > rs->n_reads - first) return fail("index range out of bounds");
    SetUse use(c, rs);
    if (use.enter()) return 1;
    HIP_OK(hipSetDevice(c->device));
    const uint64_t *d_sel = nullptr;
    if (select_bits) {
        if (upload_bits(c, rs->d_sel, select_bits, rs->n_reads)) return 1;
        d_sel = rs->d_sel;
    }
    unsigned long long *d_fed = nullptr;
    if (kmers_fed) {
        HIP_OK(hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long), c->stream));
        d_fed = c->d_counters;
    }
    HIP_OK(hipEventRecord(c->ev_i0, c->stream));
    // exact k-mer count of the launch (host copy of the per-read counts): lets the bucketed path run
    if (host_counts(rs)) return 1;
    uint64_t kmers = 0;
    for (uint64_t r = first; r < first + count; ++r)
        if (!select_bits || bit_at(select_bits, r)) kmers += rs->h_kcnt[r];
    if (launch_index(c, rs, first, count, d_sel, d_fed, kmers, false)) return 1;
    HIP_OK(hipEventRecord(c->ev_i1, c->stream));
    c->have_index_ev = true;
    if (kmers_fed) {
        HIP_OK(hipMemcpyAsync(c->h_counters, c->d_counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        *kmers_fed = c->h_counters[0];
    }
    return 0;
}

int commet_search_reads(commet_ctx *c, const commet_readset *rs, const uint8_t *active_bits, uint8_t *found_bits,
                        uint64_t *n_scanned, uint64_t *n_found)
{
    if (!rs->finalized) return fail("read set not finalized");
    if (rs->ctx != c) return fail("read set belongs to another context");
    SetUse use(c, rs);
    if (use.enter()) return 1;
    HIP_OK(hipSetDevice(c->device));
    const uint64_t *d_sel = nullptr;
    if (active_bits) {
        if (upload_bits(c, rs->d_sel, active_bits, rs->n_reads)) return 1;
        d_sel = rs->d_sel;
    }
    HIP_OK(hipMemsetAsync(c->d_counters, 0, 2 * sizeof(unsigned long long), c->stream));
    HIP_OK(hipMemsetAsync(rs->d_found, 0, bitmap_words(rs->n_reads) * 8, c->stream));
    HIP_OK(hipEventRecord(c->ev_s0, c->stream));
    if (launch_search(c, rs, d_sel, nullptr, rs->d_found, c->d_counters)) return 1;
    HIP_OK(hipEventRecord(c->ev_s1, c->stream));
    c->have_search_ev = true;
    HIP_OK(hipMemcpyAsync(c->h_counters, c->d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (found_bits)
        HIP_OK(hipMemcpyAsync(found_bits, rs->d_found, bitmap_bytes_host(rs->n_reads), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (n_scanned) *n_scanned = c->h_counters[0];
    if (n_found) *n_found = c->h_counters[1];
    return 0;
}

}  // extern "C"

/* ---- the chunk loop (index_and_search.cpp:241-277) ------------------------ */

namespace {

// one commet_index_and_search call: what its steps (plan, run, collect) hand on
struct JobRun {
    commet_ctx *c;
    const commet_readset *index_rs;
    int n_search;
    const commet_readset *const *search_rs;
    PhaseClock clk;
    double ph_plan = 0, ph_upload = 0, ph_launch = 0, ph_wait = 0;
    // host plan: chunks of the index set, visited reads of each search set
    IndexPlan plan;
    std::vector<uint64_t> visited;
    std::vector<std::vector<uint8_t>> vis;
    std::vector<char> all_visited;                // every read of the set is visited: the kernels take a null bitmap
    // the index selection as a list (fixed-length sets): chunk j's reads are the next n_reads of it from chunk_pos[j]
    const uint32_t *d_ids = nullptr;
    std::vector<uint64_t> chunk_pos;
    uint64_t ids_expected = ~0ull;
    // per (chunk, set) counters {scanned, found}; last slot: probe counter
    uint64_t n_cnt = 0;
    unsigned long long *d_cnt = nullptr, *d_probes = nullptr;
    int slice_gw = 0;                             // words per bit-sliced entry; 0 = the slot loop
    uint64_t n_index_launches = 0, n_search_launches = 0;
    JobTimer tm;
    JobRun(commet_ctx *c_, const commet_readset *irs, int n, const commet_readset *const *srs)
        : c(c_), index_rs(irs), n_search(n), search_rs(srs), visited((size_t) n, 0), vis((size_t) n), all_visited((size_t) n, 0), tm(c_, false, n)
    {
    }
    uint64_t n_chunks() const { return plan.chunks.size(); }
    uint32_t cstride() const { return (uint32_t) (2 * n_search); }
    unsigned long long *cnt_at(uint64_t ci, int s) const { return d_cnt + 2 * (ci * n_search + s); }
    const uint64_t *index_sel() const { return plan.dense ? nullptr : index_rs->d_sel; }   // a dense plan indexes whole read ranges: no bitmap needed on the device
    const uint64_t *sel_of(int s) const { return all_visited[s] ? nullptr : search_rs[s]->d_sel; }
};

int validate_job(const commet_ctx *c, const commet_readset *index_rs, int n_search, const commet_readset *const *search_rs)
{
    if (!index_rs->finalized) return fail("index read set not finalized");
    if (index_rs->ctx != c) return fail("index read set belongs to another context");
    for (int s = 0; s < n_search; ++s) {
        if (!search_rs[s]->finalized) return fail("search read set %d not finalized", s);
        if (search_rs[s]->ctx != c) return fail("search read set %d belongs to another context", s);
        if (search_rs[s] == index_rs) return fail("a set cannot be searched against itself in one call");
        for (int q = 0; q < s; ++q)
            if (search_rs[q] == search_rs[s]) return fail("search read set listed twice");
    }
    return 0;
}

// the host plan and everything the kernels read of it, on the device when this returns
int plan_job(JobRun &j, const uint8_t *index_select, const uint8_t *const *search_select)
{
    commet_ctx *c = j.c;
    const commet_readset *irs = j.index_rs;
    // an input filter that selects every read is no filter (Commet.py passes all-ones bvs when nothing was filtered)
    if (index_select && all_ones(index_select, irs->n_reads)) index_select = nullptr;
    const uint64_t max_kmer = commet_max_kmer(c);
    if (irs->n_reads && plan_blocks_ok(irs->files, index_select, irs->empty_reads, max_kmer)) {
        if (plan_index_on_device(c, irs, index_select, max_kmer, &j.plan)) return 1;
    } else {
        if (host_counts(irs)) return 1;   // the other planners read the counts on the host
        j.plan = plan_fast_ok(irs->files, index_select, irs->empty_reads, max_kmer) ? plan_index_fast(irs->h_kprefix, irs->n_reads, max_kmer)
                 : (index_select && irs->empty_reads.empty())
                     ? plan_index_select(irs->files, index_select, irs->h_kcnt.data(), irs->n_reads, max_kmer)
                     : plan_index(irs->files, index_select, irs->empty_reads, irs->h_kcnt.data(), irs->n_reads, max_kmer);
    }
    const IndexPlan &plan = j.plan;
    j.clk.lap(j.ph_plan);
    const uint32_t *d_len = nullptr;
    if (prepare_job_selection(c, irs, plan, c->sel_ids, &j.d_ids, &d_len)) return 1;
    if (j.d_ids) {
        // (the list must hold exactly the plan's indexed reads: checked when the job's stream is next synchronised)
        c->h_counters[N_COUNTERS - 1] = ~0ull;
        HIP_OK(hipMemcpyAsync(&c->h_counters[N_COUNTERS - 1], d_len, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        j.ids_expected = plan.indexed_reads;
        j.chunk_pos = chunk_positions(plan);
    }
    j.clk.lap(j.ph_upload);
    for (int s = 0; s < j.n_search; ++s) {
        const commet_readset *rs = j.search_rs[s];
        const uint8_t *ssel = search_select ? search_select[s] : nullptr;
        if (ssel && all_ones(ssel, rs->n_reads)) ssel = nullptr;
        j.all_visited[s] = plan_fast_ok(rs->files, ssel, rs->empty_reads, 1);
        if (j.all_visited[s]) j.visited[s] = rs->n_reads;   // == plan_search_fast, whose bitmap nobody would read
        else
            j.vis[s] = (ssel && rs->empty_reads.empty()) ? plan_search_select(rs->files, ssel, rs->n_reads, &j.visited[s])
                                                         : plan_search(rs->files, ssel, rs->empty_reads, rs->n_reads, &j.visited[s]);
        j.clk.lap(j.ph_plan);
        if (!j.all_visited[s] && upload_bits(c, rs->d_sel, j.vis[s].data(), rs->n_reads)) return 1;
        HIP_OK(hipMemsetAsync(rs->d_tags, 0, bitmap_words(rs->n_reads) * 8, c->stream));
        j.clk.lap(j.ph_upload);
    }
    HIP_OK(hipStreamSynchronize(c->stream));   // the host bit arrays above are pageable
    j.clk.lap(j.ph_upload);
    return 0;
}

// One pass of search set s over the g chunk filters of the group that starts at chunk ci (slots 0 .. g - 1; g > 1: their A planes
// interleaved with stride gs): which regime takes it.  In this order: long reads; the tiled search of two filters; the group kernels;
// else filter by filter, the tiled search of one or the plain kernel.
int search_pass(JobRun &j, int s, uint64_t ci, int g, int gs)
{
    commet_ctx *c = j.c;
    const commet_readset *rs = j.search_rs[s];
    unsigned long long *cnt = j.cnt_at(ci, s);
    // a pass over few of the set's reads (the host plan visits less than half of them): their list, not the set (kernels.hpp,
    // ActiveList); the tiled search probes EVERY record of the set's query list, so such a pass takes the gather kernels
    const uint64_t *sel_s = j.sel_of(s);
    const bool sparse = rs->n_reads && sparse_pass(c, rs, sel_s, j.visited[s]);
    ActiveList al{nullptr, nullptr};
    auto list_for_pass = [&]() {                    // (re-made per pass: the tags of the pass before have shrunk it; no room: the bitmap form)
        al = ActiveList{nullptr, nullptr};
        if (sparse) (void) build_active_list(c, rs, sel_s, rs->d_tags, j.visited[s], &al);
    };
    const bool lng = long_ok(c, rs);                // long reads: a wave per read (long_search.hpp), whatever the group
    // large set, two chunk filters: lane-a gathers served from L2, slice by slice
    const int tiled2 = (g == 2 && !sparse && !lng) ? try_tiled(c, rs, 2, 0, sel_s, rs->d_tags, cnt, j.cstride()) : 1;
    if (tiled2 == 2) return 1;
    if (lng) {
        list_for_pass();
        if (launch_search_long(c, rs, g, g > 1 ? gs : 1, sel_s, rs->d_tags, cnt, j.cstride(), j.d_probes, al, j.visited[s])) return 1;
        ++j.n_search_launches;
    } else if (tiled2 == 0) {
        if (rs->n_reads) ++j.n_search_launches;
    } else if (g > 1 && (gs == 8 || group_searchable(c, rs, g))) {
        list_for_pass();
        if (launch_group_pass(c, rs, g, gs, sel_s, rs->d_tags, cnt, j.cstride(), j.d_probes, al, ci == 0, j.visited[s])) return 1;
        if (rs->n_reads) ++j.n_search_launches;
    } else {
        for (int i = 0; i < g; ++i) {
            c->cur_slot = i;
            unsigned long long *cnt_i = cnt + 2 * (uint64_t) i * j.n_search;
            const int tiled1 = sparse ? 1 : try_tiled(c, rs, 1, i, sel_s, rs->d_tags, cnt_i, j.cstride());   // the same, one filter at a time
            if (tiled1 == 2) return 1;
            if (tiled1 == 1) {
                list_for_pass();
                // a ragged set visited whole, the job's first pass over it (no tags yet): its reads in order of their window counts
                const uint64_t n_listed = ordered_pass(c, rs, sel_s, ci == 0 && i == 0, &al) ? rs->n_reads : j.visited[s];
                if (launch_search(c, rs, sel_s, rs->d_tags, nullptr, cnt_i, j.d_probes, al, n_listed)) return 1;
            }
            if (rs->n_reads) ++j.n_search_launches;
        }
    }
    return 0;
}

// Wide rows or narrow tables?  The wide pass looks at EVERY chunk filter for every read; the narrow tables take 256
// chunks per pass and skip, in later passes, the reads that earlier ones have found — 2.5x the cost per chunk and
// read (configs[4]: 8.3 s against 2.6 s), but when most reads are found early there is little left to pay it on
// (10 M x 100 bp reads, t = 2: k = 20 narrow 628 ms / wide 850 ms, k = 18 664 / 1391, k = 16 649 / 1709 — random
// reads share that many short k-mers — but k = 22 491 / 384, k = 24 307 / 256).  In auto mode the first 64 chunk
// filters are therefore searched with the narrow tables against a sample of every search set (one 64-read word in 128 of a large set); with
// p = the share of them that a group of 256 chunks would find at that rate, the reads still unfound after g groups
// are taken as (1 - p)^g of the set, a narrow pass is priced at 3.7x a wide one per chunk and read (the largest
// ratio measured: reads that are found leave the narrow kernel early, too), and the cheaper plan runs.  The probe's
// reads are searched for real (tags and counters): whichever plan follows skips the found ones and finds nothing
// new in those chunks for the others.  *narrow = the narrow tables are the cheaper plan.
int probe_wide_or_narrow(JobRun &j, bool *narrow)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    const int g0 = (int) std::min<uint64_t>(64, n_chunks);
    if (launch_slice_build(c, j.index_rs, j.index_sel(), 0, g0, 2)) return 1;
    j.n_index_launches += 2;
    uint64_t sampled = 0;
    std::vector<uint64_t> smp;
    for (int s = 0; s < j.n_search; ++s) {
        const commet_readset *rs = j.search_rs[s];
        if (!rs->n_reads) continue;
        const uint64_t nw64 = bitmap_words(rs->n_reads);
        smp.assign(nw64, 0);
        const bool all = j.all_visited[s];                                                       // (else vis[s]: n/8+1 bytes, the last word may be partial)
        const uint64_t stride = rs->n_reads >= (4ull << 20) ? 128 : rs->n_reads >= (1ull << 20) ? 32 : 8;   // >= ~16 k sampled reads
        // (a block of the kernel is 4 words: only the blocks that hold a sampled word are launched)
        for (uint64_t w = 0; w < nw64; w += stride) {
            uint64_t bits = ~0ull;
            if (!all) {
                bits = 0;
                const uint64_t nbytes = bitmap_bytes_host(rs->n_reads), o = w * 8;
                memcpy(&bits, j.vis[s].data() + o, (size_t) std::min<uint64_t>(8, nbytes > o ? nbytes - o : 0));
            }
            if (w * 64 >= rs->n_reads) bits = 0;                                              // (bitmaps have a spare word)
            else if (rs->n_reads - w * 64 < 64) bits &= (1ull << (rs->n_reads - w * 64)) - 1ull;   // reads past the end
            smp[w] = bits;
            sampled += (uint64_t) __builtin_popcountll(bits);
        }
        if (hipMemcpyAsync(rs->d_found, smp.data(), nw64 * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return fail("probe bitmap upload failed");   // (smp is reused)
        if (launch_search_sliced(c, rs, g0, 2, rs->d_found, rs->d_tags, j.d_cnt + 2 * (uint64_t) s, j.cstride(), (uint32_t) (stride / 4))) return 1;
        ++j.n_search_launches;
    }
    std::vector<unsigned long long> pc((size_t) 2 * g0 * j.n_search);
    if (hipMemcpyAsync(pc.data(), j.d_cnt, pc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return fail("probe counter copy failed");
    uint64_t found = 0;
    for (size_t i = 1; i < pc.size(); i += 2) found += pc[i];
    const double p0 = sampled ? std::min(1.0, (double) found / (double) sampled) : 0.0;   // found in g0 chunks
    const double pf = 1.0 - std::pow(1.0 - p0, 256.0 / (double) g0);                       // ... in a group of 256, at that rate
    const uint64_t groups = (n_chunks + 255) / 256;
    double left = 1.0, narrow_cost = 0.0;
    for (uint64_t gi = 0; gi < groups; ++gi) narrow_cost += 3.7 * 256.0 * left, left *= 1.0 - pf;
    *narrow = narrow_cost < (double) n_chunks;   // most reads are found early: the narrow tables, group by group
    return 0;
}

// where each chunk's reads lie in the index set, for slice_build_kernel: c->d_slice_chunks (ensure_slice_buffers has sized it)
int upload_chunk_descriptors(JobRun &j)
{
    const uint64_t n_chunks = j.n_chunks();
    std::vector<SliceChunk> hc(n_chunks);
    for (uint64_t i = 0; i < n_chunks; ++i) {
        const Chunk &ch = j.plan.chunks[i];
        hc[i].first = ch.first;
        hc[i].count = ch.n_reads ? ch.last - ch.first + 1 : 0;
    }
    if (hipMemcpy(j.c->d_slice_chunks, hc.data(), n_chunks * sizeof(SliceChunk), hipMemcpyHostToDevice) != hipSuccess)
        return fail("chunk descriptor upload failed");
    return 0;
}

// The passes of jobs and profiles through the wide rows (c->wide_tables, made for w; the descriptors uploaded): the filters of a
// pass's chunks (all of them when the tables fit) are built 256 at a time into their columns of the rows, then every search set is
// scanned ONCE: launch(s, c0, c1) scans set s against chunks c0 .. c1 - 1 and returns non-zero on failure, as this does at the first
template <typename SetLaunch>
int run_wide_passes(JobRun &j, const WidePlan &w, SetLaunch launch)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += w.chunks_per_pass) {
        const uint64_t c1 = std::min<uint64_t>(n_chunks, c0 + w.chunks_per_pass);
        if (j.tm.begin_index()) return 1;
        for (uint64_t ci = c0; ci < c1; ci += 256) {
            if (launch_slice_build(c, j.index_rs, j.index_sel(), ci, (int) std::min<uint64_t>(256, c1 - ci), (int) WIDE_GROUP_WORDS, c->wide_tables, w.rw,
                                   (uint32_t) ((ci - c0) / 256 * WIDE_GROUP_WORDS)))
                return 1;
            j.n_index_launches += 2;
        }
        if (j.tm.end_index()) return 1;
        for (int s = 0; s < j.n_search; ++s) {
            if (launch(s, c0, c1)) return 1;
            if (j.search_rs[s]->n_reads) ++j.n_search_launches;
            if (j.tm.end_set(s)) return 1;
        }
    }
    return 0;
}

// The passes of jobs and profiles through the narrow tables (c->slice_tables and the staging planes sized for gw; the descriptors
// uploaded): a pass is one group of 32 x gw chunks, its filters built into the one table set, then every search set is scanned ONCE:
// launch(s, c0, c1) scans set s against chunks c0 .. c1 - 1 and returns non-zero on failure, as this does at the first
template <typename SetLaunch>
int run_narrow_passes(JobRun &j, int gw, SetLaunch launch)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    const uint64_t per_pass = 32ull * gw;
    for (uint64_t c0 = 0; c0 < n_chunks; c0 += per_pass) {
        const uint64_t c1 = std::min<uint64_t>(n_chunks, c0 + per_pass);
        if (j.tm.begin_index() || launch_slice_build(c, j.index_rs, j.index_sel(), c0, (int) (c1 - c0), gw)) return 1;
        j.n_index_launches += 2;
        if (j.tm.end_index()) return 1;
        for (int s = 0; s < j.n_search; ++s) {
            if (launch(s, c0, c1)) return 1;
            if (j.search_rs[s]->n_reads) ++j.n_search_launches;
            if (j.tm.end_set(s)) return 1;
        }
    }
    return 0;
}

// the many-small-chunks regime: the chunk filters of a group live bit-sliced in one set of tables (slice_search.hpp)
int run_sliced(JobRun &j)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    WidePlan wide = wide_plan(c, n_chunks, j.slice_gw);
    if (wide.nw && ensure_wide_tables(c, wide)) wide = WidePlan();   // no room for the wide tables: groups of 256 chunks as before
    if (ensure_slice_buffers(c, wide.nw ? 8 : j.slice_gw, n_chunks)) return 1;   // (sized by the caller already; a wide plan that fell back may need less)
    if (upload_chunk_descriptors(j)) return 1;
    if (wide.nw && c->slice_wide == 0) {
        bool narrow = false;
        if (probe_wide_or_narrow(j, &narrow)) return 1;
        if (narrow) wide = WidePlan();
    }
    if (wide.nw)
        return run_wide_passes(j, wide, [&](int s, uint64_t c0, uint64_t c1) {
            const commet_readset *rs = j.search_rs[s];
            return launch_search_wide(c, rs, wide, (int) (c1 - c0), j.sel_of(s), rs->d_tags, j.cnt_at(c0, s), j.cstride());
        });
    return run_narrow_passes(j, j.slice_gw, [&](int s, uint64_t c0, uint64_t c1) {
        const commet_readset *rs = j.search_rs[s];
        return launch_search_sliced(c, rs, (int) (c1 - c0), j.slice_gw, j.sel_of(s), rs->d_tags, j.cnt_at(c0, s), j.cstride());
    });
}

// the filters of chunks ci .. ci + g - 1 into slots 0 .. g - 1, their A planes interleaved with stride gs
int build_group(JobRun &j, uint64_t ci, int g, int gs)
{
    commet_ctx *c = j.c;
    // two lanes: when every chunk of the group takes the bucketed construction (which writes all of its filter
    // slot itself), odd chunks are built on the second stream with the second workspace, beside the even ones
    // (groups of exactly two chunks only — configs[1]: 12.57 against 12.79 ms per step; a 50 M-read set's seven chunks build
    // in 58.7-60.9 ms on one lane and in 58.9-60.7 ms on two, and the second lane's workspace is 14 GiB more to ask the driver for)
    bool lanes = g == 2 && c->index_lanes > 1 && !c->kclock.on;   // per-kernel times are additive on one stream only
    for (int i = 0; i < g && lanes; ++i) {
        const Chunk &ch = j.plan.chunks[ci + i];
        lanes = ch.n_reads && would_partition(c, j.index_rs, ch.kmers, ch.last - ch.first + 1);
    }
    // the second stream starts behind everything issued so far (the previous group's searches read the slots)
    if (lanes && (hipEventRecord(c->ev_fork, c->stream) != hipSuccess || hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0) != hipSuccess))
        return fail("stream fork failed");
    for (int i = 0; i < g; ++i) {
        const Chunk &ch = j.plan.chunks[ci + i];
        c->cur_slot = i;
        // new BloomFilter per chunk: zero it, unless the bucketed build is going to write every tile anyway
        const bool self_zeroing = ch.n_reads && would_partition(c, j.index_rs, ch.kmers, ch.last - ch.first + 1);
        if (j.tm.begin_zero() || (!self_zeroing && commet_filter_reset(c)) || j.tm.end_zero()) return 1;
        if (ch.n_reads) {
            if (launch_index(c, j.index_rs, ch.first, ch.last - ch.first + 1, j.index_sel(), nullptr, ch.kmers, true, !self_zeroing, lanes ? (i & 1) : 0,
                             j.d_ids, j.d_ids ? j.chunk_pos[ci + i] : 0, ch.n_reads))
                return 1;
            ++j.n_index_launches;
        }
    }
    if (lanes && (hipEventRecord(c->ev_join, c->aux_stream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_join, 0) != hipSuccess))
        return fail("stream join failed");
    return g > 1 ? launch_interleave(c, g, gs) : 0;
}

// The slot loop of jobs and profiles: the chunks in groups of g = min(group_cap, chunks left), their filters built into slots
// 0 .. g - 1 with the A planes interleaved at stride gs = 2 / 4 / 8, down the ladder 8 -> 4 -> 1 when the slots do not fit; every
// search set takes ONE pass per group: pass(j, s, ci, g, gs), non-zero on failure, as this returns at the first.  (The current slot
// is put back after every group: search_pass moves it; hits_pass, profile.hpp, sets it itself and does not care)
template <typename Pass>
int run_slot_groups(JobRun &j, int group_cap, Pass pass)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    for (uint64_t ci = 0; ci < n_chunks;) {
        int g = (int) std::min<uint64_t>((uint64_t) group_cap, n_chunks - ci);
        const int gs = g <= 2 ? 2 : g <= 4 ? 4 : 8;
        if (g > 1 && ensure_slots(c, g, gs)) {   // not enough memory for the group
            (void) hipGetLastError();
            if (g > 4) {                          // eight slots do not fit: groups of four
                group_cap = 4;
                continue;
            }
            g = 1;                                // one chunk at a time
            group_cap = 1;
        }
        if (j.tm.begin_index() || build_group(j, ci, g, gs) || j.tm.end_index()) return 1;
        for (int s = 0; s < j.n_search; ++s)
            if (pass(j, s, ci, g, gs) || j.tm.end_set(s)) return 1;
        c->cur_slot = 0;
        ci += (uint64_t) g;
    }
    return 0;
}

// a job's chunks in groups of up to `chunk_group`: every search set is scanned ONCE per group (search_group_kernel) instead of
// once per chunk
int run_slots(JobRun &j)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    int group_cap = (c->k >= 2) ? std::max(1, std::min(8, c->chunk_group)) : 1;
    if (n_chunks < 2) group_cap = 1;
    if (group_cap > 4) {   // more than four filters per pass: every search set must qualify for the register-mask kernel
        bool ok8 = n_chunks > 4;
        for (int s = 0; s < j.n_search && ok8; ++s) ok8 = group8_ok(c, j.search_rs[s]) || long_ok(c, j.search_rs[s]);   // (search_long_kernel keeps no masks)
        if (!ok8) group_cap = 4;
    }
    return run_slot_groups(j, group_cap, search_pass);
}

// the job's counters on the device, then its chunks through the regime that takes them
int run_job(JobRun &j, bool want_times)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    j.n_cnt = 2 * n_chunks * (uint64_t) j.n_search + 1;
    if (grow_kept(c, c->d_jobcnt, c->jobcnt_cap, j.n_cnt, std::max<uint64_t>(j.n_cnt, 64))) return 1;
    j.d_cnt = c->d_jobcnt;
    HIP_OK(hipMemsetAsync(j.d_cnt, 0, j.n_cnt * sizeof(unsigned long long), c->stream));
    j.d_probes = c->count_probes ? j.d_cnt + (j.n_cnt - 1) : nullptr;
    j.slice_gw = slice_words(c, n_chunks);
    // no room for the staging planes / tables of that regime: the job takes the slot loop (slower, same bits)
    if (j.slice_gw && ensure_slice_buffers(c, c->slice_wide == 1 || (c->slice_wide == 0 && n_chunks <= 256) ? j.slice_gw : 8, n_chunks)) {
        (void) hipGetLastError();
        j.slice_gw = 0;
    }
    const uint64_t n_events = j.slice_gw ? (n_chunks / (32 * j.slice_gw) + 1) * (uint64_t) (j.n_search + 2) : n_chunks * (uint64_t) (j.n_search + 4);
    j.tm.timed = want_times && n_events <= 16384;
    const int rc = j.slice_gw ? run_sliced(j) : run_slots(j);
    c->cur_slot = 0;
    return rc;
}

// the end of a job's device work (commet_index_and_search, commet_index_and_profile): the stream drained, the per-kernel times taken,
// the selection list's length against the plan's
int drain_job(JobRun &j, int rc)
{
    commet_ctx *c = j.c;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail("stream synchronize failed: %s", hipGetErrorString(hipGetLastError()));
    c->kclock.collect();
    j.clk.lap(j.ph_wait);
    if (!rc && j.d_ids && (c->h_counters[N_COUNTERS - 1] & 0xFFFFFFFFull) != (j.ids_expected & 0xFFFFFFFFull))
        rc = fail("internal error: the selection list holds %llu reads, the plan indexes %llu", (unsigned long long) (c->h_counters[N_COUNTERS - 1] & 0xFFFFFFFFull),
                  (unsigned long long) j.ids_expected);
    return rc;
}

// the job's account: the plan's numbers, the launches, the device times summed from the timer's brackets (stats[s].search_ms too)
void fill_job_info(JobRun &j, int rc, commet_pair_stats *stats, commet_job_info *info, uint64_t scans, uint64_t probes)
{
    const int n_search = j.n_search;
    double idx_ms = 0, srch_ms = 0, zero_ms = 0;
    if (j.tm.timed && !rc) {
        zero_ms = j.tm.zero_ms();
        float ms = 0;
        for (size_t i = 0; i < j.tm.brackets(); ++i) {
            if (j.tm.index_ms(i, &ms)) idx_ms += ms;
            for (int s = 0; s < n_search; ++s)
                if (j.tm.set_ms(i, s, &ms)) {
                    srch_ms += ms;
                    if (stats) stats[s].search_ms += ms;
                }
        }
    }
    if (info) {
        info->n_chunks = j.n_chunks();
        info->kmers_indexed = j.plan.kmers;
        info->reads_scanned = scans;
        info->reads_indexed = j.plan.indexed_reads;
        info->index_launches = j.n_index_launches;
        info->search_launches = j.n_search_launches;
        info->probes = probes;
        info->zero_ms = zero_ms;
        info->index_ms = idx_ms;
        info->index_kernel_ms = idx_ms - zero_ms;
        info->search_ms = srch_ms;
    }
}

// counters and tags to the host, the device's counts against the plan's, stats and info
int collect(JobRun &j, int rc, uint8_t *const *tags_out, commet_pair_stats *stats, commet_job_info *info)
{
    commet_ctx *c = j.c;
    const int n_search = j.n_search;
    const uint64_t n_chunks = j.n_chunks();
    std::vector<unsigned long long> h_cnt(std::max<uint64_t>(j.n_cnt, 1), 0);
    if (!rc && hipMemcpyAsync(h_cnt.data(), j.d_cnt, j.n_cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        rc = fail("counter copy failed");
    for (int s = 0; s < n_search && !rc; ++s)
        if (tags_out && tags_out[s] &&
            hipMemcpyAsync(tags_out[s], j.search_rs[s]->d_tags, bitmap_bytes_host(j.search_rs[s]->n_reads), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail("tag copy failed");
    rc = drain_job(j, rc);
    if (rc) return rc;
    uint64_t scans = 0;
    for (int s = 0; s < n_search; ++s) {
        uint64_t shared = 0, last_scanned = 0;
        for (uint64_t ci = 0; ci < n_chunks; ++ci) {
            const unsigned long long *p = &h_cnt[2 * (ci * n_search + s)];
            // an empty search set launches nothing: scanned = visited - found so far
            last_scanned = j.visited[s] - shared;
            scans += last_scanned;
            if (j.search_rs[s]->n_reads && !j.slice_gw && p[0] != last_scanned)   // (the sliced kernel counts found reads only)
                rc = fail("internal error: device scanned %llu reads, host plan says %llu (chunk %llu, set %d)",
                          p[0], (unsigned long long) last_scanned, (unsigned long long) ci, s);
            shared += p[1];
        }
        if (stats) {
            stats[s].indexed = j.plan.indexed_reads;
            stats[s].searched = n_chunks ? last_scanned : 0;
            stats[s].shared = shared;
            stats[s].search_ms = 0;
        }
    }
    fill_job_info(j, rc, stats, info, scans, h_cnt[j.n_cnt - 1]);
    return rc;
}

}  // namespace

extern "C" {

int commet_index_and_search(commet_ctx *c, const commet_readset *index_rs, const uint8_t *index_select, int n_search,
                            const commet_readset *const *search_rs, const uint8_t *const *search_select,
                            uint8_t *const *tags_out, commet_pair_stats *stats, commet_job_info *info)
{
    JobRun j(c, index_rs, n_search, search_rs);
    if (validate_job(c, index_rs, n_search, search_rs)) return 1;
    HIP_OK(hipSetDevice(c->device));
    // the sets of this call keep their cached query lists whatever memory pressure another thread meets meanwhile, and stay on the device
    SetUse in_job(c, index_rs);
    for (int s = 0; s < n_search; ++s) in_job.add(search_rs[s]);
    if (in_job.enter()) return 1;
    if (plan_job(j, index_select, search_select)) return 1;
    int rc = run_job(j, info != nullptr || stats != nullptr);
    j.clk.lap(j.ph_launch);
    rc = collect(j, rc, tags_out, stats, info);
    if (c->job_verbose) {
        double ph_tail = 0;
        j.clk.lap(ph_tail);
        fprintf(stderr, "[job] plan %.2f ms, bitmap upload %.2f ms, launches %.2f ms, wait + download %.2f ms, stats + cleanup %.2f ms\n",
                j.ph_plan, j.ph_upload, j.ph_launch, j.ph_wait, ph_tail);
    }
    if (info && !rc) info->total_ms = j.clk.total_ms();
    return rc;
}

}  // extern "C"
