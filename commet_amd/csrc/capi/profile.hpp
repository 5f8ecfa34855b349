// capi/profile.hpp — commet_index_and_profile: per-read hit counts of a job's chunk loop, the tags of every t in 1..max_hits from one call
// (a part of the one translation unit capi.hip: included there, in order, after job.hpp, whose plan, group build, timer and account it uses)
//
// Why one number per read is exact ("Hit profile"): the index does not depend on t (index_reads.h:41-63, and max_kmer
// depends on k alone), so the chunk plan and every chunk filter are the same for every t; within a filter t only decides when
// search_reads stops (search_reads.h:45-83), so a read is found at t iff max(F, R) >= t with F / R the greedy non-overlapping full
// hits of the whole forward / reverse-complement strand; across chunks the tags are ORed, and skipping tagged reads never changes
// which other reads are visited (read_iter.hpp, SetIterator::next).  Hence hits(r) = min(T, max over chunks of max(F, R)).
//
// Up to eight chunk filters per pass: the chunks go through run_slot_groups (job.hpp), the job's own slot loop — the same groups in
// the same slots, down the same ladder 8 -> 4 -> 1 when the slots do not fit — and every search set takes ONE hits pass per group
// (hit_profile_group.hpp: one walk of the read, one plane-A request per window for all g filters and both strands).  cap = option
// "chunk_group" (default 8); 1 when k < 2 or the job has one chunk.  A group of one chunk takes the one-filter kernels
// (hit_profile.hpp); chunk_group = 1 is the one-filter-per-pass form, launch for launch.  No group8_ok condition: these kernels
// keep no masks.
//
// Many small chunks (12 <= k <= 24): option "profile_wide" = 2 takes the wide bit-sliced rows instead (run_profile_wide below;
// hit_profile_wide.hpp): every chunk filter of a pass side by side in one table set, built by run_wide_passes (job.hpp) as a job's
// are, and ONE hits_wide_kernel launch per search set and pass; several passes when the rows are capped ("slice_wide_words")
// or the table budget is small, folded by the byte array's max.  No room for the tables: the slot loop.  0 = auto (profile_wide_ok
// below: more than 256 chunks and short reads, as measured); 1 = never.
//
// Large sets at 25 <= k <= 34: option "profile_tiled" = 2 sends a pass of one or two filters through the tiled probe (try_hits_tiled
// below; hit_profile_tiled.hpp): tq_probe_kernel over the set's query list of (k, t = 1) — every complete window of every read; the
// set's own list when the context's t is 1, else a second list kept with the set (commet_readset::pl) — then tq_hits_replay_kernel,
// which counts where tq_replay_kernel stops.  Sparse passes, wave-per-read sets, groups of three filters and more, and sets with no
// room for the list or the result bytes run what they ran before.  0 = auto: sets of 2^20 reads and more whose list stays within
// query_list_max_mb (profile_tiled_ok below; MEASUREMENTS.md, "Tiled probe"); 1 = never.
//
// Up to 256 chunks a pass at 12 <= k <= 24: option "profile_slice" = 2 takes the narrow bit-sliced tables where the wide rows do not take the call
// (run_profile_sliced below; hit_profile_sliced.hpp): the chunk filters of a pass, 32 x gw of them (gw as a job's: option "slice_words",
// the 1 GiB clamp), in one table set built by run_narrow_passes (job.hpp) as a job's are, and ONE hits_sliced_kernel launch per search
// set and pass.  No room for the tables: the slot loop.  1 = never; 0 = auto, which is never for now (MEASUREMENTS.md, "Hit profile").
// Several such jobs on one search set, their chunk filters in one hits pass: commet_index_many_and_profile (capi/multi_profile.hpp).
// commet_index_and_thresholds is the same job (profile_job below) with another last step: the bytes stay on the device and the tags of
// every t in 1..max_t and the per-file counts come down instead (HitsLeave, thresholds.hpp).
#pragma once

namespace {

// which hits kernel a set takes: option "long_search" as long_mode (search_dispatch.hpp) reads it; auto: sets whose longest read
// has LONG_MIN_MAX_LEN bases (such a read has more than MASK_MAX_WIN windows whatever t).  The context's t plays no part
bool hits_wave_ok(const commet_ctx *c, const commet_readset *rs)
{
    const LongMode m = long_mode(c, rs);
    return m == LongMode::always || (m == LongMode::automatic && rs->max_len >= LONG_MIN_MAX_LEN);
}

// one pass of rs over the g filters in slots 0 .. g - 1: g == 1: the filter in slot 0, the one-filter kernels; g >= 2: the group
// kernels, the A planes interleaved with stride gs.  al.ids != nullptr: over the n_launch (at most) listed reads
int launch_hits(commet_ctx *c, const commet_readset *rs, int g, int gs, int max_hits, const uint64_t *d_sel, uint8_t *d_hits,
                unsigned long long *d_walked, ActiveList al, uint64_t n_launch)
{
    if (rs->n_reads == 0) return 0;
    if (al.ids && n_launch == 0) return 0;
    const uint64_t items = al.ids ? n_launch : rs->n_reads;
    const bool wave = hits_wave_ok(c, rs);          // a wave per read on a persistent grid, else a lane per read
    if (!wave && launch_size_ok(items)) return 1;
    const dim3 lanes((unsigned) ((items + 255) / 256));
    KScope ks(c, g > 1 ? (wave ? "hits_group_wave_kernel" : "hits_group_kernel") : (wave ? "hits_wave_kernel" : "hits_kernel"), c->stream);
    with_key(c->k, [&](auto key) {
        using W = decltype(key);
        if (g == 1) {
            if (wave)
                COMMET_LAUNCH(hits_wave_kernel<W>, dim3((unsigned) resident_blocks<hits_wave_kernel<W>>(c, items)), dim3(LONG_WG), 0, c->stream, rs->view(),
                              c->view(), c->k, max_hits, d_sel, d_hits, d_walked, al);
            else
                COMMET_LAUNCH(hits_kernel<W>, lanes, dim3(256), 0, c->stream, rs->view(), c->view(), c->k, max_hits, d_sel, d_hits, d_walked, al);
            return;
        }
        const FilterGroupView fg = filter_group(c, g, 0, true);
        with_value<2, 4, 8>(gs, [&](auto NF) {
            if (wave)
                COMMET_LAUNCH((hits_group_wave_kernel<W, NF>), dim3((unsigned) resident_blocks<hits_group_wave_kernel<W, NF>>(c, items)), dim3(LONG_WG), 0,
                              c->stream, rs->view(), fg, c->k, max_hits, d_sel, d_hits, d_walked, al);
            else
                COMMET_LAUNCH((hits_group_kernel<W, NF>), lanes, dim3(256), 0, c->stream, rs->view(), fg, c->k, max_hits, d_sel, d_hits, d_walked, al);
        });
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- the tiled profile (hit_profile_tiled.hpp) ------------------------------------------------------------------------------------
// windows of the set's longest read (< 1: the set has no k-mer)
inline int64_t profile_windows(const commet_ctx *c, const commet_readset *rs) { return (int64_t) rs->max_len - c->k + 1; }

// an upper bound on the records of the set's (k, 1) list — exactly its complete k-mers: every window of every read, and no more
// windows than bases
inline uint64_t profile_records_bound(const commet_ctx *c, const commet_readset *rs)
{
    const int64_t w = profile_windows(c, rs);
    if (w < 1 || !rs->n_reads) return 0;
    const uint64_t by_reads = rs->n_reads * (uint64_t) w;
    return rs->uniform_len ? by_reads : std::min<uint64_t>(by_reads, rs->n_bases);
}

// what tq_hits_replay_kernel and the (k, 1) list can take
bool profile_geometry_ok(const commet_ctx *c, const commet_readset *rs)
{
    return tq_geometry_ok(c, rs, profile_windows(c, rs), profile_records_bound(c, rs));
}

// the list a profile scans: every complete window, t = 1 — the search's own list when that is built for t = 1
inline commet_readset::QueryList &profile_list(const commet_ctx *c, const commet_readset *rs) { return t_eff(c, rs) == 1 ? rs->ql : rs->pl; }

// does a pass of g filters over rs take the tiled profile?  Option "profile_tiled": 1 never; 2 whenever the geometry allows; 0 auto: by
// tiled_ok's auto bounds (search_dispatch.hpp) — sets of 2^20 reads and more whose (k, 1) list, estimated at 8 bytes per record,
// stays within query_list_max_mb.  Measured at 2 x 5 M x 100 bp, k = 32, one filter (MEASUREMENTS.md, "Tiled probe"): 10.8 against
// 14.2 ms per call with the list cached, rounds within 1.5 %; the call that builds the list takes 2.6 ms longer, so the second call
// has repaid it.  configs[1]'s sets (10 M reads: 5.5 GB estimated) lie above the default cap and keep the slot loop in auto, though
// forced they gain as much (23.9 against 30.6 ms): raise query_list_max_mb for them.
bool profile_tiled_ok(const commet_ctx *c, const commet_readset *rs, int g, bool sparse)
{
    if (c->profile_tiled == 1 || c->count_probes || sparse) return false;
    if (g < 1 || g > 2 || hits_wave_ok(c, rs) || !profile_geometry_ok(c, rs)) return false;
    if (profile_list(c, rs).failed) return false;
    if (c->profile_tiled == 2) return true;              // (forced: sets below auto's 2^20 reads too)
    return rs->n_reads >= (1ull << 20) && profile_records_bound(c, rs) * 8 <= c->ql_max_list;
}

// probe and counting replay of rs over the g <= 2 filters in slots 0 .. g - 1 (g == 2: interleaved A planes), its list and result bytes in place
int launch_hits_tiled(commet_ctx *c, const commet_readset *rs, const commet_readset::QueryList &q, int g, int max_hits, const uint64_t *d_sel,
                      uint8_t *d_hits, unsigned long long *d_walked)
{
    if (rs->n_reads == 0) return 0;
    if (c->qres_cap < q.n_records) return fail("internal error: tiled profile without its result buffer");
    const QueryListView v = query_list_view(q);
    const FilterGroupView fg = filter_group(c, g, 0, g > 1);
    if (launch_tq_probe(c, v, fg, g)) return 1;
    // (mask words: by every window of the set's longest read, not its first-hit windows)
    return launch_tq_replay(c, "tq_hits_replay_kernel", g, mask_words_of(profile_windows(c, rs)), [&](auto key, auto GS, auto MW, uint32_t hit_cap) {
        COMMET_LAUNCH((tq_hits_replay_kernel<decltype(key), GS, MW>), dim3(q.n_pieces), dim3(TQ_PIECE), 0, c->stream, rs->view(), v, c->d_qres, fg,
                      c->k, max_hits, d_sel, d_hits, d_walked, hit_cap);
    });
}

// 0 = launched, 1 = not for this set / group (or no room: the caller's kernels), 2 = error.  List, result bytes and launches under
// ql_mu, as try_tiled (job_parts.hpp): no other thread gives the list back in between
int try_hits_tiled(commet_ctx *c, const commet_readset *rs, int g, bool sparse, int max_hits, const uint64_t *d_sel, uint8_t *d_hits,
                   unsigned long long *d_walked)
{
    std::lock_guard<std::mutex> qlk(c->ql_mu);
    if (!profile_tiled_ok(c, rs, g, sparse)) return 1;
    commet_readset::QueryList &l = profile_list(c, rs);
    if (build_query_list(c, rs, 1, l) != 0 || ensure_query_results(c, l) != 0) return 1;
    return launch_hits_tiled(c, rs, l, g, max_hits, d_sel, d_hits, d_walked) ? 2 : 0;
}

// the list of a pass of search set s that walks few of the set's reads (sparse_pass; no tags: a read that needs no walk is skipped by
// the kernel itself), for hits_pass below and rel_pass (relative.hpp).  Empty: the pass is not sparse, or no room (the bitmap form)
ActiveList hits_pass_list(JobRun &j, int s, bool sparse)
{
    ActiveList al{nullptr, nullptr};
    if (sparse && build_active_list(j.c, j.search_rs[s], j.sel_of(s), nullptr, j.visited[s], &al)) al = ActiveList{nullptr, nullptr};
    return al;
}

// search set s against the g chunk filters in slots 0 .. g - 1: the tiled profile where it applies; else the gather kernels, a pass
// over few of the set's reads walking their list
int hits_pass(JobRun &j, int s, int g, int gs, int max_hits, uint8_t *d_hits, unsigned long long *d_walked)
{
    commet_ctx *c = j.c;
    const commet_readset *rs = j.search_rs[s];
    const uint64_t *sel_s = j.sel_of(s);
    const bool sparse = rs->n_reads && sparse_pass(c, rs, sel_s, j.visited[s]);
    c->cur_slot = 0;
    const int tiled = try_hits_tiled(c, rs, g, sparse, max_hits, sel_s, d_hits, d_walked);
    if (tiled == 2) return 1;
    if (tiled == 0) {
        if (rs->n_reads) ++j.n_search_launches;
        return 0;
    }
    const ActiveList al = hits_pass_list(j, s, sparse);
    if (launch_hits(c, rs, g, gs, max_hits, sel_s, d_hits, d_walked, al, j.visited[s])) return 1;
    if (rs->n_reads) ++j.n_search_launches;
    return 0;
}

// does the call take the wide rows?  Option "profile_wide": 1 never, 2 whenever k allows it and the job has a chunk, 0 auto: jobs of
// more than 256 chunks (the wide search's own threshold) whose search sets hold short reads only — measured 5.6x (313 chunks) and 7.2x
// (1 043 chunks) faster than the slot loop on 150-base reads (MEASUREMENTS.md, "Hit profile").  The block counters bound a strand at two
// hits, so a read of many windows has a chance hit in three blocks of most chunk filters and every such chunk is replayed: sets with a
// read of more than PROFILE_WIDE_MAX_LEN bases (twice the measured length) keep the slot loop until somebody measures them
constexpr uint32_t PROFILE_WIDE_MAX_LEN = 300;
bool profile_wide_ok(const commet_ctx *c, uint64_t n_chunks, int n_search, const commet_readset *const *search_rs)
{
    if (c->profile_wide == 1 || c->k < SLICE_MIN_K || c->k > SLICE_MAX_K || n_chunks == 0) return false;
    if (c->profile_wide == 2) return true;
    if (n_chunks <= 256) return false;
    for (int s = 0; s < n_search; ++s)
        if (search_rs[s]->max_len > PROFILE_WIDE_MAX_LEN) return false;
    return true;
}

// one pass of rs over the g chunk filters in the wide rows
int launch_hits_wide(commet_ctx *c, const commet_readset *rs, const WidePlan &w, int g, int max_hits, const uint64_t *d_sel, uint8_t *d_hits,
                     unsigned long long *d_walked)
{
    return launch_wide(rs->n_reads, w, [&](dim3 grid, auto LPR, auto NP) {
        KScope ks(c, "hits_wide_kernel", c->stream);
        COMMET_LAUNCH((hits_wide_kernel<LPR, NP>), grid, dim3(256), 0, c->stream, rs->view(), c->wide_tables, c->k, max_hits, g, w.nw, w.rw, d_sel,
                      d_hits, d_walked);
    });
}

// the profile through the wide rows: the passes of run_wide_passes (job.hpp), every search set scanned once per pass by
// hits_wide_kernel.  at[s] = where set s's bytes start in c->d_hits.  *taken = false: no room for the tables, nothing was launched
// and the caller takes the slot loop
int run_profile_wide(JobRun &j, int max_hits, const std::vector<uint64_t> &at, unsigned long long *d_walked, bool want_times, bool *taken)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    *taken = false;
    const WidePlan wide = wide_rows(c, n_chunks);
    if (!wide.nw || ensure_wide_tables(c, wide) || ensure_slice_buffers(c, (int) WIDE_GROUP_WORDS, n_chunks)) {
        (void) hipGetLastError();
        return 0;
    }
    *taken = true;
    if (upload_chunk_descriptors(j)) return 1;
    const uint64_t per_pass = wide.chunks_per_pass;
    j.tm.timed = want_times && ((n_chunks + per_pass - 1) / per_pass) * (uint64_t) (j.n_search + 2) <= 16384;
    return run_wide_passes(j, wide, [&](int s, uint64_t c0, uint64_t c1) {
        return launch_hits_wide(c, j.search_rs[s], wide, (int) (c1 - c0), max_hits, j.sel_of(s), c->d_hits + at[(size_t) s], d_walked);
    });
}

// does the call take the narrow tables (when the wide rows do not)?  Option "profile_slice": 2 whenever k allows it, the job has a chunk
// and no probes are counted; 1 never; 0 auto: never, until the measurements say where (MEASUREMENTS.md, "Hit profile")
bool profile_slice_ok(const commet_ctx *c, uint64_t n_chunks)
{
    return c->profile_slice == 2 && !c->count_probes && c->k >= SLICE_MIN_K && c->k <= SLICE_MAX_K && n_chunks > 0;
}

// the profile through the narrow tables: the passes of run_narrow_passes (job.hpp), 32 x gw chunks each, every search set scanned once
// per pass by hits_sliced_kernel; gw as a job's (slice_entry_words: option "slice_words", the 1 GiB clamp).  at[s] = where set s's
// bytes start in c->d_hits.  *taken = false: no room for the tables, nothing was launched and the caller takes the slot loop
int run_profile_sliced(JobRun &j, int max_hits, const std::vector<uint64_t> &at, unsigned long long *d_walked, bool want_times, bool *taken)
{
    commet_ctx *c = j.c;
    const uint64_t n_chunks = j.n_chunks();
    *taken = false;
    const int gw = slice_entry_words(c, n_chunks);
    if (ensure_slice_buffers(c, gw, n_chunks)) {
        (void) hipGetLastError();
        return 0;
    }
    *taken = true;
    if (upload_chunk_descriptors(j)) return 1;
    const uint64_t per_pass = 32ull * gw;
    j.tm.timed = want_times && ((n_chunks + per_pass - 1) / per_pass) * (uint64_t) (j.n_search + 2) <= 16384;
    return run_narrow_passes(j, gw, [&](int s, uint64_t c0, uint64_t c1) {
        return launch_hits_sliced(c, j.search_rs[s], (int) (c1 - c0), gw, max_hits, j.sel_of(s), c->d_hits + at[(size_t) s], d_walked);
    });
}

// What a single profile job leaves of the bytes of its search sets (HitsLeave, thresholds.hpp): the bytes themselves, hits_out[s]
// (commet_index_and_profile), or, n_t > 0, the tags of the thresholds t_first .. t_first + n_t - 1 and the per-file counts, set s's
// at tags_out[s * n_t + ti] and shared_out[s * n_t + ti] (the thresholds calls)
struct ProfileWant {
    uint8_t *const *hits_out = nullptr;
    int t_first = 0, n_t = 0;
    uint8_t *const *tags_out = nullptr;
    uint64_t *const *shared_out = nullptr;
};

// The frame of a job that keeps a byte per read of its search sets in c->d_hits — the profile job below, and the relative search
// (relative.hpp), whose bytes are found flags: open() checks, plans and zeroes; the caller runs its passes over the slot groups;
// close() queues what the call leaves, drains and accounts.  Each set's bytes start on a 256-byte line, at[s]
struct BytesJob {
    commet_ctx *c;
    JobRun j;
    SetUse in_job;                                 // offload / export cannot take a set mid-call
    std::vector<uint64_t> at;
    uint64_t n_bytes = 0;
    unsigned long long *d_walked = nullptr;        // the count of walked reads
    BytesJob(commet_ctx *c_, const commet_readset *index_rs, int n_search, const commet_readset *const *search_rs)
        : c(c_), j(c_, index_rs, n_search, search_rs), in_job(c_, index_rs), at((size_t) n_search + 1, 0)
    {
    }
    uint8_t *bytes_of(int s) const { return c->d_hits + at[(size_t) s]; }
    // the slot loop's group cap, a rule of its own (no group8_ok condition: the hits kernels keep no masks)
    int group_cap() const { return (c->k >= 2 && j.n_chunks() >= 2) ? std::max(1, std::min(8, c->chunk_group)) : 1; }

    int open(const uint8_t *index_select, const uint8_t *const *search_select, bool want_times)
    {
        const int n_search = j.n_search;
        if (validate_job(c, j.index_rs, n_search, j.search_rs)) return 1;
        HIP_OK(hipSetDevice(c->device));
        for (int s = 0; s < n_search; ++s) in_job.add(j.search_rs[s]);
        if (in_job.enter()) return 1;
        if (plan_job(j, index_select, search_select)) return 1;
        for (int s = 0; s < n_search; ++s) at[(size_t) s + 1] = at[(size_t) s] + ((j.search_rs[s]->n_reads + 255) & ~255ull);
        n_bytes = std::max<uint64_t>(at[(size_t) n_search], 256);
        if (grow_kept(c, c->d_hits, c->hits_cap, n_bytes, n_bytes) || grow_kept(c, c->d_jobcnt, c->jobcnt_cap, 1, 64)) return 1;
        d_walked = c->d_jobcnt;
        HIP_OK(hipMemsetAsync(c->d_hits, 0, n_bytes, c->stream));
        HIP_OK(hipMemsetAsync(d_walked, 0, sizeof(unsigned long long), c->stream));
        j.tm.timed = want_times && j.n_chunks() * (uint64_t) (n_search + 4) <= 16384;
        return 0;
    }

    int close(int rc, HitsLeave &leave, commet_job_info *info)
    {
        c->cur_slot = 0;
        j.clk.lap(j.ph_launch);
        if (!rc && hipMemcpyAsync(&c->h_counters[0], d_walked, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail("counter copy failed");
        if (!rc) rc = leave.queue(c);
        rc = drain_job(j, rc);
        if (rc) return rc;
        leave.finish();
        fill_job_info(j, rc, nullptr, info, c->h_counters[0], 0);
        if (info) info->total_ms = j.clk.total_ms();
        return 0;
    }
};

// the profile job behind commet_index_and_profile and commet_index_and_thresholds: everything up to the download is the same
int profile_job(commet_ctx *c, const commet_readset *index_rs, const uint8_t *index_select, int n_search, const commet_readset *const *search_rs,
                const uint8_t *const *search_select, int max_hits, const ProfileWant &want, commet_job_info *info)
{
    if (n_search < 0) return fail("n_search must not be negative (got %d)", n_search);
    if (max_hits < 1 || max_hits > 255) return fail("max_hits must be in 1..255 (got %d)", max_hits);
    BytesJob b(c, index_rs, n_search, search_rs);
    if (b.open(index_select, search_select, info != nullptr)) return 1;
    JobRun &j = b.j;
    const std::vector<uint64_t> &at = b.at;
    unsigned long long *d_walked = b.d_walked;
    const uint64_t n_chunks = j.n_chunks();
    int rc = 0;
    bool wide = false;                             // the call went through bit-sliced tables, wide or narrow
    if (profile_wide_ok(c, n_chunks, n_search, search_rs)) rc = run_profile_wide(j, max_hits, at, d_walked, info != nullptr, &wide);
    else if (profile_slice_ok(c, n_chunks)) rc = run_profile_sliced(j, max_hits, at, d_walked, info != nullptr, &wide);
    if (!rc && !wide)
        rc = run_slot_groups(j, b.group_cap(), [&](JobRun &jr, int s, uint64_t, int g, int gs) {
            return hits_pass(jr, s, g, gs, max_hits, b.bytes_of(s), d_walked);
        });
    HitsLeave leave;
    for (int s = 0; s < n_search; ++s) {
        const uint8_t *d = c->d_hits + at[(size_t) s];
        if (want.n_t)
            leave.tags_of(d, search_rs[s], want.t_first, want.n_t, want.tags_out ? want.tags_out + (size_t) s * want.n_t : nullptr,
                          want.shared_out ? want.shared_out + (size_t) s * want.n_t : nullptr);
        else if (want.hits_out && want.hits_out[s]) leave.bytes_of(d, search_rs[s]->n_reads, want.hits_out[s]);
    }
    return b.close(rc, leave, info);
}

}  // namespace

extern "C" {

int commet_index_and_profile(commet_ctx *c, const commet_readset *index_rs, const uint8_t *index_select, int n_search,
                             const commet_readset *const *search_rs, const uint8_t *const *search_select, int max_hits, uint8_t *const *hits_out,
                             commet_job_info *info)
{
    ProfileWant want;
    want.hits_out = hits_out;
    return profile_job(c, index_rs, index_select, n_search, search_rs, search_select, max_hits, want, info);
}

int commet_index_and_thresholds(commet_ctx *c, const commet_readset *index_rs, const uint8_t *index_select, int n_search,
                                const commet_readset *const *search_rs, const uint8_t *const *search_select, int max_t, uint8_t *const *tags_out,
                                uint64_t *const *shared_out, commet_job_info *info)
{
    if (max_t < 1 || max_t > 255) return fail("max_t must be in 1..255 (got %d)", max_t);
    ProfileWant want;
    want.t_first = 1, want.n_t = max_t, want.tags_out = tags_out, want.shared_out = shared_out;
    return profile_job(c, index_rs, index_select, n_search, search_rs, search_select, max_t, want, info);
}

}  // extern "C"
