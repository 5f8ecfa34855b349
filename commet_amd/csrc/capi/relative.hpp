// capi/relative.hpp — commet_index_and_search_relative and commet_readset_relative_thresholds: the search with a threshold per read,
// a share of the non-overlapping k-mers the read can hold
// (a part of the one translation unit capi.hip: included there, in order, after profile.hpp, whose frame, pass list and wave rule it uses)
//
// The rule is stated once, in include/commet_hip.h, and implemented once, by rel_threshold (relative_search.hpp).  The job is the
// profile job's frame (BytesJob, profile.hpp): the same checks, plan, slot groups under the same group cap, drain and account; its
// bytes are found flags, and beside them, in the same layout, stands one threshold per read (c->d_thr), filled once per call before
// the first pass: 0 for a read no pass walks (t_r > W_r, or not selected).  Per group of chunk filters every search set takes ONE
// pass (rel_pass below) under hits_pass's sparse-list rule; the last step is the thresholds calls' (HitsLeave::tags_of at t = 1:
// tags and per-file counts made on the device, only bits come down).
//
// Which kernel: the wave forms where hits_wave_ok says so; the lane-per-read group body counts in bytes, so a set whose largest t_r
// exceeds 255 takes the wave forms too, unless the set may not ("long_search" = 1, k < 2): it then goes a filter per pass through
// rel_kernel, which counts in int; everything else through the lane forms.
//
// Open: no tiled probe, no wide rows, no narrow tables, no passes shared between jobs for this call.
#pragma once

namespace {

// W_r of the set's longest read, and an upper bound of the set's thresholds: t_r grows with len, and where the longest read's t_r
// exceeds its W_r so does every read's (0: no read of the set is walked)
inline uint64_t rel_most_kmers(const commet_ctx *c, const commet_readset *rs) { return (uint64_t) rs->max_len / (uint64_t) c->k; }
inline uint32_t rel_largest_threshold(const commet_ctx *c, const commet_readset *rs, int percent, int min_hits)
{
    return rel_threshold(rs->max_len, c->k, percent, min_hits);
}

int rel_check_rule(const commet_ctx *c, const commet_readset *rs, int percent)
{
    if (percent < 1 || percent > 100) return fail("percent must be in 1..100 (got %d)", percent);
    if (rel_most_kmers(c, rs) > 65535)
        return fail("a read of %u bases holds %llu non-overlapping %d-mers: thresholds are held in 16 bits (at most 65535)", rs->max_len,
                    (unsigned long long) rel_most_kmers(c, rs), c->k);
    return 0;
}

int launch_rel_thresholds(commet_ctx *c, const commet_readset *rs, int percent, int min_hits, const uint64_t *d_sel, uint16_t *d_thr)
{
    if (rs->n_reads == 0) return 0;
    if (launch_size_ok(rs->n_reads)) return 1;
    KScope ks(c, "rel_thresholds_kernel", c->stream);
    COMMET_LAUNCH(rel_thresholds_kernel, dim3((unsigned) ((rs->n_reads + 255) / 256)), dim3(256), 0, c->stream, rs->view(), c->k, percent, min_hits, d_sel,
                  d_thr);
    HIP_OK(hipGetLastError());
    return 0;
}

// one pass of rs over the g filters in slots 0 .. g - 1 (launch_hits, profile.hpp, with the reads' own caps): g == 1: the filter in the
// current slot, the one-filter kernels; g >= 2: the group kernels, the A planes interleaved with stride gs
int launch_rel(commet_ctx *c, const commet_readset *rs, int g, int gs, bool wave, const uint16_t *d_thr, const uint64_t *d_sel, uint8_t *d_found,
               unsigned long long *d_walked, ActiveList al, uint64_t n_launch)
{
    if (rs->n_reads == 0) return 0;
    if (al.ids && n_launch == 0) return 0;
    const uint64_t items = al.ids ? n_launch : rs->n_reads;
    if (!wave && launch_size_ok(items)) return 1;
    const dim3 lanes((unsigned) ((items + 255) / 256));
    KScope ks(c, g > 1 ? (wave ? "rel_group_wave_kernel" : "rel_group_kernel") : (wave ? "rel_wave_kernel" : "rel_kernel"), c->stream);
    with_key(c->k, [&](auto key) {
        using W = decltype(key);
        if (g == 1) {
            if (wave)
                COMMET_LAUNCH(rel_wave_kernel<W>, dim3((unsigned) resident_blocks<rel_wave_kernel<W>>(c, items)), dim3(LONG_WG), 0, c->stream, rs->view(),
                              c->view(), c->k, d_thr, d_sel, d_found, d_walked, al);
            else
                COMMET_LAUNCH(rel_kernel<W>, lanes, dim3(256), 0, c->stream, rs->view(), c->view(), c->k, d_thr, d_sel, d_found, d_walked, al);
            return;
        }
        const FilterGroupView fg = filter_group(c, g, 0, true);
        with_value<2, 4, 8>(gs, [&](auto NF) {
            if (wave)
                COMMET_LAUNCH((rel_group_wave_kernel<W, NF>), dim3((unsigned) resident_blocks<rel_group_wave_kernel<W, NF>>(c, items)), dim3(LONG_WG), 0,
                              c->stream, rs->view(), fg, c->k, d_thr, d_sel, d_found, d_walked, al);
            else
                COMMET_LAUNCH((rel_group_kernel<W, NF>), lanes, dim3(256), 0, c->stream, rs->view(), fg, c->k, d_thr, d_sel, d_found, d_walked, al);
        });
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// search set s against the g chunk filters in slots 0 .. g - 1; largest = the set's largest threshold
int rel_pass(JobRun &j, int s, int g, int gs, uint32_t largest, const uint16_t *d_thr, uint8_t *d_found, unsigned long long *d_walked)
{
    commet_ctx *c = j.c;
    const commet_readset *rs = j.search_rs[s];
    const uint64_t *sel_s = j.sel_of(s);
    const bool sparse = rs->n_reads && sparse_pass(c, rs, sel_s, j.visited[s]);
    const ActiveList al = hits_pass_list(j, s, sparse);
    const bool wave = hits_wave_ok(c, rs) || (largest > 255 && long_mode(c, rs) != LongMode::never);
    // counts above a byte and no wave form: a filter per pass through the one-filter lane kernel
    const int per_pass = (largest > 255 && !wave) ? 1 : g;
    for (int i = 0; i < g; i += per_pass) {
        c->cur_slot = i;
        if (launch_rel(c, rs, per_pass, gs, wave, d_thr, sel_s, d_found, d_walked, al, j.visited[s])) return 1;
        if (rs->n_reads) ++j.n_search_launches;
    }
    c->cur_slot = 0;
    return 0;
}

}  // namespace

extern "C" {

int commet_readset_relative_thresholds(commet_ctx *c, const commet_readset *rs, int percent, int min_hits, uint16_t *thr_out)
{
    if (!rs->finalized) return fail("read set not finalized");
    if (rs->ctx != c) return fail("read set belongs to another context");
    if (rel_check_rule(c, rs, percent)) return 1;
    HIP_OK(hipSetDevice(c->device));
    SetUse in_call(c, rs);
    if (in_call.enter()) return 1;
    if (rs->n_reads == 0) return 0;
    if (grow_kept(c, c->d_thr, c->thr_cap, rs->n_reads, rs->n_reads)) return 1;
    if (launch_rel_thresholds(c, rs, percent, min_hits, nullptr, c->d_thr)) return 1;
    HIP_OK(hipMemcpyAsync(thr_out, c->d_thr, rs->n_reads * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail("stream synchronize failed: %s", hipGetErrorString(hipGetLastError()));
    c->kclock.collect();
    return 0;
}

int commet_index_and_search_relative(commet_ctx *c, const commet_readset *index_rs, const uint8_t *index_select, int n_search,
                                     const commet_readset *const *search_rs, const uint8_t *const *search_select, int percent, int min_hits,
                                     uint8_t *const *tags_out, uint64_t *const *shared_out, commet_job_info *info)
{
    if (n_search < 0) return fail("n_search must not be negative (got %d)", n_search);
    if (percent < 1 || percent > 100) return fail("percent must be in 1..100 (got %d)", percent);
    for (int s = 0; s < n_search; ++s)
        if (rel_check_rule(c, search_rs[s], percent)) return 1;
    BytesJob b(c, index_rs, n_search, search_rs);
    if (b.open(index_select, search_select, info != nullptr)) return 1;
    JobRun &j = b.j;
    // a threshold per read beside its found flag, filled before the first pass
    if (grow_kept(c, c->d_thr, c->thr_cap, b.n_bytes, b.n_bytes)) return 1;
    std::vector<uint32_t> largest((size_t) n_search, 0);
    int rc = 0;
    for (int s = 0; s < n_search && !rc; ++s) {
        largest[(size_t) s] = rel_largest_threshold(c, search_rs[s], percent, min_hits);
        rc = launch_rel_thresholds(c, search_rs[s], percent, min_hits, j.sel_of(s), c->d_thr + b.at[(size_t) s]);
    }
    if (!rc)
        rc = run_slot_groups(j, b.group_cap(), [&](JobRun &jr, int s, uint64_t, int g, int gs) {
            return rel_pass(jr, s, g, gs, largest[(size_t) s], c->d_thr + b.at[(size_t) s], b.bytes_of(s), b.d_walked);
        });
    HitsLeave leave;
    for (int s = 0; s < n_search; ++s)
        leave.tags_of(b.bytes_of(s), search_rs[s], 1, 1, tags_out ? tags_out + s : nullptr, shared_out ? shared_out + s : nullptr);
    return b.close(rc, leave, info);
}

}  // extern "C"
