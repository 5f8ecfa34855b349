// capi/filter.hpp — commet_readset_filter: the read filter (length, N, Shannon, -m) on a resident set.  One pass of a kernel of
// read_filter.hpp over the set's planes leaves three verdict bitmaps; the sequential part of the rule runs on the host, file by
// file, over those words (host/filter_rule.hpp: the one statement of the rule, shared with the filter_reads tool).
// (a part of the one translation unit capi.hip: included there, in order, after the kernels and state.hpp)
#pragma once

namespace {

// the Shannon terms of the lengths lo .. hi in the context's device table (kept: a matrix filters set after set of the same lengths)
int shannon_table(commet_ctx *c, uint32_t lo, uint32_t hi)
{
    if (c->d_shannon && c->shannon_lo == lo && c->shannon_hi == hi) return 0;
    std::vector<double> tab(commet_host::shannon_table_size(lo, hi));
    commet_host::fill_shannon_table(lo, hi, tab.data());
    HIP_OK(hipStreamSynchronize(c->load_stream));                 // (no filter kernel still reads the table that goes)
    (void) dm_free(c->d_shannon);
    c->d_shannon = nullptr;
    HIP_OK(dm_malloc((void **) &c->d_shannon, tab.size() * sizeof(double)));
    HIP_OK(hipMemcpy(c->d_shannon, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    c->shannon_lo = lo, c->shannon_hi = hi;
    return 0;
}

}  // namespace

extern "C" {

int commet_readset_filter(commet_ctx *c, const commet_readset *rs, int min_len, int64_t max_n, float min_shannon,
                          int64_t max_reads_per_file, uint8_t *select_out, commet_filter_stats *per_file)
{
    if (!c || !rs || !select_out) return fail("commet_readset_filter: null argument");
    if (rs->ctx != c) return fail("the read set belongs to another context");
    if (!rs->finalized) return fail("read set not finalized");
    SetUse use(c, rs);
    if (use.enter()) return 1;
    const uint64_t n = rs->n_reads, bw = bitmap_words(n);
    commet_host::FilterRule rule;
    rule.min_size = min_len;
    rule.max_N = (max_n < 0 || max_n > INT_MAX) ? INT_MAX : (int) max_n;
    rule.min_shannon = min_shannon;
    std::vector<uint64_t> words(3 * bw, 0), out(bw, 0);
    uint64_t *keep = words.data(), *by_len = keep + bw, *by_n = by_len + bw;
    if (n) {
        HIP_OK(hipSetDevice(c->device));
        ReadFilterParams p;
        p.min_len = (uint32_t) std::max(0, rule.min_size);
        p.max_other = (uint32_t) rule.max_N;
        p.min_shannon = rule.min_shannon;
        p.table = nullptr;
        p.table_lo = 1, p.table_hi = 0;
        const bool shannon = rule.min_shannon > 0;
        if (shannon) {
            const uint32_t lo = std::max(1u, rs->min_len), hi = (uint32_t) std::min<uint64_t>(rs->max_len, commet_host::SHANNON_TABLE_MAX_LEN);
            if (lo <= hi) {
                if (shannon_table(c, lo, hi)) return 1;
                p.table = c->d_shannon, p.table_lo = lo, p.table_hi = hi;
            }
        }
        const bool wave = rs->max_len > READ_FILTER_LANE_MAX_LEN;
        // reads the table does not cover: at most one per SHANNON_TABLE_MAX_LEN + 1 bases of the set
        const uint64_t long_cap = (wave && shannon && rs->max_len > commet_host::SHANNON_TABLE_MAX_LEN) ? rs->n_bases / (commet_host::SHANNON_TABLE_MAX_LEN + 1) + 1 : 0;
        const uint64_t need = (3 * bw + 1) * 8 + long_cap * sizeof(ReadFilterLong);
        if (rs->filter_ws_bytes < need) {                          // the set's own scratch, kept with it: [3 bitmaps][count][list]
            HIP_OK(hipStreamSynchronize(c->load_stream));
            (void) dm_free(rs->d_filter_ws);
            rs->d_filter_ws = nullptr, rs->filter_ws_bytes = 0;
            HIP_OK(dm_malloc((void **) &rs->d_filter_ws, need));
            rs->filter_ws_bytes = need;
        }
        uint64_t *d_keep = rs->d_filter_ws, *d_len = d_keep + bw, *d_n = d_len + bw;
        unsigned long long *d_count = (unsigned long long *) (d_n + bw);
        ReadFilterLong *d_longs = (ReadFilterLong *) (d_count + 1);
        hipStream_t st = c->load_stream;                           // (the stream of everything that makes a set ready: a second host thread may run jobs meanwhile)
        HIP_OK(hipMemsetAsync(d_keep, 0, (3 * bw + 1) * 8, st));
        hipEvent_t ev[2] = {nullptr, nullptr};
        if (c->kclock.on) {
            HIP_OK(hipEventCreate(&ev[0]));
            HIP_OK(hipEventCreate(&ev[1]));
            HIP_OK(hipEventRecord(ev[0], st));
        }
        const dim3 grid((unsigned) ((n + 255) / 256));
        if (wave) COMMET_LAUNCH(read_filter_wave_kernel, grid, dim3(256), 0, st, rs->view(), p, d_keep, d_len, d_n, d_longs, d_count, long_cap);
        else COMMET_LAUNCH(read_filter_lane_kernel, grid, dim3(256), 0, st, rs->view(), p, d_keep, d_len, d_n);
        HIP_OK(hipGetLastError());
        if (ev[1]) HIP_OK(hipEventRecord(ev[1], st));
        unsigned long long n_long = 0;
        HIP_OK(hipMemcpyAsync(words.data(), d_keep, 3 * bw * 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(&n_long, d_count, sizeof n_long, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (ev[1]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) c->kclock.add(wave ? "read_filter_wave_kernel" : "read_filter_lane_kernel", ms);
            (void) hipEventDestroy(ev[0]);
            (void) hipEventDestroy(ev[1]);
        }
        if (n_long > long_cap) return fail("commet_readset_filter: %llu reads longer than the Shannon table, room for %llu", n_long, (unsigned long long) long_cap);
        if (n_long) {                                              // decided here, with the tool's own function
            std::vector<ReadFilterLong> longs(n_long);
            HIP_OK(hipMemcpy(longs.data(), d_longs, n_long * sizeof(ReadFilterLong), hipMemcpyDeviceToHost));
            commet_host::Shannon sh;
            for (const ReadFilterLong &e : longs) {
                const uint64_t cnt[5] = {e.cnt[0], e.cnt[1], e.cnt[2], e.cnt[3], e.cnt[4]};
                if (e.read < n && !(sh(cnt, e.len) < rule.min_shannon)) keep[e.read >> 6] |= 1ull << (e.read & 63);
            }
        }
    }
    for (size_t f = 0; f < rs->files.size(); ++f) {                // the cap and the empty-record stop apply per file, as one tool run per file does
        const commet_host::FilterCounts fc = commet_host::finish_file(keep, by_len, by_n, rs->files[f].first, rs->files[f].count, rs->empty_reads.data(),
                                                                      rs->empty_reads.size(), max_reads_per_file, out.data());
        if (per_file) {
            per_file[f].reads = fc.reads, per_file[f].selected = fc.selected;
            per_file[f].removed_length = fc.removed_length, per_file[f].removed_n = fc.removed_n, per_file[f].removed_shannon = fc.removed_shannon;
        }
    }
    memcpy(select_out, out.data(), bitmap_bytes_host(n));
    return 0;
}

}  // extern "C"
