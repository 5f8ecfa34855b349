// capi/search_dispatch.hpp — which search regime runs for a set and a group of chunk filters (plain, group, group8, tiled, bit-sliced, wide rows) and its launches
// (a part of the one translation unit capi.hip: included there, in order, after the kernels and state.hpp)
#pragma once

namespace {

// min_hits as the kernels get it: a read of max_len bases holds at most max_len / k non-overlapping k-mers, so every
// t above max_len / k + 1 behaves like that value (never found, same probes); clamping keeps (t - seen - 1) * k and
// last - (t - 1) * k inside 32-bit int whatever atoi handed to commet_create
inline int t_eff(const commet_ctx *c, const commet_readset *rs)
{
    return (int) std::min<uint64_t>((uint64_t) c->t, (uint64_t) rs->max_len / (uint64_t) c->k + 1);
}

// first-hit windows of the set's longest read: the positions at which the first of t non-overlapping k-mers can start (< 1: no read
// of the set can be found)
inline int64_t first_hit_windows(const commet_ctx *c, const commet_readset *rs)
{
    return (int64_t) rs->max_len - (int64_t) t_eff(c, rs) * c->k + 1;
}

// a grid of one thread per read (or listed read), 256 per block, must stay below 2^24 blocks
inline int launch_size_ok(uint64_t n_reads)
{
    return (n_reads + 255) / 256 < (1ull << 24) ? 0 : fail("search launch too large (>= 2^32 reads in one set)");
}

// the g filters of a pass, from slot slot0 on; their A planes interleaved (c->il_a), or one filter's own plane A (stride 1)
inline FilterGroupView filter_group(const commet_ctx *c, int g, int slot0, bool interleaved)
{
    FilterGroupView fg;
    fg.il_a = interleaved ? c->il_a : c->slot_ptr(slot0);
    fg.slot0 = c->slot_ptr(slot0);
    fg.slot_words = 4 * c->plane_words;
    fg.plane_words = c->plane_words;
    fg.g = g;
    return fg;
}

// al.ids != nullptr: a pass over the n_launch (at most) listed reads (kernels.hpp, ActiveList) instead of the whole set
int launch_search(commet_ctx *c, const commet_readset *rs, const uint64_t *d_sel, uint64_t *d_tags, uint64_t *d_found,
                  unsigned long long *d_counters, unsigned long long *d_probes = nullptr, ActiveList al = ActiveList{nullptr, nullptr},
                  uint64_t n_launch = 0)
{
    if (rs->n_reads == 0) return 0;
    if (al.ids && n_launch == 0) return 0;
    const uint64_t items = al.ids ? n_launch : rs->n_reads;
    if (launch_size_ok(items)) return 1;
    const dim3 g((unsigned) ((items + 255) / 256)), b(256);
    KScope ks(c, "search_kernel", c->stream);
    with_key(c->k, [&](auto key) {
        with_value<false, true>(d_probes != nullptr, [&](auto count) {
            COMMET_LAUNCH((search_kernel<decltype(key), count>), g, b, 0, c->stream, rs->view(), c->view(), c->k, t_eff(c, rs), d_sel, d_tags,
                          d_found, d_counters, d_probes, al);
        });
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// makes `g` filter slots (+ the interleaved A planes with stride gs) available; slot contents are undefined after a grow.  The slots
// are not grown with grow_kept: the new block is taken BEFORE the old one goes, so that a context always has a filter
int ensure_slots(commet_ctx *c, int g, int gs)
{
    if (c->n_slots < g) {
        HIP_OK(hipStreamSynchronize(c->stream));
        uint32_t *nf = nullptr;
        // a whole group's worth at once (2, 4 or 8 slots): a job of seven chunks followed by one of eight (the N x N driver's J1, then its
        // shared J2 passes) used to take 14 GiB and then 16 GiB from the driver at k = 32; if that does not fit, what is needed now
        int want = std::max(g, gs);
        hipError_t e = dev_alloc(c, (void **) &nf, (size_t) want * c->filter_bytes, true);
        if (e != hipSuccess && want > g) {
            (void) hipGetLastError();
            want = g;
            e = dev_alloc(c, (void **) &nf, (size_t) want * c->filter_bytes, true);
        }
        if (e != hipSuccess) return fail("cannot allocate %d filter slots: %s", g, hipGetErrorString(e));
        (void) dm_free(c->filter);
        c->filter = nf;
        c->n_slots = want;
    }
    return grow_kept(c, c->il_a, c->il_words, (uint64_t) gs * c->plane_words, (uint64_t) gs * c->plane_words);
}

int launch_interleave(commet_ctx *c, int g, int gs)
{
    const uint64_t blocks = std::min<uint64_t>((c->plane_words + 255) / 256, 1u << 16);
    KScope ks(c, "interleave_a_kernel", c->stream);
    with_value<2, 4, 8>(gs, [&](auto GS) {
        COMMET_LAUNCH(interleave_a_kernel<GS>, dim3((unsigned) blocks), dim3(256), 0, c->stream, c->filter, 4 * c->plane_words, c->plane_words,
                      g, c->il_a);
    });
    HIP_OK(hipGetLastError());
    return 0;
}

template <typename W, int GS>
int launch_search_group_t(commet_ctx *c, const commet_readset *rs, const FilterGroupView &fg, uint32_t nw_max, const uint64_t *d_sel,
                          uint64_t *d_tags, unsigned long long *d_counters, uint32_t cstride, unsigned long long *d_probes, ActiveList al,
                          uint64_t n_launch)
{
    const dim3 g((unsigned) (((al.ids ? n_launch : rs->n_reads) + 255) / 256)), b(256);
    size_t lds = (size_t) fg.g * 2 * nw_max * 256 * sizeof(uint32_t);
    // the lanes' reads staged in LDS too (3 * nw_max words each) when that still fits 64 KiB
    uint32_t rw_nw = 0;
    if (!d_probes && nw_max <= 8 && lds + (size_t) 3 * nw_max * 256 * sizeof(uint32_t) <= (64u << 10)) {
        rw_nw = nw_max;
        lds += (size_t) 3 * nw_max * 256 * sizeof(uint32_t);
    }
    KScope ks(c, "search_group_kernel", c->stream);
    return with_value<false, true>(d_probes != nullptr, [&](auto count) {
        HIP_OK(hipFuncSetAttribute((const void *) search_group_kernel<W, GS, count>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        COMMET_LAUNCH((search_group_kernel<W, GS, count>), g, b, lds, c->stream, rs->view(), fg, c->k, t_eff(c, rs), nw_max, d_sel, d_tags,
                      d_counters, cstride, d_probes, rw_nw, al);
        HIP_OK(hipGetLastError());
        return 0;
    });
}

// mask words (32 first-hit windows each) a read of the set needs per strand and filter in the register-mask kernels
// (search_group8_kernel, tq_replay_kernel): 2, 3, 4, 6 or 8 — reads of up to 318 bases at k = 32, t = 2 (round 6; 96 windows before)
constexpr int MASK_MAX_WIN = 255;      // (= TQ_MAX_WIN)
// the one table of it: mask words for reads of up to `windows` windows (the tiled hit profile asks with every window of the read)
inline int mask_words_of(int64_t windows) { return windows <= 64 ? 2 : windows <= 96 ? 3 : windows <= 128 ? 4 : windows <= 192 ? 6 : 8; }
inline int mask_words(const commet_ctx *c, const commet_readset *rs) { return mask_words_of(first_hit_windows(c, rs)); }
template <typename F>
decltype(auto) with_mask_words(int mw, F &&f)
{
    return with_value<2, 3, 4, 6, 8>(mw, f);
}

// one pass of rs over the `g` chunk filters in slots 0..g-1 (A planes already interleaved with stride gs)
// job_mask != 0 (gs == 8 only): the g filters belong to several jobs, bit i = filter i opens one; job j's tags at d_tags + j * job_tag_words
int launch_search_group(commet_ctx *c, const commet_readset *rs, int g, int gs, const uint64_t *d_sel, uint64_t *d_tags,
                        unsigned long long *d_counters, uint32_t cstride, unsigned long long *d_probes, ActiveList al = ActiveList{nullptr, nullptr},
                        uint64_t n_launch = 0, uint32_t job_mask = 0, uint64_t job_tag_words = 0)
{
    if (rs->n_reads == 0) return 0;
    if (al.ids && n_launch == 0) return 0;
    if (launch_size_ok(rs->n_reads)) return 1;
    const FilterGroupView fg = filter_group(c, g, 0, true);
    if (gs == 8) {   // register masks, no LDS (group8_ok)
        const int mw_set = mask_words(c, rs);   // mask words per strand and filter: 2, 3, 4, 6 or 8
        auto launch = [&](int mw, ActiveList l, uint64_t n_l) {
            KScope ks(c, "search_group8_kernel", c->stream);
            const dim3 grid((unsigned) (((l.ids ? n_l : rs->n_reads) + 255) / 256)), block(256);
            with_key(c->k, [&](auto key) {
                with_mask_words(mw, [&](auto MW) {
                    COMMET_LAUNCH((search_group8_kernel<decltype(key), MW>), grid, block, 0, c->stream, rs->view(), fg, c->k, t_eff(c, rs), d_sel,
                                  d_tags, d_counters, cstride, l, job_mask, job_tag_words);
                });
            });
        };
        if (al.ids && al.ids == rs->d_len_order && rs->n_len_seg > 1 && !c->mask_split) {
            // the set's reads in order of their window counts: every segment of the list with the narrowest masks its reads fit
            // (three mask words cost 135 VGPRs and a fifth of the request rate of two; a 50-150-bp set has half its windows in
            // reads that need two)
            for (int sg = 0; sg < rs->n_len_seg; ++sg) {
                const commet_readset::LenSeg &seg = rs->len_seg[sg];
                launch(std::min(seg.mw, mw_set), ActiveList{rs->d_len_order + seg.start, rs->d_len_order + rs->n_reads + 1 + sg}, seg.count);
            }
        } else {
            launch(mw_set, al, n_launch);
        }
        HIP_OK(hipGetLastError());
        return 0;
    }
    const uint32_t nw_max = (rs->max_len + 31) / 32;
    return with_key(c->k, [&](auto key) {
        return with_value<2, 4>(gs, [&](auto GS) {
            return launch_search_group_t<decltype(key), GS>(c, rs, fg, nw_max, d_sel, d_tags, d_counters, cstride, d_probes, al, n_launch);
        });
    });
}

bool group_searchable(const commet_ctx *c, const commet_readset *rs, int g)
{
    // LDS masks: g chunks x 2 strands x ceil(max_len/32) words per lane, at most 64 KiB per workgroup
    const uint64_t nw = ((uint64_t) rs->max_len + 31) / 32;
    return c->k >= 2 && nw >= 1 && (uint64_t) g * 2 * nw * 256 * 4 <= (64u << 10);
}

// groups of 5..8 chunk filters: search_group8_kernel keeps the gathered bits of at most 255 first-hit windows per read in
// registers (kernels.hpp: two to eight mask words per strand and filter); the probe-counting builds exist for groups of <= 4 only
bool group8_ok(const commet_ctx *c, const commet_readset *rs)
{
    return c->k >= 2 && !c->count_probes && first_hit_windows(c, rs) <= MASK_MAX_WIN;
}

// ---- long reads: a wave per read (long_search.hpp) ---------------------------------------------------------------
// Sets with a read of more than MASK_MAX_WIN first-hit windows have neither the register-mask kernels nor the tiled search; the
// lane-per-read kernels that remain walk a read end to end in one lane, and a workgroup lives as long as its longest read.
// search_long_kernel gives a read a wave.  Auto takes it only in that region (every set with a fast path keeps it), and there
// by the set's LONGEST read: that is what the lane-per-read kernels' time follows.  Measured at k = 32, t = 2, three A/B pairs of
// fresh processes each (tools/long_read_bench.py; MEASUREMENTS.md, "Long reads"): the wave kernel lost every pair on sets
// whose longest read has 450..2500 bases (one length 450 / 600 / 800 / 1000 / 1500 / 2500, ragged 300-1500, 1 % of 600 / 1000 /
// 2000 among 100-300) and won every pair from 3000 on (1 % of 3000: 9.55 -> 7.8 ms; ragged 500-5000: 14.0 -> 10.6; one length
// 5500: 14.1 -> 5.7; ragged 1-10 kb: 22.2 -> 8.0).  Sets of ONE length between 2500 and 5500 were not measured, hence 5000.
constexpr uint32_t LONG_MIN_MAX_LEN = 5000;
// option "long_search" for a set: 1 never (also k < 2 and sets without a read), 2 whenever the set has a read, 0 auto — the rule
// of whoever asks (long_ok here, hits_wave_ok in profile.hpp)
enum class LongMode { never, always, automatic };
inline LongMode long_mode(const commet_ctx *c, const commet_readset *rs)
{
    if (c->long_search == 1 || c->k < 2 || rs->n_reads == 0) return LongMode::never;
    return c->long_search == 2 ? LongMode::always : LongMode::automatic;
}
bool long_ok(const commet_ctx *c, const commet_readset *rs)
{
    const LongMode m = long_mode(c, rs);
    return m == LongMode::always || (m == LongMode::automatic && first_hit_windows(c, rs) > MASK_MAX_WIN && rs->max_len >= LONG_MIN_MAX_LEN);
}

// persistent grid of a wave-per-read kernel (LONG_WG threads, four reads in flight per workgroup): the workgroups the device holds
// at once (4-8 per CU by the instantiation's registers, tools/kernel_resources.py; asked once per instantiation), or fewer when
// the pass has fewer reads
template <auto Kernel>
uint64_t resident_blocks(const commet_ctx *c, uint64_t items)
{
    static std::atomic<int> resident{0};
    int wgs = resident.load(std::memory_order_relaxed);
    if (!wgs) {
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, LONG_WG, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || per_cu < 1 || cus < 1) {
            (void) hipGetLastError();
            per_cu = 4, cus = 256;
        }
        wgs = per_cu * cus;
        resident.store(wgs, std::memory_order_relaxed);
    }
    return std::min<uint64_t>((items + 3) / 4, (uint64_t) wgs);
}

// one pass of rs over the g filters in slots 0..g-1: nf == 1 (g == 1): slot 0's own plane A; nf = 2, 4, 8: A planes interleaved with stride nf
// job_mask != 0 (nf == 8 only, no selection, list or probe counting): the g filters belong to several jobs, bit i = filter i opens one;
// job j's tags at d_tags + j * job_tag_words (zeroed by the caller)
int launch_search_long(commet_ctx *c, const commet_readset *rs, int g, int nf, const uint64_t *d_sel, uint64_t *d_tags,
                       unsigned long long *d_counters, uint32_t cstride, unsigned long long *d_probes, ActiveList al, uint64_t n_launch,
                       uint32_t job_mask = 0, uint64_t job_tag_words = 0)
{
    if (rs->n_reads == 0) return 0;
    if (al.ids && n_launch == 0) return 0;
    if (g < 1 || g > nf) return fail("internal error: %d filters in a long-read pass of stride %d", g, nf);
    const bool jobs = job_mask != 0 || job_tag_words != 0;
    if (jobs && (nf != 8 || d_sel || al.ids || d_probes || !(job_mask & 1u) || (job_mask >> g)))
        return fail("internal error: a long-read pass of several jobs (mask %#x, %d filters) of stride %d, or with a selection, a list or probe counting", job_mask, g, nf);
    const FilterGroupView fg = filter_group(c, g, 0, nf > 1);
    const uint64_t items = al.ids ? n_launch : rs->n_reads;
    KScope ks(c, "search_long_kernel", c->stream);
    with_key(c->k, [&](auto key) {
        if (jobs) {
            const uint64_t blocks = resident_blocks<search_long_kernel<decltype(key), 8, false, true>>(c, items);
            COMMET_LAUNCH((search_long_kernel<decltype(key), 8, false, true>), dim3((unsigned) blocks), dim3(LONG_WG), 0, c->stream, rs->view(), fg,
                          c->k, t_eff(c, rs), d_tags, d_counters, cstride, job_mask, job_tag_words);
            return;
        }
        with_value<1, 2, 4, 8>(nf, [&](auto NF) {
            with_value<false, true>(d_probes != nullptr, [&](auto count) {
                const uint64_t blocks = resident_blocks<search_long_kernel<decltype(key), NF, count>>(c, items);
                COMMET_LAUNCH((search_long_kernel<decltype(key), NF, count>), dim3((unsigned) blocks), dim3(LONG_WG), 0, c->stream, rs->view(), fg,
                              c->k, t_eff(c, rs), d_sel, d_tags, d_counters, cstride, d_probes, al);
            });
        });
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- sparse passes: the reads of a pass as a list (kernels.hpp, ActiveList) --------------------------------------
// A pass that searches less than half of a set's reads — Commet.py's third job of a pair searches a set restricted to the first
// job's result (Commet.py:233), ~22 % of it — walks the list of those reads (sel & ~tags, in order) instead of the set: every lane
// of a wave then has a read, where the bitmap form kept 64 lanes waiting through a read's dependent round trips for the 14 that had
// one (a J3 job of configs[3]: search 46 -> 12 ms).  `selected` = the reads the host plan visits (tags can only shrink the list).
bool sparse_pass(const commet_ctx *c, const commet_readset *rs, const uint64_t *d_sel, uint64_t selected)
{
    if (!d_sel || c->sparse_search == 1 || c->count_probes || rs->n_reads >= (1ull << 32)) return false;
    if (c->sparse_search == 2) return true;
    return rs->n_reads >= 4096 && selected * 2 < rs->n_reads;
}

// The reads whose bit is set in d_sel (and, with d_tags, not set there) as a list in `l`, in order, built on the job's stream: three
// small launches under one timing scope named `scope`, no synchronisation unless a buffer grows (n_ids: the reads the list may
// hold; alloc_ids >= n_ids: what a grown buffer is sized for).  0 = built, out = the list and its length word on the device;
// 1 = no room, or a launch failed (the caller takes the bitmap form, another path, or fails)
int build_id_list(commet_ctx *c, commet_ctx::IdList &l, const char *scope, const commet_readset *rs, const uint64_t *d_sel, const uint64_t *d_tags,
                  uint64_t n_ids, uint64_t alloc_ids, ActiveList *out)
{
    const uint64_t n_words = bitmap_words(rs->n_reads), nb = (n_words + IDS_BLOCK_WORDS - 1) / IDS_BLOCK_WORDS;
    if (grow_kept(c, l.ids, l.ids_cap, n_ids, alloc_ids) || grow_kept(c, l.blk, l.blk_cap, nb + 1, nb + 1)) return 1;
    KScope ks(c, scope, c->stream);
    COMMET_LAUNCH(sel_count_kernel, dim3((unsigned) nb), dim3(64), 0, c->stream, d_sel, n_words, l.blk, d_tags);
    COMMET_LAUNCH(sel_scan_kernel, dim3(1), dim3(1024), 0, c->stream, l.blk, (uint32_t) nb);
    COMMET_LAUNCH(sel_ids_kernel, dim3((unsigned) nb), dim3(64), 0, c->stream, d_sel, n_words, l.blk, l.ids, d_tags);
    if (hipGetLastError() != hipSuccess) return fail("selection list launch failed");
    out->ids = l.ids;
    out->n = l.blk + nb;
    return 0;
}

// a sparse pass's list: sel & ~tags (re-made per pass: the tags of the pass before have shrunk it)
inline int build_active_list(commet_ctx *c, const commet_readset *rs, const uint64_t *d_sel, const uint64_t *d_tags, uint64_t selected, ActiveList *al)
{
    return build_id_list(c, c->act_ids, "active_list_kernels", rs, d_sel, d_tags, selected, std::max<uint64_t>(selected, 1024), al);
}

// ---- ragged sets in order of their window counts (tile_search.hpp, lo_*_kernel) -------------------------------------------
// al = the set's list when a pass qualifies: a ragged set visited whole (no selection, no tags yet: the first pass of a job), no other
// list in use.  The list is made on the job's stream on first use (three small launches + the scan) and kept with the set; no room =
// the natural order, as before.
bool ordered_pass(commet_ctx *c, const commet_readset *rs, const uint64_t *d_sel, bool tags_empty, ActiveList *al)
{
    if (c->ordered_scan == 1 || rs->uniform_len != 0 || d_sel || !tags_empty || al->ids || c->count_probes || rs->len_order_failed) return false;
    if (rs->n_reads == 0 || rs->n_reads >= (1ull << 32) - 1 || (c->ordered_scan == 0 && rs->n_reads < (1u << 16))) return false;
    if (!rs->d_len_order) {
        const uint64_t n_blocks = (rs->n_reads + LO_BLOCK - 1) / LO_BLOCK, entries = n_blocks * LO_CLASSES;
        const uint32_t nb = (uint32_t) ((entries + 4095) / 4096);
        uint32_t *ids = nullptr;
        hipError_t e = dm_malloc((void **) &ids, (rs->n_reads + 8) * sizeof(uint32_t));   // (+ 1: the list's length; + 5: its segments')
        if (e == hipSuccess && grow_kept(c, c->d_lo_cnt, c->lo_cnt_cap, entries + 1 + nb + 2, entries + 1 + nb + 2)) e = hipErrorOutOfMemory;
        if (e != hipSuccess) {
            (void) hipGetLastError();
            (void) dm_free(ids);
            rs->len_order_failed = true;
            return false;
        }
        unsigned long long *cnt = c->d_lo_cnt, *totals = cnt + entries + 1;
        const uint32_t tk = (uint32_t) std::min<int64_t>((int64_t) t_eff(c, rs) * c->k, 0x7FFFFFFF);
        KScope ks(c, "len_order_kernels", c->stream);
        COMMET_LAUNCH(lo_count_kernel, dim3((unsigned) n_blocks), dim3(256), 0, c->stream, rs->view(), tk, n_blocks, cnt);
        COMMET_LAUNCH(tq_scan_blocks_kernel, dim3(nb), dim3(1024), 0, c->stream, cnt, entries, totals);
        COMMET_LAUNCH(tq_scan_totals_kernel, dim3(1), dim3(1024), 0, c->stream, totals, nb, totals + nb);
        COMMET_LAUNCH(tq_scan_add_kernel, dim3(nb), dim3(1024), 0, c->stream, cnt, entries, totals, totals + nb);
        COMMET_LAUNCH(lo_fill_kernel, dim3((unsigned) n_blocks), dim3(256), 0, c->stream, rs->view(), tk, n_blocks, cnt, ids);
        if (hipGetLastError() != hipSuccess) {
            (void) hipStreamSynchronize(c->stream);
            (void) dm_free(ids);
            rs->len_order_failed = true;
            return false;
        }
        // where the classes of 64, 96, 128 and 192 windows and more end (class = 31 - windows / 8: tile_search.hpp, lo_class; after the
        // scan cnt[class * n_blocks] = the class's first place in the list): the list's segments by mask width.  One read-back per
        // set; a segment of few reads joins its wider neighbour
        rs->n_len_seg = 0;
        unsigned long long first[4] = {0, 0, 0, 0};
        static const uint32_t cls[4] = {8, 16, 20, 24};
        static const int width[5] = {8, 6, 4, 3, 2};
        bool ok = true;
        for (int i = 0; i < 4 && ok; ++i)
            ok = hipMemcpyAsync(&first[i], cnt + (uint64_t) cls[i] * n_blocks, sizeof first[i], hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
        if (ok) {
            const uint64_t bound[6] = {0, first[0], first[1], first[2], first[3], rs->n_reads};
            const uint64_t few = c->ordered_scan == 2 ? 1 : 4096;
            for (int i = 0; i < 5; ++i) {
                const uint64_t a = bound[i], b = bound[i + 1];
                if (b <= a || b > rs->n_reads) continue;
                if (rs->n_len_seg > 0 && b - a < few)
                    rs->len_seg[rs->n_len_seg - 1].count += (uint32_t) (b - a);
                else
                    rs->len_seg[rs->n_len_seg++] = commet_readset::LenSeg{(uint32_t) a, (uint32_t) (b - a), width[i]};
            }
            uint32_t counts[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < rs->n_len_seg; ++i) counts[i] = rs->len_seg[i].count;
            ok = hipMemcpyAsync(ids + rs->n_reads + 1, counts, sizeof counts, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
                 hipStreamSynchronize(c->stream) == hipSuccess;       // (counts[] is on this stack)
        }
        if (!ok) {
            (void) hipGetLastError();
            rs->n_len_seg = 0;                                         // (the list itself is good: one launch at the set's width)
        }
        rs->d_len_order = ids;
    }
    al->ids = rs->d_len_order;
    al->n = rs->d_len_order + rs->n_reads;
    return true;
}

// ---- tiled search (tile_search.hpp) ----------------------------------------------------------------------------
constexpr int TQ_SLICE_BITS = 24;     // slice = 2^24 bits of plane A's address space: 2 MiB per chunk filter, 4 MiB for a group of two
                                      // (measured on configs[1]: 22 / 23 / 24 -> probe 2.43 / 2.56 / 2.35 ms, gpurun_out/r02_tq_ab2.log)

constexpr int TQ_MAX_K = 34;          // 64-bit keys from k = 33 (the reference's default k, index_and_search.cpp:71): 2^(k - 24) <= 1024 slices

// what the probe, the replay kernels and the query list's layout can take, whatever the mode and the group: the one statement of it.
// windows: of the list's longest read (< 1: the list is empty); records: an upper bound on the list's records
bool tq_geometry_ok(const commet_ctx *c, const commet_readset *rs, int64_t windows, uint64_t records)
{
    if (c->k <= TQ_SLICE_BITS || c->k > TQ_MAX_K) return false;
    if (windows < 1 || windows > TQ_MAX_WIN) return false;
    if (rs->max_len >= TQ_MAX_LEN) return false;        // (the replay keeps a piece's read extents in 16 + 16 bits; such reads pass the line above only with t in the hundreds)
    if (rs->n_reads >= (1ull << 32)) return false;
    return records < (1ull << 32);                      // record numbers are 32 bits (forced mode, too; build_query_list checks the exact count again)
}

// the search's list, (k, t_eff): for tiled_ok and query_list_blocks
// (rs->fhw_total: the set's first-hit windows summed over its reads — n x first_hit_windows for reads of one length, less for ragged sets)
bool tiled_geometry_ok(const commet_ctx *c, const commet_readset *rs) { return tq_geometry_ok(c, rs, first_hit_windows(c, rs), rs->fhw_total); }

// the memory of the set's list was set aside (commet_readset_reserve_cache) and no trim since has given it back: the blocks are still filed
bool list_set_aside(const commet_readset *rs) { return rs->ql_reserved.load() && rs->ql_reserved_at.load() == g_devmem.trims(); }

bool tiled_ok(const commet_ctx *c, const commet_readset *rs, int g)
{
    if (c->tiled_mode == 1 || c->count_probes || rs->ql.failed) return false;
    if (g < 1 || g > 2 || !tiled_geometry_ok(c, rs)) return false;
    if (c->tiled_mode == 2) return true;                // (forced: sets below auto's 2^20 reads too — query_list_blocks keeps that bound in every mode)
    // auto: sets of a million reads or more whose query list (8 bytes per first-hit window) stays under 4 GiB.  Measured
    // against the fused kernels: configs[1] search 9.4 -> 8.6 ms, configs[2] jobs 1.92-1.96 -> 1.84 s.
    const uint64_t est = rs->fhw_total * 8;
    // (a list above the cap when its memory was set aside beforehand, commet_readset_reserve_cache: the allocation is then not on this job's path)
    if (rs->n_reads < (1ull << 20) || (est > c->ql_max_list && !list_set_aside(rs))) return false;
    // A list of more than 4 GiB (sets of 15 M reads and up) is built for a set's SECOND such scan: a set that is scanned once —
    // every target of a rank that holds few pairs of a large matrix — would pay 12 ms of kernels and an 11 GB allocation for a
    // 7.6 ms gain (one J2 / J3 job of configs[3]: 54.7 against 62.3 ms), a set that is scanned again and again — every set of a
    // matrix on one GPU, the reference set of a rank's pairs — gets its list one scan late.
    if (est > (4ull << 30) && !rs->ql.built && rs->ql_wanted++ == 0) return false;
    return true;
}

// a query list of the set for (the context's k, t): counted, scanned, filled; kept with the set in `ql` — rs->ql for the search
// (t = t_eff), rs->pl for the tiled hit profile (t = 1; rs->ql itself where t_eff is 1: profile_list, capi/profile.hpp)
int build_query_list(commet_ctx *c, const commet_readset *rs, int t, commet_readset::QueryList &ql)
{
    if (ql.built) {
        ql.last_use = ++c->ql_clock;
        return 0;
    }
    ql.sbits = TQ_SLICE_BITS;
    ql.n_slices = 1u << (c->k - ql.sbits);
    ql.n_pieces = (uint32_t) ((rs->n_reads + TQ_PIECE - 1) / TQ_PIECE);
    const uint64_t entries = (uint64_t) ql.n_slices * ql.n_pieces;
    const uint32_t nb = (uint32_t) ((entries + 4095) / 4096);
    // The list is built on a stream of its own: at this point the job's index kernels are queued on the main streams, and the
    // list's kernels (VALU and LDS work on the SEARCH set) run beside them instead of behind them; the main stream waits for the
    // list before the probe (ev_list).  Nothing here may synchronise the device: the scan's block totals live in a scratch
    // buffer kept with the context (a hipFree would wait for the index build).
    hipStream_t ls = c->list_stream;
    // (the caller holds ql_mu: on an allocation failure here the other sets' lists are given back directly)
    auto alloc = [&](void **ptr, size_t bytes) { return dev_alloc(c, ptr, bytes, true, true); };
    hipError_t e = alloc((void **) &ql.d_tile_off, (entries + 1) * sizeof(unsigned long long));
    // (grows a few times in a context's life)
    if (e == hipSuccess && grow_kept(c, c->d_ql_totals, c->ql_totals_cap, (uint64_t) nb + 1, (uint64_t) nb + 1, true)) e = hipErrorOutOfMemory;
    unsigned long long *const d_totals = c->d_ql_totals;
    if (e == hipSuccess) {
        const size_t lds = (size_t) ql.n_slices * 4;
        {
            KScope ks(c, "tq_count_kernel", ls);
            with_key(c->k, [&](auto key) {
                COMMET_LAUNCH(tq_count_kernel<decltype(key)>, dim3(ql.n_pieces), dim3(256), lds, ls, rs->view(), c->k, t, ql.sbits, ql.n_slices,
                              ql.n_pieces, ql.d_tile_off);
            });
        }
        {
            KScope ks(c, "tq_scan_kernels", ls);
            COMMET_LAUNCH(tq_scan_blocks_kernel, dim3(nb), dim3(1024), 0, ls, ql.d_tile_off, entries, d_totals);
            COMMET_LAUNCH(tq_scan_totals_kernel, dim3(1), dim3(1024), 0, ls, d_totals, nb, d_totals + nb);
            COMMET_LAUNCH(tq_scan_add_kernel, dim3(nb), dim3(1024), 0, ls, ql.d_tile_off, entries, d_totals, d_totals + nb);
        }
        e = hipGetLastError();
        unsigned long long total = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&total, d_totals + nb, sizeof total, hipMemcpyDeviceToHost, ls);
        if (e == hipSuccess) e = hipStreamSynchronize(ls);
        ql.n_records = total;
        if (e == hipSuccess && total >= (1ull << 32)) e = hipErrorOutOfMemory;   // tstart is 32 bits (tiled_ok keeps such sets out; before any large allocation)
        if (e == hipSuccess) e = alloc((void **) &ql.d_qaddr, std::max<uint64_t>(total, 1) * 4);
        if (e == hipSuccess) e = alloc((void **) &ql.d_qwho, std::max<uint64_t>(total, 1) * 2);
        if (e == hipSuccess) e = alloc((void **) &ql.d_tstart, std::max<uint64_t>(entries, 1) * 4);
        if (e == hipSuccess) e = alloc((void **) &ql.d_tlen, std::max<uint64_t>(entries, 1) * 2);
        if (e == hipSuccess) {
            KScope ks(c, "tq_bounds_kernel", ls);
            COMMET_LAUNCH(tq_bounds_kernel, dim3((unsigned) ((entries + 255) / 256)), dim3(256), 0, ls, ql.d_tile_off, ql.n_slices,
                               ql.n_pieces, ql.d_tstart, ql.d_tlen);
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            // reads sorted per round in LDS: as many as keep rpr * (first-hit windows per read) within TQ_FILL_CAP records
            const int64_t fhw = std::max<int64_t>(1, (int64_t) rs->max_len - (int64_t) t * c->k + 1);
            // (even rounds: e.g. 256 reads x 87 windows = 22 272 records are three rounds of 86 reads)
            const uint32_t rounds = (uint32_t) (((uint64_t) TQ_PIECE * (uint64_t) fhw + TQ_FILL_CAP - 1) / TQ_FILL_CAP);
            uint32_t rpr = (TQ_PIECE + rounds - 1) / rounds;
            while (rpr > 1 && (uint64_t) rpr * (uint64_t) fhw > TQ_FILL_CAP) --rpr;
            const size_t lds_fill = ((size_t) 4 * ql.n_slices + 2 * TQ_FILL_CAP) * 4;
            e = with_key(c->k, [&](auto key) {
                hipError_t fe = hipFuncSetAttribute((const void *) tq_fill_kernel<decltype(key)>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_fill);
                if (fe != hipSuccess) return fe;
                KScope ks(c, "tq_fill_kernel", ls);
                COMMET_LAUNCH(tq_fill_kernel<decltype(key)>, dim3(ql.n_pieces), dim3(256), lds_fill, ls, rs->view(), c->k, t, ql.sbits, ql.n_slices,
                              ql.n_pieces, rpr, ql.d_tstart, ql.d_qaddr, ql.d_qwho);
                return hipGetLastError();
            });
        }
    }
    if (e == hipSuccess) e = hipEventRecord(c->ev_list, ls);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_list, 0);   // whatever the caller queues next (the probe) finds the list complete
    if (e != hipSuccess) {   // no room for the list (or a launch failed): this set keeps the gather kernels
        (void) hipGetLastError();
        ql.release();
        ql.failed = true;
        return 1;
    }
    ql.built = true;
    ql.bytes = (entries + 1) * 8 + ql.n_records * 6 + entries * 6;
    ql.last_use = ++c->ql_clock;
    c->ql_bytes += ql.bytes;
    if (c->ql_bytes > c->ql_budget) (void) shrink_query_lists(c, c->ql_budget, false);   // least recently used first; never one of this job
    return 0;
}

// the scan's result bytes (one per record of the list that is scanned); no room = this set keeps the gather kernels
int ensure_query_results(commet_ctx *c, commet_readset::QueryList &ql)
{
    const uint64_t need = std::max<uint64_t>(ql.n_records, 1);
    // (the caller holds ql_mu: the lists of sets outside this job are given back and the allocation tried once more)
    if (grow_kept(c, c->d_qres, c->qres_cap, need, need, true)) {
        ql.failed = true;
        return 1;
    }
    return 0;
}

// what build_query_list and ensure_query_results will ask for, for this context's (k, t): block sizes in bytes (upper bounds: every
// first-hit window of every read a record); false = the set does not qualify for the tiled search whatever the group
bool query_list_blocks(const commet_ctx *c, const commet_readset *rs, uint64_t out[6])
{
    // (auto mode's bound of 2^20 reads holds here in EVERY mode, where tiled_ok's forced mode passes it by: memory is set aside for
    // the sets that auto mode would scan tiled)
    if (!tiled_geometry_ok(c, rs) || rs->n_reads < (1ull << 20)) return false;
    const uint64_t records = rs->fhw_total;                   // (an upper bound: windows with a non-ACGT base make no record)
    const uint64_t entries = ((uint64_t) 1 << (c->k - TQ_SLICE_BITS)) * ((rs->n_reads + TQ_PIECE - 1) / TQ_PIECE);
    out[0] = (entries + 1) * 8, out[1] = records * 4, out[2] = records * 2, out[3] = entries * 4, out[4] = entries * 2;
    out[5] = c->qres_cap >= records ? 0 : records;            // the context's result buffer, one byte per record
    return true;
}

constexpr unsigned TQ_PROBE_WGS_PER_XCD = 64;   // probe workgroups per XCD (a multiple of the 32 CUs of an XCD keeps the sweep even;
                                                // measured: 32 or 64 (1 or 2 per CU) 2.3-2.6 ms, 128: 3.7, 256: 4.8)

// ---- what the tiled search and the tiled hit profile (capi/profile.hpp) launch alike: the probe over a list, then a replay kernel
inline QueryListView query_list_view(const commet_readset::QueryList &q)
{
    QueryListView v;
    v.tile_off = q.d_tile_off, v.qaddr = q.d_qaddr, v.qwho = q.d_qwho, v.tstart = q.d_tstart, v.tlen = q.d_tlen;
    v.n_slices = q.n_slices, v.n_pieces = q.n_pieces, v.sbits = q.sbits;
    return v;
}

// the result bytes of the whole list over fg's g <= 2 filters into c->d_qres.
// The probe is bound by L2 gathers, the replay by L2-MISSING requests and bookkeeping: different walls, but run beside each
// other (the set cut into runs of pieces, the replay of one beside the probe of the next on a second stream) they contend for
// the same memory system: measured on configs[1] 19.76 ms per step in one part, 21.8 / 23.2 / 24.6 / 25.3 in 2 / 3 / 4 / 6
// (r03_parts_*.json).  So the whole set's probe, then its replay, on the job's stream.
int launch_tq_probe(commet_ctx *c, const QueryListView &v, const FilterGroupView &fg, int g)
{
    {
        KScope ks(c, "tq_probe_kernel", c->stream);
        with_value<1, 2>(g, [&](auto GS) {
            COMMET_LAUNCH(tq_probe_kernel<GS>, dim3(8 * TQ_PROBE_WGS_PER_XCD), dim3(256), 0, c->stream, v, fg.il_a, c->d_qres, 0u, v.n_pieces);
        });
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// a replay kernel's build for (k, g filters, mw mask words): launch(key, GS, MW, hit_cap), timed under `name`
template <typename F>
int launch_tq_replay(commet_ctx *c, const char *name, int g, int mw, F &&launch)
{
    {
        KScope ks(c, name, c->stream);
        const uint32_t hit_cap = (uint32_t) std::min<int>(c->tq_hit_cap, TQ_HIT_CAP);
        with_key(c->k, [&](auto key) {
            with_value<1, 2>(g, [&](auto GS) { with_mask_words(mw, [&](auto MW) { launch(key, GS, MW, hit_cap); }); });
        });
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// one pass of rs over the g <= 2 chunk filters in slots slot0 .. slot0 + g - 1 (g == 2: slots 0, 1 with interleaved A planes)
// job_tag_words != 0 (g == 2): the two filters belong to two jobs; job j's found flags go to d_tags + j * job_tag_words (zeroed by the caller)
int launch_search_tiled(commet_ctx *c, const commet_readset *rs, int g, int slot0, const uint64_t *d_sel, uint64_t *d_tags,
                        unsigned long long *d_counters, uint32_t cstride, uint64_t job_tag_words = 0)
{
    if (rs->n_reads == 0) return 0;
    const commet_readset::QueryList &q = rs->ql;
    if (c->qres_cap < q.n_records) return fail("internal error: tiled search without its result buffer");
    const QueryListView v = query_list_view(q);
    const FilterGroupView fg = filter_group(c, g, slot0, g > 1);   // one filter: its own plane A (stride 1)
    const int t = t_eff(c, rs);
    if (launch_tq_probe(c, v, fg, g)) return 1;
    return launch_tq_replay(c, "tq_replay_kernel", g, mask_words(c, rs), [&](auto key, auto GS, auto MW, uint32_t hit_cap) {
        COMMET_LAUNCH((tq_replay_kernel<decltype(key), GS, MW>), dim3(q.n_pieces), dim3(TQ_PIECE), 0, c->stream, rs->view(), v, c->d_qres, fg, c->k, t,
                      d_sel, d_tags, d_counters, cstride, 0u, hit_cap, job_tag_words);
    });
}

// words per bit-sliced entry (32 chunk filters per word) of the narrow tables for n_chunks >= 1 chunks at SLICE_MIN_K <= k <= SLICE_MAX_K:
// option "slice_words", else by the chunk count; clamped
int slice_entry_words(const commet_ctx *c, uint64_t n_chunks)
{
    int gw = c->slice_gw ? c->slice_gw : n_chunks > 128 ? 8 : n_chunks > 64 ? 4 : n_chunks > 32 ? 2 : 1;
    while (gw > 1 && (((uint64_t) 16 * gw) << c->k) > (1ull << 30)) gw /= 2;   // the four tables: at most 1 GiB
    return gw;
}

// the same for a job of n_chunks chunks; 0 = the job takes the slot path
int slice_words(const commet_ctx *c, uint64_t n_chunks)
{
    if (c->slice_mode == 1 || c->count_probes) return 0;
    if (c->k < SLICE_MIN_K || c->k > SLICE_MAX_K || n_chunks == 0) return 0;
    if (c->slice_mode == 0 && n_chunks < 8) return 0;
    return slice_entry_words(c, n_chunks);
}

int ensure_slice_buffers(commet_ctx *c, int gw, uint64_t n_chunks)
{
    const uint64_t G = 32ull * gw;
    const uint64_t stage_words = (G * 4) << (c->k - 5), table_words = ((uint64_t) 4 * gw) << c->k;
    return grow_kept(c, c->slice_stage, c->slice_stage_words, stage_words, stage_words) ||
           grow_kept(c, c->slice_tables, c->slice_table_words, table_words, table_words) ||
           grow_kept(c, c->d_slice_chunks, c->slice_chunks_cap, n_chunks, n_chunks);
}

// filters of chunks [ci, ci + g) of the plan -> bit-sliced tables (slice_search.hpp)
int launch_slice_build(commet_ctx *c, const commet_readset *rs, const uint64_t *d_sel, uint64_t ci, int g, int gw,
                       uint32_t *tables = nullptr, uint32_t row_words = 0, uint32_t col0 = 0)
{
    if (!tables) tables = c->slice_tables, row_words = (uint32_t) gw, col0 = 0;   // the table of one group (search_sliced_kernel)
    const int tile_bits = std::min(c->k, SLICE_TILE_BITS);
    const uint32_t tiles = 1u << (c->k - tile_bits);
    const size_t lds = (size_t) 4 << (tile_bits - 5);
    HIP_OK(hipFuncSetAttribute((const void *) slice_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
    {
        KScope ks(c, "slice_build_kernel", c->stream);
        COMMET_LAUNCH(slice_build_kernel, dim3(4 * tiles, (unsigned) g), dim3(1024), lds, c->stream, rs->view(), d_sel,
                           c->d_slice_chunks + ci, c->k, tile_bits, tiles, c->slice_stage);
    }
    HIP_OK(hipGetLastError());
    const unsigned grid = (unsigned) ((((uint64_t) 4 << (c->k - 5)) + 255) / 256);
    {
        KScope ks(c, "slice_transpose_kernel", c->stream);
        with_value<1, 2, 4, 8>(gw, [&](auto GW) {
            COMMET_LAUNCH(slice_transpose_kernel<GW>, dim3(grid), dim3(256), 0, c->stream, c->slice_stage, c->k, g, tables, row_words, col0);
        });
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int launch_search_sliced(commet_ctx *c, const commet_readset *rs, int g, int gw, const uint64_t *d_sel, uint64_t *d_tags,
                         unsigned long long *d_counters, uint32_t cstride, uint32_t block_stride = 1)
{
    if (rs->n_reads == 0) return 0;
    if (launch_size_ok(rs->n_reads)) return 1;
    const uint64_t blocks = (rs->n_reads + 255) / 256;
    const dim3 grid((unsigned) ((blocks + block_stride - 1) / block_stride)), block(256);
    KScope ks(c, "search_sliced_kernel", c->stream);
    with_value<1, 2, 4, 8>(gw, [&](auto GW) {
        COMMET_LAUNCH(search_sliced_kernel<GW>, grid, block, 0, c->stream, rs->view(), c->slice_tables, c->k, t_eff(c, rs), g, d_sel, d_tags,
                      d_counters, cstride, block_stride);
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// one pass of rs over the g chunk filters in the narrow tables (hit_profile_sliced.hpp)
int launch_hits_sliced(commet_ctx *c, const commet_readset *rs, int g, int gw, int max_hits, const uint64_t *d_sel, uint8_t *d_hits,
                       unsigned long long *d_walked)
{
    if (rs->n_reads == 0) return 0;
    if (launch_size_ok(rs->n_reads)) return 1;
    const dim3 grid((unsigned) ((rs->n_reads + 255) / 256)), block(256);
    KScope ks(c, "hits_sliced_kernel", c->stream);
    with_value<1, 2, 4, 8>(gw, [&](auto GW) {
        COMMET_LAUNCH(hits_sliced_kernel<GW>, grid, block, 0, c->stream, rs->view(), c->slice_tables, c->k, max_hits, g, d_sel, d_hits, d_walked);
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- wide rows (slice_search.hpp): every chunk filter of the job — or as many as the table budget allows — in one table ----
struct WidePlan {
    uint32_t nw = 0;              // words per row that hold chunks (a multiple of WIDE_GROUP_WORDS); 0 = no wide pass
    uint32_t rw = 0;              // row stride in words (a multiple of 32: rows start on 128-byte lines)
    uint64_t chunks_per_pass = 0;
    int lpr = 0, np = 0;          // lanes per read, 16-byte pieces per lane
};

// the rows that hold n_chunks chunk filters under the table budget and option "slice_wide_words" (nw = 0: no room for a row of one group)
WidePlan wide_rows(const commet_ctx *c, uint64_t n_chunks)
{
    WidePlan w;
    if (n_chunks == 0) return w;
    const uint64_t groups = (n_chunks + 255) / 256;
    // four tables of 2^k rows: 16 bytes per row word and key; at most a third of what is free now, and 48 GiB
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return w;
    const uint64_t have = (uint64_t) c->wide_table_words * 4 + dm_filed_bytes(c->device);   // (what the context already holds, and what the library keeps for reuse, counts as free)
    const uint64_t budget = std::min<uint64_t>(((uint64_t) free_b + have) / 3, 48ull << 30);
    uint64_t cap = std::min<uint64_t>(WIDE_MAX_ROW_WORDS, budget / (16ull << c->k));
    if (c->wide_cap_words) cap = std::min<uint64_t>(cap, c->wide_cap_words);
    cap = cap / WIDE_GROUP_WORDS * WIDE_GROUP_WORDS;
    if (cap < WIDE_GROUP_WORDS) return w;
    const uint64_t passes = (groups * WIDE_GROUP_WORDS + cap - 1) / cap;
    const uint64_t groups_per_pass = (groups + passes - 1) / passes;
    w.nw = (uint32_t) (groups_per_pass * WIDE_GROUP_WORDS);
    w.rw = (w.nw + 31u) & ~31u;   // rows start on 128-byte lines: a row of 1312 bytes is 11 lines, never 12
    w.chunks_per_pass = groups_per_pass * 256;
    const uint32_t pieces = w.nw / 4;
    w.lpr = pieces <= 8 ? 8 : pieces <= 16 ? 16 : pieces <= 32 ? 32 : 64;
    w.np = pieces <= 64 ? 1 : 2;
    return w;
}

// a job's wide rows: none where option "slice_wide" or the chunk count says so
WidePlan wide_plan(const commet_ctx *c, uint64_t n_chunks, int slice_gw)
{
    if (!slice_gw || c->slice_wide == 1) return WidePlan();
    if (c->slice_wide == 0 && n_chunks <= 256) return WidePlan();    // one table of the narrow kind holds them all
    return wide_rows(c, n_chunks);
}

int ensure_wide_tables(commet_ctx *c, const WidePlan &w)
{
    const uint64_t words = ((uint64_t) 4 * w.rw) << c->k;
    return grow_kept(c, c->wide_tables, c->wide_table_words, words, words);   // 1: the caller falls back to the narrow tables
}

// a launch of 256 threads over n_reads reads in the wide rows (none: nothing to launch): f(grid, LPR, NP) with the plan's lanes per
// read and 16-byte pieces per lane as constants — the kernels of a call site exist as <64, 2> and <64 | 32 | 16 | 8, 1>
template <typename F>
int launch_wide(uint64_t n_reads, const WidePlan &w, F f)
{
    if (n_reads == 0) return 0;
    const uint64_t reads_per_block = 4ull * (64 / w.lpr);
    const uint64_t blocks = (n_reads + reads_per_block - 1) / reads_per_block;
    if (blocks >= (1ull << 31)) return fail("search launch too large");
    const dim3 grid((unsigned) blocks);
    if (w.np == 2) f(grid, std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
    else with_value<64, 32, 16, 8>(w.lpr, [&](auto LPR) { f(grid, LPR, std::integral_constant<int, 1>{}); });
    HIP_OK(hipGetLastError());
    return 0;
}

int launch_search_wide(commet_ctx *c, const commet_readset *rs, const WidePlan &w, int g, const uint64_t *d_sel, uint64_t *d_tags,
                       unsigned long long *d_counters, uint32_t cstride)
{
    return launch_wide(rs->n_reads, w, [&](dim3 grid, auto LPR, auto NP) {
        KScope ks(c, "search_wide_kernel", c->stream);
        COMMET_LAUNCH((search_wide_kernel<LPR, NP>), grid, dim3(256), 0, c->stream, rs->view(), c->wide_tables, c->k, t_eff(c, rs), g, w.nw, w.rw, d_sel,
                      d_tags, d_counters, cstride);
    });
}

}  // namespace

extern "C" {

// (here rather than in cache.hpp: they need the tiled search's geometry)
uint64_t commet_readset_cache_estimate(commet_ctx *c, const commet_readset *rs)
{
    uint64_t b[6];
    if (rs->ctx != c || !rs->finalized || !query_list_blocks(c, rs, b)) return 0;
    return b[0] + b[1] + b[2] + b[3] + b[4];
}

int commet_readset_reserve_cache(commet_ctx *c, const commet_readset *rs)
{
    if (rs->ctx != c) return fail("read set belongs to another context");
    if (!rs->finalized) return fail("read set not finalized");
    SetUse use(c, rs);
    if (use.enter()) return 1;
    HIP_OK(hipSetDevice(c->device));
    uint64_t b[6];
    {
        std::lock_guard<std::mutex> lk(c->ql_mu);
        if (rs->ql.built || list_set_aside(rs) || !g_devmem.enabled() || !query_list_blocks(c, rs, b)) return 0;
    }
    for (int i = 0; i < 6; ++i)
        if (b[i] && dm_reserve((size_t) b[i]) != hipSuccess) return 0;      // no room: the set keeps the cap's rule
    rs->ql_reserved_at.store(g_devmem.trims());
    rs->ql_reserved.store(true);
    return 0;
}

}  // extern "C"
