// capi/index_dispatch.hpp — which index construction runs for a chunk (atomic kernel or bucketed build, index_part.hpp) and its launches; commet_filter_reset
// (a part of the one translation unit capi.hip: included there, in order, after the kernels and state.hpp)
#pragma once

extern "C" {

/* ---- kernels -------------------------------------------------------------- */

int commet_filter_reset(commet_ctx *c)
{
    HIP_OK(hipSetDevice(c->device));
    KScope ks(c, "filter_memset", c->stream);
    HIP_OK(hipMemsetAsync(c->slot_ptr(c->cur_slot), 0, c->filter_bytes, c->stream));
    return 0;
}

}  // extern "C"

namespace {

// uploads a host bit array (n/8+1 bytes) into a device bitmap of bitmap_words(n) words
int upload_bits(commet_ctx *c, uint64_t *d_bits, const uint8_t *h_bits, uint64_t n)
{
    HIP_OK(hipMemsetAsync(d_bits, 0, bitmap_words(n) * 8, c->stream));
    HIP_OK(hipMemcpyAsync(d_bits, h_bits, bitmap_bytes_host(n), hipMemcpyHostToDevice, c->stream));
    return 0;
}

int launch_index_atomic(commet_ctx *c, const commet_readset *rs, uint64_t first, uint64_t count, const uint64_t *d_sel,
                        unsigned long long *d_fed)
{
    if (count == 0) return 0;
    const uint64_t blocks = (count + 255) / 256;
    if (blocks >= (1ull << 24)) return fail("index launch too large (>= 2^32 reads in one chunk)");
    KScope ks(c, "index_kernel", c->stream);
    with_key(c->k, [&](auto key) {
        COMMET_LAUNCH(index_kernel<decltype(key)>, dim3((unsigned) blocks), dim3(256), 0, c->stream, rs->view(), c->view(), c->k, first,
                      count, d_sel, d_fed);
    });
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- which construction a launch may take ----------------------------------------------------------------------------------------
// what the geometry of the bucketed construction needs (tiles of 2^19 bits, at most 2^17 buckets)
bool partition_geometry_ok(const commet_ctx *c) { return c->k >= 20 && c->k <= 34; }

// what only the round planner needs (plan_round, MODE 0 of part_hist_kernel / part_scatter1_kernel): one whole read must fit a round of
// S1_KEYS keys and S1_ITEMS items.  A set with a longer read ("oversize") takes the bucketed construction through the item list
// only (LIST), whatever its shape: the list enumerates octets, not reads, and is cut into pieces of equal ITEM counts, so a set of a
// few very long reads of one length is spread like any other (UNI cuts by reads: 20 reads would be 1 piece); the list of a job's
// selected reads (d_ids) is not used for such a set, the list builder reads the selection bitmap itself
bool oversize_reads(const commet_readset *rs)
{
    return (uint64_t) rs->max_kcnt * 4 > S1_KEYS || ((uint64_t) rs->max_len + 7) / 8 > S1_ITEMS;
}

// word triples a chunk of `count` reads spans at most (an item holds its triple, counted from the chunk's first read, in 28 bits)
uint64_t span_bound_of(const commet_readset *rs, uint64_t count)
{
    return std::min<uint64_t>((rs->n_bases >> 5) + rs->n_reads + 1, count * (((uint64_t) rs->max_len >> 5) + 2));
}

// items of a chunk at most: every selected read of it as long as the set's longest / the set's bases in octets plus one per read
uint64_t items_bound_of(const commet_readset *rs, uint64_t sel_reads)
{
    return std::min<uint64_t>(sel_reads * std::max<uint64_t>(1, ((uint64_t) rs->max_len + 7) / 8), rs->n_bases / 8 + rs->n_reads) + 1;
}

// what the item list needs of a launch over `count` reads, its buffers apart (ensure_item_buffers)
bool list_possible(const commet_ctx *c, const commet_readset *rs, uint64_t count)
{
    return !c->part_no_uni && c->part_list != 1 && span_bound_of(rs, count) < ITEM_MAX_TRIPLES &&
           (count + ITEMS_BLOCK - 1) / ITEMS_BLOCK + 1 < (1ull << 24) && items_bound_of(rs, count) < (1ull << 32);
}

// auto mode (index_mode = 0) on sets with oversize reads: not before the A/B of tools/long_read_bench.py --index-mode has been run on a
// device (MEASUREMENTS.md says what was measured); index_mode = 2 takes the build wherever partition_eligible says it can
constexpr bool LONG_INDEX_AUTO = false;

// may a launch over `count` reads of rs take the bucketed construction at all
bool partition_eligible(const commet_ctx *c, const commet_readset *rs, uint64_t count)
{
    return partition_geometry_ok(c) && (!oversize_reads(rs) || list_possible(c, rs, count));
}

// the item list's buffers in a lane's workspace: `need` items, nblk block sums; false = no room (nothing is held then)
bool ensure_item_buffers(commet_ctx *c, commet_ctx::PartWs &ws, hipStream_t stream, uint64_t need, uint64_t nblk)
{
    if (ws.items_cap >= need && ws.itemblk_cap >= nblk + 1) return true;
    if (hipStreamSynchronize(stream) != hipSuccess) return false;
    (void) dm_free(ws.items), (void) dm_free(ws.itemblk);
    ws.items = ws.itemblk = nullptr, ws.items_cap = ws.itemblk_cap = 0;
    const uint64_t cap = need + need / 8;
    ws.items_set = 0;
    if (dev_alloc(c, (void **) &ws.items, cap * sizeof(uint32_t), true) != hipSuccess ||
        dev_alloc(c, (void **) &ws.itemblk, (nblk + 1 + 1024) * sizeof(uint32_t), true) != hipSuccess) {
        (void) hipGetLastError();
        (void) dm_free(ws.items), (void) dm_free(ws.itemblk);
        ws.items = ws.itemblk = nullptr;
        return false;
    }
    ws.items_cap = cap, ws.itemblk_cap = nblk + 1 + 1024;
    return true;
}

// Bucketed construction of the filter for one chunk (index_part.hpp).  The
// filter must have been zeroed on the stream before.  kmers = exact number of
// complete k-mers of the selected reads of [first, first+count).
// d_ids != nullptr (fixed-length sets only): the chunk's selected reads are ids[pos_first .. pos_first + pos_count) (sel_ids_kernel);
// hist and scatter1 then take the arithmetic item path over that list instead of planning rounds over the bitmap
int launch_index_partitioned(commet_ctx *c, const commet_readset *rs, uint64_t first, uint64_t count, const uint64_t *d_sel,
                             uint64_t kmers, bool additive, bool zero_fill, int lane = 0, const uint32_t *d_ids = nullptr,
                             uint64_t pos_first = 0, uint64_t pos_count = 0)
{
    if (count == 0 || kmers == 0) return 0;
    const bool oversize = oversize_reads(rs);      // a read that no round of the planner holds: the item list, cut by items (see oversize_reads)
    if (!oversize && d_ids && rs->uniform_len != 0 && !c->part_no_uni && pos_count) first = pos_first, count = pos_count, d_sel = nullptr;
    else d_ids = nullptr;
    commet_ctx::PartWs &ws = c->part[lane];
    hipStream_t stream = lane ? c->aux_stream : c->stream;
    if (lane == 1 && c->stagger_armed) {   // (see behind scatter1 below)
        HIP_OK(hipStreamWaitEvent(stream, c->ev_stagger, 0));
        c->stagger_armed = false;
    }
    uint32_t *const slot = c->slot_ptr(c->cur_slot);
    PartGeom g = make_geom(c->k);
    g.packed = c->part_packed;
    if (g.b2 == 0) g.packed = 0;   // single level: scatter1 writes the final buckets itself, as plain keys
    const uint64_t total = 4 * kmers;
    if (ws.nb != g.nb) {
        (void) dm_free(ws.hist); (void) dm_free(ws.wl); (void) dm_free(ws.off); (void) dm_free(ws.goff);
        (void) dm_free(ws.cur2);
        ws.hist = ws.wl = nullptr; ws.off = ws.goff = nullptr; ws.cur2 = nullptr;
        HIP_OK(dev_alloc(c, (void **) &ws.hist, (g.nb + 1) * sizeof(uint32_t), true));
        HIP_OK(dev_alloc(c, (void **) &ws.wl, (g.nb + 1) * sizeof(uint32_t), true));
        HIP_OK(dev_alloc(c, (void **) &ws.off, (g.nb + 1) * sizeof(uint64_t), true));
        HIP_OK(dev_alloc(c, (void **) &ws.goff, (g.nb + 1) * sizeof(uint64_t), true));
        if (!ws.blockcnt) HIP_OK(dev_alloc(c, (void **) &ws.blockcnt, (size_t) S1_GRID_MAX * MAX_L1 * sizeof(uint32_t), true));
        if (!ws.blockoff) HIP_OK(dev_alloc(c, (void **) &ws.blockoff, (size_t) S1_GRID_MAX * MAX_L1 * sizeof(unsigned long long), true));
        HIP_OK(dev_alloc(c, (void **) &ws.cur2, g.nb * sizeof(unsigned long long), true));
        ws.nb = g.nb;
    }
    // bufA: one word per key.  bufB: the same when the final level holds plain keys; in the packed geometry 8-byte groups of three keys,
    // every (scatter2 slab, final bucket) run rounded up to a whole group (part_scan_kernel: a bucket of c keys gets c / 3 + the slabs
    // that overlap its coarse bucket + 1 groups): two words x (total / 3 + 2^b2 x (total / S2_KEYS + 3 x 2^b1)) — 0.73 words per key
    // at k = 32, where a full word per key was 2.3 GB per workspace asked from the driver for nothing
    const bool packed_b = g.packed && g.b2 && (1u << g.b2) <= S2P_MAX_SUB;
    auto words_b = [&](uint64_t keys) -> uint64_t {
        return packed_b ? 2 * (keys / 3 + ((uint64_t) 1 << g.b2) * (keys / S2_KEYS + 3ull * g.nb1)) + 4096 : keys;
    };
    if (ws.cap_keys < total || ws.cap_b < words_b(total)) {
        HIP_OK(hipStreamSynchronize(stream));
        (void) dm_free(ws.bufA); (void) dm_free(ws.bufB);
        ws.bufA = ws.bufB = nullptr;
        ws.cap_keys = 0, ws.cap_b = 0;
        const uint64_t cap = total + total / 16 + (1ull << 20);
        // (touched there, too: a first touch inside the first scatter launch cost 15.6 instead of 2.5 ms)
        HIP_OK(alloc_workspace(c, (void **) &ws.bufA, cap * sizeof(uint32_t), stream));
        HIP_OK(alloc_workspace(c, (void **) &ws.bufB, words_b(cap) * sizeof(uint32_t), stream));
        ws.cap_keys = cap, ws.cap_b = words_b(cap);
    }
    const bool wide = c->k > 32;
    // every read of one length and no selection bitmap: items by arithmetic, no round planning (index_part.hpp, UNI)
    const bool uni = !oversize && rs->uniform_len != 0 && d_sel == nullptr && !c->part_no_uni;   // (d_ids: positions in the list of selected reads)
    // ragged reads (with or without a selection bitmap): the chunk's items written out once, then walked like a fixed-length set
    // (index_part.hpp, LIST) — where an item's triple, counted from the chunk's first read, fits its 28 bits
    // (a set with oversize reads: any shape, launch_index has checked the conditions and made the buffers)
    bool list = oversize ? list_possible(c, rs, count)
                         : !uni && rs->uniform_len == 0 && !c->part_no_uni && c->part_list != 1 && span_bound_of(rs, count) < ITEM_MAX_TRIPLES;
    const uint32_t *d_items = nullptr, *d_nitems = nullptr;
    const uint64_t need = items_bound_of(rs, pos_count ? pos_count : count);
    if (list) {
        const uint64_t nblk = (count + ITEMS_BLOCK - 1) / ITEMS_BLOCK;
        if (nblk + 1 >= (1ull << 24) || need >= (1ull << 32)) list = false;
        if (list && !ensure_item_buffers(c, ws, stream, need, nblk)) list = false;   // no room: the round planner walks the reads, as before
        // the list of an UNSELECTED read range is a function of the set alone: a workspace that still holds it (the same chunk of the same
        // set indexed again: the reference set of a rank's J1 calls, a benchmark's steady state) does not write it again
        // (the key is set only once the launches are queued: a failed write leaves the buffer nobody's)
        const bool held = list && !d_sel && ws.items_set == rs->uid && ws.items_first == first && ws.items_count == count && ws.items_nblk == (uint32_t) nblk;
        if (list && !held) {
            ws.items_set = 0;
            {
                KScope ks(c, "part_items_kernels", stream);
                COMMET_LAUNCH(part_items_kernel<false>, dim3((unsigned) nblk), dim3(ITEMS_BLOCK), 0, stream, rs->view(), rs->d_kcnt, d_sel, first, count, c->k,
                              ws.itemblk, ws.items);
                COMMET_LAUNCH(sel_scan_kernel, dim3(1), dim3(1024), 0, stream, ws.itemblk, (uint32_t) nblk);
                if (!oversize)
                    COMMET_LAUNCH(part_items_kernel<true>, dim3((unsigned) nblk), dim3(ITEMS_BLOCK), 0, stream, rs->view(), rs->d_kcnt, d_sel, first, count,
                                  c->k, ws.itemblk, ws.items);
            }
            if (oversize) {   // the list cut by items, every piece written by a whole workgroup; need < 2^32: the grid is small
                KScope ks(c, "part_items_fill_kernel", stream);
                COMMET_LAUNCH(part_items_fill_kernel, dim3((unsigned) ((need + ITEMS_FILL_PER_WG - 1) / ITEMS_FILL_PER_WG)), dim3(ITEMS_BLOCK), 0, stream,
                              rs->view(), rs->d_kcnt, d_sel, first, count, c->k, ws.itemblk, (uint32_t) nblk, ws.items);
            }
            HIP_OK(hipGetLastError());
            ws.items_set = d_sel ? 0 : rs->uid, ws.items_first = first, ws.items_count = count, ws.items_nblk = (uint32_t) nblk;
        }
        if (list) d_items = ws.items, d_nitems = ws.itemblk + nblk;
    }
    const int mode = uni ? 1 : list ? 2 : 0;
    if (oversize && mode != 2) return fail("internal error: a set with reads of more than %u k-mers reached the round planner", S1_KEYS / 4);
    HIP_OK(hipMemsetAsync(ws.hist, 0, (g.nb + 1) * sizeof(uint32_t), stream));
    // scatter1's grid fixes how the read range is cut; hist counts with the same cut, two ranges per workgroup
    // (by the chunk's READ count: 64 reads of a few hundred bases are a few rounds.  With oversize reads the count says nothing — 51 reads
    // of 2 Mbases would be one piece — so there the host's bound on the chunk's ITEMS sizes the cut, four rounds of scatter1 per piece at
    // least; LIST cuts its pieces at equal item counts whatever their number)
    const uint32_t grid1 = (uint32_t) std::min<uint64_t>(S1_GRID_MAX, oversize ? (need + 4 * S1_ITEMS - 1) / (4 * S1_ITEMS) : (count + 63) / 64);
    if (oversize) c->kclock.count("part_scatter1_pieces", grid1);
    {
        const unsigned grid = (grid1 + 1) / 2;
        const bool full = g.nb <= HIST_MAX_BUCKETS;
        // 32-bit keys (k <= 32): at most 2^15 buckets, the LDS histogram always covers them all (FULL); 64-bit keys: never.
        // Only those six instantiations exist (tests/test_gpu_zz_dispatch_coverage.py checks that each is reached).
        if (full == wide) return fail("internal error: histogram geometry (k = %d, %u buckets)", c->k, g.nb);
        const void *fn = with_key(c->k, [&](auto key) {
            return with_value<0, 1, 2>(mode, [&](auto m) { return (const void *) part_hist_kernel<decltype(key), m, sizeof key == 4>; });
        });
        for (uint32_t b_lo = 0; b_lo < g.nb; b_lo += HIST_MAX_BUCKETS) {
            const uint32_t n_b = std::min<uint32_t>(HIST_MAX_BUCKETS, g.nb - b_lo);
            const size_t lds = ((size_t) n_b + 2 * HIST_NT + 24) * 4 + (size_t) HIST_NT * 8;
            HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
            ReadsView rv = rs->view();
            const uint32_t *kc = rs->d_kcnt;
            uint32_t *hist = ws.hist, *bcnt = ws.blockcnt;
            uint32_t nblk = grid1;
            void *args[] = {&rv, &kc, &d_sel, &first, &count, &g, &b_lo, (void *) &n_b, &hist, &nblk, &bcnt, &d_ids, &d_items, &d_nitems};
            KScope ks(c, "part_hist_kernel", stream);
            note_launch(fn);
            HIP_OK(hipLaunchKernel(fn, dim3(grid), dim3(HIST_NT), args, lds, stream));
        }
    }
    {
        const bool lds_hist = (size_t) g.nb * 4 <= (128u << 10);   // stage the histogram in LDS (coalesced loads) when it fits
        const size_t lds = lds_hist ? ((size_t) g.nb + g.nb / 32 + 1) * 4 : 0;   // (padded: see the kernel)
        if (lds) HIP_OK(hipFuncSetAttribute((const void *) part_scan_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
        KScope ks(c, "part_scan_kernel", stream);
        COMMET_LAUNCH(part_scan_kernel, dim3(1), dim3(1024), lds, stream, ws.hist, g, zero_fill ? 1 : 0, ws.off,
                           ws.cur2, ws.wl, ws.goff, lds_hist ? 1 : 0);
    }
    HIP_OK(hipGetLastError());
    {
        KScope ks(c, "part_blockoff_kernel", stream);
        COMMET_LAUNCH(part_blockoff_kernel, dim3(g.nb1), dim3(512), 0, stream, ws.blockcnt, ws.off, g, grid1,
                           ws.blockoff);
    }
    HIP_OK(hipGetLastError());
    // scatter 1 (straight into the final buckets when there is a single level)
    uint32_t *level1_out = g.b2 ? ws.bufA : ws.bufB;
    {
        const void *fn = with_key(c->k, [&](auto key) {
            return with_value<0, 1, 2>(mode, [&](auto m) { return (const void *) part_scatter1_kernel<decltype(key), m>; });
        });
        ReadsView rv = rs->view();
        const uint32_t *kc = rs->d_kcnt;
        const unsigned long long *boff = ws.blockoff;
        void *args[] = {&rv, &kc, &d_sel, &first, &count, &g, &boff, &level1_out, &d_ids, &d_items, &d_nitems};
        KScope ks(c, "part_scatter1_kernel", stream);
        note_launch(fn);
        HIP_OK(hipLaunchKernel(fn, dim3(grid1), dim3(S1_NT), args, 0, stream));
    }
    // Two lanes, staggered: the chunk on the second lane starts when this one's scatter1 is through, so that its hist and
    // scatter1 (VALU, LDS atomics, a write pattern) run beside this chunk's scatter2 and build (HBM streams) instead of beside
    // the same phases of this chunk.  Four boxes, configs[1], per step: -0.36, -0.25, 0.0 and +0.04 ms (the slower the box's
    // draw, the more); a 2 x 50 M-read pair 169.4 -> 168.1 ms.  Staggering behind hist instead: +0.5 ms.
    if (lane == 0) {
        HIP_OK(hipEventRecord(c->ev_stagger, stream));
        c->stagger_armed = true;
    }
    if (g.b2) {
        const uint64_t grid = (total + S2_KEYS - 1) / S2_KEYS;
        if (grid >= (1ull << 24)) return fail("scatter launch too large");
        {
            KScope ks(c, (g.packed && (1u << g.b2) <= S2P_MAX_SUB) ? "part_scatter2_packed_kernel" : "part_scatter2_kernel", stream);
            if (g.packed && (1u << g.b2) <= S2P_MAX_SUB)
                COMMET_LAUNCH(part_scatter2_packed_kernel, dim3((unsigned) grid), dim3(S2_NT), 0, stream, ws.bufA, (uint2 *) ws.bufB,
                                   ws.off, g, ws.cur2, total);
            else
                COMMET_LAUNCH(part_scatter2_kernel, dim3((unsigned) grid), dim3(S2_NT), 0, stream, ws.bufA, ws.bufB,
                                   ws.off, g, ws.cur2, total);
        }
        HIP_OK(hipGetLastError());
    }
    {
        const uint64_t grid = (uint64_t) g.nb + total / BUILD_CAP + 1;
        if (grid >= (1ull << 24)) return fail("build launch too large");
        if (zero_fill) {   // no memset happened: clear the tiles that several workgroups OR into
            KScope ks(c, "part_zero_split_kernel", stream);
            COMMET_LAUNCH(part_zero_split_kernel, dim3(g.nb), dim3(256), 0, stream, ws.wl, g, slot);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(hipFuncSetAttribute((const void *) part_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int) (TILE_WORDS * sizeof(uint32_t))));
        {
            KScope ks(c, "part_build_kernel", stream);
            COMMET_LAUNCH(part_build_kernel, dim3((unsigned) grid), dim3(BUILD_NT), TILE_WORDS * sizeof(uint32_t), stream,
                               ws.bufB, g.packed ? ws.goff : ws.off, ws.wl, g, slot, additive ? 1 : 0, ws.cur2);
        }
        HIP_OK(hipGetLastError());
    }
    return 0;
}

// whether a launch of `kmers` complete k-mers over `count` reads takes the bucketed construction (every caller that prepares for one
// — lanes, slots that need no zeroing, shared passes — asks here, and launch_index decides by the same call)
bool would_partition(const commet_ctx *c, const commet_readset *rs, uint64_t kmers, uint64_t count)
{
    if (kmers == ~0ull || kmers == 0 || c->index_mode == 1) return false;
    if (!partition_eligible(c, rs, count)) return false;
    if (c->index_mode == 2) return true;
    // auto: sets with oversize reads follow the rule of the others only where the A/B against index_kernel says so (MEASUREMENTS.md,
    // "Long reads: the bucketed index")
    return (LONG_INDEX_AUTO || !oversize_reads(rs)) && kmers >= c->part_min_kmers;
}

// kmers: exact complete-k-mer count of the launch when known (enables the bucketed path), else ~0.
// fresh_filter: the filter holds nothing yet; filter_zeroed: the caller has zeroed it (if not, a bucketed build
// zero-fills what it does not set; the atomic kernel always needs a zeroed filter).
int launch_index(commet_ctx *c, const commet_readset *rs, uint64_t first, uint64_t count, const uint64_t *d_sel,
                 unsigned long long *d_fed, uint64_t kmers = ~0ull, bool fresh_filter = false, bool filter_zeroed = true,
                 int lane = 0, const uint32_t *d_ids = nullptr, uint64_t pos_first = 0, uint64_t pos_count = 0)
{
    const bool oversize = oversize_reads(rs);
    if (c->index_mode == 2) {
        if (!partition_geometry_ok(c)) return fail("bucketed index construction needs 20 <= k <= 34");
        if (kmers == ~0ull) return fail("bucketed index construction needs the k-mer count of the launch");
        if (!partition_eligible(c, rs, count))
            return fail("bucketed index construction needs the item list for sets with reads of more than %u k-mers (part_list = 0, part_no_uni = 0, "
                        "a chunk of fewer than 2^28 words and 2^32 items)", S1_KEYS / 4);
    }
    bool part = would_partition(c, rs, kmers, count);
    // oversize reads: the last thing the item path needs is room for the list — asked for here, before the launch commits to a path
    if (part && oversize && count && !ensure_item_buffers(c, c->part[lane], lane ? c->aux_stream : c->stream,
                                                          items_bound_of(rs, pos_count ? pos_count : count), (count + ITEMS_BLOCK - 1) / ITEMS_BLOCK)) {
        if (c->index_mode == 2) return fail("bucketed index construction needs memory for the item list of the chunk");
        part = false;
        if (!filter_zeroed) {     // the caller counted on a build that writes every tile: the atomic kernel must meet a zeroed filter
            if (!fresh_filter) return fail("internal error: atomic index launch on a filter that was not zeroed");
            if (commet_filter_reset(c)) return 1;
            filter_zeroed = true;
        }
    }
    if (!part) {
        if (!filter_zeroed) return fail("internal error: atomic index launch on a filter that was not zeroed");
        return launch_index_atomic(c, rs, first, count, d_sel, d_fed);
    }
    if (d_fed) {
        // the count is known exactly on the host
        const unsigned long long v = kmers;
        HIP_OK(hipMemcpyAsync(d_fed, &v, sizeof v, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    return launch_index_partitioned(c, rs, first, count, d_sel, kmers, !fresh_filter, fresh_filter && !filter_zeroed, lane, d_ids, pos_first,
                                    pos_count);
}

}  // namespace
