// hit_profile.hpp — hits_kernel and hits_wave_kernel: the search that does not stop at t (commet_index_and_profile, capi/profile.hpp).
//
// A job answers "does the read have t non-overlapping k-mers in the filter" and stops a read's scan at its t-th hit; everything in
// the search kernels is built around that stop (first-hit windows, masks sized by t, query lists per (k, t), the `dead` pruning).
// But t only decides WHEN the reference stops (search_reads.h:45-83): hash.clear() after a full hit is unconditional, so the sequence
// of accepted hits on a strand is the same for every t.  With F = the greedy non-overlapping full hits over the whole forward strand
// and R = the same for the reverse complement, a read is found in one filter at threshold t iff max(F, R) >= t.  These kernels
// compute min(max_hits, max(F, R)) for one chunk filter and fold it into the read's byte with max: the byte then answers every t in
// 1..max_hits at once.
//
// Both strands in ONE walk over the read's windows: plane A is stored strand-paired (kernels.hpp, psi_a), so the load at
// psi_a(forward key) returns the reverse-complement key's lane-a bit as well (bit ^ 1; the bit itself when the key is its own
// partner; k == 1 is not paired: two loads).  Two greedy states, (free, cnt) per strand: a strand considers a window iff its k bases
// are ACGT and it starts at or after that strand's `free`; a lane-a candidate probes B, C, D with that strand's keys; a full hit is
// cnt++, free = start + k.  The walk ends when either strand has max_hits: the result is saturated.
//
// hits[r] = max(hits[r], h) with a plain load and store: a lane (a wave's lane 0) owns its read, and the passes over the chunk
// filters are ordered on the context's stream.  A read whose byte is max_hits on entry is skipped (exact: nothing can raise it).
// `walked` (optional) counts the reads a pass did walk.
//
// Included by capi.hip behind long_search.hpp (KeyCtx, ItemWords, psi_a, probe_bcd_chain, search_lane, count_walked, LONG_WG,
// wave_block_words, greedy_take); not meant to stand alone.
#pragma once

namespace commet {

// the lane-a bits of a window for both strands: one load where plane A is paired
template <typename W>
__device__ __forceinline__ void hits_lane_a(const uint32_t *__restrict__ plane_a, W kaf, W kar, int k, bool want_f, bool want_r, bool &af, bool &ar)
{
    if (k >= 2) {
        bool selfp;
        const W addr = psi_a<W>(kaf, k, selfp);
        const uint32_t fw = plane_a[addr >> 5];
        const uint32_t bit = (uint32_t) addr & 31u;
        af = (fw >> bit) & 1u;
        ar = selfp ? af : (bool) ((fw >> (bit ^ 1u)) & 1u);
    } else {
        af = want_f && test_bit<W>(plane_a, kaf);
        ar = want_r && test_bit<W>(plane_a, kar);
    }
}

// ---------------------------------------------------------------------------
// a lane per read (sel / ActiveList as in search_kernel; no tags: a profile never skips a read for an earlier chunk's answer)
// ---------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(256) COMMET_SGPRS void hits_kernel(ReadsView rv, FilterView f, int k, int max_hits, const uint64_t *__restrict__ sel,
                                                                uint8_t *__restrict__ hits, unsigned long long *__restrict__ walked, ActiveList al)
{
    const SearchLane me = search_lane(rv, al, sel, nullptr);
    const uint64_t r = me.r;
    int before = 0;
    bool walk = false;
    if (me.active) {
        before = (int) hits[r];
        walk = before < max_hits;
    }
    if (walk) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const KeyCtx<W> kc(k);
        const PlanesBCD bcd{f.b, f.c, f.d};
        W wh = 0, wl = 0;
        uint32_t run = 0;
        int free_f = 0, free_r = 0, cnt_f = 0, cnt_r = 0;
        bool done = false;
        for (uint32_t w = 0; w * 32u < len && !done; ++w) {
            const uint32_t hi = p[3 * w], lo = p[3 * w + 1], va = p[3 * w + 2];
            const uint32_t nb = min(32u, len - w * 32u);
            for (uint32_t j = 0; j < nb && !done; ++j) {
                wh = (wh >> 1) | ((W) ((hi >> j) & 1u) << (k - 1));
                wl = (wl >> 1) | ((W) ((lo >> j) & 1u) << (k - 1));
                run = ((va >> j) & 1u) ? run + 1 : 0;
                if (run < (uint32_t) k) continue;
                const int start = (int) (32u * w + j) - (k - 1);
                const bool want_f = start >= free_f, want_r = start >= free_r;
                if (!want_f && !want_r) continue;
                W kaf, kbf, kar, kbr;
                kc.strand_keys(wh, wl, 0, kaf, kbf);
                kc.strand_keys(wh, wl, 1, kar, kbr);
                bool af, ar;
                hits_lane_a<W>(f.a, kaf, kar, k, want_f, want_r, af, ar);
                if (want_f && af && probe_bcd_chain<W>(bcd, kaf, kbf)) {
                    ++cnt_f;
                    free_f = start + k;
                }
                if (want_r && ar && probe_bcd_chain<W>(bcd, kar, kbr)) {
                    ++cnt_r;
                    free_r = start + k;
                }
                done = cnt_f >= max_hits || cnt_r >= max_hits;
            }
        }
        const int h = min(max_hits, max(cnt_f, cnt_r));
        if (h > before) hits[r] = (uint8_t) h;
    }
    count_walked(walked, walk);
}

// ---------------------------------------------------------------------------
// a wave per read, for sets of long reads (the block structure of search_long_kernel: 64 consecutive windows per block, lane = window
// start - block start, the read's words staged one per lane and handed out by shuffles).  Per block one plane-A load per lane serves
// both strands; B, C, D for the candidates that start at or after next_free of their strand; one ballot of full hits per strand,
// walked greedily by the whole wave: lowest set bit at or after next_free, count it, next_free = its start + k.  (next_free, count)
// of both strands are carried from block to block (a hit in the last windows of block b forbids the first windows of block b + 1);
// windows probed behind a hit of the same block are dropped by the walk.  Persistent grid: wave w takes items w, w + waves, ...
// ---------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(LONG_WG) void hits_wave_kernel(ReadsView rv, FilterView f, int k, int max_hits, const uint64_t *__restrict__ sel,
                                                            uint8_t *__restrict__ hits, unsigned long long *__restrict__ walked, ActiveList al)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const uint64_t n_items = al.ids ? (uint64_t) *al.n : rv.n;
    const KeyCtx<W> kc(k);
    const PlanesBCD bcd{f.b, f.c, f.d};
    unsigned long long n_walked = 0;

    for (uint64_t item = wave0; item < n_items; item += n_waves) {   // (uniform per wave)
        uint64_t r = item;
        if (al.ids) r = (uint64_t) al.ids[item];
        else if (sel && !((sel[r >> 6] >> (r & 63ull)) & 1ull)) continue;
        const int before = (int) hits[r];
        if (before >= max_hits) continue;
        ++n_walked;
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int next_free[2] = {0, 0}, count[2] = {0, 0};      // [strand]
        for (int base = 0; base < n_win && count[0] < max_hits && count[1] < max_hits; base += 64) {
            const int s = base + lane, q = s + k - 1;
            ItemWords<W> it;
            wave_block_words<W>(p, n_words, base, lane, q, it);   // (every lane)
            W wh, wl;
            const bool valid = it.window((uint32_t) q & 31u, k, kc.mask, wh, wl) && s < n_win;
            const bool want_f = valid && s >= next_free[0], want_r = valid && s >= next_free[1];
            W kaf, kbf, kar, kbr;
            kc.strand_keys(wh, wl, 0, kaf, kbf);
            kc.strand_keys(wh, wl, 1, kar, kbr);
            bool af = false, ar = false;
            if (want_f || want_r) hits_lane_a<W>(f.a, kaf, kar, k, want_f, want_r, af, ar);
            const bool full_f = want_f && af && probe_bcd_chain<W>(bcd, kaf, kbf);
            const bool full_r = want_r && ar && probe_bcd_chain<W>(bcd, kar, kbr);
            const uint64_t full[2] = {__ballot(full_f), __ballot(full_r)};
#pragma unroll
            for (int strand = 0; strand < 2; ++strand) greedy_take(full[strand], base, k, max_hits, next_free[strand], count[strand]);   // (by the whole wave)
        }
        const int h = min(max_hits, max(count[0], count[1]));
        if (lane == 0 && h > before) hits[r] = (uint8_t) h;
    }
    if (walked && lane == 0 && n_walked) atomicAdd(walked, n_walked);
}

}  // namespace commet
