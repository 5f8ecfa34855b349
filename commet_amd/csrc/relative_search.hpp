// relative_search.hpp — the search with a threshold PER READ, a share of what the read can hold (commet_index_and_search_relative,
// capi/relative.hpp): rel_thresholds_kernel makes the thresholds, rel_kernel / rel_wave_kernel / rel_group_kernel /
// rel_group_wave_kernel are the four hits forms of hit_profile.hpp and hit_profile_group.hpp with the read's own stop.
//
// The rule (include/commet_hip.h states it; rel_threshold below is its one implementation): for a read of len bases, every character
// counted, W_r = len / k, t_r = max(min_hits, (percent * W_r + 99) / 100), min_hits < 1 as 1.  The read is found in one chunk filter
// iff max(F, R) >= t_r, F and R the greedy non-overlapping full hits of the two strands as hit_profile.hpp defines them; tags are ORed
// over chunks, counts are never summed over chunks.  A read with t_r > W_r can never be found: its threshold is stored as 0 and no
// pass walks it.
//
// Per read, in every form: cap = thr[r]; a read with cap == 0 (never found, or not selected) or found[r] != 0 (an earlier pass) is
// skipped and not counted in `walked`; the walk stops as soon as any filter's count on any strand reaches cap, and found[r] = 1 iff
// that happened: a plain byte store by the lane (the wave's lane 0) that owns the read.  The found bytes then go through
// hits_tags_kernel with t = 1 (hits_tags.hpp): tags and per-file counts are made on the device.
//
// The group forms ARE the bodies of the hits kernels under their compile-time switch REL (hits_lanes, hit_profile_wave_body.hpp:
// max_hits becomes the read's cap, the byte fold becomes the found flag; every instantiation without REL is what it was).  The lane
// group body keeps its counts as bytes of one word: it serves sets whose largest t_r is at most 255, the host sends the others
// elsewhere.  The one-filter forms are kernels, not bodies, in hit_profile.hpp, so their walks are written again here; they and the
// wave forms count in int and take any t_r (16 bits).
//
// Open: no tiled probe, no wide rows, no narrow tables, no passes shared between jobs for this call.
//
// Included by capi.hip behind hit_profile_group.hpp (hits_lane_a, hits_lanes, the wave body, and everything those include lists
// name); not meant to stand alone.
#pragma once

namespace commet {

// t_r of a read of len bases; 0 where t_r > W_r.  (percent in 1..100 and W_r <= 65535 are the host's checks: the product fits)
__host__ __device__ __forceinline__ uint32_t rel_threshold(uint32_t len, int k, int percent, int min_hits)
{
    const uint32_t w = len / (uint32_t) k;
    const uint32_t share = ((uint32_t) percent * w + 99u) / 100u;
    const uint32_t least = min_hits < 1 ? 1u : (uint32_t) min_hits;
    const uint32_t t = share > least ? share : least;
    return t > w ? 0u : t;
}

// a lane per read, streaming: thr[r] = t_r, 0 for a read no pass needs to walk (t_r > W_r, or not selected)
__global__ __launch_bounds__(256) void rel_thresholds_kernel(ReadsView rv, int k, int percent, int min_hits, const uint64_t *__restrict__ sel,
                                                            uint16_t *__restrict__ thr)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256ull + threadIdx.x;
    if (r >= rv.n) return;
    uint64_t t0;
    uint32_t len;
    read_extent(rv, r, t0, len);
    const bool selected = !sel || ((sel[r >> 6] >> (r & 63ull)) & 1ull);
    thr[r] = selected ? (uint16_t) rel_threshold(len, k, percent, min_hits) : (uint16_t) 0;
}

// ---------------------------------------------------------------------------
// one filter, a lane per read: the walk of hits_kernel, counts in int
// ---------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(256) COMMET_SGPRS void rel_kernel(ReadsView rv, FilterView f, int k, const uint16_t *__restrict__ thr,
                                                               const uint64_t *__restrict__ sel, uint8_t *__restrict__ found,
                                                               unsigned long long *__restrict__ walked, ActiveList al)
{
    const SearchLane me = search_lane(rv, al, sel, nullptr);
    const uint64_t r = me.r;
    int cap = 0;
    bool walk = false;
    if (me.active) {
        cap = (int) thr[r];
        walk = cap != 0 && found[r] == 0;
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
                done = cnt_f >= cap || cnt_r >= cap;
            }
        }
        if (done) found[r] = 1;
    }
    count_walked(walked, walk);
}

// ---------------------------------------------------------------------------
// one filter, a wave per read: the blocks of hits_wave_kernel; cap is uniform over the wave
// ---------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(LONG_WG) void rel_wave_kernel(ReadsView rv, FilterView f, int k, const uint16_t *__restrict__ thr,
                                                           const uint64_t *__restrict__ sel, uint8_t *__restrict__ found,
                                                           unsigned long long *__restrict__ walked, ActiveList al)
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
        const int cap = __builtin_amdgcn_readfirstlane((int) thr[r]);
        if (cap == 0 || found[r] != 0) continue;
        ++n_walked;
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int next_free[2] = {0, 0}, count[2] = {0, 0};      // [strand]
        for (int base = 0; base < n_win && count[0] < cap && count[1] < cap; base += 64) {
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
            for (int strand = 0; strand < 2; ++strand) greedy_take(full[strand], base, k, cap, next_free[strand], count[strand]);   // (by the whole wave)
        }
        if (lane == 0 && (count[0] >= cap || count[1] >= cap)) found[r] = 1;
    }
    if (walked && lane == 0 && n_walked) atomicAdd(walked, n_walked);
}

// ---------------------------------------------------------------------------
// a group of filters: the bodies of hits_group_kernel and hits_group_wave_kernel under REL
// ---------------------------------------------------------------------------
template <typename W, int NF>
__global__ __launch_bounds__(256) COMMET_SGPRS void rel_group_kernel(ReadsView rv, FilterGroupView fg, int k, const uint16_t *__restrict__ thr,
                                                                     const uint64_t *__restrict__ sel, uint8_t *__restrict__ found,
                                                                     unsigned long long *__restrict__ walked, ActiveList al)
{
    hits_lanes<W, NF, false, true>(rv, fg, k, 0, JobSlots{0, 0}, sel, found, 0, walked, al, thr);
}

template <typename W, int NF>
__global__ __launch_bounds__(LONG_WG) void rel_group_wave_kernel(ReadsView rv, FilterGroupView fg, int k, const uint16_t *__restrict__ thr,
                                                                 const uint64_t *__restrict__ sel, uint8_t *__restrict__ found,
                                                                 unsigned long long *__restrict__ walked, ActiveList al)
{
    constexpr bool JOBS = false, REL = true;
    constexpr JobSlots js{0, 0};
    constexpr uint32_t lines = 0;
    constexpr int max_hits = 0;
    uint8_t *__restrict__ const hits = found;
#include "hit_profile_wave_body.hpp"
}

}  // namespace commet
