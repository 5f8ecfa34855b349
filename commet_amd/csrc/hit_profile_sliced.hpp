// hit_profile_sliced.hpp — hits_sliced_kernel: the hit profile (hit_profile.hpp) through the narrow bit-sliced tables (slice_search.hpp).
//
// A job of up to 256 chunk filters at 12 <= k <= 24 scans a search set once per table set of 32 * GW chunks (search_sliced_kernel); the
// slot kernels of the profile scan it once per eight chunks.  Here the profile reads the same tables in the same way: a lane per read,
// entry T_p[key * GW + (c >> 5)] bit (c & 31), plane A at psi_a addresses, for GW <= 2 one load of 2 * GW words for both strands.
// The kernel writes hits[r] = max(hits[r], min(cap, max over the pass's chunks c < g of max(F_c, R_c))), cap = min(max_hits, len / k),
// F_c / R_c = the reference's greedy non-overlapping full four-lane hits of the forward / reverse-complement strand in chunk c
// (search_reads.h:45-83 run to the end of the read): the quantity hits_kernel computes, one filter at a time.
//
//   (1) row pass over EVERY complete window (a profile has no t: no `pe`, no `lim`), both strands: search_sliced_kernel's entry test
//       (slice_window_masks), so a set bit is a FULL hit of that window in that chunk.  Window end positions are cut into blocks of k
//       (roll_blocks); per chunk bit and strand a 2-bit saturating counter of the blocks that hold a hit (wide_fold on every word of a
//       SliceWord): 4 * GW registers, and 2 * GW for the open block.
//   (2) the counters bound the greedy count from BOTH sides.  Hits inside one block end fewer than k positions apart, so they overlap
//       pairwise; hits in blocks i and i + 2 end more than k apart, so they do not; and the greedy scan takes the largest set of
//       non-overlapping hits.  Hence
//           counter 1: exactly 1        counter 2: 1 or 2        counter 3 (saturated: three blocks or more): at least 2.
//       best starts at max(the byte in hits[r], min(cap, the largest lower bound)).  A counter of 1 never needs a replay, a counter of
//       2 only while best < 2, a saturated one while best < cap.  The replay of one chunk and strand is search_sliced_kernel's
//       single-bit walk (slice_strand_count) without pruning: it counts to the end of the strand, or to where its bound or cap stops it.  Saturated
//       counters first (the higher bound), then the counters of 2; max is order-free, so the order decides speed only.
//
// Columns at or past g are masked out of the counters: they are never read as chunks.  A read that is not selected, has fewer than k
// bases or stands at cap already makes no table request.  `walked` (optional) counts the reads the pass did walk.  No early return:
// every thread reaches the barrier of add_walked.
#pragma once

#include "slice_search.hpp"

namespace commet {

template <int GW>
__device__ __forceinline__ void slice_fold(SliceWord<GW> &cur, SliceWord<GW> &c0, SliceWord<GW> &c1)
{
#pragma unroll
    for (int i = 0; i < GW; ++i) wide_fold(cur.x[i], c0.x[i], c1.x[i]);
}

template <int GW>
__global__ __launch_bounds__(256) void hits_sliced_kernel(ReadsView rv, const uint32_t *__restrict__ tables, int k, int max_hits, int g,
                                                          const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                          unsigned long long *__restrict__ walked)
{
    const uint64_t r = (uint64_t) blockIdx.x * 256ull + threadIdx.x;
    bool active = r < rv.n;
    if (active && sel) active = (sel[r >> 6] >> (r & 63)) & 1ull;
    const SlicePlanes T(tables, k, GW);
    uint64_t t0 = 0;
    uint32_t len = 0;
    int before = 0;
    if (active) {
        read_extent(rv, r, t0, len);
        before = (int) hits[r];
    }
    const int cap = min(max_hits, (int) (len / (uint32_t) k));
    const bool walk = active && before < cap;             // (a read of fewer than k bases has cap 0)
    if (walk) {
        const uint32_t *p = rv.planes + 3 * t0;
        const int last = (int) len - 1;
        SliceWord<GW> f0, f1, r0, r1;                     // blocks with a hit per chunk bit: 2-bit counters (f1 f0), (r1 r0)
        f0.clear(), f1.clear(), r0.clear(), r1.clear();
        // (1) row pass over all windows
        {
            SliceWord<GW> cur_f, cur_r;
            cur_f.clear(), cur_r.clear();
            roll_blocks(
                p, bases_to(last), k,
                [&](uint32_t wh, uint32_t wl) {
                    SliceWord<GW> mf, mr;
                    const int reached = slice_window_masks<GW>(T, k, wh, wl, mf, mr);
                    if (reached & 1) {
#pragma unroll
                        for (int i = 0; i < GW; ++i) cur_f.x[i] |= mf.x[i];
                    }
                    if (reached & 2) {
#pragma unroll
                        for (int i = 0; i < GW; ++i) cur_r.x[i] |= mr.x[i];
                    }
                },
                [&]() { slice_fold(cur_f, f0, f1), slice_fold(cur_r, r0, r1); });
        }
        // columns at or past g are no chunks of this pass
        uint32_t any1 = 0, any3 = 0;
#pragma unroll
        for (int i = 0; i < GW; ++i) {
            const int left = g - 32 * i;
            const uint32_t gm = left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << left) - 1u : 0u;
            f0.x[i] &= gm, f1.x[i] &= gm, r0.x[i] &= gm, r1.x[i] &= gm;
            any1 |= f0.x[i] | f1.x[i] | r0.x[i] | r1.x[i];
            any3 |= (f0.x[i] & f1.x[i]) | (r0.x[i] & r1.x[i]);
        }
        // (2) the lower bounds, then the exact replay of the counters whose upper bound exceeds best: the saturated ones while
        // best < cap, the counters of 2 while best < 2 (cap >= 2 then: best >= 1 from the lower bound, and best < cap)
        int best = max(before, min(cap, any3 ? 2 : any1 ? 1 : 0));
#pragma unroll 1
        for (int want = 3; want >= 2; --want) {
            const int stop = want == 3 ? cap : min(cap, 2);
#pragma unroll 1
            for (int cw = 0; cw < GW && best < stop; ++cw) {
                const uint32_t a0 = slice_pick<GW>(f0, cw), a1 = slice_pick<GW>(f1, cw), b0 = slice_pick<GW>(r0, cw), b1 = slice_pick<GW>(r1, cw);
                const uint32_t mfw = want == 3 ? (a0 & a1) : (a1 & ~a0), mrw = want == 3 ? (b0 & b1) : (b1 & ~b0);
                uint32_t m = mfw | mrw;
                while (m && best < stop) {
                    const int cb = __ffs((int) m) - 1;
                    m &= m - 1u;
                    for (int strand = 0; strand < 2 && best < stop; ++strand) {
                        if (!(((strand ? mrw : mfw) >> cb) & 1u)) continue;
                        best = max(best, slice_strand_count<GW, false>(p, last, T, k, cw, cb, strand, stop));
                    }
                }
            }
        }
        if (best > before) hits[r] = (uint8_t) best;
    }
    count_walked(walked, walk);
}

}  // namespace commet
