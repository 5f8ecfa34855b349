// hit_profile_tiled.hpp — tq_hits_replay_kernel: the hit profile of a large set at 25 <= k <= 34 through the tiled probe.
//
// hits_kernel (hit_profile.hpp) makes one plane-A request per window of a read, each of them an L2 miss: 0.90 of the chip's
// random-request ceiling and no way past it.  The tiled search (tile_search.hpp) serves the same requests from L2, slice by slice,
// out of a query list that depends on (k, t) alone.  The list of a set at (k, t = 1) holds EVERY complete window of every read
// (tq_for_each_window: pe = len - 1), so after tq_probe_kernel — unchanged — and the sweep of planes B, C, D the replay's LDS masks
// hold all full hits of both strands of both filters, and max(F, R) of hit_profile.hpp is a greedy count over mask words: no tail,
// no `dead` pruning, no tags.  Steps (1) and (2) are the tiled replay's own (tq_collect, tq_sweep: tile_search.hpp); step (3) here is that count.
//
// Included by capi.hip behind tile_search.hpp and hit_profile.hpp; not meant to stand alone.
#pragma once

namespace commet {

// The greedy count of one strand over a word of full hits (or of lane-a candidates, is_hit probing B, C, D): bit b = the window that
// STARTS at start_of_bit0 + b; a window counts iff it starts at or after `free`, then free = start + k (hits_kernel's rule; the twin
// of StrandScan::walk, which closes at t and prunes by the room left — a count has neither).  Stops at max_hits.
struct HitCount {
    int cnt = 0, free = 0;
    template <typename F> __device__ __forceinline__ void walk(uint32_t m, int start_of_bit0, int k, int max_hits, F &&is_hit)
    {
        while (m && cnt < max_hits) {
            const int s = start_of_bit0 + (__ffs((int) m) - 1);
            m &= m - 1u;
            if (s < free) continue;                    // overlaps the last hit
            if (!is_hit(s)) continue;
            ++cnt;
            free = s + k;
        }
    }
};

// one workgroup per piece of 256 reads, one thread per read (launch bounds, scalar cap and LDS as tq_replay_kernel's)
template <typename W, int GS, int MW>
__global__ __launch_bounds__(TQ_PIECE) COMMET_SGPRS void tq_hits_replay_kernel(ReadsView rv, QueryListView ql, const uint8_t *__restrict__ qres,
                                                                               FilterGroupView fg, int k, int max_hits,
                                                                               const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits_out,
                                                                               unsigned long long *__restrict__ walked, uint32_t hit_cap)
{
    __shared__ uint32_t masks[GS * 2 * MW * TQ_PIECE];   // [chunk][strand][word][read]
    __shared__ uint32_t hits[TQ_HIT_CAP];
    __shared__ uint32_t rd_ext[TQ_PIECE];
    __shared__ unsigned int wg_walked;
    constexpr int NS = 2 * GS;                           // scan index = chunk * 2 + strand
    tq_collect<GS, MW>(ql, qres, blockIdx.x, masks);
    if (threadIdx.x == 0) wg_walked = 0;                 // (before the sweep's barriers)
    static_assert(TQ_PIECE == 256, "search_lane is written for workgroups of 256 threads");
    const ActiveList no_list{nullptr, nullptr};
    const SearchLane me = search_lane(rv, no_list, sel, nullptr);        // thread x of piece p has read 256 p + x; no tags
    const uint64_t r = me.r;
    // active: selected and not saturated on entry (nothing can raise a byte that is max_hits)
    int before = 0;
    if (me.active) before = (int) hits_out[r];
    const bool active = me.active && before < max_hits;
    const KeyCtx<W> kc(k);
    TqSwept<GS, MW> sw;
    tq_sweep<W, GS, MW>(rv, fg, kc, k, r, active, hit_cap, masks, hits, rd_ext, sw);
    // (3) per filter and strand the greedy count over the mask words; the read's byte is the largest of them.  The list covers every
    // window of the read: nothing lies behind the masks.
    int best = 0;
    if (active) {
        const uint32_t *p = rv.planes + 3 * sw.t0;
        for (int i = 0; i < NS && best < max_hits; ++i) {
            const int strand = i & 1;
            const uint32_t *pb = fg.slot0 + (uint64_t) (i >> 1) * (4 * fg.plane_words) + fg.plane_words;
            const PlanesBCD f{pb, pb + fg.plane_words, pb + 2 * fg.plane_words};
            const bool hscan = ((sw.hv >> i) & 1u) || sw.all_self;
            HitCount hc;
            for (int h = 0; h < MW && hc.cnt < max_hits; ++h)
                hc.walk(tq_walk_word(masks, sw, i, h, hscan), 32 * h, k, max_hits, [&](int s) -> bool {
                    if (!hscan) return true;
                    W ka, kb;
                    (void) kc.window_keys(p, s + k - 1, strand, ka, kb);
                    return probe_bcd_together<W>(f, ka, kb);
                });
            best = max(best, hc.cnt);
        }
        const int h = min(max_hits, best);
        if (h > before) hits_out[r] = (uint8_t) h;       // plain load and store: this thread owns its read, the passes are ordered on the stream
    }
    if (walked) add_walked(walked, active, wg_walked);
}

}  // namespace commet
