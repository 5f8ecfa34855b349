// hit_profile_tiled.hpp — tq_hits_replay_kernel: the hit profile of a large set at 25 <= k <= 34 through the tiled probe.
//
// hits_kernel (hit_profile.hpp) makes one plane-A request per window of a read, each of them an L2 miss: 0.90 of the chip's
// random-request ceiling and no way past it.  The tiled search (tile_search.hpp) serves the same requests from L2, slice by slice,
// out of a query list that depends on (k, t) alone.  The list of a set at (k, t = 1) holds EVERY complete window of every read
// (tq_for_each_window: pe = len - 1), so after tq_probe_kernel — unchanged — and the sweep of planes B, C, D the replay's LDS masks
// hold all full hits of both strands of both filters, and max(F, R) of hit_profile.hpp is a greedy count over mask words: no tail,
// no `dead` pruning, no tags.  This kernel is tq_replay_kernel with that count in the place of its step (3).
//
// Steps (1) and (2) below are COPIES of tq_replay_kernel's (tile_search.hpp): the twin is kept byte for byte as it was, its register
// counts and its time with it; a change to the collect loop or the balanced sweep there belongs here as well, and the other way round.
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

// one workgroup per piece of 256 reads, one thread per read (launch bounds, scalar cap and LDS as tq_replay_kernel's).  The group holds
// exactly GS filters (fg.g == GS: the host instantiates by g), and a slot is four planes (slot stride = 4 * fg.plane_words, as
// filter_group lays it out) — fg.g and fg.slot_words are not read: with them live the builds of two filters and two mask words kept
// scalar values in vector lanes under the 80-register cap; without, no build spills anything.
template <typename W, int GS, int MW>
__global__ __launch_bounds__(TQ_PIECE) COMMET_SGPRS void tq_hits_replay_kernel(ReadsView rv, QueryListView ql, const uint8_t *__restrict__ qres,
                                                                               FilterGroupView fg, int k, int max_hits,
                                                                               const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits_out,
                                                                               unsigned long long *__restrict__ walked, uint32_t hit_cap)
{
    const uint32_t piece = blockIdx.x;
    __shared__ uint32_t masks[GS * 2 * MW * TQ_PIECE];   // [chunk][strand][word][read]
    auto mask_at = [&](int c, int strand, int h, uint32_t rd) -> uint32_t & { return masks[(((c * 2 + strand) * MW) + h) * TQ_PIECE + rd]; };
    for (uint32_t i = threadIdx.x; i < GS * 2 * MW * TQ_PIECE; i += TQ_PIECE) masks[i] = 0;
    __syncthreads();
    // (1) the piece's results (tq_replay_kernel, step (1)): wave w takes slices w, w + 16, ... in batches of 64 tiles, the batch's
    // records as one flat list, TQ_COLLECT_U of them per lane in flight
    {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        constexpr uint32_t NWAVE = TQ_PIECE / 64;
        for (uint32_t s0 = wave; s0 < ql.n_slices; s0 += 64 * NWAVE) {
            const uint32_t sl = s0 + lane * NWAVE;                       // this lane's tile of the batch
            unsigned long long ta = 0, te = 0;
            if (sl < ql.n_slices) {
                ta = ql.tstart[(uint64_t) piece * ql.n_slices + sl];
                te = ta + ql.tlen[(uint64_t) piece * ql.n_slices + sl];
            }
            const uint32_t len = (uint32_t) (te - ta);
            uint32_t inc = len;                                           // inclusive prefix of the tile lengths over the lanes
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t x = __shfl_up(inc, o, 64);
                if ((int) lane >= o) inc += x;
            }
            const uint32_t total = __shfl(inc, 63, 64);
            for (uint32_t f0 = 0; f0 < total; f0 += 64 * TQ_COLLECT_U) {              // (uniform trip count: every lane takes part in the shuffles)
                unsigned long long ri[TQ_COLLECT_U];
                bool ok[TQ_COLLECT_U];
#pragma unroll
                for (int u = 0; u < TQ_COLLECT_U; ++u) {
                    const uint32_t f = f0 + 64u * (uint32_t) u + lane;
                    // tile of flat record f = number of lanes whose inclusive prefix is <= f (binary search over the 64 prefixes)
                    uint32_t lo = 0, hi = 64;
#pragma unroll
                    for (int step = 0; step < 7; ++step) {
                        const uint32_t mid = min((lo + hi) >> 1, 63u);
                        const uint32_t pm = __shfl(inc, (int) mid, 64);
                        if (lo < hi) {
                            if (pm <= f) lo = mid + 1;
                            else hi = mid;
                        }
                    }
                    const uint32_t src = min(lo, 63u);
                    const uint32_t before_raw = __shfl(inc, (int) (src ? src - 1 : 0), 64);
                    const unsigned long long tbase = __shfl((unsigned long long) ta, (int) src, 64);
                    ok[u] = f < total;
                    ri[u] = ok[u] ? tbase + (f - (src ? before_raw : 0u)) : 0ull;     // (record 0 exists whenever the batch has one)
                }
                uint32_t res[TQ_COLLECT_U], who[TQ_COLLECT_U];
#pragma unroll
                for (int u = 0; u < TQ_COLLECT_U; ++u) {
                    res[u] = __builtin_nontemporal_load(qres + ri[u]);
                    who[u] = __builtin_nontemporal_load(ql.qwho + ri[u]);
                }
#pragma unroll
                for (int u = 0; u < TQ_COLLECT_U; ++u) {
                    if (!ok[u] || !res[u]) continue;
                    const uint32_t rd = who[u] & 255u, win = who[u] >> 8;
                    if ((win >> 5) >= (uint32_t) MW) continue;            // (the host sizes MW by the set's longest read: never taken)
#pragma unroll
                    for (int c = 0; c < GS; ++c) {
                        if ((res[u] >> c) & 1u) atomicOr(&mask_at(c, 0, (int) (win >> 5), rd), 1u << (win & 31u));
                        if ((res[u] >> (GS + c)) & 1u) atomicOr(&mask_at(c, 1, (int) (win >> 5), rd), 1u << (win & 31u));
                    }
                }
            }
        }
    }
    __syncthreads();
    // (2) planes B, C, D for the lane-a candidates of the light scans, balanced over the workgroup (tq_replay_kernel, step (2)); the
    // full hits go to the bounded list and back into the masks
    __shared__ uint32_t hits[TQ_HIT_CAP];
    __shared__ uint32_t hit_n;
    __shared__ uint32_t rd_ext[TQ_PIECE];                // (first triple - the piece's first triple) | length << 16
    __shared__ unsigned long long piece_t0;
    __shared__ uint32_t pre[TQ_PIECE];
    __shared__ uint32_t scan_ws[TQ_PIECE / 64];
    __shared__ unsigned int wg_walked;
    constexpr int NS = 2 * GS;                           // scan index = chunk * 2 + strand
    auto word_at = [&](uint32_t *arr, int i, int h, uint32_t rd) -> uint32_t & { return arr[((i * MW) + h) * TQ_PIECE + rd]; };
    if (threadIdx.x == 0) hit_n = 0, wg_walked = 0;
    static_assert(TQ_PIECE == 256, "search_lane is written for workgroups of 256 threads");
    const ActiveList no_list{nullptr, nullptr};
    const SearchLane me = search_lane(rv, no_list, sel, nullptr);        // thread x of piece p has read 256 p + x; no tags
    const uint64_t r = me.r;
    // active: selected and not saturated on entry (nothing can raise a byte that is max_hits)
    int before = 0;
    if (me.active) before = (int) hits_out[r];
    const bool active = me.active && before < max_hits;
    uint64_t my_t0 = 0;
    uint32_t my_len = 0;
    if (r < rv.n) read_extent(rv, r, my_t0, my_len);
    if (threadIdx.x == 0) piece_t0 = my_t0;                          // (the piece's first read exists: the grid covers pieces of the set only)
    const KeyCtx<W> kc(k);
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int h = 0; h < MW; ++h)
            if (!active) word_at(masks, i, h, threadIdx.x) = 0;   // reads that are not walked have no candidates
    __syncthreads();
    rd_ext[threadIdx.x] = (r < rv.n) ? ((uint32_t) (my_t0 - piece_t0) & 0xFFFFu) | (my_len << 16) : 0u;   // (first read before the sweep's first barrier)
    // heavy scans (more than TQ_HEAVY lane-a candidates: a read that shares sequence with the index set) keep their candidates in
    // registers and their thread probes B, C, D itself in step (3), where saturation ends the walk; the read's other scans stay in the sweep
    constexpr uint32_t TQ_HEAVY = 20;
    uint32_t am[NS][MW];
    uint32_t hv = 0;                    // bit i: scan i is heavy
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        uint32_t n = 0;
#pragma unroll
        for (int h = 0; h < MW; ++h) am[i][h] = word_at(masks, i, h, threadIdx.x), n += __popc(am[i][h]);
        if (n > TQ_HEAVY) {
            hv |= 1u << i;
#pragma unroll
            for (int h = 0; h < MW; ++h) word_at(masks, i, h, threadIdx.x) = 0;   // (the sweep's first barrier comes before anyone else reads them)
        }
    }
    const uint32_t *const piece_planes = rv.planes + 3 * piece_t0;
    auto keys_of = [&](uint32_t owner, int strand, int q, W &ka, W &kb) {
        (void) kc.window_keys(piece_planes + 3u * (rd_ext[owner] & 0xFFFFu), q, strand, ka, kb);   // complete: only complete windows are in the list
    };
    {
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i)
#pragma unroll
            for (int h = 0; h < MW; ++h) cnt += __popc(word_at(masks, i, h, threadIdx.x));
        uint32_t total;
        const uint32_t ex = block_scan<TQ_PIECE>(cnt, scan_ws, &total);
        pre[threadIdx.x] = ex + cnt;                      // inclusive
        __syncthreads();
        constexpr int U = TQ_SWEEP_U;
        for (uint32_t f0 = threadIdx.x; f0 < total; f0 += U * TQ_PIECE) {
            uint32_t owner[U], bitn[U], fw[U], fbit[U];
            W ka[U], kb[U];
            int sc[U], hw[U];
            bool have[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t f = f0 + (uint32_t) u * TQ_PIECE;
                have[u] = f < total;
                owner[u] = 0, bitn[u] = 0, sc[u] = 0, hw[u] = 0;
                if (!have[u]) continue;
                uint32_t lo = 0, hi = TQ_PIECE - 1;       // first read whose inclusive prefix exceeds f
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (pre[mid] <= f) lo = mid + 1;
                    else hi = mid;
                }
                uint32_t local = f - (lo ? pre[lo - 1] : 0u), wd = 0;
                bool got = false;
#pragma unroll
                for (int i = 0; i < NS; ++i)
#pragma unroll
                    for (int h = 0; h < MW; ++h) {
                        if (got) continue;
                        const uint32_t x = word_at(masks, i, h, lo);
                        const uint32_t c = __popc(x);
                        if (local < c) sc[u] = i, hw[u] = h, wd = x, got = true;
                        else local -= c;
                    }
                for (uint32_t v = 0; v < local; ++v) wd &= wd - 1u;        // drop the `local` lowest set bits
                owner[u] = lo, bitn[u] = (uint32_t) __ffs((int) wd) - 1u;
                have[u] = got && wd != 0;                                  // (always: f < total)
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {                                  // keys: the owners' read words (L1 / L2)
                ka[u] = kb[u] = 0;
                if (have[u]) keys_of(owner[u], sc[u] & 1, (int) (32 * hw[u] + bitn[u]) + (k - 1), ka[u], kb[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {                                  // plane B: U probes in flight
                fw[u] = 0, fbit[u] = (uint32_t) kb[u] & 31u;
                if (have[u]) fw[u] = fg.slot0[(uint64_t) (sc[u] >> 1) * (4 * fg.plane_words) + fg.plane_words + (kb[u] >> 5)];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!have[u] || !((fw[u] >> fbit[u]) & 1u)) continue;
                // the one in nine that passes B goes through C and D at once
                const uint32_t *pc = fg.slot0 + (uint64_t) (sc[u] >> 1) * (4 * fg.plane_words) + 2 * fg.plane_words, *pd = pc + fg.plane_words;
                const W kx = ka[u] ^ kb[u], ko = ka[u] | kb[u];
                const uint32_t vc = pc[kx >> 5], vd = pd[ko >> 5];
                if ((vc >> ((uint32_t) kx & 31u)) & (vd >> ((uint32_t) ko & 31u)) & 1u) {
                    const uint32_t at = atomicAdd(&hit_n, 1u);
                    if (at < hit_cap) hits[at] = owner[u] | ((uint32_t) sc[u] << 8) | ((uint32_t) hw[u] << 12) | (bitn[u] << 16);
                }
            }
        }
        __syncthreads();
    }
    // (behind the sweep's last barrier: nobody reads the masks any more) the full hits into the masks array
#pragma unroll
    for (int i = 0; i < NS; ++i)
#pragma unroll
        for (int h = 0; h < MW; ++h) word_at(masks, i, h, threadIdx.x) = 0;
    __syncthreads();
    const uint32_t nh = hit_n;
    const bool all_self = nh > hit_cap;   // the list overflowed: every scan walks its own lane-a candidates (am[])
    for (uint32_t e = threadIdx.x; e < min(nh, hit_cap); e += TQ_PIECE) {
        const uint32_t x = hits[e];
        atomicOr(&word_at(masks, (int) ((x >> 8) & 15u), (int) ((x >> 12) & 15u), x & 255u), 1u << (x >> 16));
    }
    __syncthreads();
    // (3) per filter and strand the greedy count over the mask words; the read's byte is the largest of them.  The list covers every
    // window of the read: nothing lies behind the masks.
    int best = 0;
    if (active) {
        const uint32_t *p = rv.planes + 3 * my_t0;
        for (int i = 0; i < NS && best < max_hits; ++i) {
            const int strand = i & 1;
            const uint32_t *pb = fg.slot0 + (uint64_t) (i >> 1) * (4 * fg.plane_words) + fg.plane_words;
            const PlanesBCD f{pb, pb + fg.plane_words, pb + 2 * fg.plane_words};
            const bool hscan = ((hv >> i) & 1u) || all_self;
            HitCount hc;
            for (int h = 0; h < MW && hc.cnt < max_hits; ++h) {
                uint32_t m = masks[((i * MW) + h) * TQ_PIECE + threadIdx.x];    // light scans: full hits (step 2)
                if (hscan) {                                                     // heavy scans: lane-a candidates, probed here
                    m = 0;
#pragma unroll
                    for (int ii = 0; ii < NS; ++ii)
#pragma unroll
                        for (int hh = 0; hh < MW; ++hh)
                            if (ii == i && hh == h) m = am[ii][hh];
                }
                hc.walk(m, 32 * h, k, max_hits, [&](int s) -> bool {
                    if (!hscan) return true;
                    W ka, kb;
                    (void) kc.window_keys(p, s + k - 1, strand, ka, kb);
                    return probe_bcd_together<W>(f, ka, kb);
                });
            }
            best = max(best, hc.cnt);
        }
        const int h = min(max_hits, best);
        if (h > before) hits_out[r] = (uint8_t) h;       // plain load and store: this thread owns its read, the passes are ordered on the stream
    }
    if (walked) {
        // one add per workgroup (wg_walked was zeroed before the sweep's barriers)
        const uint64_t wb = __ballot(active);
        if ((threadIdx.x & 63) == 0 && wb) atomicAdd(&wg_walked, (unsigned int) __popcll(wb));
        __syncthreads();
        if (threadIdx.x == 0 && wg_walked) atomicAdd(walked, (unsigned long long) wg_walked);
    }
}

}  // namespace commet
