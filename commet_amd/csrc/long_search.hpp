// long_search.hpp — search_long_kernel: one WAVE per read, for sets whose reads have more first-hit windows than the register-mask
// kernels and the tiled search take (capi/search_dispatch.hpp, long_ok): merged pairs, contigs, ONT / PacBio reads.
//
// The lane-per-read kernels (kernels.hpp) walk such a read from end to end in one lane, one dependent request at a time, and a
// workgroup lives as long as its longest read.  Here the 64 lanes of a wave take 64 CONSECUTIVE windows of one read (a block),
// lane = window start - block start, and the reference's control flow (search_reads.h:45-83) runs on the ballots of their answers:
//   per filter of the pass and strand, (next_free, count) — the first window start that no longer overlaps the last full hit, and
//   the full hits so far.  A lane probes filter i for its window iff the window's k bases are ACGT, filter i is still open and the
//   window starts at or after next_free[i]; plane A first (one load of NF interleaved words serves every filter), B, C, D only
//   for the survivors.  __ballot gives the block's full hits of filter i as 64 bits, and the whole wave walks them greedily:
//   lowest set bit at or after next_free, count it, next_free = its start + k, again.  Both values are carried into the next block
//   (a hit in the last windows of block b forbids the first windows of block b + 1).  t hits end the filter's scan; forward strand
//   over the whole read first, the reverse complement only for filters that did not reach t, from a fresh state.
// Windows probed in parallel behind a hit of the same block are windows the reference never looks at: their answers are dropped
// by the walk, and the COUNT builds count a probe only where the walk passes (P_ref of the lane-per-read kernels, exactly).
// Blocks behind the one that ends the last open scan are never loaded.
//
// Pruning (exact, not in COUNT builds; see search_kernel): with `count` hits a window starting at s can still lead to t of them
// only if s <= len - (t - count) * k.  That bound grows with every hit, so it is applied by the wave between blocks and after
// each hit, never per lane within a block.
//
// Included by capi.hip behind kernels.hpp (KeyCtx, ItemWords, psi_a, probe_bcd_*, ActiveList); not meant to stand alone.
#pragma once

namespace commet {

constexpr int LONG_WG = 256;             // four waves, four reads in flight per workgroup
constexpr int LONG_STAGE_WORDS = 7;      // read words a block's windows can touch: words w0 - 2 .. w0 + 4 of the read (k <= 64)

// the NF interleaved plane-A words of one address: one request
template <int NF> __device__ __forceinline__ void long_load_a(const uint32_t *__restrict__ q, uint32_t (&x)[NF])
{
    if constexpr (NF == 1) {
        x[0] = q[0];
    } else if constexpr (NF == 2) {
        const uint2 v = *(const uint2 *) q;
        x[0] = v.x, x[1] = v.y;
    } else if constexpr (NF == 4) {
        const uint4 v = *(const uint4 *) q;
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
    } else {
        static_assert(NF == 8, "groups of 1, 2, 4 or 8 filters");
        const uint4 v = *(const uint4 *) q, u = *(const uint4 *) (q + 4);
        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w, x[4] = u.x, x[5] = u.y, x[6] = u.z, x[7] = u.w;
    }
}

// fg.il_a: the A planes of the pass interleaved with stride NF (NF == 1: the filter's own plane A); fg.g <= NF filters.
// The grid is persistent: wave w of the launch takes items w, w + waves, ... of the pass — reads of the set (sel and tags decide) or
// entries of its ActiveList.  Found flags leave as one atomic OR per found read (the reads of a tag word belong to different waves);
// counters as in search_group_kernel, {scanned_i, found_i} at counters[i * cstride], added once per wave at its end.
template <typename W, int NF, bool COUNT>
__global__ __launch_bounds__(LONG_WG) void search_long_kernel(ReadsView rv, FilterGroupView fg, int k, int t, const uint64_t *__restrict__ sel,
                                                              uint64_t *__restrict__ tags, unsigned long long *__restrict__ counters,
                                                              uint32_t cstride, unsigned long long *__restrict__ probe_counter, ActiveList al)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const uint64_t n_items = al.ids ? (uint64_t) *al.n : rv.n;
    const KeyCtx<W> kc(k);
    const uint32_t all = (fg.g >= 32) ? ~0u : ((1u << fg.g) - 1u);   // filters of the pass, one bit each
    unsigned long long probes = 0;
    uint32_t n_scanned[NF], n_found[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) n_scanned[i] = 0, n_found[i] = 0;

    for (uint64_t item = wave0; item < n_items; item += n_waves) {   // (uniform per wave)
        uint64_t r = item;
        if (al.ids) {
            r = (uint64_t) al.ids[item];
        } else {
            const uint64_t selw = sel ? sel[r >> 6] : ~0ull, tagw = tags ? tags[r >> 6] : 0ull;
            if (!(((selw & ~tagw) >> (r & 63ull)) & 1ull)) continue;
        }
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int found_chunk = -1;                              // lowest filter of the pass that tagged the read
        unsigned long long fprobes[NF];                    // (COUNT) what the reference loads for filter i if it gets that far
#pragma unroll
        for (int i = 0; i < NF; ++i) fprobes[i] = 0;
        uint32_t want = all;                               // filters whose answer still matters: below the lowest one that found the read
        for (int strand = 0; strand < 2 && want; ++strand) {
            int next_free[NF], count[NF];
#pragma unroll
            for (int i = 0; i < NF; ++i) next_free[i] = 0, count[i] = 0;
            uint32_t open = want;                          // filters whose scan of this strand goes on
            if constexpr (!COUNT) {
                if ((int64_t) len < (int64_t) t * k) open = 0;   // no room for t windows
            }
            for (int base = 0; base < n_win && open; base += 64) {
                // the read's words this block's windows stand on, one per lane, handed out by shuffles
                const int w0 = base >> 5;
                uint32_t staged = 0;
                {
                    const int wi = w0 - 2 + lane / 3;
                    if (lane < 3 * LONG_STAGE_WORDS && wi >= 0 && wi < n_words) staged = p[3 * wi + lane % 3];
                }
                const int s = base + lane, q = s + k - 1;
                // (every lane takes every shuffle: a lane that sat out would hand out nothing.  Words in front of the read are staged
                // as zeros, which is what ItemWords::load puts there)
                ItemWords<W> it;
                constexpr int NWD = sizeof(W) == 4 ? 2 : 3;
#pragma unroll
                for (int j = 0; j < NWD; ++j) {
                    const int src = 3 * ((q >> 5) - (NWD - 1) + j - (w0 - 2));   // 0 .. 3 * LONG_STAGE_WORDS - 3
                    it.hi[j] = (uint32_t) __shfl((int) staged, src, 64);
                    it.lo[j] = (uint32_t) __shfl((int) staged, src + 1, 64);
                    it.va[j] = (uint32_t) __shfl((int) staged, src + 2, 64);
                }
                W ka, kb;
                const bool valid = kc.window_keys(it, q, strand, ka, kb) && s < n_win;
                // which filters this lane asks: open ones whose last hit the window does not overlap
                uint32_t ask = 0;
#pragma unroll
                for (int i = 0; i < NF; ++i)
                    if (valid && ((open >> i) & 1u) && s >= next_free[i]) ask |= 1u << i;
                uint32_t xa[NF];
                uint32_t bit = 0;
                if (ask) {
                    const W addr = psi_a<W>(ka, k);
                    long_load_a<NF>(fg.il_a + (uint64_t) (addr >> 5) * NF, xa);
                    bit = (uint32_t) addr & 31u;
                } else {
#pragma unroll
                    for (int i = 0; i < NF; ++i) xa[i] = 0;
                }
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    if (!((open >> i) & 1u)) continue;     // (uniform)
                    const bool asked = (ask >> i) & 1u;
                    const bool ha = asked && ((xa[i] >> bit) & 1u);
                    bool full = false;
                    uint64_t m_valid = 0, m_a = 0, m_b = 0, m_c = 0;
                    const PlanesBCD f = planes_bcd(fg, i);
                    if constexpr (COUNT) {
                        const bool hb = ha && test_bit<W>(f.b, kb);
                        const bool hc = hb && test_bit<W>(f.c, ka ^ kb);
                        full = hc && test_bit<W>(f.d, ka | kb);
                        m_valid = __ballot(asked), m_a = __ballot(ha), m_b = __ballot(hb), m_c = __ballot(hc);
                    } else {
                        full = ha && probe_bcd_chain<W>(f, ka, kb);
                    }
                    uint64_t m = __ballot(full);
                    // the greedy walk, by the whole wave; `passed` = the window starts of this block the reference looks at
                    uint64_t passed = 0;
                    int from = max(next_free[i] - base, 0);          // (block-relative)
                    bool ends = false;
                    while (true) {
                        if (from < 64) m &= ~0ull << from;
                        else m = 0;
                        if (!m) {
                            if (from < 64) passed |= ~0ull << from;
                            break;
                        }
                        const int b = __ffsll((unsigned long long) m) - 1;
                        passed |= (~0ull << from) & (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1ull));
                        ++count[i];
                        next_free[i] = base + b + k;
                        from = b + k;
                        if (count[i] >= t) {
                            ends = true;
                            if (found_chunk < 0 || i < found_chunk) found_chunk = i;
                            break;
                        }
                        if constexpr (!COUNT) {
                            if (next_free[i] > (int) len - (t - count[i]) * k) {   // the missing hits no longer fit
                                ends = true;
                                break;
                            }
                        }
                    }
                    if constexpr (COUNT)
                        fprobes[i] += (unsigned long long) (__popcll(passed & m_valid) + __popcll(passed & m_a) + __popcll(passed & m_b) + __popcll(passed & m_c));
                    if (ends) open &= ~(1u << i);
                }
                if (found_chunk >= 0) {
                    // the reference does not search a read in the chunks behind the one that tagged it
                    want &= (1u << found_chunk) - 1u;
                    open &= want;
                }
                if constexpr (!COUNT) {
                    // first window of the next block past every place a missing hit could start: the scan of this strand is over
#pragma unroll
                    for (int i = 0; i < NF; ++i)
                        if (((open >> i) & 1u) && max(base + 64, next_free[i]) > (int) len - (t - count[i]) * k) open &= ~(1u << i);
                }
            }
        }
        // scanned_i: the read reached chunk i (no earlier chunk of the pass tagged it); found_i: chunk i tagged it
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            if (i < fg.g && (found_chunk < 0 || found_chunk >= i)) {
                ++n_scanned[i];
                if constexpr (COUNT) probes += fprobes[i];
            }
            if (found_chunk == i) ++n_found[i];
        }
        if (found_chunk >= 0 && tags && lane == 0)
            (void) __hip_atomic_fetch_or(tags + (r >> 6), 1ull << (r & 63ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
        if (counters) {
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                if (n_scanned[i]) atomicAdd(&counters[(uint64_t) i * cstride], (unsigned long long) n_scanned[i]);
                if (n_found[i]) atomicAdd(&counters[(uint64_t) i * cstride + 1], (unsigned long long) n_found[i]);
            }
        }
        if (COUNT && probe_counter && probes) atomicAdd(probe_counter, probes);
    }
}

}  // namespace commet
