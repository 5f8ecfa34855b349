// hit_profile_wide.hpp — hits_wide_kernel: the hit profile (hit_profile.hpp) through the wide bit-sliced rows (slice_search.hpp).
//
// At small k a job has hundreds to thousands of chunk filters, and the slot kernels of the profile take at most eight of them per
// pass over a search set.  Here all chunk filters of a pass sit side by side in the rows of one table set, as for search_wide_kernel,
// and the mapping is that kernel's: a group of LPR lanes works on ONE read, lane sl owns the 16-byte pieces sl + LPR * i of every row.
// The kernel writes hits[r] = max(hits[r], min(T, max over the pass's chunks c of max(F_c, R_c))), F_c / R_c = the reference's greedy
// non-overlapping full four-lane hits of the forward / reverse-complement strand in chunk c (search_reads.h:45-83 run to the end of
// the read): the quantity hits_kernel computes, one filter at a time.
//
//   (1) row pass over EVERY complete window of the read (a profile has no t, so there is no `lim`), both strands, the rows of planes
//       A, B, C ANDed (plane D is left to the replay).  Window end positions are cut into blocks of k; per chunk bit and strand a
//       2-bit saturating counter of the blocks that hold a hit (wide_fold).  The counter is an UPPER BOUND on F_c / R_c: the ends of
//       two non-overlapping hits lie at least k apart, so they fall into different blocks, and a full hit is an A & B & C hit.  The
//       saturated value 3 means "no bound".  Registers: two masks per strand and piece = 16 * NP VGPRs for the counters (kept
//       through stage 2), 8 * NP more for the open block's masks (stage 1 only).
//   (2) exact replay with pruning.  best starts at the byte already in hits[r] (a later pass profits from earlier ones);
//       cap = min(T, len / k), no read holds more non-overlapping k-mers, and a read already at cap makes no request.  A chunk is
//       replayed only if its bound on at least one strand exceeds best, and only on the strands whose own bound does; chunks of
//       the higher bound first (ties: the smaller chunk), until best == cap or no bound exceeds best.  The replay of one chunk and
//       strand is search_wide_kernel's lane-per-window ballot walk with all four planes, without a stop at t: it counts to the end
//       of the strand, or to cap.  max is order-free, so the order decides speed only, and skipping a chunk whose bound is at most
//       best is exact.
//
// Columns past the pass's last chunk are not looked at (they may hold an earlier pass's chunks); the columns of empty chunks hold zeros.
// `walked` (optional) counts the reads the pass did walk: selected, of at least k bases, not yet at cap.
// Every __any, __ballot and __shfl sits in control flow that is uniform over the wave; a group without work runs with its predicate off.
#pragma once

#include "slice_search.hpp"

namespace commet {

template <int LPR, int NP>
__global__ __launch_bounds__(256) void hits_wide_kernel(ReadsView rv, const uint32_t *__restrict__ tables, int k, int max_hits, int g, uint32_t nw,
                                                        uint32_t rw, const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                        unsigned long long *__restrict__ walked)
{
    constexpr int RPW = 64 / LPR;                         // reads per wave
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / LPR, sl = lane % LPR;
    const uint64_t r = ((uint64_t) blockIdx.x * 4 + wave) * RPW + grp;
    bool active = r < rv.n;
    if (active && sel) active = (sel[r >> 6] >> (r & 63)) & 1ull;
    const SlicePlanes T(tables, k, rw);
    uint64_t t0 = 0;
    uint32_t len = 0;
    int before = 0;
    if (active) {
        read_extent(rv, r, t0, len);
        before = (int) hits[r];
    }
    const int cap = min(max_hits, (int) (len / (uint32_t) k));
    const bool walk = active && before < cap;             // (a read of fewer than k bases has cap 0)
    const uint32_t *p = rv.planes + 3 * t0;
    const int sh = 32 - k;
    const uint32_t mask = (1u << k) - 1u;
    const int last = walk ? (int) len - 1 : -1;           // a group that does not walk has no window
    uint4 f0[NP], f1[NP], r0[NP], r1[NP];                 // blocks with a hit per chunk bit: 2-bit counters (f1 f0), (r1 r0)
    bool have[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const uint32_t pc = (uint32_t) (sl + LPR * i);
        have[i] = 4u * pc < nw && (int) (128u * pc) < g;  // the piece holds a chunk of this pass
        f0[i] = f1[i] = r0[i] = r1[i] = make_uint4(0, 0, 0, 0);
    }
    // (1) row pass over all windows; every lane of the group rolls the same window.  This is search_wide_kernel's wide_row_pass, and the
    // window test of (2) its wide_window_hit, both written out: through the functions this kernel's registers moved (88 -> 78 VGPRs, a
    // wave more) and its search time rose by about 1 % (MEASUREMENTS.md); as written here its code is what it was before they existed
    {
        uint4 cur_f[NP], cur_r[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) cur_f[i] = cur_r[i] = make_uint4(0, 0, 0, 0);
        uint32_t wh = 0, wl = 0, run = 0;
        int in_block = 0;                                  // window positions since the block began
        for (uint32_t w = 0; (int) (w * 32u) <= last; ++w) {
            const uint32_t hi = p[3 * w], lo = p[3 * w + 1], va = p[3 * w + 2];
            const uint32_t nb = (uint32_t) min(32, last - (int) (w * 32u) + 1);
            for (uint32_t j = 0; j < nb; ++j) {
                wh = (wh >> 1) | (((hi >> j) & 1u) << (k - 1));
                wl = (wl >> 1) | (((lo >> j) & 1u) << (k - 1));
                run = ((va >> j) & 1u) ? run + 1 : 0;
                if ((int) (32u * w + j) < k - 1) continue;              // not a window position yet
                if (run >= (uint32_t) k) {
                    const uint32_t ka = __brev(wh) >> sh, kb = __brev(wl) >> sh;
                    const uint32_t ra = ~wh & mask, rb = ~wl & mask;
                    bool selfp;
                    const uint32_t addr = psi_a<uint32_t>(ka, k, selfp);
                    const uint4 *af = (const uint4 *) (T.a + (uint64_t) addr * rw), *ar = (const uint4 *) (T.a + (uint64_t) (selfp ? addr : addr ^ 1u) * rw);
                    const uint4 *bf = (const uint4 *) (T.b + (uint64_t) kb * rw), *br = (const uint4 *) (T.b + (uint64_t) rb * rw);
                    const uint4 *cf = (const uint4 *) (T.c + (uint64_t) (ka ^ kb) * rw), *cr = (const uint4 *) (T.c + (uint64_t) (ra ^ rb) * rw);
                    uint4 x[NP][6];
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        if (!have[i]) continue;
                        const int pc = sl + LPR * i;
                        x[i][0] = af[pc], x[i][1] = bf[pc], x[i][2] = cf[pc];
                        x[i][3] = ar[pc], x[i][4] = br[pc], x[i][5] = cr[pc];
                    }
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        if (!have[i]) continue;
                        or_into(cur_f[i], and3(x[i][0], x[i][1], x[i][2]));
                        or_into(cur_r[i], and3(x[i][3], x[i][4], x[i][5]));
                    }
                }
                if (++in_block == k) {                      // the block is complete
                    in_block = 0;
#pragma unroll
                    for (int i = 0; i < NP; ++i) wide_fold(cur_f[i], f0[i], f1[i]), wide_fold(cur_r[i], r0[i], r1[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) wide_fold(cur_f[i], f0[i], f1[i]), wide_fold(cur_r[i], r0[i], r1[i]);   // the last, partial block
    }
    // (2) exact replay, the chunks of the highest bound first.  The loops are uniform over the wave (ballots and shuffles inside); a
    // group without work runs them with its predicate off.  (The read's byte is loaded again here and at the end rather than kept
    // through the row pass: NP = 2 stands at the register count that costs a wave.)
    int best = walk ? (int) hits[r] : 0;
    for (;;) {
        // this lane's pick: (3 - bound) in the bits above the chunk number, so that the group's smallest key is its highest bound's
        // smallest chunk (a chunk number has 14 bits: WIDE_MAX_ROW_WORDS * 32 chunks per pass)
        uint32_t key = NONE;
        if (walk && best < cap) {
            uint32_t k1 = NONE, k2 = NONE, k3 = NONE;
#pragma unroll
            for (int i = NP - 1; i >= 0; --i) {
                const uint32_t w0 = 4u * (uint32_t) (sl + LPR * i);
#pragma unroll
                for (int j = 3; j >= 0; --j) {
                    const uint32_t a0 = wide_word(f0[i], (uint32_t) j), a1 = wide_word(f1[i], (uint32_t) j);
                    const uint32_t b0 = wide_word(r0[i], (uint32_t) j), b1 = wide_word(r1[i], (uint32_t) j);
                    const uint32_t m1 = a0 | a1 | b0 | b1, m2 = a1 | b1, m3 = (a0 & a1) | (b0 & b1);
                    const uint32_t base = (w0 + (uint32_t) j) * 32u - 1u;
                    if (m1) k1 = base + (uint32_t) __ffs((int) m1);
                    if (m2) k2 = base + (uint32_t) __ffs((int) m2);
                    if (m3) k3 = base + (uint32_t) __ffs((int) m3);
                }
            }
            key = k3 != NONE ? k3 : k2 != NONE ? ((1u << 14) | k2) : k1 != NONE ? ((2u << 14) | k1) : NONE;
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) key = min(key, (uint32_t) __shfl_xor((int) key, o, LPR));   // the group's pick
        const int bound = 3 - (int) (key >> 14);           // 3 = saturated: no bound
        const bool pend = key != NONE && (bound == 3 || bound > best);
        if (!__any(pend)) break;                           // no group has a chunk whose bound exceeds its best
        const uint32_t chunk = key & 0x3FFFu, cw = chunk >> 5, cb = chunk & 31u;
        // the owner of word cw reads the chunk's two counters and drops the chunk
        uint32_t cnts = 0;                                 // bits 0-1 forward, 2-3 reverse
        if (pend) {
            const uint32_t pc = cw >> 2, wj = cw & 3u, keep = ~(1u << cb);
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (pc == (uint32_t) (sl + LPR * i)) {
                    cnts = ((wide_word(f0[i], wj) >> cb) & 1u) | (((wide_word(f1[i], wj) >> cb) & 1u) << 1) |
                           (((wide_word(r0[i], wj) >> cb) & 1u) << 2) | (((wide_word(r1[i], wj) >> cb) & 1u) << 3);
                    wide_drop(f0[i], wj, keep), wide_drop(f1[i], wj, keep), wide_drop(r0[i], wj, keep), wide_drop(r1[i], wj, keep);
                }
        }
        cnts = (uint32_t) __shfl((int) cnts, (int) ((cw >> 2) % (uint32_t) LPR), LPR);
        const bool go = pend && (int) chunk < g;
        for (int strand = 0; strand < 2; ++strand) {
            const int sb = (int) ((cnts >> (2 * strand)) & 3u);
            const bool flagged = go && best < cap && (sb == 3 || sb > best);   // (best may have grown on the forward strand)
            int seen = 0, next_ok = 0;
            for (int qb = k - 1; __any(flagged && seen < cap && qb <= last); qb = max(qb + LPR, next_ok)) {
                const int q = qb + sl;
                bool hit = false;
                if (flagged && seen < cap && q <= last && q >= next_ok) {
                    ItemWords<uint32_t> it;
                    it.load(p, (uint32_t) q >> 5);
                    uint32_t wh, wl;
                    if (it.window((uint32_t) q & 31u, k, mask, wh, wl)) {
                        uint32_t ka, kb;
                        if (strand == 0) ka = __brev(wh) >> sh, kb = __brev(wl) >> sh;
                        else ka = ~wh & mask, kb = ~wl & mask;
                        const uint32_t va = T.a[(uint64_t) psi_a<uint32_t>(ka, k) * rw + cw], vb = T.b[(uint64_t) kb * rw + cw];
                        const uint32_t vc = T.c[(uint64_t) (ka ^ kb) * rw + cw], vd = T.d[(uint64_t) (ka | kb) * rw + cw];
                        hit = ((va & vb & vc & vd) >> cb) & 1u;
                    }
                }
                uint64_t m = __ballot(hit);
                if constexpr (LPR < 64) m = (m >> (grp * LPR)) & ((1ull << LPR) - 1ull);
                while (m && seen < cap) {
                    const int qq = qb + (__ffsll((long long) m) - 1);
                    m &= m - 1ull;
                    if (qq < next_ok) continue;
                    ++seen;
                    next_ok = qq + k;                       // hash.clear(), search_reads.h:60: the next complete window ends k bases on
                }
            }
            best = max(best, seen);                         // (seen <= cap)
        }
    }
    const bool mine = walk && sl == 0;
    if (mine && best > (int) hits[r]) hits[r] = (uint8_t) best;
    count_walked(walked, mine);
}

}  // namespace commet
