// hit_profile_jobs.hpp — hits_jobs_kernel: the hits pass of hit_profile_group.hpp over the chunk filters of SEVERAL jobs that search
// the same read set, up to eight filter slots side by side, a byte array per job (commet_index_many_and_profile, capi/multi_profile.hpp).
//
// The walk is hits_group_kernel's: a lane per read, plane A interleaved at stride NF, ONE long_load_a per window for every slot and
// both strands, B, C, D probed in the slot's own planes for the (slot, strand) pairs that want the window and whose lane-a bit is
// set; a hit in slot i moves `free` of slot i and that strand alone.  What differs is who owns a slot.  Consecutive slots belong to
// one job (the chunks of its index set); the layout comes as packed scalars, no pointer tables (JobSlots below):
//   mates  byte i = the mask of the slots of slot i's job (slot i among them); 0 for a slot behind the pass's filters
//   caps   byte i = max_hits of slot i's job
// Slot i is the first of its job when it is the lowest bit of its own mask; the job's number in the pass is the count of first slots
// below i.  Every job's byte array is `lines` lines of 256 bytes long.
// Per job: byte = min(cap, max over ITS slots of max(F, R)), written to hits + job_in_pass * 256 * lines + r.
//
// The stop is per job.  When a slot's count on a strand reaches its job's cap, the job's byte is decided: every state of that job,
// both strands of all mates, stops wanting windows (free = INT_MAX).  The walk of a read ends only when no state wants a window
// (min_free == INT_MAX) or the read ends: a job that reaches its cap does not end the walk for the others — hits_group_kernel's
// `best < max_hits` test is global, one job there.  Counts never pass the cap (<= 255): bytes of one word per strand.
//
// No `before` skip and a plain store: the host zeroes the byte arrays per call and never splits a job across passes, so a job's
// bytes are written by exactly one pass, and by the one lane that owns the read; a zero is not stored.  `walked` counts the reads
// the pass walked (the active lanes).
//
// A kernel of its own, not a flag on hits_group_kernel: that kernel's twelve instantiations (and their rows in
// tools/kernel_resources.py) stay as they are.  Every loop over NF unrolls fully, no array is indexed by a run-time value.
// A lane per read only; the host sends search sets that take the wave-per-read kernels job by job.
//
// Included by capi.hip behind hit_profile_group.hpp (long_load_a, planes_bcd, FilterGroupView, search_lane); not meant to stand alone.
#pragma once

namespace commet {

// which job owns a slot of the pass, and its cap (see above)
struct JobSlots {
    uint64_t mates;
    uint64_t caps;
};

// The layout words live in vector registers: they are uniform, but the kernel is at its scalar budget (COMMET_SGPRS) without them,
// and their bytes are picked by a per-lane slot number anyway.  Passes of up to four slots hold the low halves only
template <int NF>
__device__ __forceinline__ uint64_t layout_in_vgprs(uint64_t packed)
{
    uint32_t lo, hi = 0;
    asm("v_mov_b32 %0, %1" : "=v"(lo) : "s"((uint32_t) packed));
    if (NF > 4) asm("v_mov_b32 %0, %1" : "=v"(hi) : "s"((uint32_t) (packed >> 32)));
    return ((uint64_t) hi << 32) | lo;
}

// byte i of a layout word
template <int NF>
__device__ __forceinline__ uint32_t slot_byte(uint64_t packed, int i)
{
    if (NF <= 4) return ((uint32_t) packed >> (8 * i)) & 255u;
    return (uint32_t) (packed >> (8 * i)) & 255u;
}

template <typename W, int NF>
__global__ __launch_bounds__(256) COMMET_SGPRS void hits_jobs_kernel(ReadsView rv, FilterGroupView fg, int k, JobSlots js,
                                                                     const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits, uint32_t lines,
                                                                     unsigned long long *__restrict__ walked)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "passes of 2, 4 or 8 filter slots");
    const SearchLane me = search_lane(rv, ActiveList{nullptr, nullptr}, sel, nullptr);
    const uint64_t r = me.r;
    const bool walk = me.active;
    if (walk) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const KeyCtx<W> kc(k);
        const uint64_t slot_mates = layout_in_vgprs<NF>(js.mates), slot_caps = layout_in_vgprs<NF>(js.caps);
        W wh = 0, wl = 0;
        uint32_t run = 0;
        // [slot]: first window start the strand's state takes again (never, for the slots behind the pass's filters and for the
        // slots of a job that has reached its cap); the hits of slot i on a strand are byte i of cnt_f / cnt_r
        int free_f[NF], free_r[NF];
        uint64_t cnt_f = 0, cnt_r = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) free_f[i] = free_r[i] = i < fg.g ? 0 : INT_MAX;
        int min_free = 0;                           // the lowest of the 2 NF: a window in front of it is wanted by nobody
        for (uint32_t w = 0; w * 32u < len && min_free != INT_MAX; ++w) {
            const uint32_t hi = p[3 * w], lo = p[3 * w + 1], va = p[3 * w + 2];
            const uint32_t nb = min(32u, len - w * 32u);
            for (uint32_t j = 0; j < nb && min_free != INT_MAX; ++j) {
                wh = (wh >> 1) | ((W) ((hi >> j) & 1u) << (k - 1));
                wl = (wl >> 1) | ((W) ((lo >> j) & 1u) << (k - 1));
                run = ((va >> j) & 1u) ? run + 1 : 0;
                if (run < (uint32_t) k) continue;
                const int start = (int) (32u * w + j) - (k - 1);
                if (start < min_free) continue;
                W kaf, kbf, kar, kbr;
                kc.strand_keys(wh, wl, 0, kaf, kbf);
                kc.strand_keys(wh, wl, 1, kar, kbr);
                bool selfp;
                const W addr = psi_a<W>(kaf, k, selfp);
                uint32_t xa[NF];
                long_load_a<NF>(fg.il_a + (uint64_t) (addr >> 5) * NF, xa);
                const uint32_t bit_f = (uint32_t) addr & 31u, bit_r = selfp ? bit_f : bit_f ^ 1u;
                // the lane-a candidates among the states that want the window: bit i = slot i forward, bit NF + i = its reverse complement
                uint32_t cand = 0;
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    if (start >= free_f[i]) cand |= ((xa[i] >> bit_f) & 1u) << i;
                    if (start >= free_r[i]) cand |= ((xa[i] >> bit_r) & 1u) << (NF + i);
                }
                bool hit = false;
                while (cand) {
                    const int b = __ffs((int) cand) - 1;
                    cand &= cand - 1u;
                    const int i = b & (NF - 1);
                    const bool rev = b >= NF;
                    if (!probe_bcd_chain<W>(planes_bcd(fg, i), rev ? kar : kaf, rev ? kbr : kbf)) continue;
                    hit = true;
                    uint64_t &cnt = rev ? cnt_r : cnt_f;
                    cnt += 1ull << (8 * i);
                    const uint32_t mine = (uint32_t) (cnt >> (8 * i)) & 255u, cap = slot_byte<NF>(slot_caps, i);
                    // the job's byte is decided: none of its states wants a window any more, the candidates of its mates in this window included
                    const uint32_t stop = mine >= cap ? slot_byte<NF>(slot_mates, i) : 0u;
                    cand &= ~(stop | (stop << NF));
#pragma unroll
                    for (int q = 0; q < NF; ++q) {
                        if (q == i && !rev) free_f[q] = start + k;
                        if (q == i && rev) free_r[q] = start + k;
                        if ((stop >> q) & 1u) free_f[q] = free_r[q] = INT_MAX;
                    }
                }
                if (hit) {
                    min_free = INT_MAX;
#pragma unroll
                    for (int i = 0; i < NF; ++i) min_free = min(min_free, min(free_f[i], free_r[i]));
                }
            }
        }
        // per job, at its first slot: the fold over its slots
        int job = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const uint32_t mates = slot_byte<NF>(slot_mates, i);
            if ((mates & (0u - mates)) != (1u << i)) continue;      // (not the first slot of a job, or no job's)
            uint32_t best = 0;
#pragma unroll
            for (int q = 0; q < NF; ++q)
                if ((mates >> q) & 1u) best = max(best, max((uint32_t) (cnt_f >> (8 * q)) & 255u, (uint32_t) (cnt_r >> (8 * q)) & 255u));
            const uint32_t h = min(best, slot_byte<NF>(slot_caps, i));
            if (h) hits[(uint64_t) job * lines * 256ull + r] = (uint8_t) h;
            ++job;
        }
    }
    if (walked) {
        __shared__ unsigned int wg_walked;
        if (threadIdx.x == 0) wg_walked = 0;
        __syncthreads();
        add_walked(walked, walk, wg_walked);
    }
}

}  // namespace commet
