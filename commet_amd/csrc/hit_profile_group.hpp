// hit_profile_group.hpp — hits_group_kernel and hits_group_wave_kernel: the hits passes of hit_profile.hpp over a GROUP of up to eight
// chunk filters, one walk of the read and one plane-A request per window for all of them (commet_index_and_profile, capi/profile.hpp)
// — and the two bodies that these kernels share with the passes over the filters of SEVERAL jobs (hit_profile_jobs.hpp: JOBS = true):
// hits_lanes below, a lane per read, and hit_profile_wave_body.hpp, a wave per read.  The four kernels only name their body: a
// carry or block-bound fix is made once.
//
// Why grouping is exact.  Per chunk filter c and strand, the accepted hits are one greedy sequence that depends on that filter
// alone (hit_profile.hpp), and hits = min(T, max over c of max(F_c, R_c)): a max fold is order-free.  Holding the (free, cnt) state
// of g filters side by side and walking the read once therefore gives the same F_c, R_c as g separate walks.  Two stops stay exact:
// a read whose byte equals max_hits on entry is skipped, and the walk of a read ends as soon as ANY filter reaches max_hits on ANY
// strand, because the byte is then max_hits.  A window is loaded iff at least one of the 2 g states still wants it: its k bases are
// ACGT and it starts at or after `free` of that filter and strand.
//
// Plane A of the group is word-interleaved (interleave_a_kernel: il_a[w * NF + i] = word w of filter slot i), so the ONE load of NF
// words at psi_a(forward key) gives, in word i, filter i's forward lane-a bit and its reverse-complement bit at bit ^ 1 (the bit
// itself when the key is its own partner).  B, C, D are probed in slot i's own planes, only for the (filter, strand) pairs that
// want the window and whose lane-a bit is set.  Filters i >= fg.g of a remainder group play no part: their state never wants a
// window, their interleaved words are not looked at, their slots are not touched.  Groups need k >= 2 (k == 1 has no paired
// plane A): the host takes such a job one filter per pass.
//
// The per-filter state lives in registers: every loop over NF unrolls fully, no array is indexed by a run-time value, the counts
// (<= max_hits <= 255) are bytes of one word per strand.  The lane body walks its lane-a candidates bit by bit and addresses each
// one's slot per lane; the wave body keeps its uniform state in the lanes of two registers and loops over the g filters.  Either
// way no table of per-slot plane pointers is held in scalar registers, and none of the twenty-four instantiations spills.
//
// Included by capi.hip behind hit_profile.hpp (long_load_a, wave_block_words, greedy_take, planes_bcd, FilterGroupView, search_lane,
// count_walked as well); not meant to stand alone.
#pragma once

namespace commet {

// (JOBS) which job owns a slot of the pass, and its cap, as packed scalars, no pointer tables.  Consecutive slots belong to one job:
//   mates  byte i = the mask of the slots of slot i's job (slot i among them); 0 for a slot behind the pass's filters
//   caps   byte i = max_hits of slot i's job
// Slot i is the first of its job when it is the lowest bit of its own mask; the job's number in the pass is the count of first slots
// below i
struct JobSlots {
    uint64_t mates;
    uint64_t caps;
};

// The layout words live in vector registers: they are uniform, but the lane kernel is at its scalar budget (COMMET_SGPRS) without
// them, and their bytes are picked by a per-lane slot number anyway.  Passes of up to four slots hold the low halves only
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

// ---------------------------------------------------------------------------
// a lane per read: the walk of hits_kernel, NF filters' states side by side.  JOBS = false: the filters of one job fold into the
// read's byte of `hits` (max_hits, al; js and lines are not looked at).  JOBS = true: the slots belong to the jobs of js, a byte
// array of `lines` lines of 256 bytes per job (js, lines; max_hits and al are not looked at).  REL (one job; relative_search.hpp):
// the cap is the read's own, thr[r] <= 255, max_hits is not looked at, and `hits` holds found flags: a read with no cap or a flag is
// not walked, and its flag is set iff a count reaches the cap.
// ---------------------------------------------------------------------------
template <typename W, int NF, bool JOBS, bool REL = false>
__device__ __forceinline__ void hits_lanes(const ReadsView &rv, const FilterGroupView &fg, int k, int max_hits, JobSlots js,
                                           const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits, uint32_t lines,
                                           unsigned long long *__restrict__ walked, ActiveList al, const uint16_t *__restrict__ thr = nullptr)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "passes of 2, 4 or 8 filter slots");
    static_assert(!(JOBS && REL), "a cap per read is one job's");
    const SearchLane me = search_lane(rv, al, sel, nullptr);
    const uint64_t r = me.r;
    int before = 0;
    int cap = max_hits;                             // (one job) where the walk of the read stops
    bool walk = me.active;
    if constexpr (REL) {
        if (walk) {
            cap = (int) thr[r];
            walk = cap != 0 && hits[r] == 0;
        }
    } else if constexpr (!JOBS) {
        if (walk) {
            before = (int) hits[r];
            walk = before < max_hits;
        }
    }
    // (JOBS) no `before` skip: the host zeroes the byte arrays per call and never splits a job across passes, so a job's bytes are
    // written by exactly one pass, and by the one lane that owns the read.  `walked` then counts the active lanes
    if (walk) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const KeyCtx<W> kc(k);
        uint64_t slot_mates = 0, slot_caps = 0;
        if constexpr (JOBS) slot_mates = layout_in_vgprs<NF>(js.mates), slot_caps = layout_in_vgprs<NF>(js.caps);
        W wh = 0, wl = 0;
        uint32_t run = 0;
        // [slot]: first window start the strand's state takes again (never, for the slots behind the pass's filters and (JOBS) for the
        // slots of a job that has reached its cap); the hits of slot i on a strand are byte i of cnt_f / cnt_r
        int free_f[NF], free_r[NF];
        uint64_t cnt_f = 0, cnt_r = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) free_f[i] = free_r[i] = i < fg.g ? 0 : INT_MAX;
        int min_free = 0;                           // the lowest of the 2 NF: a window in front of it is wanted by nobody
        int best = 0;                               // (one job) the highest of the 2 NF counts
        // One job: the walk ends as soon as any count is max_hits, the byte is then max_hits.  Several: it ends only when no state
        // wants a window (or the read ends) — a job that reaches its cap does not end the walk for the others
        const auto more = [&] {
            if constexpr (JOBS) return min_free != INT_MAX;
            else return best < cap;
        };
        for (uint32_t w = 0; w * 32u < len && more(); ++w) {
            const uint32_t hi = p[3 * w], lo = p[3 * w + 1], va = p[3 * w + 2];
            const uint32_t nb = min(32u, len - w * 32u);
            for (uint32_t j = 0; j < nb && more(); ++j) {
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
                // B, C, D of each candidate in its slot's planes (the slot is per lane here: addresses, not a table of pointers)
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
                    const uint32_t mine = (uint32_t) (cnt >> (8 * i)) & 255u;
                    uint32_t stop = 0;
                    if constexpr (JOBS) {
                        // The stop is per job.  When a slot's count on a strand reaches its job's cap, the job's byte is decided: none
                        // of its states, both strands of all mates, wants a window any more (free = INT_MAX), the candidates of its
                        // mates in this window included.  Counts never pass the cap (<= 255): bytes of one word per strand
                        if (mine >= slot_byte<NF>(slot_caps, i)) stop = slot_byte<NF>(slot_mates, i);
                        cand &= ~(stop | (stop << NF));
                    } else {
                        best = max(best, (int) mine);
                    }
#pragma unroll
                    for (int q = 0; q < NF; ++q) {
                        if (q == i && !rev) free_f[q] = start + k;
                        if (q == i && rev) free_r[q] = start + k;
                        if (JOBS && ((stop >> q) & 1u)) free_f[q] = free_r[q] = INT_MAX;
                    }
                }
                if (hit) {
                    min_free = INT_MAX;
#pragma unroll
                    for (int i = 0; i < NF; ++i) min_free = min(min_free, min(free_f[i], free_r[i]));
                }
            }
        }
        if constexpr (JOBS) {
            // per job, at its first slot: the fold over its slots, byte = min(cap, max over ITS slots of max(F, R)), a plain store to
            // hits + job_in_pass * 256 * lines + r; a zero is not stored
            int job = 0;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const uint32_t mates = slot_byte<NF>(slot_mates, i);
                if ((mates & (0u - mates)) != (1u << i)) continue;      // (not the first slot of a job, or no job's)
                uint32_t most = 0;
#pragma unroll
                for (int q = 0; q < NF; ++q)
                    if ((mates >> q) & 1u) most = max(most, max((uint32_t) (cnt_f >> (8 * q)) & 255u, (uint32_t) (cnt_r >> (8 * q)) & 255u));
                const uint32_t h = min(most, slot_byte<NF>(slot_caps, i));
                if (h) hits[(uint64_t) job * lines * 256ull + r] = (uint8_t) h;
                ++job;
            }
        } else if constexpr (REL) {
            if (best >= cap) hits[r] = 1;
        } else {
            const int h = min(max_hits, best);
            if (h > before) hits[r] = (uint8_t) h;
        }
    }
    count_walked(walked, walk);
}

template <typename W, int NF>
__global__ __launch_bounds__(256) COMMET_SGPRS void hits_group_kernel(ReadsView rv, FilterGroupView fg, int k, int max_hits,
                                                                      const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                                      unsigned long long *__restrict__ walked, ActiveList al)
{
    hits_lanes<W, NF, false>(rv, fg, k, max_hits, JobSlots{0, 0}, sel, hits, 0, walked, al);
}

// ---------------------------------------------------------------------------
// a wave per read: the body is hit_profile_wave_body.hpp, text included here and into hits_jobs_wave_kernel
// ---------------------------------------------------------------------------
template <typename W, int NF>
__global__ __launch_bounds__(LONG_WG) void hits_group_wave_kernel(ReadsView rv, FilterGroupView fg, int k, int max_hits,
                                                                  const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                                  unsigned long long *__restrict__ walked, ActiveList al)
{
    constexpr bool JOBS = false, REL = false;
    constexpr const uint16_t *thr = nullptr;
    constexpr JobSlots js{0, 0};
    constexpr uint32_t lines = 0;
#include "hit_profile_wave_body.hpp"
}

}  // namespace commet
