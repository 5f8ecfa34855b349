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
// hits_jobs_kernel takes a lane per read; search sets of long reads (hits_wave_ok, capi/profile.hpp) take hits_jobs_wave_kernel
// below, a wave per read: same owners, same stop, same bytes.
//
// Included by capi.hip behind hit_profile_group.hpp (long_load_a, planes_bcd, FilterGroupView, search_lane, and through it LONG_WG,
// LONG_STAGE_WORDS, ItemWords); not meant to stand alone.
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

// ---------------------------------------------------------------------------
// a wave per read, for search sets of long reads: the blocks of hits_group_wave_kernel (64 consecutive window starts per block, the
// read's words staged one per lane and shuffled into ItemWords, persistent grid, `sel` skips the unvisited reads), the owners and the
// stop of hits_jobs_kernel.  Per block ONE interleaved plane-A load per lane serves every slot and both strands; per (slot, strand) one
// ballot of full hits, walked greedily by the whole wave up to the cap of the slot's job.  All uniform per-slot state lives in lanes,
// lane i the forward strand of slot i and lane NF + i its reverse complement: (next_free, count) in st_next / st_count, the slot's
// cap and mates in lane_cap / lane_mates (the bytes of JobSlots, spread once per wave); the whole wave reads them with readlane, their
// lane writes them, and the slots of a pass are a loop over i < g with no table in scalar registers.  (next_free, count) are carried
// from block to block: slot i's hit in the last windows of block b forbids slot i's first windows of block b + 1, and nobody else's.
//
// When a slot reaches its job's cap, every state of that job gets next_free = INT_MAX: mates later in this block's slot loop take
// no more hits, and no state of the job wants a window of a later block.  Mates EARLIER in the slot loop may already have counted
// hits of this block that lie behind the capping hit — which the lane form, window by window, never sees.  That changes no byte:
// every count still stops at the cap, and byte = min(cap, max over the job's slots of max(F, R)) is the cap either way.
// The block loop ends when no state wants a window (min_next == INT_MAX) or the read ends; a job that is decided does not end it for
// the others, and blocks behind the one in which every job is decided are not loaded.
// ---------------------------------------------------------------------------
template <typename W, int NF>
__global__ __launch_bounds__(LONG_WG) void hits_jobs_wave_kernel(ReadsView rv, FilterGroupView fg, int k, JobSlots js,
                                                                 const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits, uint32_t lines,
                                                                 unsigned long long *__restrict__ walked)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "passes of 2, 4 or 8 filter slots");
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const KeyCtx<W> kc(k);
    const int g = fg.g;
    // the lane's slot (lanes 0 .. 2 NF - 1 hold a state), its job's cap and the slots of its job
    const int my_slot = lane & (NF - 1);
    const bool holds_state = lane < 2 * NF && my_slot < g;
    const uint32_t lane_cap = holds_state ? slot_byte<NF>(js.caps, my_slot) : 0u;
    const uint32_t lane_mates = holds_state ? slot_byte<NF>(js.mates, my_slot) : 0u;
    unsigned long long n_walked = 0;

    for (uint64_t r = wave0; r < rv.n; r += n_waves) {     // (uniform per wave)
        if (sel && !((sel[r >> 6] >> (r & 63ull)) & 1ull)) continue;
        ++n_walked;
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int st_next = holds_state ? 0 : INT_MAX, st_count = 0;
        int min_next = 0;                                  // the lowest next_free of the 2 g: a window in front of it is wanted by nobody
        for (int base = 0; base < n_win && min_next != INT_MAX; base += 64) {
            // the read's words this block's windows stand on: words w0 - 2 .. w0 + 4, one per lane (zeros outside the read)
            const int w0 = base >> 5;
            uint32_t staged = 0;
            {
                const int wi = w0 - 2 + lane / 3;
                if (lane < 3 * LONG_STAGE_WORDS && wi >= 0 && wi < n_words) staged = p[3 * wi + lane % 3];
            }
            const int s = base + lane, q = s + k - 1;
            ItemWords<W> it;                               // (every lane takes every shuffle)
            constexpr int NWD = sizeof(W) == 4 ? 2 : 3;
#pragma unroll
            for (int j = 0; j < NWD; ++j) {
                const int src = 3 * ((q >> 5) - (NWD - 1) + j - (w0 - 2));   // 0 .. 3 * LONG_STAGE_WORDS - 3
                it.hi[j] = (uint32_t) __shfl((int) staged, src, 64);
                it.lo[j] = (uint32_t) __shfl((int) staged, src + 1, 64);
                it.va[j] = (uint32_t) __shfl((int) staged, src + 2, 64);
            }
            W wh, wl;
            const bool valid = it.window((uint32_t) q & 31u, k, kc.mask, wh, wl) && s < n_win;
            const bool wanted = valid && s >= min_next;    // by at least one of the 2 g states
            W kaf, kbf, kar, kbr;
            kc.strand_keys(wh, wl, 0, kaf, kbf);
            kc.strand_keys(wh, wl, 1, kar, kbr);
            uint32_t xa[NF];
            uint32_t bit_f = 0, bit_r = 0;
            if (wanted) {
                bool selfp;
                const W addr = psi_a<W>(kaf, k, selfp);
                long_load_a<NF>(fg.il_a + (uint64_t) (addr >> 5) * NF, xa);
                bit_f = (uint32_t) addr & 31u, bit_r = selfp ? bit_f : bit_f ^ 1u;
            } else {
#pragma unroll
                for (int i = 0; i < NF; ++i) xa[i] = 0;
            }
            bool any_hit = false;
#pragma unroll 1
            for (int i = 0; i < g; ++i) {                  // (uniform)
                uint32_t x = xa[0];                        // slot i's word of the load
#pragma unroll
                for (int j = 1; j < NF; ++j) x = (i == j) ? xa[j] : x;
                const PlanesBCD bcd = planes_bcd(fg, i);
                const int cap = __builtin_amdgcn_readlane((int) lane_cap, i);
#pragma unroll
                for (int strand = 0; strand < 2; ++strand) {
                    const int slot = i + strand * NF;
                    int next_free = __builtin_amdgcn_readlane(st_next, slot), count = __builtin_amdgcn_readlane(st_count, slot);
                    // (a state of a decided job: next_free = INT_MAX, no lane is full)
                    const bool full = wanted && s >= next_free && ((x >> (strand ? bit_r : bit_f)) & 1u) &&
                                      probe_bcd_chain<W>(bcd, strand ? kar : kaf, strand ? kbr : kbf);
                    // the greedy walk, by the whole wave (block-relative window starts), up to the job's cap
                    uint64_t m = __ballot(full);
                    if (!m) continue;
                    int from = max(next_free - base, 0);
                    while (from < 64 && count < cap) {
                        m &= ~0ull << from;
                        if (!m) break;
                        const int b = __ffsll((unsigned long long) m) - 1;
                        ++count;
                        next_free = base + b + k;
                        from = b + k;
                    }
                    if (lane == slot) st_next = next_free, st_count = count;
                    // the job's byte is decided: none of its states, both strands of all mates, wants a window any more
                    if (count >= cap) {
                        const uint32_t stop = (uint32_t) __builtin_amdgcn_readlane((int) lane_mates, i);
                        if (lane < 2 * NF && ((stop >> my_slot) & 1u)) st_next = INT_MAX;
                    }
                    any_hit = true;
                }
            }
            if (any_hit) {
                min_next = INT_MAX;
#pragma unroll 1
                for (int i = 0; i < g; ++i)
                    min_next = min(min_next, min(__builtin_amdgcn_readlane(st_next, i), __builtin_amdgcn_readlane(st_next, i + NF)));
            }
        }
        // per job, at its first slot: the fold over its slots (lane i < NF: max(F, R) of slot i)
        const int both = max(st_count, __shfl(st_count, lane + NF, 64));
        int job = 0;
#pragma unroll 1
        for (int i = 0; i < g; ++i) {                      // (uniform)
            const uint32_t mates = (uint32_t) __builtin_amdgcn_readlane((int) lane_mates, i);
            if ((mates & (0u - mates)) != (1u << i)) continue;      // (not the first slot of a job)
            int best = 0;
#pragma unroll
            for (int j = 0; j < NF; ++j)
                if ((mates >> j) & 1u) best = max(best, __builtin_amdgcn_readlane(both, j));
            const int h = min(best, __builtin_amdgcn_readlane((int) lane_cap, i));
            if (lane == 0 && h) hits[(uint64_t) job * lines * 256ull + r] = (uint8_t) h;
            ++job;
        }
    }
    if (walked && lane == 0 && n_walked) atomicAdd(walked, n_walked);
}

}  // namespace commet
