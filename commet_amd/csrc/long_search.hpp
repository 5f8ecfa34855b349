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
// Several jobs in a pass (commet_index_many_and_search, capi/multi.hpp): a second kernel template of the same name and body with a
// job_mask — see JOBS below.
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

// The loader of a block (the 64 consecutive windows from window start `base`, one per lane): the read's words the block's windows
// stand on, words w0 - 2 .. w0 + 4, are staged one per lane (zeros outside the read, which is what ItemWords::load puts in front of
// it) and shuffled into `it` for the window that ends at base q = base + lane + k - 1, NWD words per plane.  EVERY lane of the wave
// must call it, whatever its window: a lane that sat out would hand out nothing
template <typename W>
__device__ __forceinline__ void wave_block_words(const uint32_t *__restrict__ p, int n_words, int base, int lane, int q, ItemWords<W> &it)
{
    const int w0 = base >> 5;
    uint32_t staged = 0;
    {
        const int wi = w0 - 2 + lane / 3;
        if (lane < 3 * LONG_STAGE_WORDS && wi >= 0 && wi < n_words) staged = p[3 * wi + lane % 3];
    }
    constexpr int NWD = sizeof(W) == 4 ? 2 : 3;
#pragma unroll
    for (int j = 0; j < NWD; ++j) {
        const int src = 3 * ((q >> 5) - (NWD - 1) + j - (w0 - 2));   // 0 .. 3 * LONG_STAGE_WORDS - 3
        it.hi[j] = (uint32_t) __shfl((int) staged, src, 64);
        it.lo[j] = (uint32_t) __shfl((int) staged, src + 1, 64);
        it.va[j] = (uint32_t) __shfl((int) staged, src + 2, 64);
    }
}

// The greedy walk of a block's ballot of full hits by the whole wave, for the kernels that count hits up to a cap (hit_profile*.hpp;
// the walk of search_long_kernel also records what it passes, ends scans and prunes: a loop of its own).  m: bit b = the window that
// starts at base + b is a full hit; lowest set bit at or after next_free, count it, next_free = its start + k, again
__device__ __forceinline__ void greedy_take(uint64_t m, int base, int k, int cap, int &next_free, int &count)
{
    int from = max(next_free - base, 0);                   // (block-relative)
    while (from < 64 && count < cap) {
        m &= ~0ull << from;
        if (!m) break;
        const int b = __ffsll((unsigned long long) m) - 1;
        ++count;
        next_free = base + b + k;
        from = b + k;
    }
}

// (several jobs in a pass) the filters of filter i's job behind it, and in front of it.  opens: bit j = filter j opens a job (bit 0
// is set); all: the filters of the pass.  Uniform over the wave
__device__ __forceinline__ uint32_t job_behind(uint32_t opens, uint32_t all, int i)
{
    const uint32_t above = all & ~((2u << i) - 1u);
    const uint32_t next = opens & above;                   // the jobs opened behind i: the lowest of them ends i's job
    return next ? above & ((next & (0u - next)) - 1u) : above;
}
__device__ __forceinline__ uint32_t job_before(uint32_t opens, int i)
{
    const uint32_t upto = opens & ((2u << i) - 1u);        // the jobs opened up to i: the highest of them is i's job
    return ((1u << i) - 1u) & ~((1u << (31 - __clz((int) upto))) - 1u);
}

// fg.il_a: the A planes of the pass interleaved with stride NF (NF == 1: the filter's own plane A); fg.g <= NF filters.
// The grid is persistent: wave w of the launch takes items w, w + waves, ... of the pass — reads of the set (sel and tags decide) or
// entries of its ActiveList.  Found flags leave as one atomic OR per found read (the reads of a tag word belong to different waves);
// counters as in search_group_kernel, {scanned_i, found_i} at counters[i * cstride], added once per wave at its end.
//
// JOBS (NF == 8, no probe counting): the filters of the pass belong to SEVERAL jobs that search this one set (capi/multi.hpp), the
// contract of search_group8_kernel: bit i of job_mask = filter i opens a job, a job's filters are consecutive slots, job j's found
// flags go to tags + j * job_tag_words (zeroed by the host: a job never spans passes); tags is not read, sel is null, there is no
// list.  The plane-A load of a window serves every job; the rule "not searched in the chunks behind the one that tagged it" holds
// within a job only, so `found` is a mask over the filter bits (the lowest bit of a job's filters is the chunk that tagged the read
// for that job) and a hit closes the later filters of its own job alone: the read stays in flight while any job wants an answer.
// The jobs are uniform over the wave: job_behind / job_before are scalar work on job_mask, no per-job arrays.
template <typename W, int NF, bool COUNT>
__global__ __launch_bounds__(LONG_WG) void search_long_kernel(ReadsView rv, FilterGroupView fg, int k, int t, const uint64_t *__restrict__ sel,
                                                              uint64_t *__restrict__ tags, unsigned long long *__restrict__ counters,
                                                              uint32_t cstride, unsigned long long *__restrict__ probe_counter, ActiveList al)
{
    constexpr bool JOBS = false;
    constexpr uint32_t job_mask = 0;
    constexpr uint64_t job_tag_words = 0;
#include "long_search_body.hpp"
}

// the filters of several jobs in one pass (JOBS = true, NF = 8, COUNT = false is the one case there is)
template <typename W, int NF, bool COUNT, bool JOBS>
__global__ __launch_bounds__(LONG_WG) void search_long_kernel(ReadsView rv, FilterGroupView fg, int k, int t, uint64_t *__restrict__ tags,
                                                              unsigned long long *__restrict__ counters, uint32_t cstride, uint32_t job_mask,
                                                              uint64_t job_tag_words)
{
    static_assert(JOBS && NF == 8 && !COUNT, "several jobs: passes of eight slots, no probe counting");
    constexpr const uint64_t *sel = nullptr;
    constexpr unsigned long long *probe_counter = nullptr;
    const ActiveList al{nullptr, nullptr};
#include "long_search_body.hpp"
}

}  // namespace commet
