// hit_profile_jobs.hpp — hits_jobs_kernel and hits_jobs_wave_kernel: the hits passes of hit_profile_group.hpp over the chunk filters
// of SEVERAL jobs that search the same read set, up to eight filter slots side by side, a byte array per job
// (commet_index_many_and_profile, capi/multi_profile.hpp).
//
// The walks are the grouped kernels' own, the same text with JOBS = true: hits_lanes (hit_profile_group.hpp) and
// hit_profile_wave_body.hpp.  Plane A
// interleaved at stride NF, ONE long_load_a per window for every slot and both strands, B, C, D probed in the slot's own planes for
// the (slot, strand) pairs that want the window and whose lane-a bit is set; a hit in slot i moves `free` of slot i and that strand
// alone.  What differs is who owns a slot, and each difference is an `if constexpr (JOBS)` branch of the body with its reason beside
// it.  Consecutive slots belong to one job (the chunks of its index set); the layout comes as packed scalars (JobSlots).  Every
// job's byte array is `lines` lines of 256 bytes long.
// Per job: byte = min(cap, max over ITS slots of max(F, R)), written to hits + job_in_pass * 256 * lines + r.
//
// The stop is per job.  When a slot's count on a strand reaches its job's cap, the job's byte is decided: every state of that job,
// both strands of all mates, stops wanting windows.  The walk of a read ends only when no state wants a window or the read ends: a
// job that reaches its cap does not end the walk for the others — the grouped kernels' `best < max_hits` test is global, one job
// there.
//
// No `before` skip and a plain store: the host zeroes the byte arrays per call and never splits a job across passes, so a job's
// bytes are written by exactly one pass, and by the one lane that owns the read; a zero is not stored.  `walked` counts the reads
// the pass walked.  There is no list: `sel` skips the unvisited reads.
//
// Kernels of their own, not a run-time flag on the grouped ones: JOBS is a compile-time constant of the shared body, so the twelve
// instantiations on either side (and their rows in tools/kernel_resources.py) stay as they are.  hits_jobs_kernel takes a lane per
// read; search sets of long reads (hits_wave_ok, capi/profile.hpp) take hits_jobs_wave_kernel, a wave per read: same owners, same
// stop, same bytes.
//
// Included by capi.hip behind hit_profile_group.hpp (hits_lanes, JobSlots, and what that file names); not meant to stand alone.
#pragma once

namespace commet {

template <typename W, int NF>
__global__ __launch_bounds__(256) COMMET_SGPRS void hits_jobs_kernel(ReadsView rv, FilterGroupView fg, int k, JobSlots js,
                                                                     const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits, uint32_t lines,
                                                                     unsigned long long *__restrict__ walked)
{
    hits_lanes<W, NF, true>(rv, fg, k, 0, js, sel, hits, lines, walked, ActiveList{nullptr, nullptr});
}

template <typename W, int NF>
__global__ __launch_bounds__(LONG_WG) void hits_jobs_wave_kernel(ReadsView rv, FilterGroupView fg, int k, JobSlots js,
                                                                 const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits, uint32_t lines,
                                                                 unsigned long long *__restrict__ walked)
{
    constexpr bool JOBS = true, REL = false;
    constexpr const uint16_t *thr = nullptr;
    constexpr int max_hits = 0;
    const ActiveList al{nullptr, nullptr};
#include "hit_profile_wave_body.hpp"
}

}  // namespace commet
