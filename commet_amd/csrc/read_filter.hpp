// read_filter.hpp — the read filter on a resident set (reference: src/filter_reads.cpp:186-205, 265-306; the rule is
// stated once in host/filter_rule.hpp).
//
// Everything the rule looks at is in the set's planes (kernels.hpp): per read, len from the offsets and, by popcounts,
//   other = len - popc(valid),  T = popc(hi & lo & valid),  G = popc(hi & ~lo & valid),  C = popc(~hi & lo & valid),
//   A = popc(valid & ~hi & ~lo)
// (hi = 1 for G/T, lo = 1 for C/T, valid = 1 for ACGTacgt).  One streaming pass over the planes, 12 bytes per 32 bases.
//
// Verdicts in the rule's order: (empty ->) length -> N -> Shannon.  The Shannon verdict is exact by construction: no
// device transcendental decides it.  A term f * log(f) / log(2) depends on (count, len) only, the host fills a table
// of them with the very expression the tool evaluates (fill_shannon_table) and the device sums five entries in the
// reference's order and types: index = (float) ((double) index + term) over A, C, G, T, other, skipping absent classes,
// then fabsf, then < min_shannon as floats.  A read longer than the table covers is not decided here: its number and
// counts go to a compact list, the host decides it with the same function.
//
// Out: three bitmaps over the set, 64 reads per word (keep, removed by length, removed by N; a read in none of them was
// removed by Shannon, is empty, or is on the list).  The sequential part of the rule (the stop at an empty record or at
// the -m cap, per file) runs on the host over these words (finish_file).
#pragma once

#include "kernels.hpp"

namespace commet {

struct ReadFilterParams {
    uint32_t      min_len;       // reads shorter than this are removed by length
    uint32_t      max_other;     // reads with more non-ACGT bases are removed by N (0x7FFFFFFF: any)
    float         min_shannon;   // <= 0: no Shannon test
    const double *table;         // Shannon terms of the lengths table_lo .. table_hi (host/filter_rule.hpp, shannon_table_at)
    uint32_t      table_lo, table_hi;
};

// a read the device leaves to the host (longer than the table covers)
struct ReadFilterLong {
    uint64_t read;
    uint32_t cnt[5];             // A C G T other
    uint32_t len;
};

constexpr uint32_t READ_FILTER_LANE_MAX_LEN = 512;   // sets whose longest read is longer take a wave per read

constexpr int RF_KEEP = 0, RF_LENGTH = 1, RF_N = 2, RF_SHANNON = 3, RF_NONE = 4, RF_LONG = 5;

// the verdict of a read from its length and counts; nv = valid bases, nt / ng / nc = T / G / C among them
__device__ __forceinline__ int read_filter_verdict(const ReadFilterParams &p, uint32_t len, uint32_t nv, uint32_t nt, uint32_t ng,
                                                   uint32_t nc)
{
    if (len == 0) return RF_NONE;
    if (len < p.min_len) return RF_LENGTH;
    const uint32_t other = len - nv;
    if (other > p.max_other) return RF_N;
    if (!(p.min_shannon > 0.0f)) return RF_KEEP;
    if (len < p.table_lo || len > p.table_hi) return RF_LONG;
    const double *row = p.table + ((uint64_t) len * (len + 1) - (uint64_t) p.table_lo * (p.table_lo + 1)) / 2;
    const uint32_t cnt[5] = {nv - nt - ng - nc, nc, ng, nt, other};
    float index = 0.0f;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        if (cnt[i]) index = (float) ((double) index + row[cnt[i]]);
    return fabsf(index) < p.min_shannon ? RF_SHANNON : RF_KEEP;
}

// the counts of one word triple of a read; rem = bases of the read from this word on (the bits past it do not count)
__device__ __forceinline__ void read_filter_word(const uint32_t *__restrict__ t, uint32_t rem, uint32_t &nv, uint32_t &nt, uint32_t &ng,
                                                 uint32_t &nc)
{
    uint32_t va = t[2];
    if (rem < 32u) va &= (1u << rem) - 1u;
    const uint32_t hi = t[0] & va, lo = t[1] & va;
    nv += __popc(va);
    nt += __popc(hi & lo);
    ng += __popc(hi & ~lo);
    nc += __popc(lo & ~hi);
}

// A lane per read: the common 100-150 bp sets (neighbouring lanes read neighbouring triples).  One ballot per bitmap
// and wave; the wave of reads [64 w, 64 w + 64) writes word w of each bitmap.
__global__ __launch_bounds__(256) void read_filter_lane_kernel(ReadsView rv, ReadFilterParams p, uint64_t *__restrict__ keep,
                                                               uint64_t *__restrict__ rm_length, uint64_t *__restrict__ rm_n)
{
    const uint64_t r = blockIdx.x * 256ull + threadIdx.x;
    int v = RF_NONE;
    if (r < rv.n) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *tp = rv.planes + 3 * t0;
        uint32_t nv = 0, nt = 0, ng = 0, nc = 0;
        for (uint32_t w = 0; w * 32u < len; ++w) read_filter_word(tp + 3 * w, len - w * 32u, nv, nt, ng, nc);
        v = read_filter_verdict(p, len, nv, nt, ng, nc);
    }
    const uint64_t bk = __ballot(v == RF_KEEP), bl = __ballot(v == RF_LENGTH), bn = __ballot(v == RF_N);
    const uint64_t r0 = blockIdx.x * 256ull + (threadIdx.x & ~63u);   // the wave's first read
    if ((threadIdx.x & 63u) == 0 && r0 < rv.n) {
        keep[r0 >> 6] = bk;
        rm_length[r0 >> 6] = bl;
        rm_n[r0 >> 6] = bn;
    }
}

// A wave per read, for sets with long reads: the lanes share a read's words and a wave reduction gives every lane the
// counts; a wave takes the 64 reads of one bitmap word, one after the other, and writes the word.  Reads the table does
// not cover go to `longs` (at most long_cap entries; *n_long counts them all, so the host sees an overflow).
__global__ __launch_bounds__(256) void read_filter_wave_kernel(ReadsView rv, ReadFilterParams p, uint64_t *__restrict__ keep,
                                                               uint64_t *__restrict__ rm_length, uint64_t *__restrict__ rm_n,
                                                               ReadFilterLong *__restrict__ longs, unsigned long long *__restrict__ n_long,
                                                               uint64_t long_cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r0 = blockIdx.x * 256ull + (threadIdx.x & ~63u);
    if (r0 >= rv.n) return;                                           // (the whole wave)
    uint64_t bk = 0, bl = 0, bn = 0;
    for (uint32_t i = 0; i < 64u && r0 + i < rv.n; ++i) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r0 + i, t0, len);
        const uint32_t *tp = rv.planes + 3 * t0;
        const uint32_t words = (len + 31u) >> 5;
        uint32_t nv = 0, nt = 0, ng = 0, nc = 0;
        for (uint32_t w = lane; w < words; w += 64u) read_filter_word(tp + 3ull * w, len - w * 32u, nv, nt, ng, nc);
        for (int o = 32; o > 0; o >>= 1) {
            nv += __shfl_xor(nv, o, 64);
            nt += __shfl_xor(nt, o, 64);
            ng += __shfl_xor(ng, o, 64);
            nc += __shfl_xor(nc, o, 64);
        }
        const int v = read_filter_verdict(p, len, nv, nt, ng, nc);   // the same in every lane
        bk |= (uint64_t) (v == RF_KEEP) << i;
        bl |= (uint64_t) (v == RF_LENGTH) << i;
        bn |= (uint64_t) (v == RF_N) << i;
        if (v == RF_LONG && lane == 0) {
            const unsigned long long at = atomicAdd(n_long, 1ull);
            if (at < long_cap) {
                ReadFilterLong e;
                e.read = r0 + i;
                e.cnt[0] = nv - nt - ng - nc, e.cnt[1] = nc, e.cnt[2] = ng, e.cnt[3] = nt, e.cnt[4] = len - nv;
                e.len = len;
                longs[at] = e;
            }
        }
    }
    if (lane == 0) {
        keep[r0 >> 6] = bk;
        rm_length[r0 >> 6] = bl;
        rm_n[r0 >> 6] = bn;
    }
}

}  // namespace commet
