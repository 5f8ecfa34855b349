// hits_tags.hpp — from the hit-count bytes of a profile (hit_profile*.hpp) to the tag vectors of every wanted threshold and the
// per-file counts of the matrix, on the device: what api.tags_at, matrix_io.popcount and split_bits do on the host, in one stream
// over the bytes (commet_hits_to_tags, commet_index_and_thresholds, commet_index_many_and_thresholds; capi/thresholds.hpp).
//
// A tile = 4096 reads = 64 tag words = one step of a workgroup of 256: lane i loads the 16 bytes of reads 16 i .. 16 i + 15 ONCE and
// keeps them in registers for all n_t thresholds.  Per batch of HT_BATCH thresholds every lane leaves its 16 compare bits in LDS, where four
// neighbouring lanes make one 64-bit word; behind a barrier wave w takes thresholds w, w + 4 of the batch and its lane l the word l
// of the tile: 64 lanes store 512 contiguous bytes of that threshold's vector, and the word's popcount is summed over the wave.
// Counts: a workgroup walks a contiguous run of tiles and keeps, per threshold, the sum of the tiles that lie within ONE file in LDS
// (acc[ti], written by lane 0 of the one wave that serves ti: no atomic); the sums go to `shared` when the file changes and at the
// end — n_t atomics per workgroup and file.  A tile that straddles a file boundary (or ends on one) takes the slow path: every lane
// cuts its word at the boundaries and adds each piece's popcount itself.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace commet {

constexpr int HT_TILE = 4096;       // reads per tile: 256 lanes x 16 bytes
constexpr int HT_BATCH = 8;         // thresholds per LDS round

// the file of read r: the first f with file_end[f] > r (file_end: running totals of the files' read counts; an empty file is never
// the answer).  r below file_end[n_files - 1]
__device__ __forceinline__ int ht_file_of(const uint64_t *__restrict__ file_end, int n_files, uint64_t r)
{
    int lo = 0, hi = n_files - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (file_end[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// hits: n bytes, 16-byte aligned.  tags: n_t vectors of tag_words = n / 64 + 1 words each, every word written (bits past n zero).
// shared: n_t x n_files counts, zeroed by the caller; nullptr: no counts (file_end is then not read).  The grid's workgroups share
// the ceil(tag_words / 64) tiles in contiguous runs of tiles_per_block
__global__ __launch_bounds__(256) void hits_tags_kernel(const uint8_t *__restrict__ hits, uint64_t n, int t_first, int n_t, uint64_t *__restrict__ tags,
                                                        uint64_t tag_words, const uint64_t *__restrict__ file_end, int n_files,
                                                        unsigned long long *__restrict__ shared, uint64_t tiles_per_block)
{
    __shared__ uint64_t words[HT_BATCH * 64];      // [threshold of the batch][word of the tile]; written as 16-bit pieces
    __shared__ unsigned long long acc[256];        // per threshold: reads of acc_file counted by this workgroup and not yet added
    uint16_t *const pieces = reinterpret_cast<uint16_t *>(words);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t n_tiles = (tag_words + 63) / 64;
    const uint64_t tile0 = blockIdx.x * tiles_per_block, tile1 = min(tile0 + tiles_per_block, n_tiles);
    acc[tid] = 0;
    int acc_file = -1, f = 0;                       // (uniform over the workgroup)
    auto flush = [&]() {                            // called by every lane, behind a barrier
        if (acc_file >= 0 && tid < n_t && acc[tid]) atomicAdd(&shared[(uint64_t) tid * n_files + acc_file], acc[tid]);
        acc[tid] = 0;
        __syncthreads();
    };
    __syncthreads();
    for (uint64_t tile = tile0; tile < tile1; ++tile) {
        const uint64_t r0 = tile * HT_TILE, r1 = min(r0 + HT_TILE, n);
        // ---- the lane's 16 bytes, zero past n
        const uint64_t at = r0 + 16ull * tid;
        uint32_t b[4] = {0, 0, 0, 0};
        if (at + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4 *>(hits + at);
            b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
        } else {
            for (uint64_t i = at; i < n; ++i) b[(i - at) >> 2] |= (uint32_t) hits[i] << (8 * ((i - at) & 3));
        }
        // ---- how the tile's reads are counted: 0 not at all, 1 all in file f, 2 lane by lane
        int how = 0;
        if (shared && r0 < n) {
            if (tile == tile0) f = ht_file_of(file_end, n_files, r0);
            while (file_end[f] <= r0) ++f;              // (the tiles of a run follow each other: so do their files)
            how = file_end[f] >= r1 ? 1 : 2;
            if (how == 1 && acc_file != f) {
                flush();
                acc_file = f;
            }
        }
        for (int tb = 0; tb < n_t; tb += HT_BATCH) {
            const int nb = min(HT_BATCH, n_t - tb);
            for (int q = 0; q < nb; ++q) {
                const uint32_t t = (uint32_t) (t_first + tb + q);
                uint32_t m = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) m |= (uint32_t) (((b[i >> 2] >> (8 * (i & 3))) & 0xFFu) >= t) << i;
                pieces[q * 256 + tid] = (uint16_t) m;
            }
            __syncthreads();
            for (int q = wave; q < nb; q += 4) {
                const uint64_t w = tile * 64 + lane, word = words[q * 64 + lane];
                const int ti = tb + q;
                if (w < tag_words) tags[(uint64_t) ti * tag_words + w] = word;
                if (how == 1) {
                    uint32_t cnt = (uint32_t) __popcll(word);
                    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
                    if (lane == 0) acc[ti] += cnt;
                } else if (how == 2 && word) {
                    // the word's reads [p, e) file by file; its set bits all lie below n
                    uint64_t p = w * 64;
                    const uint64_t e = min(p + 64, n);
                    int g = f;
                    while (p < e) {
                        while (file_end[g] <= p) ++g;
                        const uint64_t stop = min(file_end[g], e);
                        const uint64_t lo = p - w * 64, len = stop - p;
                        const uint64_t mask = (len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << lo;
                        const int cnt = __popcll(word & mask);
                        if (cnt) atomicAdd(&shared[(uint64_t) ti * n_files + g], (unsigned long long) cnt);
                        p = stop;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (shared) flush();
}

}  // namespace commet
