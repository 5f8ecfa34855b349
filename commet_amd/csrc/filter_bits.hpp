// filter_bits.hpp — the set bits of a filter slot AS STORED, one 64-bit word per bit; tests only (commet_filter_set_bits).
//
// A chunk of a few thousand reads sets 10^5 .. 10^6 of the up to 2^40 bits of a slot: their list is exact at every k where the
// reference's byte layout (export_reference_kernel, 2^(k-1) bytes) no longer fits a host.  The scan knows nothing of keys: plane A
// is reported at the address the bit sits at, psi_a is NOT applied — the test's own mirror of it is the independent side.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace commet {

// slot: the four planes of one filter slot, plane p at words [p * plane_words, (p + 1) * plane_words) — 4 * plane_words words, so a
// whole number of 16-byte vectors whatever k (a slot starts on a 16-byte boundary).  plane_bits = 2^k: k < 5 leaves most of a plane's
// one word unused, and what lies there is no bit of the filter.
// out[pos] = (plane << 56) | address for every set bit, pos taken from *count (which ends as the number of set bits: past cap
// nothing is written); order unspecified.
__global__ __launch_bounds__(256) void filter_set_bits_kernel(const uint32_t *__restrict__ slot, uint64_t plane_words, uint64_t plane_bits,
                                                              uint64_t cap, uint64_t *__restrict__ out, unsigned long long *__restrict__ count)
{
    const uint64_t stride = (uint64_t) gridDim.x * 256ull;
    for (uint64_t v = blockIdx.x * 256ull + threadIdx.x; v < plane_words; v += stride) {
        const uint4 x = ((const uint4 *) slot)[v];
        if (!(x.x | x.y | x.z | x.w)) continue;
        const uint32_t w4[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t w = 4 * v + j, plane = w / plane_words, base = (w - plane * plane_words) << 5;
            uint32_t bits = w4[j];
            if (plane_bits < 32) bits &= (1u << plane_bits) - 1u;
            if (!bits) continue;
            unsigned long long pos = atomicAdd(count, (unsigned long long) __popc(bits));
            for (; bits; bits &= bits - 1, ++pos)
                if (pos < cap) out[pos] = (plane << 56) | (base + (uint64_t) (__ffs(bits) - 1));
        }
    }
}

}  // namespace commet
