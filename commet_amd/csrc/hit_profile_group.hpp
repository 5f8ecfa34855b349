// hit_profile_group.hpp — hits_group_kernel and hits_group_wave_kernel: the hits passes of hit_profile.hpp over a GROUP of up to eight
// chunk filters, one walk of the read and one plane-A request per window for all of them (commet_index_and_profile, capi/profile.hpp).
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
// (<= max_hits <= 255) are bytes of one word per strand.  The lane kernel walks its lane-a candidates bit by bit and addresses each
// one's slot per lane; the wave kernel keeps its uniform state in the lanes of two registers and loops over the g filters.  Either
// way no table of per-slot plane pointers is held in scalar registers, and none of the twelve instantiations spills.
//
// Included by capi.hip behind hit_profile.hpp (long_load_a, planes_bcd, FilterGroupView as well); not meant to stand alone.
#pragma once

namespace commet {

// ---------------------------------------------------------------------------
// a lane per read: the walk of hits_kernel, NF filters' states side by side
// ---------------------------------------------------------------------------
template <typename W, int NF>
__global__ __launch_bounds__(256) COMMET_SGPRS void hits_group_kernel(ReadsView rv, FilterGroupView fg, int k, int max_hits,
                                                                      const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                                      unsigned long long *__restrict__ walked, ActiveList al)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "groups of 2, 4 or 8 filter slots");
    const SearchLane me = search_lane(rv, al, sel, nullptr);
    const uint64_t r = me.r;
    int before = 0;
    bool walk = false;
    if (me.active) {
        before = (int) hits[r];
        walk = before < max_hits;
    }
    if (walk) {
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const KeyCtx<W> kc(k);
        W wh = 0, wl = 0;
        uint32_t run = 0;
        // [filter]: first window start the strand's state takes again (never, for the slots behind the group's filters); the hits of
        // filter i on a strand are byte i of cnt_f / cnt_r
        int free_f[NF], free_r[NF];
        uint64_t cnt_f = 0, cnt_r = 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) free_f[i] = free_r[i] = i < fg.g ? 0 : INT_MAX;
        int min_free = 0;                           // the lowest of the 2 NF: a window in front of it is wanted by nobody
        int best = 0;                               // the highest of the 2 NF counts
        for (uint32_t w = 0; w * 32u < len && best < max_hits; ++w) {
            const uint32_t hi = p[3 * w], lo = p[3 * w + 1], va = p[3 * w + 2];
            const uint32_t nb = min(32u, len - w * 32u);
            for (uint32_t j = 0; j < nb && best < max_hits; ++j) {
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
                // the lane-a candidates among the states that want the window: bit i = filter i forward, bit NF + i = its reverse complement
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
                    best = max(best, (int) ((cnt >> (8 * i)) & 255ull));
#pragma unroll
                    for (int q = 0; q < NF; ++q) {
                        if (q == i && !rev) free_f[q] = start + k;
                        if (q == i && rev) free_r[q] = start + k;
                    }
                }
                if (hit) {
                    min_free = INT_MAX;
#pragma unroll
                    for (int i = 0; i < NF; ++i) min_free = min(min_free, min(free_f[i], free_r[i]));
                }
            }
        }
        const int h = min(max_hits, best);
        if (h > before) hits[r] = (uint8_t) h;
    }
    if (walked) {
        __shared__ unsigned int wg_walked;
        if (threadIdx.x == 0) wg_walked = 0;
        __syncthreads();
        add_walked(walked, walk, wg_walked);
    }
}

// ---------------------------------------------------------------------------
// a wave per read: the blocks of hits_wave_kernel (64 consecutive windows per block, staged words, shuffles, persistent grid).  Per
// block one interleaved plane-A load per lane serves every filter and both strands; per filter and strand one ballot of full hits,
// walked greedily by the whole wave.  (next_free, count) per filter and strand are uniform over the wave and carried from block to
// block: filter i's hit in the last windows of block b forbids filter i's first windows of block b + 1, and nobody else's.  Blocks
// behind the one in which any count reaches max_hits are not loaded.
// ---------------------------------------------------------------------------
template <typename W, int NF>
__global__ __launch_bounds__(LONG_WG) void hits_group_wave_kernel(ReadsView rv, FilterGroupView fg, int k, int max_hits,
                                                                  const uint64_t *__restrict__ sel, uint8_t *__restrict__ hits,
                                                                  unsigned long long *__restrict__ walked, ActiveList al)
{
    static_assert(NF == 2 || NF == 4 || NF == 8, "groups of 2, 4 or 8 filter slots");
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const uint64_t n_items = al.ids ? (uint64_t) *al.n : rv.n;
    const KeyCtx<W> kc(k);
    const int g = fg.g;
    unsigned long long n_walked = 0;

    for (uint64_t item = wave0; item < n_items; item += n_waves) {   // (uniform per wave)
        uint64_t r = item;
        if (al.ids) r = (uint64_t) al.ids[item];
        else if (sel && !((sel[r >> 6] >> (r & 63ull)) & 1ull)) continue;
        const int before = (int) hits[r];
        if (before >= max_hits) continue;
        ++n_walked;
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        // (next_free, count) of filter i: lane i of the two state registers holds the forward strand's, lane NF + i the reverse
        // complement's.  Uniform values, read with readlane by the whole wave and written by their lane: the filters of the group
        // are then a loop over i < g, with no table of 2 NF states and 3 NF plane pointers to keep in scalar registers
        int st_next = 0, st_count = 0;
        int min_next = 0;                                  // the lowest next_free of the 2 g: a window in front of it is wanted by nobody
        int best = 0;                                      // the highest of the 2 g counts
        for (int base = 0; base < n_win && best < max_hits; base += 64) {
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
                uint32_t x = xa[0];                        // filter i's word of the load
#pragma unroll
                for (int j = 1; j < NF; ++j) x = (i == j) ? xa[j] : x;
                const PlanesBCD bcd = planes_bcd(fg, i);
#pragma unroll
                for (int strand = 0; strand < 2; ++strand) {
                    const int slot = i + strand * NF;
                    int next_free = __builtin_amdgcn_readlane(st_next, slot), count = __builtin_amdgcn_readlane(st_count, slot);
                    const bool full = wanted && s >= next_free && ((x >> (strand ? bit_r : bit_f)) & 1u) &&
                                      probe_bcd_chain<W>(bcd, strand ? kar : kaf, strand ? kbr : kbf);
                    // the greedy walk, by the whole wave (block-relative window starts)
                    uint64_t m = __ballot(full);
                    if (!m) continue;
                    int from = max(next_free - base, 0);
                    while (from < 64 && count < max_hits) {
                        m &= ~0ull << from;
                        if (!m) break;
                        const int b = __ffsll((unsigned long long) m) - 1;
                        ++count;
                        next_free = base + b + k;
                        from = b + k;
                    }
                    if (lane == slot) st_next = next_free, st_count = count;
                    best = max(best, count);
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
        const int h = min(max_hits, best);
        if (lane == 0 && h > before) hits[r] = (uint8_t) h;
    }
    if (walked && lane == 0 && n_walked) atomicAdd(walked, n_walked);
}

}  // namespace commet
