// search_replay.hpp — the reference's control flow (search_reads.h:45-83), once, for the kernels that gather the lane-a bits of a
// read's windows first and replay the scan on them: search_group_kernel, search_group8_kernel (kernels.hpp), tq_replay_kernel
// (tile_search.hpp).  Device code only, everything inlined.  kernels.hpp includes this file behind the primitives it stands on
// (KeyTraits, test_bit, psi_a, ItemWords); it is not meant to be included on its own.
//
// A scan = one filter, one strand of one read: windows in order of their end q; a window is probed iff its k bases are ACGT and
// it ends at least k bases behind the scan's last full (4-lane) hit; t hits tag the read.  Exact pruning (see search_kernel): with
// `seen` hits a window ending at q matters only if q + (t-seen-1)*k <= last = len-1.  So the kernels gather the windows that can
// be a FIRST hit (q <= pe = last-(t-1)*k) and fetch later ones (the tail) only for a scan that has a hit, cooperatively.
#pragma once

namespace commet {

// keys of a window held LSB = oldest base (kernels.hpp, top): forward by bit reversal, reverse complement by complement
template <typename W> struct KeyCtx {
    int k, sh;
    W   mask;
    __device__ __forceinline__ explicit KeyCtx(int k_)
        : k(k_), sh(KeyTraits<W>::BITS - k_), mask((k_ == KeyTraits<W>::BITS) ? ~(W) 0 : (((W) 1 << k_) - 1)) {}
    __device__ __forceinline__ W key(W w, int strand) const { return strand ? (W) (~w & mask) : (W) (KeyTraits<W>::brev(w) >> sh); }
    // (a branch on purpose: written as two selects, tq_replay_kernel's balanced sweep holds 4-6 more VGPRs and its <uint64_t, 1, 6> and
    // <uint64_t, 1, 8> builds lose a workgroup per CU)
    __device__ __forceinline__ void strand_keys(W wh, W wl, int strand, W &ka, W &kb) const
    {
        if (strand) ka = ~wh & mask, kb = ~wl & mask;
        else ka = KeyTraits<W>::brev(wh) >> sh, kb = KeyTraits<W>::brev(wl) >> sh;
    }
    // keys of the window ending at base q of the read whose triples start at p; false if one of its bases is not ACGT
    __device__ __forceinline__ bool window_keys(const uint32_t *p, int q, int strand, W &ka, W &kb) const
    {
        ItemWords<W> it;
        it.load(p, (uint32_t) q >> 5);
        return window_keys(it, q, strand, ka, kb);
    }
    __device__ __forceinline__ bool window_keys(const ItemWords<W> &it, int q, int strand, W &ka, W &kb) const
    {
        W wh, wl;
        const bool complete = it.window((uint32_t) q & 31u, k, mask, wh, wl);
        strand_keys(wh, wl, strand, ka, kb);
        return complete;
    }
};

// planes B, C, D of filter slot i of a group (plane A is read through the interleaved copy)
struct PlanesBCD {
    const uint32_t *b, *c, *d;
};
__device__ __forceinline__ PlanesBCD planes_bcd(const FilterGroupView &fg, int i)
{
    const uint32_t *pb = fg.slot0 + (uint64_t) i * fg.slot_words + fg.plane_words;
    return {pb, pb + fg.plane_words, pb + 2 * fg.plane_words};
}

// Lanes b, c, d of a lane-a candidate, two forms (the difference is measured, each call site keeps its own):
// chain: short circuit b -> c -> d as the reference does (bloom_filter.h:124-131) — chance candidates, most fail at b;
template <typename W> __device__ __forceinline__ bool probe_bcd_chain(const PlanesBCD &f, W ka, W kb)
{
    return test_bit<W>(f.b, kb) && test_bit<W>(f.c, ka ^ kb) && test_bit<W>(f.d, ka | kb);
}
// together: three independent loads, one round trip — the candidates of a heavy scan and of a tail behind a full hit are almost
// all true k-mers of the index set, the short circuit would only serialise them.
template <typename W> __device__ __forceinline__ bool probe_bcd_together(const PlanesBCD &f, W ka, W kb)
{
    const W kc = ka ^ kb, kd = ka | kb;
    const uint32_t vb = f.b[kb >> 5], vc = f.c[kc >> 5], vd = f.d[kd >> 5];
    return (vb >> ((uint32_t) kb & 31u)) & (vc >> ((uint32_t) kc & 31u)) & (vd >> ((uint32_t) kd & 31u)) & 1u;
}

// State of one scan.  dead: no room left for the missing hits (or nothing to scan: the read is not searched, or an earlier filter
// of the job found it); found: t hits.  Either ends the scan.
struct StrandScan {
    int  seen = 0, next_ok = 0;   // full hits so far; first window end that no longer overlaps the last of them
    bool dead, found = false;
    __device__ __forceinline__ explicit StrandScan(bool searched) : dead(!searched) {}
    __device__ __forceinline__ bool open() const { return !found && !dead; }
    // Greedy walk of the set bits of m, lowest first; bit b = the window ending at q_of_bit0 + b.  is_hit(q): whether that window is
    // a full hit (`true` for a word of full hits, a B/C/D probe for a word of lane-a candidates).  The loop stops when the scan
    // does; a caller need not test open() first.
    template <typename F> __device__ __forceinline__ void walk(uint32_t m, int q_of_bit0, int t, int k, int last, F &&is_hit)
    {
        while (m && open()) {
            const int q = q_of_bit0 + (__ffs((int) m) - 1);
            m &= m - 1u;
            if (q < next_ok) continue;                 // overlaps the last hit: the reference has not refilled its window yet
            if (q + (t - seen - 1) * k > last) {       // the missing hits no longer fit behind this window
                dead = true;
                break;
            }
            if (!is_hit(q)) continue;
            ++seen;
            next_ok = q + k;                           // hash.clear(), search_reads.h:60: the next complete window ends k bases later
            if (seen >= t) found = true;
        }
    }
};

// The tail of a scan: windows behind the gathered ones (q > pe) matter only after a first full hit.  Their lane-a bits are fetched
// by the whole workgroup, WIN windows per request: the threads whose scan needs a tail post (thread, first window end qb), thread p
// takes window p % WIN of request p / WIN — one round trip with every lane busy, where a thread fetching its own windows kept the
// other lanes of its wave waiting through four (tq_replay_kernel: 1.8 ms of tails to 1.1) —, ORs a set lane-a bit into the
// owner's tail_bits word, and the owner walks that word.
//   tail_req[256], tail_bits[256], tail_n : LDS of the calling kernel
//   window_of(owner, q, wh, wl)           : the window ending at base q of thread `owner`'s read; false if the read ends before q
//                                           or a base of the window is not ACGT (no k-mer there)
//   il_a, fi                              : the group's interleaved A planes (stride GS) and the scan's filter
//   is_hit(q)                             : B/C/D probe of a window of the calling thread's own read
// Holds three barriers per round (uniform trip count): every thread of the 256 of the workgroup must call it, unconditionally and
// from uniform control flow, whether its scan is open or not.
template <typename W, int WIN, int GS, typename WindowOf, typename IsHit>
__device__ __forceinline__ void cooperative_tail(StrandScan &sc, uint32_t *tail_req, uint32_t *tail_bits, uint32_t &tail_n, const KeyCtx<W> &kc,
                                                 int strand, int t, int pe, int last, const uint32_t *__restrict__ il_a, int fi,
                                                 WindowOf &&window_of, IsHit &&is_hit)
{
    static_assert(WIN <= 32 && (WIN & (WIN - 1)) == 0, "a request's answers are one word of tail_bits");
    for (int qb = max(pe + 1, sc.next_ok);; qb += WIN) {
        const bool want = sc.open() && sc.seen >= 1 && qb <= last && qb + (t - sc.seen - 1) * kc.k <= last;
        if (threadIdx.x == 0) tail_n = 0;
        if (!__syncthreads_or(want)) break;
        if (want) {
            tail_req[atomicAdd(&tail_n, 1u)] = threadIdx.x | ((uint32_t) qb << 8);
            tail_bits[threadIdx.x] = 0;
        }
        __syncthreads();
        const uint32_t n_pairs = tail_n * (uint32_t) WIN;
        for (uint32_t pr = threadIdx.x; pr < n_pairs; pr += 256) {
            const uint32_t rq = tail_req[pr / WIN], owner = rq & 255u, wi = pr % WIN;
            W wh, wl;
            if (!window_of(owner, (int) (rq >> 8) + (int) wi, wh, wl)) continue;
            const W addr = psi_a<W>(kc.key(wh, strand), kc.k);
            const uint32_t v = il_a[(uint64_t) (addr >> 5) * GS + (uint32_t) fi];
            if ((v >> ((uint32_t) addr & 31u)) & 1u) atomicOr(&tail_bits[owner], 1u << wi);
        }
        __syncthreads();
        if (want) sc.walk(tail_bits[threadIdx.x], qb, t, kc.k, last, is_hit);
    }
}

}  // namespace commet
