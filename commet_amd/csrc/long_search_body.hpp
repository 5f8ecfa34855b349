// long_search_body.hpp — the body of search_long_kernel (long_search.hpp), included there into both kernel templates: text, not a
// function.  (Inlined through a __device__ function the instantiations of one job allocate their registers differently — NF = 8:
// 58 -> 64 SGPRs kept in VGPR lanes — and their lines in tools/kernel_resources.py are to stay as measured.)
// Expects W, NF, COUNT, JOBS and rv, fg, k, t, sel, tags, counters, cstride, probe_counter, al, job_mask, job_tag_words.
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const uint64_t n_items = (!JOBS && al.ids) ? (uint64_t) *al.n : rv.n;
    const KeyCtx<W> kc(k);
    const uint32_t all = (fg.g >= 32) ? ~0u : ((1u << fg.g) - 1u);   // filters of the pass, one bit each
    const uint32_t opens = (job_mask | 1u) & all;                    // (JOBS) filters that open a job
    unsigned long long probes = 0;
    uint32_t n_scanned[NF], n_found[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) n_scanned[i] = 0, n_found[i] = 0;

    for (uint64_t item = wave0; item < n_items; item += n_waves) {   // (uniform per wave)
        uint64_t r = item;
        if constexpr (JOBS) {
            // (every read of the set, for every job)
        } else if (al.ids) {
            r = (uint64_t) al.ids[item];
        } else {
            const uint64_t selw = sel ? sel[r >> 6] : ~0ull, tagw = tags ? tags[r >> 6] : 0ull;
            if (!(((selw & ~tagw) >> (r & 63ull)) & 1ull)) continue;
        }
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int found_chunk = -1;                              // lowest filter of the pass that tagged the read
        uint32_t found = 0;                                // (JOBS) filters that reached t hits
        unsigned long long fprobes[NF];                    // (COUNT) what the reference loads for filter i if it gets that far
#pragma unroll
        for (int i = 0; i < NF; ++i) fprobes[i] = 0;
        uint32_t want = all;                               // filters whose answer still matters: below the lowest one that found the read
        for (int strand = 0; strand < 2 && want; ++strand) {
            int next_free[NF], count[NF];
#pragma unroll
            for (int i = 0; i < NF; ++i) next_free[i] = 0, count[i] = 0;
            uint32_t open = want;                          // filters whose scan of this strand goes on
            if constexpr (!COUNT) {
                if ((int64_t) len < (int64_t) t * k) open = 0;   // no room for t windows
            }
            for (int base = 0; base < n_win && open; base += 64) {
                // the read's words this block's windows stand on, one per lane, handed out by shuffles (every lane)
                const int s = base + lane, q = s + k - 1;
                ItemWords<W> it;
                wave_block_words<W>(p, n_words, base, lane, q, it);
                W ka, kb;
                const bool valid = kc.window_keys(it, q, strand, ka, kb) && s < n_win;
                // which filters this lane asks: open ones whose last hit the window does not overlap
                uint32_t ask = 0;
#pragma unroll
                for (int i = 0; i < NF; ++i)
                    if (valid && ((open >> i) & 1u) && s >= next_free[i]) ask |= 1u << i;
                uint32_t xa[NF];
                uint32_t bit = 0;
                if (ask) {
                    const W addr = psi_a<W>(ka, k);
                    long_load_a<NF>(fg.il_a + (uint64_t) (addr >> 5) * NF, xa);
                    bit = (uint32_t) addr & 31u;
                } else {
#pragma unroll
                    for (int i = 0; i < NF; ++i) xa[i] = 0;
                }
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    if (!((open >> i) & 1u)) continue;     // (uniform)
                    const bool asked = (ask >> i) & 1u;
                    const bool ha = asked && ((xa[i] >> bit) & 1u);
                    bool full = false;
                    uint64_t m_valid = 0, m_a = 0, m_b = 0, m_c = 0;
                    const PlanesBCD f = planes_bcd(fg, i);
                    if constexpr (COUNT) {
                        const bool hb = ha && test_bit<W>(f.b, kb);
                        const bool hc = hb && test_bit<W>(f.c, ka ^ kb);
                        full = hc && test_bit<W>(f.d, ka | kb);
                        m_valid = __ballot(asked), m_a = __ballot(ha), m_b = __ballot(hb), m_c = __ballot(hc);
                    } else {
                        full = ha && probe_bcd_chain<W>(f, ka, kb);
                    }
                    uint64_t m = __ballot(full);
                    // the greedy walk, by the whole wave; `passed` = the window starts of this block the reference looks at
                    uint64_t passed = 0;
                    int from = max(next_free[i] - base, 0);          // (block-relative)
                    bool ends = false;
                    while (true) {
                        if (from < 64) m &= ~0ull << from;
                        else m = 0;
                        if (!m) {
                            if (from < 64) passed |= ~0ull << from;
                            break;
                        }
                        const int b = __ffsll((unsigned long long) m) - 1;
                        passed |= (~0ull << from) & (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1ull));
                        ++count[i];
                        next_free[i] = base + b + k;
                        from = b + k;
                        if (count[i] >= t) {
                            ends = true;
                            if constexpr (JOBS) {
                                // filter i is answered, and the chunks behind it in ITS job are not searched; the other jobs go on
                                const uint32_t closed = (1u << i) | job_behind(opens, all, i);
                                found |= 1u << i;
                                want &= ~closed, open &= ~closed;
                            } else if (found_chunk < 0 || i < found_chunk) {
                                found_chunk = i;
                            }
                            break;
                        }
                        if constexpr (!COUNT) {
                            if (next_free[i] > (int) len - (t - count[i]) * k) {   // the missing hits no longer fit
                                ends = true;
                                break;
                            }
                        }
                    }
                    if constexpr (COUNT)
                        fprobes[i] += (unsigned long long) (__popcll(passed & m_valid) + __popcll(passed & m_a) + __popcll(passed & m_b) + __popcll(passed & m_c));
                    if (ends) open &= ~(1u << i);
                }
                if (found_chunk >= 0) {
                    // the reference does not search a read in the chunks behind the one that tagged it
                    want &= (1u << found_chunk) - 1u;
                    open &= want;
                }
                if constexpr (!COUNT) {
                    // first window of the next block past every place a missing hit could start: the scan of this strand is over
#pragma unroll
                    for (int i = 0; i < NF; ++i)
                        if (((open >> i) & 1u) && max(base + 64, next_free[i]) > (int) len - (t - count[i]) * k) open &= ~(1u << i);
                }
            }
        }
        if constexpr (JOBS) {
            // scanned_i: no earlier chunk of filter i's job tagged the read; found_i: chunk i did, and with it its job: one atomic OR
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                if (i >= fg.g || (found & job_before(opens, i))) continue;     // (uniform)
                ++n_scanned[i];
                if (!((found >> i) & 1u)) continue;
                ++n_found[i];
                const uint32_t job = (uint32_t) __popc(opens & ((2u << i) - 1u)) - 1u;
                if (tags && lane == 0)
                    (void) __hip_atomic_fetch_or(tags + (uint64_t) job * job_tag_words + (r >> 6), 1ull << (r & 63ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            continue;
        }
        // scanned_i: the read reached chunk i (no earlier chunk of the pass tagged it); found_i: chunk i tagged it
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            if (i < fg.g && (found_chunk < 0 || found_chunk >= i)) {
                ++n_scanned[i];
                if constexpr (COUNT) probes += fprobes[i];
            }
            if (found_chunk == i) ++n_found[i];
        }
        if (found_chunk >= 0 && tags && lane == 0)
            (void) __hip_atomic_fetch_or(tags + (r >> 6), 1ull << (r & 63ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) {
        if (counters) {
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                if (n_scanned[i]) atomicAdd(&counters[(uint64_t) i * cstride], (unsigned long long) n_scanned[i]);
                if (n_found[i]) atomicAdd(&counters[(uint64_t) i * cstride + 1], (unsigned long long) n_found[i]);
            }
        }
        if (COUNT && probe_counter && probes) atomicAdd(probe_counter, probes);
    }
