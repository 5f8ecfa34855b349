// hit_profile_wave_body.hpp — the body of hits_group_wave_kernel (hit_profile_group.hpp, JOBS = false) and hits_jobs_wave_kernel
// (hit_profile_jobs.hpp, JOBS = true), included into both: text, not a function, as long_search_body.hpp is.  (Inlined through a
// __device__ function, the six hits_group_wave_kernel number their scalar registers differently, 98 -> 100 and 100 -> 102 SGPRs in
// code of the same size, and their lines in tools/kernel_resources.py are to stay as measured; hits_lanes, the lane-per-read body, is
// a function because there nothing moves.)
// Expects W, NF, JOBS, REL and rv, fg, k, max_hits, js, sel, hits, lines, walked, al, thr.  JOBS = false: max_hits and al are the
// kernel's, js and lines are not looked at.  JOBS = true: js and lines are the kernel's, max_hits is not looked at, al is empty.
// REL (one job; rel_group_wave_kernel, relative_search.hpp): the cap is the read's own, thr[r], max_hits is not looked at, and `hits`
// holds found flags: a read with no cap or a flag is not walked, and its flag is set iff a count reaches the cap.
//
// A wave per read: the blocks of hits_wave_kernel (64 consecutive windows per block, staged words, shuffles, persistent grid; (JOBS)
// `sel` skips the unvisited reads, there is no list).  Per block ONE interleaved plane-A load per lane serves every slot and both
// strands; per (slot, strand) one ballot of full hits, walked greedily by the whole wave up to max_hits, (JOBS) the cap of the slot's
// job.  All uniform per-slot state lives in lanes, lane i the forward strand of slot i and lane NF + i its reverse complement:
// (next_free, count) in st_next / st_count, (JOBS) the slot's cap and mates in lane_cap / lane_mates (the bytes of JobSlots, spread
// once per wave); the whole wave reads them with readlane, their lane writes them, and the slots of a pass are a loop over i < g with
// no table of 2 NF states and 3 NF plane pointers in scalar registers.  (next_free, count) are carried from block to block: slot i's
// hit in the last windows of block b forbids slot i's first windows of block b + 1, and nobody else's.
// One job: blocks behind the one in which any count reaches max_hits are not loaded.  Several: the block loop ends when no state
// wants a window (min_next == INT_MAX) or the read ends; a job that is decided does not end it for the others, and blocks behind the
// one in which every job is decided are not loaded.
    static_assert(NF == 2 || NF == 4 || NF == 8, "passes of 2, 4 or 8 filter slots");
    const int lane = threadIdx.x & 63;
    const uint64_t wave0 = (uint64_t) blockIdx.x * (LONG_WG / 64) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t) gridDim.x * (LONG_WG / 64);
    const uint64_t n_items = al.ids ? (uint64_t) *al.n : rv.n;   // ((JOBS) no list)
    const KeyCtx<W> kc(k);
    const int g = fg.g;
    // the lane's slot (lanes 0 .. 2 NF - 1 hold a state), (JOBS) its job's cap and the slots of its job
    const int my_slot = lane & (NF - 1);
    const bool holds_state = lane < 2 * NF && my_slot < g;
    const uint32_t lane_cap = JOBS && holds_state ? slot_byte<NF>(js.caps, my_slot) : 0u;
    const uint32_t lane_mates = JOBS && holds_state ? slot_byte<NF>(js.mates, my_slot) : 0u;
    unsigned long long n_walked = 0;

    for (uint64_t item = wave0; item < n_items; item += n_waves) {   // (uniform per wave)
        uint64_t r = item;
        if (al.ids) r = (uint64_t) al.ids[item];
        else if (sel && !((sel[r >> 6] >> (r & 63ull)) & 1ull)) continue;
        int before = 0;
        int read_cap = max_hits;                           // (one job) where the walk of the read stops
        if constexpr (REL) {
            read_cap = __builtin_amdgcn_readfirstlane((int) thr[r]);
            if (read_cap == 0 || hits[r] != 0) continue;
        } else if constexpr (!JOBS) {
            before = (int) hits[r];
            if (before >= max_hits) continue;
        }
        ++n_walked;
        uint64_t t0;
        uint32_t len;
        read_extent(rv, r, t0, len);
        const uint32_t *p = rv.planes + 3 * t0;
        const int n_words = (int) ((len + 31u) >> 5);
        const int n_win = (int) len - k + 1;               // windows of the read, by their start (<= 0: none)
        int st_next = JOBS && !holds_state ? INT_MAX : 0, st_count = 0;
        int min_next = 0;                                  // the lowest next_free of the 2 g: a window in front of it is wanted by nobody
        int best = 0;                                      // (one job) the highest of the 2 g counts
        const auto more = [&] {                            // the block loop's end: see the last paragraph above
            if constexpr (JOBS) return min_next != INT_MAX;
            else return best < read_cap;
        };
        for (int base = 0; base < n_win && more(); base += 64) {
            const int s = base + lane, q = s + k - 1;
            ItemWords<W> it;
            wave_block_words<W>(p, n_words, base, lane, q, it);   // (every lane)
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
                int cap = read_cap;
                if constexpr (JOBS) cap = __builtin_amdgcn_readlane((int) lane_cap, i);
#pragma unroll
                for (int strand = 0; strand < 2; ++strand) {
                    const int slot = i + strand * NF;
                    int next_free = __builtin_amdgcn_readlane(st_next, slot), count = __builtin_amdgcn_readlane(st_count, slot);
                    // ((JOBS) a state of a decided job: next_free = INT_MAX, no lane is full)
                    const bool full = wanted && s >= next_free && ((x >> (strand ? bit_r : bit_f)) & 1u) &&
                                      probe_bcd_chain<W>(bcd, strand ? kar : kaf, strand ? kbr : kbf);
                    const uint64_t m = __ballot(full);
                    if (!m) continue;
                    greedy_take(m, base, k, cap, next_free, count);   // (by the whole wave)
                    if (lane == slot) st_next = next_free, st_count = count;
                    if constexpr (JOBS) {
                        // The job's byte is decided: every state of that job, both strands of all mates, gets next_free = INT_MAX: mates
                        // later in this block's slot loop take no more hits, and no state of the job wants a window of a later block.
                        // Mates EARLIER in the slot loop may already have counted hits of this block that lie behind the capping hit —
                        // which the lane form, window by window, never sees.  That changes no byte: every count still stops at the
                        // cap, and byte = min(cap, max over the job's slots of max(F, R)) is the cap either way
                        if (count >= cap) {
                            const uint32_t stop = (uint32_t) __builtin_amdgcn_readlane((int) lane_mates, i);
                            if (lane < 2 * NF && ((stop >> my_slot) & 1u)) st_next = INT_MAX;
                        }
                    } else {
                        best = max(best, count);
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
        if constexpr (JOBS) {
            // per job, at its first slot: the fold over its slots (lane i < NF: max(F, R) of slot i)
            const int both = max(st_count, __shfl(st_count, lane + NF, 64));
            int job = 0;
#pragma unroll 1
            for (int i = 0; i < g; ++i) {                  // (uniform)
                const uint32_t mates = (uint32_t) __builtin_amdgcn_readlane((int) lane_mates, i);
                if ((mates & (0u - mates)) != (1u << i)) continue;      // (not the first slot of a job)
                int most = 0;
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    if ((mates >> j) & 1u) most = max(most, __builtin_amdgcn_readlane(both, j));
                const int h = min(most, __builtin_amdgcn_readlane((int) lane_cap, i));
                if (lane == 0 && h) hits[(uint64_t) job * lines * 256ull + r] = (uint8_t) h;
                ++job;
            }
        } else if constexpr (REL) {
            if (lane == 0 && best >= read_cap) hits[r] = 1;
        } else {
            const int h = min(max_hits, best);
            if (lane == 0 && h > before) hits[r] = (uint8_t) h;
        }
    }
    if (walked && lane == 0 && n_walked) atomicAdd(walked, n_walked);
