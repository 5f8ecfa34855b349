// capi/state.hpp — what every part of the C-ABI implementation shares: error reporting, launch bookkeeping, the context and
// read-set objects behind the opaque handles of include/commet_hip.h, the per-launch timing scope.
// (a part of the one translation unit capi.hip: included there first, after the kernel headers)
#pragma once

using namespace commet;

namespace {

thread_local std::string g_err;

constexpr int HITS_TAGS_BLOCKS = 2048;          // workgroups of a hits_tags_kernel launch at most: eight per CU (capi/thresholds.hpp)

// Every kernel launch of the library notes its entry point here (the host-side handle hipLaunchKernel takes): the
// test-suite resolves the addresses against the library's symbol table and checks that every instantiation compiled
// into it was reached by a parity test (commet_launched_kernels, tests/test_gpu_zz_dispatch_coverage.py).
std::mutex g_launch_mu;
std::set<const void *> g_launched;
inline void note_launch(const void *entry)
{
    // (the sliced / wide regimes issue thousands of launches per job, from two host threads: only an entry point this thread has
    // not noted lately takes the lock)
    thread_local const void *recent[16] = {nullptr};
    thread_local unsigned next = 0;
    for (const void *r : recent)
        if (r == entry) return;
    recent[next++ & 15u] = entry;
    std::lock_guard<std::mutex> lk(g_launch_mu);
    g_launched.insert(entry);
}
// a call site notes its kernel once (a template's call site: once per instantiation)
#define COMMET_LAUNCH(kernel, ...)                                   \
    do {                                                              \
        static std::atomic<bool> noted_{false};                       \
        if (!noted_.load(std::memory_order_relaxed)) {                \
            note_launch((const void *) (kernel));                     \
            noted_.store(true, std::memory_order_relaxed);            \
        }                                                             \
        hipLaunchKernelGGL(kernel, __VA_ARGS__);                      \
    } while (0)

// Run-time choices -> template arguments: f is called with the case that applies, and a call site instantiates its kernels
// for every case listed and no other.
// f(W{}) with W the key type of k-mers of length k: uint32_t up to 32, uint64_t above
template <typename F>
decltype(auto) with_key(int k, F &&f)
{
    if (k <= 32) return f(uint32_t{});
    return f(uint64_t{});
}
// f(std::integral_constant<V>) for the first of the listed values V that equals v; the last one when none does
template <auto V, auto... Vs, typename T, typename F>
decltype(auto) with_value(T v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<decltype(V), V>{});
    } else {
        if (v == V) return f(std::integral_constant<decltype(V), V>{});
        return with_value<Vs...>(v, f);
    }
}

// ---- device memory kept for reuse: the cache of host/devmem.hpp (why, and its rules, there) over the HIP runtime ----------------------
struct HipDriver {
    using Err = hipError_t;
    using Stream = hipStream_t;
    static constexpr Err ok = hipSuccess, oom = hipErrorOutOfMemory;
    static Err cleared(Err e)                                        // an error answered is HIP's last error no longer
    {
        if (e != hipSuccess) (void) hipGetLastError();
        return e;
    }
    Err current(int *dev) { return hipGetDevice(dev); }
    void set_device(int dev) { (void) hipSetDevice(dev); }
    Err alloc(void **p, size_t bytes) { return cleared(hipMalloc(p, bytes)); }
    Err free(void *p) { return hipFree(p); }
    Stream new_stream()
    {
        Stream st = nullptr;
        return cleared(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) == hipSuccess ? st : nullptr;
    }
    Err pool_alloc(void **p, size_t bytes, Stream st)
    {
        const Err e = hipMallocAsync(p, bytes, st);
        return cleared(e == hipSuccess ? hipStreamSynchronize(st) : e);
    }
    void pool_free(void *p, Stream st) { (void) hipFreeAsync(p, st), (void) hipStreamSynchronize(st); }
    void pool_trim(int dev)
    {
        int cur = 0;
        hipMemPool_t pool;
        const bool have = hipGetDevice(&cur) == hipSuccess;
        if (hipSetDevice(dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) (void) hipMemPoolTrimTo(pool, 0);
        if (have) (void) hipSetDevice(cur);
        (void) hipGetLastError();
    }
    Err sync() { return hipDeviceSynchronize(); }
    size_t total_bytes()
    {
        size_t fr = 0, tot = 0;
        return hipMemGetInfo(&fr, &tot) == hipSuccess ? tot : (size_t) 128 << 30;   // (not known: as a device of 128 GiB)
    }
    Err copy(void *dst, const void *src, size_t bytes) { return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice); }
};
HipDriver g_hip_driver;
DevMemCache<HipDriver> g_devmem(g_hip_driver);

hipError_t dm_malloc(void **p, size_t bytes, bool shareable = false) { return g_devmem.malloc(p, bytes, shareable); }
hipError_t dm_free(void *p) { return g_devmem.free(p); }
hipError_t dm_reserve(size_t bytes) { return g_devmem.reserve(bytes); }
hipError_t dm_make_shareable(void **p) { return g_devmem.make_shareable(p); }
size_t dm_trim(int device) { return g_devmem.trim(device); }
size_t dm_filed_bytes(int device) { return g_devmem.filed_bytes(device); }
size_t dm_pooled_bytes(int device) { return g_devmem.pooled_bytes(device); }

int fail(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define HIP_OK_NULL(expr)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);           \
            return nullptr;                                                                            \
        }                                                                                              \
    } while (0)

inline uint64_t bitmap_words(uint64_t n) { return n / 64 + 1; }
inline uint64_t bitmap_bytes_host(uint64_t n) { return n / 8 + 1; }   // boolean_vector.h:130

constexpr uint64_t STAGE_BASES = 64ull << 20;
constexpr uint64_t STAGE_READS = 1ull << 20;
constexpr int      N_COUNTERS = 8;

}  // namespace

struct commet_ctx {
    int device = 0;
    int k = 0, t = 0;
    hipStream_t stream = nullptr;
    uint32_t *filter = nullptr;       // 4 planes, contiguous
    uint64_t plane_words = 0;
    uint64_t filter_bytes = 0;
    unsigned long long *d_counters = nullptr;
    unsigned long long *h_counters = nullptr;   // pinned
    hipEvent_t ev_i0 = nullptr, ev_i1 = nullptr, ev_s0 = nullptr, ev_s1 = nullptr;
    bool have_index_ev = false, have_search_ev = false;
    bool count_probes = false;
    int index_mode = 0;               // 0 auto, 1 atomic kernel, 2 bucketed construction
    int part_packed = 1;              // option: final buckets as groups of three 19-bit keys in 8 bytes (index_part.hpp)
    int part_no_uni = 0;              // option: never take the uniform-length fast path of hist / scatter1 (tests, A/B timing)
    int part_list = 0;                // option: 0 = ragged sets take the item list in hist / scatter1 (index_part.hpp, LIST), 1 = never (the round planner)
    uint64_t part_min_kmers = 8ull << 20;
    // workspaces of the bucketed construction (index_part.hpp): two, so that the chunks of a group can be built on two
    // streams at once (the compute-bound hist / scatter1 of one chunk overlap the HBM-bound scatter2 / build of another)
    struct PartWs {
        uint32_t *bufA = nullptr, *bufB = nullptr;
        uint64_t cap_keys = 0, cap_b = 0;                          // bufA in keys; bufB in words (fewer in the packed geometry)
        uint32_t *hist = nullptr, *wl = nullptr;
        uint64_t *off = nullptr, *goff = nullptr;   // bucket offsets in keys / in 8-byte groups (packed final level)
        unsigned long long *cur2 = nullptr, *blockoff = nullptr;   // final-bucket cursors; scatter1 start positions [workgroup][coarse bucket]
        uint32_t *blockcnt = nullptr;                              // keys per [scatter1 workgroup][coarse bucket]
        uint32_t *items = nullptr, *itemblk = nullptr;             // ragged sets: the chunk's item list and the builder's block sums (index_part.hpp, LIST)
        uint64_t items_cap = 0, itemblk_cap = 0;
        uint64_t items_set = 0, items_first = 0, items_count = 0;  // whose list the buffer holds: (set uid, read range), no selection — 0 = nobody's
        uint32_t items_nblk = 0;
        uint32_t nb = 0;
        void release()
        {
            (void) dm_free(bufA); (void) dm_free(bufB); (void) dm_free(hist); (void) dm_free(wl); (void) dm_free(off); (void) dm_free(goff);
            (void) dm_free(cur2); (void) dm_free(blockoff); (void) dm_free(blockcnt); (void) dm_free(items); (void) dm_free(itemblk);
            *this = PartWs();
        }
    } part[2];
    unsigned long long *d_jobcnt = nullptr;   // per (chunk, set) counters of commet_index_and_search, kept between calls
    // the set bits of a bitmap over a set's reads as a list of read numbers, in order (sel_ids_kernel), and the block sums of the scan
    // that places them (blk[blocks] = the list's length); made by build_id_list (search_dispatch.hpp), kept and grown between calls
    struct IdList {
        uint32_t *ids = nullptr, *blk = nullptr;
        uint64_t ids_cap = 0, blk_cap = 0;
        void release()
        {
            (void) dm_free(ids); (void) dm_free(blk);
            *this = IdList();
        }
    };
    IdList sel_ids;                                  // the index selection of the running job
    IdList sel_ids2;                                 // the same for the second of two jobs whose chunks are built side by side (multi.hpp, two jobs per tiled scan)
    IdList act_ids;                                  // a sparse search pass: sel & ~tags
    uint64_t *d_mtags = nullptr;                     // found flags of the jobs of a commet_index_many_and_search pass (up to eight bitmaps over the search set)
    uint64_t mtags_cap = 0;
    uint8_t *d_hits = nullptr;                       // commet_index_and_profile: a hit-count byte per read of every search set of the call, kept between calls
    uint64_t hits_cap = 0;
    uint64_t *d_twords = nullptr;                    // the thresholds calls (capi/thresholds.hpp): file ends, per-file counts and tag words of a call's byte arrays, kept between calls
    uint64_t twords_cap = 0;
    uint16_t *d_thr = nullptr;                       // the relative search (capi/relative.hpp): a threshold per read of every search set of the call, in d_hits' layout, kept between calls
    uint64_t thr_cap = 0;
    int multi_job = 0;                               // option: 0 = commet_index_many_and_search shares passes between jobs where it can, 1 = job by job, 2 = as 0 + search sets of long reads; commet_index_many_and_profile the same (2 also shares hits passes on long-read search sets)
    int sparse_search = 0;                           // option: 0 auto (a pass over less than half of a set's reads), 1 never, 2 whenever a selection applies
    unsigned long long *d_plansum = nullptr;  // per-block k-mer sums of a selection (host planner input)
    uint64_t plansum_cap = 0;
    uint64_t jobcnt_cap = 0;
    hipStream_t aux_stream = nullptr;         // second lane of a chunk group's index phase
    hipStream_t load_stream = nullptr;        // everything that makes a read set (uploads, k-mer counts): a set may be loaded by one
                                              // host thread while another runs jobs on sets that are complete
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int index_lanes = 2;                      // option: 1 = build the chunks of a group one after the other
    bool stagger_armed = false;               // the second lane's chunk starts behind the first lane's scatter1 (index_dispatch.hpp)
    hipEvent_t ev_stagger = nullptr;

    int n_slots = 1;                  // filter slots allocated behind `filter` (chunk groups, kernels.hpp)
    int cur_slot = 0;                 // slot the index / search launch helpers work on
    int export_slot = 0;              // option "export_slot" (tests): the slot commet_filter_export_reference copies
    uint32_t *il_a = nullptr;         // interleaved A planes of a chunk group
    uint64_t il_words = 0;            // ... as allocated: stride x plane_words
    // option "kernel_timing": a hipEvent pair around every kernel launch of commet_index_and_search, on the stream the
    // kernel is launched on; per-kernel totals are read with commet_kernel_times (bench.py's roofline leg)
    struct KernelClock {
        struct Rec { const char *name; hipEvent_t a, b; };
        bool on = false;
        std::vector<Rec> open;                         // launches of the current call
        std::vector<hipEvent_t> spare;                 // events kept for the next call
        std::vector<std::string> names;                // totals, in first-seen order
        std::vector<uint64_t> launches;
        std::vector<double> total_ms;
        std::mutex mu;                                 // the totals: commet_readset_filter adds its kernel from the thread that makes the sets
        void add(const char *name, double ms)
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t i = 0;
            while (i < names.size() && names[i] != name) ++i;
            if (i == names.size()) names.push_back(name), launches.push_back(0), total_ms.push_back(0);
            launches[i] += 1;
            total_ms[i] += ms;
        }
        void count(const char *name, uint64_t n)         // a launch fact that is no time: `launches` of the entry grows by n
        {
            if (!on) return;
            std::lock_guard<std::mutex> lk(mu);
            size_t i = 0;
            while (i < names.size() && names[i] != name) ++i;
            if (i == names.size()) names.push_back(name), launches.push_back(0), total_ms.push_back(0);
            launches[i] += n;
        }
        hipEvent_t get()
        {
            hipEvent_t e = nullptr;
            if (!spare.empty()) e = spare.back(), spare.pop_back();
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
            return e;
        }
        void collect()                                  // after the stream has been synchronised
        {
            for (Rec &r : open) {
                float ms = 0;
                if (r.a && r.b && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) add(r.name, ms);
                if (r.a) spare.push_back(r.a);
                if (r.b) spare.push_back(r.b);
            }
            open.clear();
        }
        void reset()
        {
            std::lock_guard<std::mutex> lk(mu);
            names.clear(), launches.clear(), total_ms.clear();
        }
        void release()
        {
            collect();
            for (hipEvent_t e : spare) (void) hipEventDestroy(e);
            spare.clear();
        }
    } kclock;
    // the many-small-chunks regime (slice_search.hpp): staging bit-planes, bit-sliced tables, chunk descriptors
    uint32_t *slice_stage = nullptr, *slice_tables = nullptr;
    SliceChunk *d_slice_chunks = nullptr;
    uint64_t slice_stage_words = 0, slice_table_words = 0, slice_chunks_cap = 0;
    hipStream_t list_stream = nullptr;        // query lists are built here, beside the job's index kernels (build_query_list)
    hipEvent_t ev_list = nullptr;
    unsigned long long *d_ql_totals = nullptr;   // scratch of the list build's scan, kept (no hipFree on the job path)
    uint64_t ql_totals_cap = 0;
    uint8_t *d_qres = nullptr;        // tiled search (tile_search.hpp): one result byte per query record of the set being scanned
    uint64_t qres_cap = 0;
    int tq_hit_cap = TQ_HIT_CAP;      // option "tq_hit_cap" (tests): full hits a piece of the replay may post before its scans walk their own candidates
    int hits_tags_blocks = HITS_TAGS_BLOCKS;   // option "hits_tags_blocks" (tests): the most workgroups of a hits_tags_kernel launch
    int ordered_scan = 0;             // option "ordered_scan": 0 = ragged sets of 2^16 reads and more are walked in order of their window counts by the
                                      // gather kernels' first pass, 1 = never, 2 = whenever the set is ragged (tests)
    int mask_split = 0;               // option "mask_split": 0 = a pass over that list runs segment by segment, each with the mask width its reads need, 1 = one launch
    unsigned long long *d_lo_cnt = nullptr;   // scratch of that list's counting sort (class-major block counts), kept
    uint64_t lo_cnt_cap = 0;
    int tiled_mode = 0;               // option "tiled_search": 0 auto (large sets, groups of 1 or 2 chunks), 1 never, 2 whenever possible
    int profile_tiled = 0;            // option "profile_tiled": commet_index_and_profile through the tiled probe (hit_profile_tiled.hpp): 0 auto (sets of 2^20 reads and more whose list stays within query_list_max_mb), 1 never, 2 whenever the set's geometry allows it (capi/profile.hpp)
    // environment knobs, read ONCE in commet_create (nothing on the launch path calls getenv)
    bool job_verbose = false;         // COMMET_JOB_VERBOSE: host-side phase times of every commet_index_and_search call on stderr
    bool ingest_verbose = false;      // COMMET_INGEST_VERBOSE
    int slice_mode = 0;               // option: 0 auto, 1 never, 2 whenever k allows it
    int slice_gw = 0;                 // option: words per bit-sliced entry (32 chunks each); 0 = by the number of chunks
    int slice_wide = 0;               // option: wide rows (all chunk filters side by side, slice_search.hpp): 0 auto (more than 256 chunks), 1 never, 2 whenever the regime applies
    uint32_t wide_cap_words = 0;      // option "slice_wide_words": at most this many words per row (tests: several passes); 0 = the budget decides
    int profile_wide = 0;             // option: commet_index_and_profile through the wide rows (hit_profile_wide.hpp): 0 auto (more than 256 chunks, no search read of more than 300 bases), 1 never, 2 whenever 12 <= k <= 24 and the job has a chunk
    int profile_slice = 0;            // option: commet_index_and_profile through the narrow bit-sliced tables (hit_profile_sliced.hpp) where the wide rows do not apply: 0 auto (never, for now), 1 never, 2 whenever 12 <= k <= 24, the job has a chunk and no probes are counted
    uint32_t *wide_tables = nullptr;
    uint64_t wide_table_words = 0;
    uint64_t max_kmer_test = 0;       // option "max_kmer": chunk size override for tests (0 = the reference's constant)
    double *d_shannon = nullptr;      // Shannon terms of the read lengths shannon_lo .. shannon_hi (commet_readset_filter, host/filter_rule.hpp), kept between calls
    uint32_t shannon_lo = 0, shannon_hi = 0;
    int long_search = 0;              // option "long_search": 0 auto (sets outside the register-mask kernels and the tiled search whose longest read has LONG_MIN_MAX_LEN bases), 1 never, 2 whenever the set has a read (tests)
    int chunk_group = 8;              // option: chunks searched per pass (1 = one pass per chunk; more than 4 only where group8_ok)
    // pinned / device staging buffers of the parallel host ingest, kept for the next read set (hipHostMalloc is slow)
    struct IngestBuf {
        uint32_t *h_planes = nullptr;
        uint64_t *h_goff = nullptr;
        hipEvent_t done = nullptr;
    };
    std::vector<IngestBuf> ingest_pool;
    // pinned staging of commet_readset_offload / _restore (capi/residency.hpp): made on first use and kept — hipHostMalloc and
    // hipHostFree are slow, synchronising calls; one host thread moves sets at a time (the thread that makes read sets)
    struct AwayStage {
        uint8_t *h = nullptr;
        hipEvent_t done = nullptr;
        bool inflight = false;
    } away[2];

    // Derived data cached with the read sets (the tiled search's query lists, ~6 bytes per first-hit window: several times
    // the packed set itself) is accounted here and given back under pressure: least recently used lists first when the
    // budget is exceeded, every list that is not part of the running job when a device allocation fails.
    std::mutex ql_mu;                                 // guards the registry and every query list of the context
    std::vector<commet_readset *> sets;               // read sets alive on this context
    uint64_t ql_bytes = 0, ql_budget = 64ull << 30, ql_clock = 0, ql_evictions = 0;   // (budget: half the device when that is more, commet_create)
    uint64_t ql_max_list = 4ull << 30;                // auto mode: sets whose list (8 bytes per first-hit window, estimated) is larger keep the gather kernels

    uint32_t *slot_ptr(int i) const { return filter + (uint64_t) i * 4 * plane_words; }
    FilterView view() const { return view_of(cur_slot); }
    FilterView view_of(int slot) const
    {
        uint32_t *base = slot_ptr(slot);
        FilterView f;
        f.a = base;
        f.b = base + plane_words;
        f.c = base + 2 * plane_words;
        f.d = base + 3 * plane_words;
        return f;
    }
};

struct commet_readset {
    commet_ctx *ctx = nullptr;
    uint64_t max_reads = 0, max_bases = 0;
    uint64_t n_reads = 0, n_bases = 0;
    uint32_t *d_planes = nullptr;
    uint64_t *d_goff = nullptr;
    uint32_t *d_kcnt = nullptr;
    uint32_t *d_lenmm = nullptr;
    uint64_t *d_sel = nullptr, *d_tags = nullptr, *d_found = nullptr;   // bitmaps, bitmap_words(max_reads)
    struct Stage {
        uint8_t *h_bases = nullptr;
        uint64_t *h_offs = nullptr;
        uint8_t *d_bases = nullptr;
        uint64_t *d_offs = nullptr;
        hipEvent_t done = nullptr;
        bool inflight = false;
    } st[2];
    int cur = 0;
    bool acquired = false;
    uint64_t stage_bases = 0, stage_reads = 0;
    std::vector<FileSpan> files;
    std::vector<uint64_t> empty_reads;
    mutable std::vector<uint32_t> h_kcnt;      // host copy of d_kcnt, made on first use (host_counts)
    mutable std::vector<uint64_t> h_kprefix;   // prefix sums of h_kcnt (fast chunk planning)
    mutable bool have_host_counts = false;
    uint32_t uniform_len = 0;
    uint32_t max_kcnt = 0;
    uint32_t max_len = 0, min_len = 0;
    uint64_t uid = 0;                          // unique per read set of the process (a pointer may come back; a uid does not)
    uint64_t fhw_total = 0;                    // first-hit windows of all reads for the context's (k, t): sum of max(0, len - t k + 1) (finalize)
    // query list of the tiled search (tile_search.hpp): the set's lane-a addresses sorted by address slice, made on first use
    struct QueryList {
        unsigned long long *d_tile_off = nullptr;
        uint32_t *d_qaddr = nullptr, *d_tstart = nullptr;
        uint16_t *d_qwho = nullptr, *d_tlen = nullptr;
        uint64_t n_records = 0;
        uint32_t n_slices = 0, n_pieces = 0;
        int sbits = 0;
        bool built = false, failed = false;
        uint64_t bytes = 0, last_use = 0;           // HBM held; the context's ql_clock at the last scan that used the list
        void release()
        {
            (void) dm_free(d_tile_off); (void) dm_free(d_qaddr); (void) dm_free(d_qwho); (void) dm_free(d_tstart); (void) dm_free(d_tlen);
            *this = QueryList();
        }
    };
    mutable QueryList ql;
    // ... and the list of the tiled hit profile (hit_profile_tiled.hpp), built with t = 1: every complete window of every read.  When the
    // context's t_eff is 1 the profile uses `ql` itself; under the same rules as `ql` (accounted, evicted, dropped, offloaded)
    mutable QueryList pl;
    // the set's reads in order of their first-hit window counts (tile_search.hpp, lo_*_kernel): ragged sets only, made on the first pass
    // of a gather kernel that visits the whole set; ids[n_reads] = n_reads closes the list
    mutable uint32_t *d_len_order = nullptr;
    mutable bool len_order_failed = false;
    // ... cut by mask width (round 6): the list starts with the reads of most windows, so the register-mask kernel runs segment by
    // segment with the narrowest masks the segment's reads fit (search_dispatch.hpp, launch_search_group); segment s = reads
    // [start, start + count) of the list, its count also at d_len_order[n_reads + 1 + s] for the kernel
    struct LenSeg { uint32_t start, count; int mw; };
    mutable LenSeg len_seg[5];
    mutable int n_len_seg = 0;
    mutable uint32_t ql_wanted = 0;                 // scans that would have taken the tiled search had the set's (large) list existed (tiled_ok)
    mutable std::atomic<uint64_t> ql_reserved_at{0};  // g_devmem.trims() when the memory was set aside: a trim since then has given it back
    mutable std::atomic<bool> ql_reserved{false};   // the memory of the set's list waits in the library's device cache (commet_readset_reserve_cache): a list above the cap may be built
    mutable int in_job = 0;                         // calls that are using the set now (a depth: commet_index_many_and_search nests commet_index_and_search); written under
                                                    // ql_mu (SetUse below).  While it is not 0 the set's list stays, and the set is neither exported nor offloaded
    mutable uint64_t *d_filter_ws = nullptr;   // scratch of commet_readset_filter: three verdict bitmaps, the count and the list of its long reads; made on first use
    mutable uint64_t filter_ws_bytes = 0;
    bool host_packed = false;                  // some reads were packed on the host (host/ingest_pack.hpp): counts come from kmer_counts_kernel
    uint32_t host_min_len = 0xFFFFFFFFu, host_max_len = 0;
    bool finalized = false;
    // residency (capi/residency.hpp): an offloaded set keeps what defines it in pageable host memory of its own and holds no device block
    bool resident = true;                      // written under ql_mu; false from the moment an offload is accepted until a restore is complete
    bool moving = false;                       // an offload or a restore of the set is under way (ql_mu)
    uint8_t *h_away = nullptr;                 // planes, then the read offsets (ragged sets), as they lay on the device
    uint64_t away_bytes = 0;

    ReadsView view() const
    {
        ReadsView v;
        v.planes = d_planes;
        v.goff = d_goff;
        v.uniform_len = uniform_len;
        v.n = n_reads;
        return v;
    }
};

namespace {
// The sets a call works on, from its checks to its return: every entry point that reads a set's device buffers enters here.  enter()
// refuses an offloaded set and counts the call in the sets' in_job, both under ql_mu — so commet_readset_offload, which looks at in_job
// and clears `resident` under the same mutex, never takes the buffers from under a call that has passed its check (no check-then-act).
struct SetUse {
    commet_ctx *c;
    std::vector<const commet_readset *> sets;
    bool held = false;
    explicit SetUse(commet_ctx *c_) : c(c_) {}
    SetUse(commet_ctx *c_, const commet_readset *rs) : c(c_), sets(1, rs) {}
    void add(const commet_readset *rs) { sets.push_back(rs); }
    int enter()
    {
        std::lock_guard<std::mutex> lk(c->ql_mu);
        for (const commet_readset *rs : sets)
            if (!rs->resident) return fail("read set is offloaded");
        for (const commet_readset *rs : sets) ++rs->in_job;
        held = true;
        return 0;
    }
    ~SetUse()
    {
        if (!held) return;
        std::lock_guard<std::mutex> lk(c->ql_mu);
        for (const commet_readset *rs : sets) --rs->in_job;
    }
    SetUse(const SetUse &) = delete;
    SetUse &operator=(const SetUse &) = delete;
};

// times one kernel launch when option "kernel_timing" is on (no-op otherwise)
struct KScope {
    commet_ctx::KernelClock &kc;
    hipStream_t stream;
    size_t idx = ~(size_t) 0;
    KScope(commet_ctx *c, const char *name, hipStream_t s) : kc(c->kclock), stream(s)
    {
        if (!kc.on) return;
        commet_ctx::KernelClock::Rec r{name, kc.get(), kc.get()};
        if (r.a) (void) hipEventRecord(r.a, stream);
        idx = kc.open.size();
        kc.open.push_back(r);
    }
    ~KScope()
    {
        if (idx != ~(size_t) 0 && kc.open[idx].b) (void) hipEventRecord(kc.open[idx].b, stream);
    }
};
}  // namespace
