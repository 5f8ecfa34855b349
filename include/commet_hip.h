/*
 * commet_hip.h — C ABI of the MI355X-native index_and_search hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * The reference (pierrepeterlongo/commet) has no FFI for this path: its
 * boundary is the two free functions
 *     BloomFilter * index_reads (FileManager*, k, min_hits, max_kmer, &nb_indexed_reads)   include/index_reads.h:41
 *     unsigned long search_reads(const BloomFilter*, FileManager*, k, min_hits, &nb_searched) include/search_reads.h:34
 * plus the chunk loop of main() (src/index_and_search.cpp:241-277).  Those are
 * pull-based on a std::string iterator, which a device path cannot use, so the
 * entry points below are the batch-based equivalents.  Each
 * declaration cites the reference interface it replaces.  INTEGRATION.md shows
 * the binding a Commet maintainer would add in src/index_and_search.cpp.
 *
 * Conventions
 *   - every function returning int returns 0 on success, non-zero on error;
 *     commet_last_error() then gives a message (thread-local).
 *   - bit arrays are LSB-first per byte, exactly BooleanVector's layout
 *     (include/boolean_vector.h:73-80, 222-233): read i = byte i/8, mask 1<<(i%8).
 *     A bit array over n reads has n/8+1 bytes (boolean_vector.h:130).
 *   - one ctx per (device, stream); calls on one ctx are serialised by the
 *     caller; several ctxs may be used from several host threads.  One exception:
 *     read sets are made on a stream of their own, so ONE host thread may build read
 *     sets of a ctx (commet_readset_create ... commet_readset_finalize,
 *     commet_readset_from_*, commet_readset_load, commet_readset_filter, commet_readset_offload,
 *     commet_readset_restore) while another runs commet_index_and_search on sets that are
 *     complete (commet_amd/matrix.py does).  That thread may offload or restore set X while the
 *     job thread works on other sets; a set some call is using is never offloaded (refused).
 *   - there is NO CPU fallback: without a usable HIP device commet_create fails.
 */
#ifndef COMMET_HIP_H_
#define COMMET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct commet_ctx     commet_ctx;
typedef struct commet_readset commet_readset;

/* ---- library / device ---------------------------------------------------- */
const char *commet_version(void);
const char *commet_last_error(void);
/* number of HIP devices visible (0 if none / no driver) */
int         commet_device_count(void);

/* ---- context: k, t, the Bloom filter in HBM ------------------------------ */
/* Replaces `HashKey hash(kmer_size)` + `new BloomFilter(kmer_size)`
 * (hash_key.h:40-49, bloom_filter.h:61-81): binds a device, creates a stream,
 * allocates the 4-lane filter (2^(k-1) bytes of HBM, laid out as four bit-planes
 * of 2^k bits).  1 <= k <= 38; t < 1 behaves as t = 1 (search_reads.h:55).
 * Returns NULL on error. */
commet_ctx *commet_create(int device, int kmer_size, int min_hits);
void        commet_destroy(commet_ctx *ctx);
int         commet_kmer_size(const commet_ctx *ctx);
int         commet_min_hits(const commet_ctx *ctx);
/* max_kmer = (unsigned long)(1e9 / 2^(33-k))  (src/index_and_search.cpp:73,146) */
uint64_t    commet_max_kmer(const commet_ctx *ctx);
/* free / total memory of the context's device (a resident server decides from it which sets to keep) */
int         commet_device_memory(const commet_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/* blocks until everything queued on the ctx's stream has finished */
int         commet_synchronize(commet_ctx *ctx);

/* ---- read sets resident in HBM ------------------------------------------- */
/* Replaces FileManager + ReadFile as the *source of reads* (file_manager.h:38-49,
 * read_file.h:34-47): a read set is the virtual concatenation of its files;
 * reads are 2-bit packed on the device into bit-planes (+ a validity plane for
 * non-ACGT, alphabet.h:44-58).  max_reads / max_bases are capacity bounds
 * (e.g. #'>' lines and file size). */
commet_readset *commet_readset_create(commet_ctx *ctx, uint64_t max_reads, uint64_t max_bases);
void            commet_readset_destroy(commet_readset *rs);
/* Marks the start of a new file of the set (FileManager::addFile,
 * file_manager.h:117-171).  Must be called before the first append of each file. */
int             commet_readset_begin_file(commet_readset *rs);
/* Pinned staging, double-buffered.  acquire() hands out a pinned host buffer
 * (waiting for the copy that last used it); the parser writes sequence bytes
 * (ASCII, no separators) into *bases and read boundaries into *offsets
 * (offsets[0] = 0 ... offsets[n_reads] = bytes used); commit() queues the
 * hipMemcpyAsync + the packing kernel and returns at once. */
int             commet_readset_stage_acquire(commet_readset *rs, uint8_t **bases, uint64_t *bases_cap,
                                             uint64_t **offsets, uint64_t *reads_cap);
int             commet_readset_stage_commit(commet_readset *rs, uint64_t n_reads);
/* Convenience: copies (bases, offsets[n_reads+1]) through the staging buffers. */
int             commet_readset_append(commet_readset *rs, const uint8_t *bases, const uint64_t *offsets,
                                      uint64_t n_reads);
/* Host ingest of a whole set: opens the read files (FASTA or FASTQ, plain or gzip,
 * sniffed like file_manager.h:125-157; one per file of the set, in order), counts
 * their records, creates the read set and streams every record through the pinned
 * staging buffers (records as the reference reads them, fasta_file.h:155-175,
 * fastq_file.h:139-190).  Replaces FileManager::addFile + the ReadFile parsers for
 * resident sets (file_manager.h:117-171).  The set is NOT finalized.  NULL on error. */
commet_readset *commet_readset_from_fasta(commet_ctx *ctx, const char *const *paths, int n_paths);
/* Same, from file contents already in memory (plain FASTA / FASTQ text, one buffer per file of the set;
 * the buffers must stay valid until the call returns).  Records are parsed by several host threads
 * (COMMET_INGEST_THREADS, default 8) and uploaded out of order at their final positions. */
commet_readset *commet_readset_from_buffers(commet_ctx *ctx, const char *const *data, const uint64_t *sizes, int n_files);
/* reads of file `file_index` of the set (all records, selected or not) */
uint64_t        commet_readset_file_reads(const commet_readset *rs, uint64_t file_index);
/* Ends loading: waits for the uploads, fetches the per-read counts of complete
 * k-mers (what index_reads.h:55-57 would feed) needed for exact chunking. */
int             commet_readset_finalize(commet_readset *rs);
/* Packed image of a finalized read set (the bit-planes as they lie in HBM + file spans; independent of k): written
 * once by whoever parsed the files, loaded by every other context that needs the set — other GPUs of the node in the
 * N x N driver (one parse per set instead of one per GPU), or a later process.  load returns a set that still has to
 * be finalized; its per-read k-mer counts are recomputed on the device for the loading context's k.  The reference
 * has no counterpart: every index_and_search process re-parses its files (file_manager.h:117-171). */
int             commet_readset_save(const commet_readset *rs, const char *path);
commet_readset *commet_readset_load(commet_ctx *ctx, const char *path);
/* The same hand-over WITHOUT a file, for the processes of one node: export writes a descriptor (file spans, lengths, and the
 * HIP IPC handles of the set's device buffers — dmabuf mode, HSA_ENABLE_IPC_MODE_LEGACY=0) into blob (blob == NULL: only
 * *blob_bytes, the size needed); import, in another process on any device of the node that reaches the owner's (xGMI), or
 * on the same device, opens the handles, copies the planes device to device into a set of its own (2.4 GB of a 50 M-read
 * set: a few tens of ms, against 0.5 s to write and 0.2 s to read the image through /dev/shm) and closes them.  The
 * imported set still has to be finalized.  The OWNER'S SET MUST STAY ALIVE until every importer has returned. */
int             commet_readset_export(const commet_readset *rs, void *blob, uint64_t cap, uint64_t *blob_bytes);
commet_readset *commet_readset_import(commet_ctx *ctx, const void *blob, uint64_t blob_bytes);
uint64_t        commet_readset_num_reads(const commet_readset *rs);
uint64_t        commet_readset_num_files(const commet_readset *rs);
/* kmers_out[n_reads]: complete k-mers of each read (valid after finalize) */
int             commet_readset_kmer_counts(const commet_readset *rs, uint32_t *kmers_out);
/* Replaces one `filter_reads <file> -l -n -e -m` run per file of the set (src/filter_reads.cpp:186-205, 265-306; Commet.py:103-121) for a
 * FINALIZED resident set: one pass over the packed planes gives every read's length and A / C / G / T / other counts, the verdicts
 * follow the tool's order (length, then N, then Shannon: index < min_shannon as floats, the terms f * log(f) / log(2) taken from a
 * table the host fills with the tool's own expression, so no device transcendental decides), and the tool's sequential loop — stop
 * at the first empty record or once max_reads_per_file reads are selected, counters over the reads before the stop,
 * untag_last_reads — runs per file, as one tool run per file does.  min_len: -l; max_n: -n (< 0: any); min_shannon: -e (<= 0: not
 * computed, as in the tool); max_reads_per_file: -m (< 0: all).  select_out (n/8+1 bytes over the set-wide read numbers, padding
 * bits zero) is bit for bit the tool's vectors, file after file: the form commet_index_and_search takes as index_select /
 * search_select.  per_file (num_files entries, may be NULL) carries what the tool prints for each file.  Runs on the stream that
 * makes read sets (see Conventions). */
typedef struct {
    uint64_t reads;            /* records of the file                                  */
    uint64_t selected;         /* "Number of selected reads"                           */
    uint64_t removed_length;   /* "Length filter [l]: ... reads removed"               */
    uint64_t removed_n;        /* "Number of N filter [n]: ... reads removed"          */
    uint64_t removed_shannon;  /* "Shannon filter [e]: ... reads removed"              */
} commet_filter_stats;
int             commet_readset_filter(commet_ctx *ctx, const commet_readset *rs, int min_len, int64_t max_n /* <0: any */,
                                      float min_shannon, int64_t max_reads_per_file /* <0: all */,
                                      uint8_t *select_out /* set-wide, n/8+1 bytes */, commet_filter_stats *per_file /* num_files, may be NULL */);
/* Derived data cached WITH a resident set: the query list of the tiled search (the set's lane-a addresses sorted by
 * address slice; depends on (k, t) and the set only, made on the set's first scan, ~6 bytes per first-hit window — 2.2 GB
 * for 10 M x 100 bp reads at k = 32, t = 2, against 0.5 GB for the packed set).  The lists of a context are held to a
 * budget (option "query_list_budget_mb", COMMET_QUERY_LIST_GB; default: half the device's memory, at least 64 GiB): the least recently used ones are given
 * back first, and all of them (but the running job's) when a device allocation of the context fails, which is then
 * tried again.  cache_bytes: HBM the set's list holds now; drop_cache: give it back (rebuilt on the next scan that
 * wants it; no-op while a job uses the set); cache_stats: the context's totals.  No counterpart in the reference. */
uint64_t        commet_readset_cache_bytes(const commet_readset *rs);
void            commet_readset_drop_cache(commet_readset *rs);
int             commet_cache_stats(commet_ctx *ctx, uint64_t *bytes, uint64_t *budget_bytes, uint64_t *evictions);
/* A finalized set leaves HBM and comes back.  The reference runs one job at a time from disk, so the number of sets it compares is
 * unbounded (Commet.py:186-240, file_manager.h:117-171); a driver whose sets together exceed the device sends the ones it does not need
 * for a while to host memory.  offload copies what defines the set — the planes, the read offsets of a ragged set; file spans and
 * lengths are host data already — into PAGEABLE host memory the set owns (chunk-wise through two pinned staging buffers), releases every device block of the set to the library's device cache
 * (commet_device_cache_trim gives them to the driver) and drops the set's query list and length-order list, which the next scan that
 * wants them rebuilds as after commet_readset_drop_cache.  restore allocates again, copies back and recomputes the per-read k-mer
 * counts on the device as commet_readset_load does: from then on the set is what it was — commet_readset_save writes the same bytes,
 * every job gives the same tags and stats, commet_readset_filter the same bits.  When the device is out of memory restore gives the
 * device cache and the query lists of other sets back once, then fails and leaves the set offloaded and usable.
 * Both run on the stream that makes read sets (see Conventions).  Both are refused, with a message and nothing changed: on a set that
 * is not finalized; offload while any call is using the set (decided and marked under one lock with the jobs' own entry: there is no
 * window between the check and the release) or when it is offloaded already; restore when it is resident.  While a set is offloaded
 * commet_index_reads, commet_search_reads, commet_index_and_search, commet_index_many_and_search, commet_readset_filter, _export,
 * _save, _kmer_counts and _reserve_cache fail with "read set is offloaded"; commet_readset_destroy works in either state.
 * is_resident: 1 when the set is on the device.  device_bytes: what the set's own buffers (not its query list: cache_bytes) hold on
 * the device now, 0 when offloaded.  packed_bytes: what they hold when resident, in either state — a planner's number.  Both count the
 * blocks as the library asks for them (rounded to its size classes); a block handed out by the device cache may be up to a quarter
 * larger than asked, and the blocks an offload releases stay in that cache (at most half the device, COMMET_DEVMEM_CACHE_GB) until an
 * allocation needs them or commet_device_cache_trim is called: a budget kept with these numbers bounds the sets that are live, the
 * device cache comes on top and is the first thing given back under pressure.  The pinned staging buffers (2 x 8 MiB) are the
 * context's, made on first use and kept. */
int             commet_readset_offload(commet_readset *rs);
int             commet_readset_restore(commet_readset *rs);
int             commet_readset_is_resident(const commet_readset *rs);
uint64_t        commet_readset_device_bytes(const commet_readset *rs);
uint64_t        commet_readset_packed_bytes(const commet_readset *rs);
/* packed_bytes of the set commet_readset_from_fasta would make of these files, from a count of their records on the host (no device
 * is touched): what a planner needs BEFORE any set is parsed.  reads / bases / packed_bytes may each be NULL. */
int             commet_files_packed_bytes(const char *const *paths, int n_paths, uint64_t *reads, uint64_t *bases, uint64_t *packed_bytes);
/* Device memory the library keeps for reuse.  On this driver a hipMalloc of GBs costs 15-30 ms per GiB and now and then blocks
 * for 50-150 ms behind the hipFree of tens of GB, so blocks of 8 MiB or more that a context, a read set or a cache gives up are
 * filed per device (at most half the device, COMMET_DEVMEM_CACHE_GB) and handed to the next allocation they fit; they go back to
 * the driver when an allocation is out of memory, or here.  commet_device_cache_trim(device; -1 = every device) returns the bytes
 * released, commet_device_cache_bytes(device) what is filed now.  COMMET_DEVMEM_CACHE=0 turns the mechanism off.  Nothing in the
 * reference corresponds to it (its filters are plain `new char[]`, bloom_filter.h:73). */
uint64_t        commet_device_cache_trim(int device);
/* A query list above the cap (option "query_list_max_mb": 4 GiB, sets of ~15 M reads) costs its first user 15-30 ms per GiB of
 * driver time on a box whose device memory has not been touched yet — on the job's path.  A driver that knows a set will be scanned
 * again and again (the N x N matrix: a 50 M-read set's list is 11 GB and saves 12 ms per scan) calls commet_readset_reserve_cache
 * from a helper thread while its jobs run: the blocks the list will need (for the context's k and t) are asked from the driver there
 * and filed in the device cache; from then on the set may get its list whatever the cap says (built, as every list above 4 GiB,
 * for its second eligible scan).  _estimate returns the bytes such a list takes (0: the set does not qualify for the tiled search).
 * No-ops when the list exists, when the device cache is off, or when there is no room. */
uint64_t        commet_readset_cache_estimate(commet_ctx *ctx, const commet_readset *rs);
int             commet_readset_reserve_cache(commet_ctx *ctx, const commet_readset *rs);
uint64_t        commet_device_cache_bytes(int device);
/* COMMET_DEVMEM_POOL=1 (off by default): new blocks of 256 MiB or more come from the driver's stream-ordered pool (hipMallocAsync
 * on a stream of the library's own, drained before the block is used): 0.4-0.9 ms per GiB on every box, where hipMalloc takes
 * 30-60 ms per GiB on some and nothing on others (tools/exp/alloc_cost*.hip) — but kernels gather ~4 % more slowly from pool
 * memory and on a box of the second kind the 10-set matrix lost 1.8 s of 10.9 s with it (profiles/r05_pool), hence off.  No HIP
 * IPC handle exists for such memory: commet_readset_export moves the set's buffers into hipMalloc blocks first (once per set, a
 * device-to-device copy), and a caller that shares library memory by other means checks here.
 * commet_device_pooled_bytes(device): bytes of such blocks in use now. */
uint64_t        commet_device_pooled_bytes(int device);
/* What the library asked the DRIVER for on `device` (-1: every device) since the process started: host time its threads spent
 * inside hipMalloc / hipMallocAsync (ms), the bytes they returned and the number of calls — blocks taken from the library's own
 * cache do not count.  A box that charges a process for its first use of device memory (15-30 ms per GiB) shows
 * HERE and not in any kernel's time; the N x N driver reports the difference over a matrix leg as alloc_wait_ms / fresh_device_bytes.
 * Nothing in the reference corresponds to it. */
int             commet_device_alloc_stats(int device, double *wait_ms, uint64_t *fresh_bytes, uint64_t *calls);
/* Test hooks, off by default: the library's device allocations refused on request, as the driver refuses them when the device is
 * full (hipErrorOutOfMemory, before the device cache or the driver is asked), so that every no-room fallback can be run on small
 * shapes.  Process-wide.  at_least_bytes: every request of that many bytes or more is refused while armed (0 = off); nth: the nth
 * request from this call on is refused, once (1 = the next one, 0 = off) — the retry that follows it is request nth + 1 and goes
 * through.  Arming restarts the numbers that commet_device_alloc_requests reports: requests seen, requests refused, the byte count
 * of the last one refused (each may be NULL).  (0, 0) disarms.  Pinned host memory and blocks set aside ahead of time
 * (commet_readset_reserve_cache) are not refused. */
void            commet_device_alloc_refuse(uint64_t at_least_bytes, uint64_t nth);
void            commet_device_alloc_requests(uint64_t *requests, uint64_t *refused, uint64_t *last_refused_bytes);

/* ---- the two kernels ------------------------------------------------------ */
/* Replaces `new BloomFilter` per chunk (index_and_search.cpp:256-262,
 * bloom_filter.h:73-76): zeroes the filter (asynchronous). */
int commet_filter_reset(commet_ctx *ctx);

/* Replaces the body of index_reads (index_reads.h:49-61) for reads
 * [first, first+count) of rs whose select bit is 1 (select_bits indexed by the
 * set-wide read number, NULL = all): every complete k-mer sets its 4 lane bits
 * (bloom_filter.h:112-118).  Chunking (max_kmer, the dropped look-ahead read)
 * is decided by the caller / commet_index_and_search.  *kmers_fed (optional)
 * receives the number of k-mers fed; asking for it synchronises. */
int commet_index_reads(commet_ctx *ctx, const commet_readset *rs, uint64_t first, uint64_t count,
                       const uint8_t *select_bits, uint64_t *kmers_fed);

/* Replaces search_reads (search_reads.h:34-87) for the reads of rs whose
 * active bit is 1 (NULL = all): a read is found iff it has >= t non-overlapping
 * k-mers present in all 4 lanes, scanning forward keys first and
 * reverse-complement keys only if the forward scan failed.  found_bits
 * (n/8+1 bytes, caller-allocated) gets 1 for found reads and 0 for all others.
 * n_scanned = active reads, n_found = found reads (both optional). */
int commet_search_reads(commet_ctx *ctx, const commet_readset *rs, const uint8_t *active_bits,
                        uint8_t *found_bits, uint64_t *n_scanned, uint64_t *n_found);

/* ---- the chunk loop on resident sets --------------------------------------- */
typedef struct {
    uint64_t indexed;       /* nb_indexed_reads  (index_and_search.cpp:286: excludes dropped reads) */
    uint64_t searched;      /* nb_searched_reads of the LAST search pass (search_reads.h:39)        */
    uint64_t shared;        /* nb_found_reads summed over chunks                                    */
    double   search_ms;     /* device time of this set's search kernels (search_times[set_pos], :272) */
} commet_pair_stats;

typedef struct {
    uint64_t n_chunks;          /* filters built                          */
    uint64_t kmers_indexed;     /* k-mers fed over all chunks             */
    uint64_t reads_scanned;     /* search-read scans over all chunks/sets */
    uint64_t reads_indexed;     /* reads fed to a filter (dropped look-ahead reads excluded) */
    uint64_t index_launches;    /* index kernel launches                  */
    uint64_t search_launches;   /* search kernel launches                 */
    uint64_t probes;            /* filter words loaded by the search kernels = P_ref of the reference's
                                   control flow; 0 unless option "count_probes" is set */
    double   zero_ms;           /* device time: filter zeroing (hipEvents on the ctx stream) */
    double   index_ms;          /* device time: filter zeroing + index kernels */
    double   index_kernel_ms;   /* device time: index kernels only        */
    double   search_ms;         /* device time: search kernels            */
    double   total_ms;          /* host wall time of the call             */
} commet_job_info;

/* Replaces the while loop of main() (index_and_search.cpp:241-277) together
 * with the FileManager iteration rules it relies on (file_manager.h:88-112:
 * input-filter bits, skipping of already tagged reads, file switching;
 * index_reads.h:49,60: the look-ahead read that is dropped when a chunk fills):
 *   while reads remain in index_rs: build the filter of the next chunk, search
 *   every search set against it, OR the found bits into that set's tags.
 * index_select / search_select[i]: per-file input-filter bits concatenated over
 * the set (ReadFile::bv), NULL = all ones.  tags_out[i]: n_i/8+1 bytes, the
 * FileManager::file_bvs of search set i at the end (what save_bv writes).
 * stats[i] / info are optional. */
int commet_index_and_search(commet_ctx *ctx,
                            const commet_readset *index_rs, const uint8_t *index_select,
                            int n_search, const commet_readset *const *search_rs,
                            const uint8_t *const *search_select,
                            uint8_t *const *tags_out, commet_pair_stats *stats,
                            commet_job_info *info);
/* Several such jobs that search the SAME read set — Commet.py's J2 jobs of a reference set (Commet.py:220: for every other set S_i,
 * "S_ref in (S_i restricted to J1's result)") and its J3 jobs of a target (Commet.py:233) — in one call: job j indexes index_rs[j]
 * (restricted to index_select[j], may be NULL) and searches search_rs (search_select as above); tags_out[j], stats[j] are what
 * commet_index_and_search(index_rs[j], ..., 1, &search_rs, ...) gives for job j alone, bit for bit.  Where the jobs allow it
 * (index sets whose chunks, at most eight per job, take the bucketed construction; a search set that is visited
 * whole) the chunk filters of several jobs share a pass over the search set: the lane-a gathers of its reads, two thirds of a
 * job's memory requests, are then made once per pass instead of once per job: up to eight chunk filters per pass of the gather
 * kernel; on a search set that takes the tiled search, jobs of one chunk filter each two per scan (one probe of the set's query list,
 * one replay that keeps the two jobs apart).  A search set that takes the wave-per-read kernel (option "long_search") shares passes
 * under option "multi_job" = 2 only (not measured against the jobs alone yet, so not auto's choice): up to eight chunk filters of
 * several jobs per pass of search_long_kernel, one plane-A load per window for all of them; for such a search set the chunks may
 * also take the atomic index kernel (their slots are zeroed first).  Otherwise (and with option "multi_job" = 1, under a selection
 * on the search set, with "count_probes", for k <= 24 unless "slice_mode" = 1, for a job of more than eight chunks, or when the
 * device has no room for the slots of a shared pass) the jobs run one after the other.  info (may be NULL) sums over the jobs. */
int commet_index_many_and_search(commet_ctx *ctx, int n_jobs, const commet_readset *const *index_rs,
                                 const uint8_t *const *index_select, const commet_readset *search_rs,
                                 const uint8_t *search_select, uint8_t *const *tags_out, commet_pair_stats *stats,
                                 commet_job_info *info);

/* Hit profile: the chunk loop above with a search that does not stop at t.  No counterpart in the reference, whose tools answer one t
 * per run; one call here answers every t in 1..max_hits, and the filters, which do not depend on t, are built once.
 * hits_out[i]: n_i bytes, one per read of search set i (set-wide read numbers):
 * 0 for a read the search pass does not visit (search_select bit 0, plan_search), else
 * min(max_hits, max over the index set's chunks of max(F, R)), F / R = the greedy non-overlapping full hits of the
 * forward / reverse-complement scan of search_reads.h:45-83 run to the end of the read.  For every t in 1..max_hits,
 * (hits_out[i][r] >= t) is bit for bit the tag commet_index_and_search gives on a context of this k and that t.
 * The context's own t is not used.  max_hits in 1..255.
 * Up to eight chunk filters per pass over a search set, by option "chunk_group" (groups formed as in a job; 1 when k < 2): one walk
 * of the read and one plane-A request per window serve the whole group and both strands (hits_group_kernel, a lane per read;
 * hits_group_wave_kernel, a wave per read, by option "long_search").  A group of one chunk, and every chunk at chunk_group = 1,
 * takes the one-filter kernels (hits_kernel, hits_wave_kernel).  The bytes do not depend on the grouping.  index_mode, max_kmer and
 * index_lanes are honoured.  info (may be NULL) as in a job; search_launches = the passes (groups x non-empty search sets),
 * reads_scanned = the reads the passes walked (once per group pass; a read whose count has reached max_hits is not walked again),
 * probes = 0.
 * Many small chunks (12 <= k <= 24), by option "profile_wide": every chunk filter of a pass side by side in the wide bit-sliced rows
 * (as option "slice_wide" of a job), ONE hits_wide_kernel launch per search set and pass: a row pass over every window bounds each
 * chunk's count by the blocks of k window ends that hold a hit, and a chunk is replayed exactly only while its bound exceeds the
 * read's best count so far.  Several passes when "slice_wide_words" caps the rows or the table budget is small, folded by the bytes'
 * max; no room for the tables: the loop above.  search_launches = passes x non-empty search sets; reads_scanned = the reads a pass
 * walked (a read of fewer than k bases, or one already at min(max_hits, len / k), is not walked).  The bytes do not depend on it.
 * Large sets at 25 <= k <= 34, by option "profile_tiled": a pass of one or two chunk filters goes through the tiled probe — tq_probe_kernel
 * over the set's query list of (k, t = 1), which holds every complete window of every read (the search's own list on a context of
 * t = 1, else a second list cached with the set under the same rules: commet_readset_cache_bytes counts both), then
 * tq_hits_replay_kernel: the search's tq_replay_kernel with another last step — both collect the probe's results and sweep planes B, C, D
 * with the same code (tq_collect, tq_sweep); the search then stops at t hits and walks the tails, the profile counts the full hits
 * greedily per filter and strand.  Sparse passes, sets that take long_search, groups
 * of three filters and more, count_probes, and sets without room for the list run the kernels above.  The bytes do not depend on it.
 * Up to 256 chunks a pass (12 <= k <= 24), by option "profile_slice" where the wide rows do not take the call: the chunk filters of a pass, 32 x
 * slice_words of them, in the narrow bit-sliced tables (as option "slice_mode" of a job; slice_words and its 1 GiB clamp apply), ONE
 * hits_sliced_kernel launch per search set and pass, a lane per read: a row pass over every window ANDs all four planes and counts,
 * per chunk and strand, the blocks of k window ends that hold a full hit (1: the count is 1; 2: it is 1 or 2; three or more: at least
 * 2), and a chunk is replayed exactly only while its upper bound exceeds the read's best count so far.  Several passes fold by the
 * bytes' max; no room for the tables: the loop above.  search_launches, reads_scanned and index_launches (2 per pass) as for the wide
 * rows.  The bytes do not depend on it.
 * Several such jobs on one search set: commet_index_many_and_profile below. */
int commet_index_and_profile(commet_ctx *ctx, const commet_readset *index_rs, const uint8_t *index_select,
                             int n_search, const commet_readset *const *search_rs, const uint8_t *const *search_select,
                             int max_hits, uint8_t *const *hits_out, commet_job_info *info);
/* Several hit-profile jobs that search the SAME read set, in one call: job j indexes index_rs[j] (restricted to index_select[j], may
 * be NULL) and searches search_rs under search_select (may be NULL; the same for every job) with max_hits[j] in 1..255.
 * hits_out[j] (n bytes, n = the reads of search_rs) is byte for byte what commet_index_and_profile(ctx, index_rs[j],
 * index_select[j], 1, &search_rs, &search_select, max_hits[j], ...) gives for job j alone.  Jobs may index the same read set under
 * different selections (the threshold sweep of the symmetric comparison does: commet_amd/sweep.py --full).
 * The jobs, in their order, share a hits pass while their chunk filters fit min(8, chunk_group) slots (a job that runs alone, see below,
 * does not close a pass), a job never split between two passes:
 * one walk of a read and one plane-A request per window serve the filters of every job of the pass (hits_jobs_kernel, a lane per
 * read; hits_jobs_wave_kernel, a wave per read, for a search set of long reads under "multi_job" = 2); per job the byte is min(max_hits[j], max over ITS chunks of max(F, R)), and a job that reaches its cap stops for itself
 * alone.  The jobs' chunks are built one after the other on the context's stream (index_lanes plays no part here).
 * Through commet_index_and_profile itself, with the same bytes: every job when n_jobs < 2, k < 2, under count_probes, with option
 * "multi_job" = 1 or "chunk_group" = 1, for an empty search set or, unless "multi_job" is 2, one that takes the wave-per-read
 * hits kernel ("long_search"), and when the device has no room for the slots or the byte arrays of a pass; a single job when the device planner does not take it
 * (an empty read in its set, a file without a selected read, an empty selection), when it has no chunk or more chunks than a pass
 * holds, or when it is alone in its pass — such a job picks its own regime (wide rows, narrow tables, tiled probe) and its
 * neighbours still share.  "multi_job" = 0 (auto) shares where the search set takes a lane per read, as 2 does: measured faster
 * than the jobs one by one (MEASUREMENTS.md, "Jobs that share a hits pass"); a search set of long reads shares under 2 only.
 * info (may be NULL) sums over the jobs: search_launches = the passes (plus the launches of the jobs that ran alone), reads_scanned =
 * the reads the passes walked, probes = 0.
 * Open: the tiled probe and the bit-sliced tables for shared passes; shared passes for jobs
 * whose search selections differ (the third pass of the symmetric sweep). */
int commet_index_many_and_profile(commet_ctx *ctx, int n_jobs, const commet_readset *const *index_rs,
                                  const uint8_t *const *index_select, const commet_readset *search_rs,
                                  const uint8_t *search_select, const int *max_hits, uint8_t *const *hits_out,
                                  commet_job_info *info);

/* Thresholds: the profile calls above with the step behind the search made on the device too — hits_tags_kernel (hits_tags.hpp)
 * streams over the final hit-count bytes once and leaves, for every wanted threshold, the BooleanVector of the reads with at least
 * that many hits and, per file of the searched set (files are contiguous runs of set-wide read numbers, commet_readset_file_reads;
 * a file may hold no read), how many of its reads have them — the cells of the similarity matrix.  Only bits come down: no host
 * code thresholds bytes or counts bits.  Tag arrays have n / 8 + 1 bytes like every tag array of this header, padding bits zero.
 * When the device has no room for the tag words the bytes come down and a plain host loop makes the same tags and counts.
 *
 * commet_hits_to_tags: the kernel on HOST bytes (uploaded, thresholded, downloaded): tags_out[ti] = the reads r with
 * hits[r] >= t_first + ti for ti in 0..n_t - 1 (1 <= t_first, t_first + n_t - 1 <= 255), shared_out[ti * n_files + f] (may be NULL)
 * = those of them in file f; file_reads[0..n_files) must sum to n_reads.  A fast tags_at for large arrays, and the tests' handle. */
int commet_hits_to_tags(commet_ctx *ctx, const uint8_t *hits, uint64_t n_reads, int n_files, const uint64_t *file_reads,
                        int t_first, int n_t, uint8_t *const *tags_out, uint64_t *shared_out);
/* commet_index_and_profile with max_hits = max_t (1..255), leaving tags and counts instead of bytes: tags_out[s * max_t + (t - 1)]
 * is bit for bit what commet_index_and_search leaves for search set s on a context of this k and that t; shared_out (may be NULL;
 * same indexing) points to one count per file of set s.  Any entry of either array may be NULL.  The context's own t is not used. */
int commet_index_and_thresholds(commet_ctx *ctx, const commet_readset *index_rs, const uint8_t *index_select,
                                int n_search, const commet_readset *const *search_rs, const uint8_t *const *search_select,
                                int max_t, uint8_t *const *tags_out, uint64_t *const *shared_out, commet_job_info *info);
/* commet_index_many_and_profile with max_hits[j] = t[j], leaving job j's tags at t[j] in tags_out[j] and its per-file counts (one
 * per file of search_rs) in shared_out[j] (the array, and any entry of either, may be NULL): the many-job search with a threshold
 * per job.  The jobs share hits passes as there; a job that runs alone, and every job when a pass has no room, goes through the
 * single-job thresholds path. */
int commet_index_many_and_thresholds(commet_ctx *ctx, int n_jobs, const commet_readset *const *index_rs,
                                     const uint8_t *const *index_select, const commet_readset *search_rs,
                                     const uint8_t *search_select, const int *t, uint8_t *const *tags_out,
                                     uint64_t *const *shared_out, commet_job_info *info);

/* The search with a threshold PER READ, a share of what the read can hold (mixed-length sets: merged pairs, long reads).
 * The rule, for a read of len bases (every character counts, ACGT or not) on a context of k-mer size k:
 *     W_r = len / k                                       integer division: the most non-overlapping k-mers the read can hold
 *     t_r = max(min_hits, (percent * W_r + 99) / 100)     integer arithmetic; percent in 1..100; min_hits < 1 behaves as 1
 * Read r is found in one chunk filter iff max(F, R) >= t_r, F and R the greedy non-overlapping full hits of its forward and
 * reverse-complement scan, as for commet_index_and_profile.  Tags are ORed over the chunks of the index set, as in every job; counts
 * are never summed over chunks: a read whose k-mers are spread over two chunk filters is judged in each alone, as the reference
 * judges it.  A read with t_r > W_r can never be found and is not walked.  The plan (chunks, the dropped look-ahead read, selections,
 * file rules) is commet_index_and_profile's and does not depend on the rule.  Hence, where the rule gives every read the same t_r = t,
 * tags and counts are bit for bit commet_index_and_search's on a context of that t; and on any set, the bit of read r equals
 * (its byte of commet_index_and_profile at max_hits = T) >= t_r wherever t_r <= T <= 255.
 * t_r is held in 16 bits: a set whose longest read gives W_r > 65535 is refused with a message (k = 1 on reads above 65 kb and
 * its like).
 *
 * commet_readset_relative_thresholds: thr_out[r] = t_r of every read of rs under no selection, 0 where t_r > W_r
 * (rel_thresholds_kernel, relative_search.hpp): a planner's number, and the tests' handle on that kernel. */
int commet_readset_relative_thresholds(commet_ctx *ctx, const commet_readset *rs, int percent, int min_hits,
                                       uint16_t *thr_out /* n_reads */);
/* The job: the chunks of index_rs (restricted to index_select) in groups of up to "chunk_group" filters (1 when k < 2 or the job has
 * one chunk), every search set ONE pass per group by rel_kernel / rel_group_kernel (a lane per read) or, for sets that take
 * "long_search" as a profile does, rel_wave_kernel / rel_group_wave_kernel (a wave per read): the walks of the hit profile with the
 * read's own stop — a read found by an earlier pass, one with t_r > W_r and one not selected are not walked; the walk of a read ends
 * at its t_r-th hit in any filter on any strand.  A set whose largest t_r exceeds 255 takes the wave forms too, unless "long_search"
 * is 1 (or k < 2): then a filter per pass through rel_kernel.  Passes over few of a set's reads walk their list ("sparse_search").
 * tags_out[s] (n / 8 + 1 bytes, padding bits zero) = the BooleanVector of search set s, shared_out[s] = one count per file of set s,
 * both made on the device (hits_tags_kernel); the arrays' entries may be NULL.  The context's own t is not used.
 * info (may be NULL) as in a job: search_launches = the passes, reads_scanned = the reads the passes walked, probes = 0.
 * When the device has no room for the thresholds or the found flags the call fails with a message; the context stays usable.
 * Open: the tiled probe, the wide rows, the narrow tables and passes shared between jobs for this call. */
int commet_index_and_search_relative(commet_ctx *ctx, const commet_readset *index_rs, const uint8_t *index_select,
                                     int n_search, const commet_readset *const *search_rs, const uint8_t *const *search_select,
                                     int percent, int min_hits, uint8_t *const *tags_out, uint64_t *const *shared_out,
                                     commet_job_info *info);

/* ---- test / measurement hooks --------------------------------------------- */
/* Tunables / diagnostics, by name.  Unknown names are an error.  None of them changes a result bit, except the test
 * hook max_kmer.
 *   count_probes (0/1)   the search kernels count the filter words the REFERENCE flow loads (P_ref)
 *   index_mode (0/1/2)   0 auto, 1 atomic-OR kernel, 2 bucketed (LDS-tile) construction (20 <= k <= 34; an error where a launch cannot
 *                        take it).  Read length is no limit: a set with a read of more than 4096 k-mers or bases is built through the
 *                        chunk's item list, written by whole workgroups (part_items_fill_kernel) and cut into pieces of equal item
 *                        counts; such a set needs the list (part_list = 0, part_no_uni = 0, a chunk of fewer than 2^28 words and
 *                        2^32 items, room for the list) — without it auto takes the atomic kernel on a zeroed filter and 2 fails
 *   part_min_kmers       auto mode: chunks with fewer k-mers take the atomic kernel
 *   index_lanes (1/2)    2 = the chunks of a group are built on two streams (default)
 *   drop_workspaces      frees the scatter workspaces (the next bucketed index build allocates them again)
 *   chunk_group (1..8)   chunk filters searched per pass over a set (1 = the reference's order; in a job 5..8 only
 *                        for read sets with at most 255 first-hit windows per read — reads of up to 318 bases at k = 32, t = 2 — and for
 *                        sets that take long_search, else 4).  It governs commet_index_and_profile as well, whose kernels keep no
 *                        masks: any set takes 5..8 there; 1 = one hits pass per chunk filter
 *   tiled_search (0/1/2) large search sets against 1 or 2 chunk filters (25 <= k <= 34): lane-a gathers served from L2 slice
 *                        by slice from the set's cached query list; 0 = sets of 2^20 reads or more whose list fits 4 GiB,
 *                        1 = never, 2 = whenever possible
 *   slice_mode (0/1/2)   many-small-chunks regime (12 <= k <= 24): the filters of 32..256 chunks bit-sliced in one table
 *                        set and searched in ONE pass; 0 = from 8 chunks on, 1 = never, 2 = always
 *   slice_words          chunk filters per pass / 32 in that regime (0 auto, 1, 2, 4, 8)
 *   slice_wide (0/1/2)   that regime with EVERY chunk filter (up to 16 384 per pass) side by side in rows of one table and a
 *                        group of lanes per read (search_wide_kernel): 0 = jobs of more than 256 chunks, after a probe of the
 *                        first 64 chunk filters on a sample of the reads (few reads found early: wide rows; most: the narrow
 *                        tables, whose later passes skip the reads already found), 1 = never, 2 = always
 *   slice_wide_words     cap on the words per wide row (a multiple of 8, 32 chunk filters per word; 0 = by the memory free)
 *   profile_wide (0/1/2) commet_index_and_profile through the wide rows (hits_wide_kernel): 0 = jobs of more than 256 chunks whose
 *                        search sets hold no read of more than 300 bases (measured on 150-base reads), 1 = never (the slot loop,
 *                        launch for launch), 2 = whenever 12 <= k <= 24 and the job has a chunk; slice_wide_words caps its rows too
 *   profile_slice (0/1/2) commet_index_and_profile through the narrow bit-sliced tables (hits_sliced_kernel) where profile_wide does not take
 *                        the call: 0 = auto: never, until it is measured to pay, 1 = never, 2 = whenever 12 <= k <= 24, the job has a
 *                        chunk and count_probes is off; slice_words sets the chunk filters per pass as in a job
 *   profile_tiled (0/1/2) commet_index_and_profile through the tiled probe (tq_hits_replay_kernel): 0 = auto: sets of 2^20 reads or more whose
 *                        list, estimated at 8 bytes per k-mer, stays within query_list_max_mb (the bounds of tiled_search), 1 = never, 2 = every pass of one or two chunk filters over a set
 *                        with 25 <= k <= 34, 1..255 windows per read and fewer than 2^32 k-mers (tests; sets below 2^20 reads too);
 *                        independent of tiled_search; tq_hit_cap applies
 *   query_list_budget_mb HBM the cached query lists of the context's read sets may hold (see commet_readset_cache_bytes)
 *   query_list_max_mb    auto mode of tiled_search: largest list (estimated) a set may get, default 4096 (sets of up to ~15 M reads;
 *                        larger lists — a 50 M-read set's is 11 GB — pay in long-lived contexts only: allocating them costs
 *                        15-30 ms per GiB; lists of more than 4 GiB are built for a set's second eligible scan)
 *   multi_job (0/1/2)    commet_index_many_and_search: 0 = chunk filters of several jobs in one pass where possible (search sets that
 *                        take long_search: job by job), 1 = job by job, 2 = as 0, and search sets that take long_search share passes too;
 *                        commet_index_many_and_profile: 0 = jobs share hits passes where possible (search sets that take long_search:
 *                        job by job), 1 = job by job, 2 = as 0, and search sets that take long_search share hits passes too
 *   sparse_search (0/1/2) a pass over a SELECTION of a search set (a filter bv that leaves few reads: file_manager.h:88-112 skips the
 *                        others) walks the list of the selected, not yet tagged reads instead of the set's bitmap, so that every
 *                        lane of a wave has a read: 0 = when the host plan visits less than half of the set's reads, 1 = never,
 *                        2 = whenever a selection applies (tests)
 *   long_search (0/1/2)  sets with a read of more than 255 first-hit windows (no register masks, no tiled search): a WAVE per read, 64
 *                        consecutive windows per step, the reference's greedy rule on the ballots (search_long_kernel), groups of up to
 *                        eight chunk filters: 0 = such sets whose longest read has 5000 bases or more (measured: the lane-per-read
 *                        kernels win below 2500, the wave from 3000 on), 1 = never, 2 = whenever the set has a read (tests);
 *                        commet_index_many_and_search and commet_index_many_and_profile let the jobs of such a search set share
 *                        passes under multi_job = 2
 *   ordered_scan (0/1/2) ragged sets (reads of several lengths): the first pass of a gather kernel over a whole set walks its reads in
 *                        order of their first-hit window counts (a list made once per set: a workgroup lives as long as its longest
 *                        read, its other lanes idle meanwhile): 0 = sets of 2^16 reads and more, 1 = never, 2 = any ragged set (tests)
 *   mask_split (0/1)     a pass of the register-mask gather kernel over that list: 0 = segment by segment, each launched with the
 *                        narrowest masks its reads fit (the list starts with the reads of most windows), 1 = one launch at the set's width
 *   tq_hit_cap           TEST HOOK of the tiled search's replay: full hits a piece of 256 reads may post for its owners (default and
 *                        at most 1024; beyond it every scan of the piece walks its own candidates — same bits, slower); 0 forces that path
 *   hits_tags_blocks     TEST HOOK: the most workgroups a hits_tags_kernel launch takes (1..2048, default 2048: a launch of more tiles
 *                        of 4096 reads gives every workgroup a contiguous run of them; tests reach that walk at small sizes)
 *   part_no_uni (0/1)    1 = never take the fixed-read-length fast path of hist / scatter1 (nor the item list of ragged sets)
 *   part_list (0/1)      ragged sets (reads of several lengths): 0 = hist / scatter1 walk the chunk's item list (written out once per
 *                        chunk; the words of the coming round's items prefetched as on fixed-length sets), 1 = the round planner
 *   kernel_timing (0/1)  time every kernel launch of commet_index_and_search (commet_kernel_times)
 *   max_kmer             TEST HOOK: k-mers per index chunk instead of the reference's constant (0 = reference; the
 *                        results are then those of a reference built with that constant, index_and_search.cpp:73)
 *   export_slot (0..7)   TEST HOOK: the filter slot commet_filter_export_reference copies (default 0; a job builds the chunk filters
 *                        of a group into slots 0 .. g - 1 and leaves them there); the export fails when the context has no such slot
 *   poison (0..255)      TEST HOOK, an action: waits for the context's two job streams, fills every device buffer of the context that
 *                        is a BIT ARRAY with the byte — all filter slots, the interleaved A planes, the staging planes and the tables
 *                        of the bit-sliced regimes — and waits again.  A job must give the same bits afterwards: the bucketed build
 *                        zeroes no slot, it defines every tile itself.  No other buffer is touched (keys, offsets, lists, counters:
 *                        a stale one of those misread would be an address) */
int commet_set_option(commet_ctx *ctx, const char *name, int64_t value);
/* Copies the filter to the host in the REFERENCE byte layout (byte key/2,
 * even keys 0x80/40/20/10, odd keys 0x08/04/02/01 for a/b/c/d,
 * bloom_filter.h:63-70,114-117); out has 2^(k-1) bytes.  For parity tests.
 * The slot of option "export_slot" (default 0). */
int commet_filter_export_reference(commet_ctx *ctx, uint8_t *out, uint64_t out_bytes);
/* TEST HOOK. The set bits of the filter slot of option "export_slot", as stored: one 64-bit word per bit,
 * (plane << 56) | bit address within the plane (plane 0 = A at its psi_a address, 1..3 = B, C, D at `key`).
 * Only addresses below 2^k are reported. Order unspecified. Writes at most cap words; *n_out = set bits found
 * (> cap: the caller's list is incomplete). Fails like commet_filter_export_reference when the context has no such slot. */
int commet_filter_set_bits(commet_ctx *ctx, uint64_t *out, uint64_t cap, uint64_t *n_out);
/* Device time in ms of the most recent index / search kernel launch on this
 * ctx, measured with hipEvents on the ctx's stream (synchronises). */
int commet_last_kernel_ms(commet_ctx *ctx, double *index_ms, double *search_ms);
/* Per-kernel device times of the commet_index_and_search calls made since option "kernel_timing" was set to 1:
 * a hipEvent pair around every launch, on the stream the kernel runs on (the chunks of a group are then built on
 * one stream, so that the durations add up).  Fills at most cap entries, *n_out = kernels seen.  Synchronises.
 * One entry is no kernel: "part_scatter1_pieces" (launches = pieces the hist / scatter1 launches of long-read chunks were cut
 * into, summed; total_ms = 0). */
typedef struct {
    char     name[48];
    uint64_t launches;
    double   total_ms;
} commet_kernel_time;
int commet_kernel_times(commet_ctx *ctx, commet_kernel_time *out, int cap, int *n_out);
/* Entry points (host-side kernel handles, addresses inside this library) of every kernel the library has launched in
 * this process so far, whatever the context.  The test-suite resolves them against the library's symbol table to check
 * that every kernel instantiation compiled into the library is reached by a parity test.  Fills at most cap entries,
 * *n_out = how many there are. */
int commet_launched_kernels(const void **out, int cap, int *n_out);
/* Random 4-byte-gather / atomic-OR microbenchmarks over a table of
 * table_bytes (practical random-access ceilings): n_access
 * accesses, returns elapsed device ms in *ms.  atomic: 0 plain gather, 1 atomic
 * OR, 2 non-temporal gather, 3 agent-scope (L1-bypassing) gather; 4 / 5 time a
 * device-to-device copy / a fill of table_bytes instead (streaming ceilings). */
int commet_membench(commet_ctx *ctx, int atomic, uint64_t table_bytes, uint64_t n_access, double *ms);
/* LDS microbenchmark (what bounds the bucketed index construction): n_access
 * operations on uniformly random words of an n_words-word LDS table (power of
 * two, <= 32768) per workgroup of 512.  mode 0 atomic add, 1 atomic add with
 * the old value used (rank), 2 atomic OR, 3 store, 4 load, 5 as 1 but on
 * lane-private words (no two lanes share an address). */
int commet_ldsbench(commet_ctx *ctx, int mode, uint32_t n_words, uint64_t n_access, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* COMMET_HIP_H_ */
