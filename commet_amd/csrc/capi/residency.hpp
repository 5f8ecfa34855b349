// capi/residency.hpp — a finalized resident set leaves HBM and comes back: commet_readset_offload / _restore, what a set holds on the device, what a set of given files will hold
// (a part of the one translation unit capi.hip: included there, in order, after images.hpp)
//
// The reference runs one job at a time from disk, so the number of sets it can compare is unbounded (Commet.py:186-240,
// file_manager.h:117-171); here every set of a job is packed in HBM.  A driver whose sets together exceed the device (commet_amd/matrix.py
// under --set-budget-gb) sends the sets it does not need for a while to host memory and takes them back: plain copies on the stream
// that makes read sets, through two pinned staging buffers of the context; the host copy itself is pageable (a hundred sets away must not pin a
// hundred sets' worth of memory).  What is derived from the planes — the per-read k-mer counts, as commet_readset_load recomputes them;
// the query list and the length-order list, rebuilt by the next scan that wants them — does not travel.
#pragma once

namespace {

constexpr uint64_t AWAY_STAGE_BYTES = 8ull << 20;     // one pinned staging buffer of a set on its way out or back

// bytes the buffers of a set of this capacity hold on the device (commet_readset_create's allocations, as dm_malloc rounds them)
uint64_t set_device_bytes(uint64_t max_reads, uint64_t max_bases)
{
    const uint64_t triples = (max_bases >> 5) + max_reads + 1, bw = bitmap_words(max_reads);
    const uint64_t sizes[7] = {triples * 12, (max_reads + 1) * 8, (max_reads + 1) * 4, 8 * 4, bw * 8, bw * 8, bw * 8};
    uint64_t total = 0;
    for (uint64_t b : sizes) total += g_devmem.request_bytes((size_t) b);
    return total;
}

struct AwayLayout {
    uint64_t planes_bytes, goff_bytes, total;
    explicit AwayLayout(const commet_readset *rs)
    {
        planes_bytes = ((rs->n_bases >> 5) + rs->n_reads + 1) * 12;        // the triples in use (what a packed image carries)
        goff_bytes = rs->uniform_len ? 0 : (rs->n_reads + 1) * 8;          // (no kernel reads the offsets of a fixed-length set)
        total = planes_bytes + goff_bytes;
    }
};

// the context's two pinned staging buffers, made on first use (the set's own were given back by finalize; these stay with the context)
hipError_t away_stage_open(commet_ctx *c)
{
    for (commet_ctx::AwayStage &s : c->away) {
        hipError_t e = hipSuccess;
        if (!s.h) e = hipHostMalloc((void **) &s.h, AWAY_STAGE_BYTES);
        if (e == hipSuccess && !s.done) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        s.inflight = false;
    }
    return hipSuccess;
}

// device -> host memory of the set, chunk by chunk: the copy of one chunk into its pinned buffer runs while the host moves the
// chunk before it out of the other one
hipError_t away_copy_out(commet_readset *rs, const uint8_t *d_src, uint8_t *h_dst, uint64_t bytes)
{
    hipStream_t st = rs->ctx->load_stream;
    uint8_t *pend_dst[2] = {nullptr, nullptr};
    uint64_t pend_n[2] = {0, 0};
    int cur = 0;
    auto drain = [&](int b) -> hipError_t {
        commet_ctx::AwayStage &s = rs->ctx->away[b];
        if (!s.inflight) return hipSuccess;
        const hipError_t e = hipEventSynchronize(s.done);
        s.inflight = false;
        if (e == hipSuccess) memcpy(pend_dst[b], s.h, pend_n[b]);
        return e;
    };
    for (uint64_t off = 0; off < bytes; off += AWAY_STAGE_BYTES, cur ^= 1) {
        const uint64_t n = std::min(AWAY_STAGE_BYTES, bytes - off);
        commet_ctx::AwayStage &s = rs->ctx->away[cur];
        hipError_t e = drain(cur);
        if (e == hipSuccess) e = hipMemcpyAsync(s.h, d_src + off, n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(s.done, st);
        if (e != hipSuccess) return e;
        s.inflight = true, pend_dst[cur] = h_dst + off, pend_n[cur] = n;
    }
    hipError_t e = drain(cur);
    const hipError_t e2 = drain(cur ^ 1);
    return e != hipSuccess ? e : e2;
}

// and back: the host fills one pinned buffer while the other one's upload runs
hipError_t away_copy_in(commet_readset *rs, uint8_t *d_dst, const uint8_t *h_src, uint64_t bytes)
{
    hipStream_t st = rs->ctx->load_stream;
    int cur = 0;
    for (uint64_t off = 0; off < bytes; off += AWAY_STAGE_BYTES, cur ^= 1) {
        const uint64_t n = std::min(AWAY_STAGE_BYTES, bytes - off);
        commet_ctx::AwayStage &s = rs->ctx->away[cur];
        hipError_t e = hipSuccess;
        if (s.inflight) e = hipEventSynchronize(s.done), s.inflight = false;
        if (e != hipSuccess) return e;
        memcpy(s.h, h_src + off, n);
        e = hipMemcpyAsync(d_dst + off, s.h, n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(s.done, st);
        if (e != hipSuccess) return e;
        s.inflight = true;
    }
    const hipError_t e = hipStreamSynchronize(st);
    rs->ctx->away[0].inflight = rs->ctx->away[1].inflight = false;
    return e;
}

void free_set_blocks(commet_readset *rs)
{
    (void) dm_free(rs->d_planes), (void) dm_free(rs->d_goff), (void) dm_free(rs->d_kcnt), (void) dm_free(rs->d_lenmm);
    (void) dm_free(rs->d_sel), (void) dm_free(rs->d_tags), (void) dm_free(rs->d_found);
    rs->d_planes = nullptr, rs->d_goff = nullptr, rs->d_kcnt = nullptr, rs->d_lenmm = nullptr;
    rs->d_sel = rs->d_tags = rs->d_found = nullptr;
}

}  // namespace

extern "C" {

int commet_readset_is_resident(const commet_readset *rs)
{
    std::lock_guard<std::mutex> lk(rs->ctx->ql_mu);
    return rs->resident ? 1 : 0;
}

uint64_t commet_readset_packed_bytes(const commet_readset *rs) { return set_device_bytes(rs->max_reads, rs->max_bases); }

uint64_t commet_readset_device_bytes(const commet_readset *rs)
{
    std::lock_guard<std::mutex> lk(rs->ctx->ql_mu);
    return rs->resident && !rs->moving ? set_device_bytes(rs->max_reads, rs->max_bases) : 0;
}

int commet_readset_offload(commet_readset *rs)
{
    if (!rs) return fail("null read set");
    commet_ctx *c = rs->ctx;
    if (!rs->finalized) return fail("read set not finalized");
    commet_readset::QueryList list, plist;                 // what is derived from the set leaves with it (freed outside the mutex)
    uint32_t *len_order = nullptr;
    {
        // the check and the change in one critical section: a job that enters later (SetUse) finds the set offloaded
        std::lock_guard<std::mutex> lk(c->ql_mu);
        if (rs->moving) return fail("read set is being offloaded or restored");
        if (!rs->resident) return fail("read set is already offloaded");
        if (rs->in_job) return fail("read set is part of a running job: offload it before or after");
        rs->resident = false, rs->moving = true;
        if (rs->ql.built || rs->ql.bytes) {
            c->ql_bytes -= std::min(c->ql_bytes, rs->ql.bytes);
            list = rs->ql;
            rs->ql = commet_readset::QueryList();
        }
        if (rs->pl.built || rs->pl.bytes) {
            c->ql_bytes -= std::min(c->ql_bytes, rs->pl.bytes);
            plist = rs->pl;
            rs->pl = commet_readset::QueryList();
        }
        rs->ql.failed = rs->pl.failed = false;
        len_order = rs->d_len_order;
        rs->d_len_order = nullptr, rs->len_order_failed = false, rs->n_len_seg = 0;
        rs->ql_reserved.store(false);
    }
    auto done = [&](bool away) {
        std::lock_guard<std::mutex> lk(c->ql_mu);
        rs->resident = !away, rs->moving = false;
    };
    hipError_t e = hipSetDevice(c->device);
    list.release();
    plist.release();
    (void) dm_free(len_order);
    (void) dm_free(rs->d_filter_ws);
    rs->d_filter_ws = nullptr, rs->filter_ws_bytes = 0;
    const AwayLayout lay(rs);
    uint8_t *h = (uint8_t *) malloc(lay.total ? lay.total : 1);
    if (!h) {
        done(false);
        return fail("no host memory for the offloaded read set (%llu bytes)", (unsigned long long) lay.total);
    }
    if (e == hipSuccess) e = away_stage_open(c);
    if (e == hipSuccess) e = hipStreamSynchronize(c->load_stream);
    if (e == hipSuccess) e = away_copy_out(rs, (const uint8_t *) rs->d_planes, h, lay.planes_bytes);
    if (e == hipSuccess && lay.goff_bytes) e = away_copy_out(rs, (const uint8_t *) rs->d_goff, h + lay.planes_bytes, lay.goff_bytes);
    if (e != hipSuccess) {
        free(h);
        (void) hipGetLastError();
        done(false);                                       // still resident, its lists gone as after commet_readset_drop_cache
        return fail("read set offload failed: %s", hipGetErrorString(e));
    }
    rs->h_away = h, rs->away_bytes = lay.total;
    free_set_blocks(rs);                                   // (dm_free waits for the device, as hipFree does)
    done(true);
    return 0;
}

int commet_readset_restore(commet_readset *rs)
{
    if (!rs) return fail("null read set");
    commet_ctx *c = rs->ctx;
    if (!rs->finalized) return fail("read set not finalized");
    {
        std::lock_guard<std::mutex> lk(c->ql_mu);
        if (rs->moving) return fail("read set is being offloaded or restored");
        if (rs->resident) return fail("read set is already resident");
        rs->moving = true;                                 // (not resident: no job can enter meanwhile)
    }
    auto done = [&](bool back) {
        std::lock_guard<std::mutex> lk(c->ql_mu);
        rs->resident = back, rs->moving = false;
    };
    const AwayLayout lay(rs);
    const uint64_t triples = (rs->max_bases >> 5) + rs->max_reads + 1, bw = bitmap_words(rs->max_reads);
    hipError_t e = hipSetDevice(c->device);
    // as commet_readset_create; out of memory: the device cache and the query lists are given back once (dm_malloc, dev_alloc)
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_planes, triples * 3 * sizeof(uint32_t), false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_goff, (rs->max_reads + 1) * sizeof(uint64_t), false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_kcnt, (rs->max_reads + 1) * sizeof(uint32_t), false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_lenmm, 8 * sizeof(uint32_t), false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_sel, bw * 8, false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_tags, bw * 8, false);
    if (e == hipSuccess) e = dev_alloc(c, (void **) &rs->d_found, bw * 8, false);
    if (e == hipSuccess) e = away_stage_open(c);
    if (e == hipSuccess && triples * 12 > lay.planes_bytes)   // (capacity the reads do not fill: zero, as after create)
        e = hipMemsetAsync((uint8_t *) rs->d_planes + lay.planes_bytes, 0, triples * 12 - lay.planes_bytes, c->load_stream);
    const uint32_t mm[3] = {rs->n_reads ? rs->min_len : 0xFFFFFFFFu, rs->max_len, 0u};
    if (e == hipSuccess) e = hipMemcpyAsync(rs->d_lenmm, mm, sizeof mm, hipMemcpyHostToDevice, c->load_stream);
    if (e == hipSuccess) e = away_copy_in(rs, (uint8_t *) rs->d_planes, rs->h_away, lay.planes_bytes);
    if (e == hipSuccess && lay.goff_bytes) e = away_copy_in(rs, (uint8_t *) rs->d_goff, rs->h_away + lay.planes_bytes, lay.goff_bytes);
    if (e == hipSuccess && rs->n_reads) {
        // the per-read counts of complete k-mers, from the validity plane (as commet_readset_load)
        COMMET_LAUNCH(kmer_counts_kernel, dim3((unsigned) ((rs->n_reads + 255) / 256)), dim3(256), 0, c->load_stream, rs->view(), c->k, rs->d_kcnt,
                      rs->d_lenmm);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->load_stream);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        (void) hipStreamSynchronize(c->load_stream);
        free_set_blocks(rs);
        done(false);                                       // still offloaded, its host copy intact
        return fail("read set restore failed (%llu bytes): %s", (unsigned long long) set_device_bytes(rs->max_reads, rs->max_bases), hipGetErrorString(e));
    }
    free(rs->h_away);
    rs->h_away = nullptr, rs->away_bytes = 0;
    done(true);
    return 0;
}

int commet_files_packed_bytes(const char *const *paths, int n_paths, uint64_t *reads, uint64_t *bases, uint64_t *packed_bytes)
{
    uint64_t nr = 0, nb = 0;
    const int T = commet_host::ingest_threads();
    for (int i = 0; i < n_paths; ++i) {
        commet_host::ReadFileData f;
        if (!f.open_file(paths[i])) return fail("Cannot open file %s", paths[i]);
        const commet_host::ReadFormat fmt = f.format();
        if (fmt == commet_host::ReadFormat::Unknown) return fail("Unknown format: %s", paths[i]);
        std::vector<commet_host::IngestPiece> pieces;
        commet_host::split_file(i, fmt, f.data(), f.size(), (fmt == commet_host::ReadFormat::Fasta && f.size() > (8u << 20)) ? T * 4 : 1, pieces);
        commet_host::parallel_items(T, pieces.size(), [&](int, size_t p) { commet_host::count_piece(pieces[p]); });
        for (const commet_host::IngestPiece &p : pieces) nr += p.n_reads, nb += p.n_bases;
    }
    if (reads) *reads = nr;
    if (bases) *bases = nb;
    if (packed_bytes) *packed_bytes = set_device_bytes(nr, nb);
    return 0;
}

}  // extern "C"
