// capi/cache.hpp — device memory under pressure: the query lists cached with resident sets (accounted, least recently used first), allocations that retry after giving lists back, scatter workspaces; the cache entry points of the ABI
// (a part of the one translation unit capi.hip: included there, in order, after the kernels and state.hpp)
#pragma once

namespace {
// drops one query list of a set (caller holds ql_mu); hipFree waits for the kernels that read it
void drop_query_list(commet_ctx *c, commet_readset::QueryList &ql)
{
    if (!ql.built && !ql.bytes) return;
    c->ql_bytes -= std::min(c->ql_bytes, ql.bytes);
    ql.release();
    ++c->ql_evictions;
}
// both lists of a set: the search's (ql) and the profile's (pl)
void drop_query_list(commet_ctx *c, const commet_readset *rs)
{
    drop_query_list(c, rs->ql);
    drop_query_list(c, rs->pl);
}

// gives cached query lists back until at most `target` bytes of them are left: least recently used first — judged list by
// list, a set's search list and its profile list apart —, never a list
// of the running job unless `even_in_job` (the job thread itself is out of memory and holds no list between build and
// launch).  Returns the bytes released.  Caller holds ql_mu.
uint64_t shrink_query_lists(commet_ctx *c, uint64_t target, bool even_in_job)
{
    uint64_t freed = 0;
    while (c->ql_bytes > target) {
        commet_readset::QueryList *victim = nullptr;
        for (const commet_readset *rs : c->sets) {
            if (!even_in_job && rs->in_job) continue;
            for (commet_readset::QueryList *l : {&rs->ql, &rs->pl})
                if (l->built && (!victim || l->last_use < victim->last_use)) victim = l;
        }
        if (!victim) break;
        freed += victim->bytes;
        drop_query_list(c, *victim);
    }
    return freed;
}

// hipMalloc that gives the cached query lists back and tries once more when the device is out of memory.  job_thread: the lists of the
// running job's sets go too (shrink_query_lists, even_in_job).  ql_locked: the caller HOLDS ql_mu (build_query_list,
// ensure_query_results) — the mutex is not taken again, and job_thread is then IGNORED: only the lists of sets outside the running job
// go, whatever it says (the caller is about to use the job's own)
hipError_t dev_alloc(commet_ctx *c, void **p, size_t bytes, bool job_thread, bool ql_locked = false)
{
    hipError_t e = dm_malloc(p, bytes);
    if (e != hipErrorOutOfMemory) return e;
    (void) hipGetLastError();
    uint64_t freed;
    {
        std::unique_lock<std::mutex> lk(c->ql_mu, std::defer_lock);
        if (!ql_locked) lk.lock();
        freed = shrink_query_lists(c, 0, job_thread && !ql_locked);
    }
    if (!freed) return e;
    e = dm_malloc(p, bytes);
    if (e == hipErrorOutOfMemory) (void) hipGetLastError();
    return e;
}

// A device buffer kept with the context between calls (hipMalloc / hipFree per job cost more than the kernels that use such a
// buffer) and grown when a job needs more: ptr holds cap elements.  0 = it holds `need` now (nothing is done, and nothing
// synchronised, when it did already); 1 = no room: the HIP error is cleared, ptr and cap are null / 0 — never a stale capacity — and
// the caller decides what that means (an error, another regime).  A grow waits for the context's job streams, frees, and allocates
// alloc_elems (>= need: some callers round up).  ql_locked: the caller holds ql_mu.
template <typename T>
int grow_kept(commet_ctx *c, T *&ptr, uint64_t &cap, uint64_t need, uint64_t alloc_elems, bool ql_locked = false)
{
    if (cap >= need) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess || hipStreamSynchronize(c->aux_stream) != hipSuccess)
        return fail("stream synchronize failed: %s", hipGetErrorString(hipGetLastError()));
    (void) dm_free(ptr);
    ptr = nullptr, cap = 0;
    void *p = nullptr;
    const size_t bytes = (size_t) alloc_elems * sizeof(T);
    const hipError_t e = dev_alloc(c, &p, bytes, true, ql_locked);
    if (e != hipSuccess) {
        (void) hipGetLastError();
        return fail("cannot allocate %zu bytes of device memory: %s", bytes, hipGetErrorString(e));
    }
    ptr = (T *) p, cap = alloc_elems;
    return 0;
}

// A scatter workspace (several GB that kernels sweep as a whole): allocated and touched here, not inside the first scatter launch
// (measured: 15.6 ms instead of 2.5 ms for that one launch).  Rounds 3 and 4 picked these buffers from several timed candidates —
// how hipMalloc backs a multi-GB buffer decides how fast kernels sweep it, drawn once per allocation: one in three ~20 % faster on
// some boxes — but on the boxes of round 4 the candidates lay within 5 % of each other, a fill's time did not predict the scatter
// kernels' inside that range, the spread of the step over fresh contexts was 6.1 % with the pool against 8.8 % without
// (profiles/r04_ws_candidates), and the selection cost ~10 ms of every cold first job and three extra 8.5 GB allocations: removed
// in round 5.
hipError_t alloc_workspace(commet_ctx *c, void **p, size_t bytes, hipStream_t stream)
{
    *p = nullptr;
    hipError_t e = dev_alloc(c, p, bytes, true);
    if (e != hipSuccess) return e;
    return hipMemsetAsync(*p, 0, bytes, stream);
}
}  // namespace

extern "C" {

uint64_t commet_readset_cache_bytes(const commet_readset *rs)
{
    std::lock_guard<std::mutex> lk(rs->ctx->ql_mu);
    return (rs->ql.built ? rs->ql.bytes : 0) + (rs->pl.built ? rs->pl.bytes : 0);
}

void commet_readset_drop_cache(commet_readset *rs)
{
    commet_ctx *c = rs->ctx;
    (void) hipSetDevice(c->device);
    std::lock_guard<std::mutex> lk(c->ql_mu);
    if (rs->in_job) return;                              // (never under a running job)
    drop_query_list(c, rs);
    rs->ql.failed = rs->pl.failed = false;               // a list that did not fit once may fit now
}

uint64_t commet_device_cache_trim(int device)
{
    return (uint64_t) dm_trim(device);
}

uint64_t commet_device_cache_bytes(int device)
{
    return (uint64_t) dm_filed_bytes(device);
}

uint64_t commet_device_pooled_bytes(int device)
{
    return (uint64_t) dm_pooled_bytes(device);
}

int commet_device_alloc_stats(int device, double *wait_ms, uint64_t *fresh_bytes, uint64_t *calls)
{
    uint64_t ns, by, n;
    g_devmem.driver_stats(device, &ns, &by, &n);
    if (wait_ms) *wait_ms = (double) ns * 1e-6;
    if (fresh_bytes) *fresh_bytes = by;
    if (calls) *calls = n;
    return 0;
}

void commet_device_alloc_refuse(uint64_t at_least_bytes, uint64_t nth)
{
    g_devmem.refuse(at_least_bytes, nth);
}

void commet_device_alloc_requests(uint64_t *requests, uint64_t *refused, uint64_t *last_refused_bytes)
{
    g_devmem.requests(requests, refused, last_refused_bytes);
}

int commet_cache_stats(commet_ctx *c, uint64_t *bytes, uint64_t *budget_bytes, uint64_t *evictions)
{
    std::lock_guard<std::mutex> lk(c->ql_mu);
    if (bytes) *bytes = c->ql_bytes;
    if (budget_bytes) *budget_bytes = c->ql_budget;
    if (evictions) *evictions = c->ql_evictions;
    return 0;
}

}  // extern "C"
