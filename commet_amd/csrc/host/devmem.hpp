// host/devmem.hpp — device memory kept for reuse: the policy (size classes, filed blocks, the per-device cap, trim and retry, pooled and
// shareable blocks, the refusal hook, blocks set aside in advance) over a driver it is given.  No HIP here: capi/state.hpp instantiates
// the cache over the HIP runtime, host/devmem_check.cpp over a fake device (tests/test_devmem_cpu.py, with sanitizer builds).
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace commet {

// ---- device memory kept for reuse ----------------------------------------------------------------------------------------
// On this driver a hipMalloc of GBs costs 15-30 ms per GiB on some boxes (and ~0 on others: tools/exp/alloc_cost*.hip — where a
// 16 GiB hipMalloc took 483 ms, and 965 ms again after its hipFree, sixteen of 1 GiB took 0.3 ms and a hipMallocAsync of 16 GiB
// 14 ms), and one that follows the hipFree of tens of GB now and then blocks for 50-150 ms (seen up to 2 s): a context created after another one was closed, a query list built after one was dropped, a
// workspace that grows — all of them on some job's path (bench.py's configs[2] leg behind the headline: 1.50 s of device time
// against 1.15 s in a fresh process, the difference being the GPU idling behind such calls; profiles/r05_c2_variance).  So the
// library never gives a block of 8 MiB or more back while the process lives: dm_free waits for the device, as hipFree does (its
// callers count on that), and files the block; dm_malloc takes the smallest filed block of the current device that is large enough
// and at most a quarter larger, else asks hipMalloc — and when hipMalloc is out of memory, everything filed is given back and
// it is asked once more.  Blocks are never split (an exported set's IPC handle must be that of a whole allocation).
// COMMET_DEVMEM_POOL=1 (off by default): a new block of 256 MiB or more comes from hipMallocAsync on a stream of the cache's own,
// drained before the block is handed out — 0.4-0.9 ms per GiB on either kind of box in isolation, but on a box whose hipMalloc
// is free anyway the 10-set matrix of bench.py took 12.7 s with it against 10.9 s without (device time +4 %: kernels gather more
// slowly from pool memory; the loader thread's waits 1.5 s against 0.6 s; profiles/r05_pool), and the box of the other kind has
// not come up again to be measured.  No IPC handle can be had for such a block, so commet_readset_export first moves a set's
// planes into a hipMalloc block (dm_make_shareable).
// At most half the device (COMMET_DEVMEM_CACHE_GB) is kept, the largest blocks going first; commet_device_cache_trim gives all of
// it back.  COMMET_DEVMEM_CACHE=0: plain hipMalloc / hipFree.

// devices the cache keeps a table for: a block of a device numbered outside it comes straight from the driver, goes straight back and is never filed
constexpr int DEVMEM_MAX_DEVICES = 16;
constexpr size_t DEVMEM_MIN_FILED = (size_t) 8 << 20;

// Size classes: a block of 8 MiB or more is asked for in steps of 1/16 .. 1/32 of its size (a request of 8.5 GB becomes one of 8.6 GB).
// The objects a context makes — scatter workspaces sized by a chunk's k-mer count, a set's planes, a query list — come out a few
// hundred bytes apart from one set to the next; filed under their exact sizes, a block that was 100 bytes short served nobody and
// the next context asked the driver for the same 17 GB again (the first process on a box that charges for fresh device memory pays
// 30 ms per GiB for that, DESIGN section 4: bench.py's matrix legs, commet_device_alloc_stats).
inline size_t dm_size_class(size_t bytes)
{
    if (bytes < DEVMEM_MIN_FILED) return bytes;
    const int lg = 63 - __builtin_clzll((unsigned long long) bytes);
    const size_t granule = (size_t) 1 << (lg - 4);
    return (bytes + granule - 1) & ~(granule - 1);
}

// Drv, the driver (the one seam: HIP in the library, a fake in the check program), supplies
//   Err, ok, oom                       its error type and the two values the cache tells apart
//   Stream, new_stream()               what stream-ordered blocks of one device are ordered on (Stream{}: none)
//   current(&dev), set_device(dev)     the calling thread's device: read, changed (the only call that changes it)
//   alloc(&p, n), free(p)              plain blocks
//   pool_alloc(&p, n, st), pool_free(p, st)     stream-ordered blocks, each call drained before it returns
//   pool_trim(dev)                     the pool of device dev keeps nothing; the calling thread's device is afterwards what it was
//   sync(), total_bytes(), copy(dst, src, n) on the current device
// alloc, pool_alloc, new_stream and pool_trim leave no error of theirs behind in the driver's own error state (HIP's last error): the
// cache asks again after an out-of-memory answer without clearing anything itself.
template <typename Drv>
class DevMemCache {
public:
    using Err = typename Drv::Err;
    using Stream = typename Drv::Stream;
    explicit DevMemCache(Drv &driver) : drv(driver) {}

    bool enabled() const { return settings().on; }
    size_t request_bytes(size_t n) const { return enabled() ? dm_size_class(n) : n; }   // what a request of n bytes really takes

    // `shareable`: the block may be exported to another process (commet_readset_export), so it comes from hipMalloc
    Err malloc(void **p, size_t bytes, bool shareable = false)
    {
        *p = nullptr;
        {   // the refusal hook: the caller's byte count, before anything else; a refusal touches nothing but the hook's own numbers
            const uint64_t n = n_requests.fetch_add(1, std::memory_order_relaxed) + 1;
            const uint64_t at_least = refuse_at_least.load(std::memory_order_relaxed), nth = refuse_nth.load(std::memory_order_relaxed);
            if ((at_least && bytes >= at_least) || (nth && n == nth)) {
                n_refused.fetch_add(1, std::memory_order_relaxed);
                last_refused.store(bytes, std::memory_order_relaxed);
                return Drv::oom;
            }
        }
        const size_t exact = bytes;
        bytes = request_bytes(bytes);
        int dev = 0;
        if (drv.current(&dev) != Drv::ok || !in_table(dev)) return drv.alloc(p, bytes);
        bool pooled = false;
        if (!enabled()) return driver_alloc(p, bytes, dev, true, &pooled);   // (plain)
        Device &D = devs[dev];
        if (bytes >= DEVMEM_MIN_FILED) {
            std::lock_guard<std::mutex> lk(mu);
            for (auto it = D.filed.lower_bound(bytes); it != D.filed.end() && it->first <= bytes + bytes / 4; ++it) {
                if (shareable && it->second.pooled) continue;
                *p = it->second.p;
                D.filed_bytes -= it->first;
                live[*p] = {dev, it->first, it->second.pooled};
                D.filed.erase(it);
                return Drv::ok;
            }
        }
        if (settings().verbose) {
            std::lock_guard<std::mutex> lk(mu);
            fprintf(stderr, "[devmem] driver alloc %.1f MiB (filed: %.1f GiB in %zu blocks)\n", bytes / 1048576.0, D.filed_bytes / 1073741824.0, D.filed.size());
        }
        Err e = driver_alloc(p, bytes, dev, shareable, &pooled);
        if (e == Drv::oom && trim(dev)) e = driver_alloc(p, bytes, dev, shareable, &pooled);
        // the class rounds up by as much as 1/16: what the caller asked for may still fit.  Also when the trim released nothing and no
        // retry was made: an out-of-memory answer to a rounded size costs a second driver call before it reaches the caller
        if (e == Drv::oom && bytes != exact) e = driver_alloc(p, bytes = exact, dev, shareable, &pooled);
        if (e == Drv::ok && bytes >= DEVMEM_MIN_FILED) {
            std::lock_guard<std::mutex> lk(mu);
            live[*p] = {dev, bytes, pooled};
        }
        return e;
    }

    Err free(void *p)
    {
        if (!p) return Drv::ok;
        const Block what = handed_out(p, true);
        if (what.device < 0) return drv.free(p);
        const int d = what.device;
        int cur = d;
        if (drv.current(&cur) != Drv::ok) cur = d;
        if (cur != d) drv.set_device(d);                               // (the block's device, whatever device the calling thread is on)
        (void) drv.sync();                                             // what hipFree does: no kernel still reads the block when somebody else gets it
        file(d, p, what.bytes, what.pooled, true);
        if (cur != d) drv.set_device(cur);
        return Drv::ok;
    }

    // a block of `bytes` asked from the driver NOW and filed at once, for an allocation that will come later on some job's path (a helper
    // thread pays the driver's price instead of the job thread); never taken from the filed blocks themselves
    Err reserve(size_t bytes)
    {
        if (!enabled() || bytes < DEVMEM_MIN_FILED) return Drv::ok;
        bytes = dm_size_class(bytes);
        int dev = 0;
        if (drv.current(&dev) != Drv::ok || !in_table(dev)) return Drv::oom;   // (nothing can be set aside there: to the caller — who asks "ok?" only — no room; an invalid-device error before)
        void *p = nullptr;
        bool pooled = false;
        const Err e = driver_alloc(&p, bytes, dev, false, &pooled);
        if (e != Drv::ok) return e;
        file(dev, p, bytes, pooled, false);                            // NOT held to the cap: the list these blocks wait for may be larger than it, and is asked for next
        return Drv::ok;
    }

    // gives every filed block of `device` (-1: all) back to the driver; returns the bytes released
    size_t trim(int device)
    {
        std::vector<std::pair<Filed, Stream>> drop;
        std::vector<int> pools;                                        // devices in scope that have a pool
        size_t bytes = 0;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (int d = 0; d < DEVMEM_MAX_DEVICES; ++d) {
                if (device >= 0 && d != device) continue;
                Device &D = devs[d];
                for (auto &b : D.filed) drop.push_back({b.second, D.pool_stream}), bytes += b.first;
                D.filed.clear(), D.filed_bytes = 0;
                if (D.pool_stream != Stream{}) pools.push_back(d);
            }
            if (!drop.empty()) n_trims += 1;                           // (a trim that found nothing filed has taken nothing from anybody)
        }
        bool any_pooled = false;
        for (auto &q : drop) driver_free(q.first, q.second), any_pooled |= q.first.pooled;
        if (any_pooled)                                                // the pool itself keeps nothing either
            for (int d : pools) drv.pool_trim(d);
        return bytes;
    }
    uint64_t trims() const { return n_trims.load(); }                  // times filed blocks went back to the driver (trim): what was set aside before is gone

    size_t filed_bytes(int device)
    {
        std::lock_guard<std::mutex> lk(mu);
        return in_table(device) ? devs[device].filed_bytes : 0;
    }
    size_t pooled_bytes(int device)                                    // ... of the blocks handed out
    {
        std::lock_guard<std::mutex> lk(mu);
        size_t n = 0;
        for (auto &b : live)
            if (b.second.device == device && b.second.pooled) n += b.second.bytes;
        return n;
    }

    // the block at *p made exportable: one that came from the stream-ordered pool is copied into a hipMalloc block of its own (the
    // device drained first; the caller sees to it that no other host thread uses the block meanwhile) and filed
    Err make_shareable(void **p)
    {
        if (!*p) return Drv::ok;
        const Block what = handed_out(*p, false);
        if (what.device < 0 || !what.pooled) return Drv::ok;
        void *q = nullptr;
        Err e = malloc(&q, what.bytes, true);
        if (e != Drv::ok) return e;
        e = drv.sync();
        if (e == Drv::ok) e = drv.copy(q, *p, what.bytes);
        if (e == Drv::ok) e = drv.sync();
        if (e == Drv::ok) std::swap(*p, q);                            // q: the block that goes — the old one, or the new one that could not be filled
        (void) free(q);
        return e;
    }

    // test hook (commet_device_alloc_refuse; off = 0, 0): malloc refuses a request of at_least bytes or more, and the nth request
    // since arming (once), as the driver does when it is out of memory; requests(): what malloc saw since arming
    void refuse(uint64_t at_least, uint64_t nth)
    {
        refuse_at_least = 0, refuse_nth = 0;                           // (nothing is refused while the numbers restart)
        n_requests = 0, n_refused = 0, last_refused = 0;
        refuse_at_least = at_least, refuse_nth = nth;
    }
    void requests(uint64_t *requests, uint64_t *refused, uint64_t *last_refused_bytes) const
    {
        if (requests) *requests = n_requests.load();
        if (refused) *refused = n_refused.load();
        if (last_refused_bytes) *last_refused_bytes = last_refused.load();
    }

    // what the DRIVER was asked for on `device` (-1: all; commet_device_alloc_stats): time the calling thread spent inside hipMalloc /
    // hipMallocAsync, bytes and calls — a box that charges for a process's first use of device memory shows here, not in kernel time
    void driver_stats(int device, uint64_t *ns, uint64_t *bytes, uint64_t *calls) const
    {
        *ns = *bytes = *calls = 0;
        for (int d = 0; d < DEVMEM_MAX_DEVICES; ++d)
            if (device < 0 || d == device) *ns += devs[d].drv_ns.load(), *bytes += devs[d].drv_bytes.load(), *calls += devs[d].drv_calls.load();
    }

private:
    // bytes: as allocated; pooled: from hipMallocAsync (no IPC handle can be had for it)
    struct Block { int device; size_t bytes; bool pooled; };
    struct Filed { void *p; bool pooled; };
    struct Device {
        std::multimap<size_t, Filed> filed;                            // by size
        size_t filed_bytes = 0, cap = 0;                               // cap: bytes kept at most (COMMET_DEVMEM_CACHE_GB; default: half the device), known from the first block filed
        Stream pool_stream{};                                          // the stream the stream-ordered allocations are ordered on (always drained before use); under mu
        std::atomic<uint64_t> drv_ns{0}, drv_bytes{0}, drv_calls{0};
    };
    // the environment, read once per process at the cache's first use (a Python caller may set it after import, before the first context)
    struct Settings {
        static long long env(const char *name, long long unset) { return getenv(name) ? atoll(getenv(name)) : unset; }
        bool on = env("COMMET_DEVMEM_CACHE", 1) != 0, pool = env("COMMET_DEVMEM_POOL", 0) != 0;
        bool verbose = env("COMMET_DEVMEM_VERBOSE", 0) != 0;           // one line on stderr per block asked from or returned to the driver
        size_t pool_min = std::max((size_t) env("COMMET_DEVMEM_POOL_MIN_MB", 256) << 20, DEVMEM_MIN_FILED);   // (tests: a set of a few MB in pooled blocks)
        double cap_gb = getenv("COMMET_DEVMEM_CACHE_GB") ? std::max(0.0, atof(getenv("COMMET_DEVMEM_CACHE_GB"))) : -1.0;   // below 0: not given
    };
    static const Settings &settings() { static const Settings s; return s; }
    static bool in_table(int dev) { return dev >= 0 && dev < DEVMEM_MAX_DEVICES; }
    // the record of a block handed out (device -1: not one of the cache's); take: it is handed out no longer
    Block handed_out(void *p, bool take)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = live.find(p);
        if (it == live.end()) return {-1, 0, false};
        const Block b = it->second;
        if (take) live.erase(it);
        return b;
    }

    // one block from the driver, the call timed into the device's stats (every block the cache asks for comes through here):
    // stream-ordered from 256 MiB on unless an IPC handle will be asked for it
    Err driver_alloc(void **p, size_t bytes, int dev, bool shareable, bool *pooled)
    {
        Device &D = devs[dev];
        const auto t0 = std::chrono::steady_clock::now();
        const Err e = [&] {
            *pooled = false;
            if (shareable || !settings().pool || bytes < settings().pool_min) return drv.alloc(p, bytes);
            Stream st;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (D.pool_stream == Stream{}) D.pool_stream = drv.new_stream();
                st = D.pool_stream;
            }
            if (st == Stream{}) return drv.alloc(p, bytes);
            const Err pe = drv.pool_alloc(p, bytes, st);
            *pooled = pe == Drv::ok;
            return pe == Drv::ok || pe == Drv::oom ? pe : drv.alloc(p, bytes);   // (not supported here, ...: the plain call)
        }();
        D.drv_ns += (uint64_t) std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        D.drv_calls += 1;
        if (e == Drv::ok) D.drv_bytes += bytes;
        return e;
    }
    void driver_free(const Filed &q, Stream st) { q.pooled ? drv.pool_free(q.p, st) : (void) drv.free(q.p); }
    // files a block of device d, which is the current device and idle; enforce_cap: the largest filed blocks go back to the driver until
    // the device keeps no more than its cap (other processes may share the device)
    void file(int d, void *p, size_t bytes, bool pooled, bool enforce_cap)
    {
        Device &D = devs[d];
        std::vector<Filed> over;
        Stream st;
        {
            std::lock_guard<std::mutex> lk(mu);
            D.filed.emplace(bytes, Filed{p, pooled}), D.filed_bytes += bytes;
            if (enforce_cap && !D.cap) D.cap = settings().cap_gb >= 0 ? (size_t) (settings().cap_gb * (double) (1ull << 30)) + 1 : drv.total_bytes() / 2;
            while (enforce_cap && D.filed_bytes > D.cap && !D.filed.empty()) {
                auto last = --D.filed.end();
                over.push_back(last->second), D.filed_bytes -= last->first;
                D.filed.erase(last);
            }
            st = D.pool_stream;
        }
        // (D.cap: written once, under the mutex, before this thread left it)
        if (!over.empty() && settings().verbose) fprintf(stderr, "[devmem] over the cap of %.1f GiB: %zu block(s) back to the driver\n", D.cap / 1073741824.0, over.size());
        for (auto &q : over) driver_free(q, st);
    }

    Drv &drv;
    std::mutex mu;
    std::map<void *, Block> live;                                      // blocks handed out
    Device devs[DEVMEM_MAX_DEVICES];
    std::atomic<uint64_t> n_trims{0}, refuse_at_least{0}, refuse_nth{0};
    std::atomic<uint64_t> n_requests{0}, n_refused{0}, last_refused{0};
};

}  // namespace commet
