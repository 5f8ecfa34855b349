// devmem_check.cpp — CPU-only driver of host/devmem.hpp for the tests (tests/test_devmem_cpu.py: a plain build and two sanitizer
// builds): the device-memory cache over a fake driver of N devices of a fixed capacity, whose block addresses are invented and never
// dereferenced and which logs every call in order.  One line per scenario on stdout; exit status 1 at the first expectation that fails.
//   devmem_check          the environment decides what runs: COMMET_DEVMEM_CACHE=0 the cache-off scenarios, COMMET_DEVMEM_POOL=1
//                         (with COMMET_DEVMEM_POOL_MIN_MB=8) also the scenarios that need stream-ordered blocks
#include "devmem.hpp"

#include <thread>

#include <unistd.h>

using namespace commet;

namespace {

constexpr size_t MiB = (size_t) 1 << 20;
const char *g_scenario = "";

#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            printf("FAIL %s: %s (line %d)\n", g_scenario, #cond, __LINE__);       \
            fflush(stdout);                                                       \
            _exit(1);                                                             \
        }                                                                         \
    } while (0)

struct Fake {
    using Err = int;
    using Stream = int;
    static constexpr Err ok = 0, oom = 2, invalid = 1;
    enum Kind { ALLOC, POOL_ALLOC, FREE, POOL_FREE, POOL_TRIM, SYNC, COPY, SET_DEVICE };
    struct Call {
        Kind kind;
        int dev;
        size_t bytes;
        void *p;
        bool granted;
    };
    struct Out {
        int dev;
        size_t bytes;
        bool pooled;
    };
    const int n_dev;
    const size_t capacity;
    std::mutex mu;
    std::vector<Call> log;
    std::map<void *, Out> out;                                     // blocks the cache holds, live or filed
    std::vector<size_t> used;
    uintptr_t next = (uintptr_t) 1 << 32;
    static thread_local int cur;                                   // the calling thread's device, as in HIP

    Fake(int devices, size_t cap) : n_dev(devices), capacity(cap), used(devices, 0) {}

    Err take(void **p, size_t bytes, bool pooled)
    {
        std::lock_guard<std::mutex> lk(mu);
        const bool fits = used[cur] + bytes <= capacity;
        if (fits) {
            *p = (void *) next;
            next += 4096;
            used[cur] += bytes;
            out[*p] = {cur, bytes, pooled};
        }
        log.push_back({pooled ? POOL_ALLOC : ALLOC, cur, bytes, fits ? *p : nullptr, fits});
        return fits ? ok : oom;
    }
    Err give(void *p, bool pooled)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = out.find(p);
        const bool known = it != out.end() && it->second.pooled == pooled;
        log.push_back({pooled ? POOL_FREE : FREE, known ? it->second.dev : -1, known ? it->second.bytes : 0, p, known});
        EXPECT(known);                                             // never a block twice, never one of the other kind
        used[it->second.dev] -= it->second.bytes;
        out.erase(it);
        return ok;
    }
    void note(Kind kind, size_t bytes = 0, void *p = nullptr)
    {
        std::lock_guard<std::mutex> lk(mu);
        log.push_back({kind, cur, bytes, p, true});
    }

    Err current(int *dev) { return *dev = cur, ok; }
    void set_device(int dev) { cur = dev, note(SET_DEVICE); }
    Err alloc(void **p, size_t bytes) { return take(p, bytes, false); }
    Err free(void *p) { return give(p, false); }
    Stream new_stream() { return cur + 1; }
    Err pool_alloc(void **p, size_t bytes, Stream st) { return st == cur + 1 ? take(p, bytes, true) : invalid; }
    void pool_free(void *p, Stream) { (void) give(p, true); }
    void pool_trim(int dev) { note(POOL_TRIM, (size_t) dev); }     // (which pool: in `bytes`)
    Err sync() { return note(SYNC), ok; }
    size_t total_bytes() { return capacity; }
    Err copy(void *dst, const void *, size_t bytes) { return note(COPY, bytes, dst), ok; }

    // calls since log position `from` that asked the driver for a block / gave it one back
    std::vector<Call> traffic(size_t from)
    {
        std::lock_guard<std::mutex> lk(mu);
        std::vector<Call> t;
        for (size_t i = from; i < log.size(); ++i)
            if (log[i].kind <= POOL_FREE) t.push_back(log[i]);
        return t;
    }
    size_t mark()
    {
        std::lock_guard<std::mutex> lk(mu);
        return log.size();
    }
};
thread_local int Fake::cur = 0;
using Cache = DevMemCache<Fake>;

bool is_alloc(const Fake::Call &c) { return c.kind == Fake::ALLOC || c.kind == Fake::POOL_ALLOC; }
bool is_free(const Fake::Call &c) { return c.kind == Fake::FREE || c.kind == Fake::POOL_FREE; }
size_t allocs(Fake &f, size_t from)
{
    size_t n = 0;
    for (auto &c : f.traffic(from)) n += is_alloc(c);
    return n;
}

void *get(Cache &c, size_t bytes, bool shareable = false)
{
    void *p = nullptr;
    EXPECT(c.malloc(&p, bytes, shareable) == Fake::ok && p);
    return p;
}
// a free, and what the log must show of it: a block that is filed was filed behind a device synchronise, and whatever went back to the
// driver to stay within the cap went behind it too.  (put and filed_has read f.out without the fake's mutex: for the scenarios that run on
// one thread only; `threads` uses neither while its workers run)
void put(Cache &c, Fake &f, void *p)
{
    const bool large = f.out.at(p).bytes >= DEVMEM_MIN_FILED;
    const size_t from = f.mark();
    EXPECT(c.free(p) == Fake::ok);
    std::lock_guard<std::mutex> lk(f.mu);
    bool synced = false;
    for (size_t i = from; i < f.log.size(); ++i) {
        synced |= f.log[i].kind == Fake::SYNC;
        if (large && is_free(f.log[i])) EXPECT(synced);
    }
    EXPECT(synced == large);
}
// (a block the scenario has given back and the driver still counts as out: the cache has filed it)
bool filed_has(Fake &f, void *p) { return f.out.count(p) != 0; }

void size_classes()
{
    const size_t at[] = {8 * MiB - 1, 8 * MiB, 8 * MiB + 1, (size_t) 8500000000ull, (size_t) 17000000000ull};
    for (size_t n : at) {
        const size_t c = dm_size_class(n);
        if (n < 8 * MiB) {
            EXPECT(c == n);
            continue;
        }
        EXPECT(c >= n && dm_size_class(c) == c && c - n < n / 16);
    }
    EXPECT(dm_size_class(1) == 1 && dm_size_class(8 * MiB) == 8 * MiB && dm_size_class(8 * MiB + 1) == 8 * MiB + MiB / 2);
}

void small_blocks()
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    void *p = get(c, MiB);
    const size_t from = f.mark();
    put(c, f, p);
    const auto t = f.traffic(from);
    EXPECT(t.size() == 1 && t[0].kind == Fake::FREE && t[0].p == p);
    EXPECT(c.filed_bytes(0) == 0 && f.out.empty());
}

void reuse()
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    void *a = get(c, 64 * MiB);
    put(c, f, a);
    EXPECT(c.filed_bytes(0) == 64 * MiB);
    size_t from = f.mark();
    void *b = get(c, 60 * MiB);                                     // 64 <= 1.25 x 60
    EXPECT(b == a && f.traffic(from).empty() && c.filed_bytes(0) == 0);
    put(c, f, b);
    EXPECT(c.filed_bytes(0) == 64 * MiB);                           // recorded under the size it has, not the size asked for
    from = f.mark();
    void *d = get(c, 48 * MiB);                                     // 64 > 1.25 x 48
    EXPECT(d != a && allocs(f, from) == 1 && c.filed_bytes(0) == 64 * MiB && filed_has(f, a));
    EXPECT(c.trim(0) == 64 * MiB);
    void *x = get(c, 40 * MiB), *y = get(c, 44 * MiB);
    put(c, f, y);
    put(c, f, x);
    from = f.mark();
    EXPECT(get(c, 40 * MiB) == x && f.traffic(from).empty() && filed_has(f, y));   // the smallest that fits
}

void shareable_requests()                                           // (pooled blocks: COMMET_DEVMEM_POOL=1)
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    void *pooled = get(c, 32 * MiB), *plain = get(c, 32 * MiB, true);
    EXPECT(c.pooled_bytes(0) == 32 * MiB && f.out[pooled].pooled && !f.out[plain].pooled);
    put(c, f, plain);
    put(c, f, pooled);
    size_t from = f.mark();
    EXPECT(get(c, 32 * MiB, true) == plain && f.traffic(from).empty());
    void *fresh = get(c, 32 * MiB, true);                           // only the pooled one is filed now: it stays
    const auto t = f.traffic(from);
    EXPECT(fresh != pooled && t.size() == 1 && t[0].kind == Fake::ALLOC && filed_has(f, pooled) && c.filed_bytes(0) == 32 * MiB);
    EXPECT(get(c, 32 * MiB) == pooled);                             // (a request that is not shareable takes it)
}

void cap()                                                          // (100 MiB: main sets COMMET_DEVMEM_CACHE_GB)
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    void *a = get(c, 64 * MiB), *b = get(c, 32 * MiB), *d = get(c, 16 * MiB);
    put(c, f, a);
    put(c, f, b);
    EXPECT(c.filed_bytes(0) == 96 * MiB);
    const size_t from = f.mark();
    put(c, f, d);                                                   // 112 MiB: the largest goes (behind the synchronise: put)
    const auto t = f.traffic(from);
    EXPECT(t.size() == 1 && is_free(t[0]) && t[0].p == a);
    EXPECT(c.filed_bytes(0) == 48 * MiB && filed_has(f, b) && filed_has(f, d) && f.out.size() == 2);
}

void trim()
{
    Fake f(2, 1024 * MiB);
    Cache c(f);
    put(c, f, get(c, 16 * MiB));
    Fake::cur = 1;
    put(c, f, get(c, 32 * MiB));
    Fake::cur = 0;
    const uint64_t t0 = c.trims();
    EXPECT(c.trim(0) == 16 * MiB && c.filed_bytes(0) == 0 && c.filed_bytes(1) == 32 * MiB && c.trims() == t0 + 1);
    EXPECT(c.trim(0) == 0 && c.trims() == t0 + 1);                  // nothing released: nobody's set-aside memory is voided
    put(c, f, get(c, 16 * MiB));
    EXPECT(c.trim(-1) == 48 * MiB && c.filed_bytes(0) == 0 && c.filed_bytes(1) == 0 && c.trims() == t0 + 2 && f.out.empty());
    EXPECT(c.trim(-1) == 0 && c.trims() == t0 + 2 && Fake::cur == 0);
}

void out_of_memory()
{
    Fake f(1, 128 * MiB);
    Cache c(f);
    void *a = get(c, 64 * MiB);
    put(c, f, a);
    size_t from = f.mark();
    void *b = get(c, 96 * MiB);
    auto t = f.traffic(from);
    EXPECT(t.size() == 3 && is_alloc(t[0]) && !t[0].granted && t[0].bytes == 96 * MiB && is_free(t[1]) && t[1].p == a &&
           is_alloc(t[2]) && t[2].granted && t[2].p == b);
    EXPECT(c.filed_bytes(0) == 0);
    from = f.mark();                                                // nothing filed: the driver's answer comes back after one call
    void *p = nullptr;
    EXPECT(c.malloc(&p, 96 * MiB) == Fake::oom && !p);
    t = f.traffic(from);
    EXPECT(t.size() == 1 && is_alloc(t[0]) && !t[0].granted && f.out.at(b).bytes == 96 * MiB && f.out.size() == 1);
}

void exact_size_last_attempt()
{
    const size_t n = 70 * MiB;                                      // its class: 72 MiB
    EXPECT(dm_size_class(n) == 72 * MiB);
    Fake f(1, 71 * MiB);
    Cache c(f);
    void *p = get(c, n);
    const auto t = f.traffic(0);
    EXPECT(t.size() == 2 && !t[0].granted && t[0].bytes == 72 * MiB && t[1].granted && t[1].bytes == n);
    put(c, f, p);
    EXPECT(c.filed_bytes(0) == n);                                  // recorded under the size allocated
    Fake small(1, 60 * MiB);                                        // neither size fits, nothing is filed: refused twice, 72 then 70 MiB
    Cache c2(small);
    void *q = nullptr;
    EXPECT(c2.malloc(&q, n) == Fake::oom && !q);
    const auto t2 = small.traffic(0);
    EXPECT(t2.size() == 2 && !t2[0].granted && t2[0].bytes == 72 * MiB && !t2[1].granted && t2[1].bytes == n);
}

void refusal_hook()
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    put(c, f, get(c, 16 * MiB));
    void *p = nullptr;
    (void) get(c, 32 * MiB);
    const size_t out = f.out.size();
    uint64_t req, ref, last;
    size_t from = f.mark();
    c.refuse(32 * MiB, 0);                                          // by size
    EXPECT(c.malloc(&p, 64 * MiB) == Fake::oom && !p);
    EXPECT(f.mark() == from && c.filed_bytes(0) == 16 * MiB && f.out.size() == out);
    c.requests(&req, &ref, &last);
    EXPECT(req == 1 && ref == 1 && last == 64 * MiB);
    (void) get(c, MiB);
    c.requests(&req, &ref, &last);
    EXPECT(req == 2 && ref == 1 && last == 64 * MiB);
    c.refuse(0, 2);                                                 // the second request from now, once
    c.requests(&req, &ref, &last);
    EXPECT(req == 0 && ref == 0 && last == 0);
    (void) get(c, 2 * MiB);
    from = f.mark();
    EXPECT(c.malloc(&p, 3 * MiB) == Fake::oom && !p && f.mark() == from);
    c.requests(&req, &ref, &last);
    EXPECT(req == 2 && ref == 1 && last == 3 * MiB);
    (void) get(c, 3 * MiB);                                         // the retry is request 3
    c.requests(&req, &ref, &last);
    EXPECT(req == 3 && ref == 1);
    c.refuse(0, 0);
}

void reserve()
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    put(c, f, get(c, 64 * MiB));
    size_t from = f.mark();
    EXPECT(c.reserve(64 * MiB) == Fake::ok);
    EXPECT(allocs(f, from) == 1 && f.out.size() == 2);
    EXPECT(c.filed_bytes(0) == 128 * MiB);                          // above the cap of 100 MiB: blocks set aside are not held to it
    from = f.mark();
    EXPECT(c.reserve(MiB) == Fake::ok && f.mark() == from);
}

void make_shareable()                                               // (pooled blocks: COMMET_DEVMEM_POOL=1)
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    void *p = get(c, 32 * MiB), *q = p;
    EXPECT(c.pooled_bytes(0) == 32 * MiB);
    EXPECT(c.make_shareable(&q) == Fake::ok);
    EXPECT(q != p && f.out.at(q).bytes == 32 * MiB && !f.out[q].pooled && c.pooled_bytes(0) == 0);
    EXPECT(filed_has(f, p) && f.out[p].pooled && c.filed_bytes(0) == 32 * MiB);
    bool copied = false;
    for (auto &call : f.log) copied |= call.kind == Fake::COPY && call.p == q && call.bytes == 32 * MiB;
    EXPECT(copied);
    size_t from = f.mark();
    void *r = q, *unknown = (void *) 0x1234, *u = unknown;
    EXPECT(c.make_shareable(&r) == Fake::ok && r == q && c.make_shareable(&u) == Fake::ok && u == unknown && f.mark() == from);
}

void devices()
{
    Fake f(DEVMEM_MAX_DEVICES + 4, 1024 * MiB);
    Cache c(f);
    Fake::cur = 1;
    void *p = get(c, 16 * MiB);
    Fake::cur = 0;
    put(c, f, p);
    EXPECT(c.filed_bytes(1) == 16 * MiB && c.filed_bytes(0) == 0 && Fake::cur == 0 && f.out[p].dev == 1);
    Fake::cur = DEVMEM_MAX_DEVICES + 1;                             // outside the table: the driver's own block
    size_t from = f.mark();
    void *q = get(c, 16 * MiB);
    EXPECT(c.free(q) == Fake::ok);
    const auto t = f.traffic(from);
    EXPECT(t.size() == 2 && t[0].kind == Fake::ALLOC && t[1].kind == Fake::FREE && t[1].p == q);
    EXPECT(c.filed_bytes(Fake::cur) == 0 && c.reserve(16 * MiB) != Fake::ok && f.out.size() == 1);
    Fake::cur = 0;
}

void cache_off()                                                    // (COMMET_DEVMEM_CACHE=0)
{
    Fake f(1, 1024 * MiB);
    Cache c(f);
    EXPECT(!c.enabled() && c.request_bytes(70 * MiB) == 70 * MiB);
    void *p = get(c, 70 * MiB);
    EXPECT(c.free(p) == Fake::ok);
    const auto t = f.traffic(0);
    EXPECT(t.size() == 2 && t[0].kind == Fake::ALLOC && t[0].bytes == 70 * MiB && t[1].kind == Fake::FREE && t[1].p == p);
    EXPECT(c.reserve(64 * MiB) == Fake::ok && f.traffic(0).size() == 2);
    uint64_t ns, bytes, calls;
    c.driver_stats(0, &ns, &bytes, &calls);
    EXPECT(calls == 1 && bytes == 70 * MiB && c.filed_bytes(0) == 0 && f.out.empty());
}

void threads()
{
    Fake f(1, 4096 * MiB);
    Cache c(f);
    std::atomic<int> running{4};
    std::vector<std::thread> pool;
    for (int w = 0; w < 4; ++w)
        pool.emplace_back([&, w] {
            const size_t sizes[4] = {MiB, 8 * MiB, 20 * MiB, 70 * MiB};
            uint32_t r = 12345u + (uint32_t) w;
            for (int i = 0; i < 2000; ++i) {
                r = r * 1664525u + 1013904223u;
                void *p = nullptr;
                EXPECT(c.malloc(&p, sizes[r >> 30]) == Fake::ok && p);
                EXPECT(c.free(p) == Fake::ok);
            }
            --running;
        });
    pool.emplace_back([&] {
        while (running.load()) {
            uint64_t a, b, d;
            (void) c.trim(-1);
            (void) c.filed_bytes(0);
            (void) c.pooled_bytes(0);
            (void) c.trims();
            c.driver_stats(-1, &a, &b, &d);
            c.requests(&a, &b, &d);
            std::this_thread::yield();
        }
    });
    for (auto &t : pool) t.join();
    size_t sum = 0;                                                 // every block is back: what the driver counts as out is what is filed
    for (auto &b : f.out) sum += b.second.bytes;
    EXPECT(sum == c.filed_bytes(0));
    EXPECT(c.trim(-1) == sum && f.out.empty());
    uint64_t req, ref, last;
    c.requests(&req, &ref, &last);
    EXPECT(req == 8000 && ref == 0);
}

void run(const char *name, void (*scenario)())
{
    g_scenario = name;
    scenario();
    printf("ok %s\n", name);
}

}  // namespace

int main()
{
    setenv("COMMET_DEVMEM_CACHE_GB", "0.09765625", 1);                // 100 MiB
    const char *off = getenv("COMMET_DEVMEM_CACHE"), *pool = getenv("COMMET_DEVMEM_POOL");
    run("size classes", size_classes);
    run("threads", threads);                                          // first: the settings' first use is then five threads at once
    if (off && atoi(off) == 0) {
        run("cache off", cache_off);
    } else {
        run("small blocks", small_blocks);
        run("reuse", reuse);
        run("cap", cap);
        run("trim", trim);
        run("out of memory", out_of_memory);
        run("exact-size last attempt", exact_size_last_attempt);
        run("refusal hook", refusal_hook);
        run("reserve", reserve);
        run("devices", devices);
        if (pool && atoi(pool) != 0) {
            run("shareable requests", shareable_requests);
            run("make shareable", make_shareable);
        }
    }
    return 0;
}
