"""Python mirror of the C ABI (include/commet_hip.h): same names, same argument
meaning, errors raised as CommetError with the library's message.  All compute
happens in the HIP library; numpy arrays only carry host buffers."""
import ctypes as C
import os
import weakref

import numpy as np

from . import lib as _l


class CommetError(RuntimeError):
    pass


def _err(lib):
    msg = lib.commet_last_error()
    return msg.decode() if msg else "unknown error"


def bits_nbytes(n):
    """bytes of a BooleanVector over n reads (boolean_vector.h:130)"""
    return n // 8 + 1


def tags_at(hits, t):
    """BooleanVector bytes (bits_nbytes(n) long, padding bits zero) of the reads with at least t hits: from the counts of
    Context.index_and_profile, the tags of a job at threshold t"""
    h = np.asarray(hits, dtype=np.uint8)
    out = np.zeros(bits_nbytes(h.size), dtype=np.uint8)
    packed = np.packbits(h >= int(t), bitorder="little")
    out[:packed.size] = packed
    return out


def _as_bits(arr, n, what):
    if arr is None:
        return None
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    if a.size < bits_nbytes(n):
        raise CommetError(f"{what}: need {bits_nbytes(n)} bytes for {n} reads, got {a.size}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _handles(sets):
    return (C.c_void_p * max(len(sets), 1))(*[rs._h for rs in sets])


def _selections(selects, sets, what):
    """one optional selection per set -> their byte arrays (None: no selection)"""
    if selects is None:
        return [None] * len(sets)
    return [_as_bits(s, rs.num_reads, what) for s, rs in zip(selects, sets)]


def _ptrs(arrays):
    """c_void_p array over host arrays; None, and an array without bytes, is a null pointer"""
    return (C.c_void_p * max(len(arrays), 1))(*[(_ptr(a).value if a is not None and a.size else None) for a in arrays])


def _info_dict(info):
    return {f: getattr(info, f) for f, _ in _l.JobInfo._fields_}


def _stats_list(stats, n):
    return [dict(indexed=int(stats[i].indexed), searched=int(stats[i].searched), shared=int(stats[i].shared),
                 search_ms=float(stats[i].search_ms)) for i in range(n)]


def device_count():
    """commet_device_count: HIP devices this process sees (0 without one; counting initialises nothing a later fork would mind)"""
    return int(_l.load().commet_device_count())


def device_cache_trim(device=-1):
    """commet_device_cache_trim: gives the device memory the library keeps for reuse back to the driver; returns the bytes released"""
    return int(_l.load().commet_device_cache_trim(int(device)))


def device_cache_bytes(device=0):
    """commet_device_cache_bytes: device memory filed for reuse on `device`"""
    return int(_l.load().commet_device_cache_bytes(int(device)))


def device_pooled_bytes(device=0):
    """commet_device_pooled_bytes: bytes in use on `device` that came from the stream-ordered pool (not shareable over HIP IPC)"""
    return int(_l.load().commet_device_pooled_bytes(int(device)))


def device_alloc_stats(device=-1):
    """commet_device_alloc_stats: what the library asked the driver for since the process started (blocks reused from its own
    cache do not count): {"wait_ms": host time inside hipMalloc, "fresh_bytes", "calls"}"""
    ms, by, n = C.c_double(0), C.c_uint64(0), C.c_uint64(0)
    _l.load().commet_device_alloc_stats(int(device), C.byref(ms), C.byref(by), C.byref(n))
    return {"wait_ms": float(ms.value), "fresh_bytes": int(by.value), "calls": int(n.value)}


def device_alloc_refuse(at_least=0, nth=0):
    """commet_device_alloc_refuse (test hook): from now on the library's device allocations of `at_least` bytes or more are refused,
    and the `nth` one from now on once, as by a full device; restarts the numbers of device_alloc_requests.  (0, 0) disarms"""
    _l.load().commet_device_alloc_refuse(int(at_least), int(nth))


def device_alloc_requests():
    """commet_device_alloc_requests: {"requests", "refused", "last_refused_bytes"} since the last device_alloc_refuse call"""
    n, r, b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _l.load().commet_device_alloc_requests(C.byref(n), C.byref(r), C.byref(b))
    return {"requests": int(n.value), "refused": int(r.value), "last_refused_bytes": int(b.value)}


class refusing_device_allocs:
    """with refusing_device_allocs(at_least=..., nth=...) as r: ... — armed inside, always disarmed on exit; r.requests() reads the
    numbers while armed, r.seen holds them as they were at exit"""

    def __init__(self, at_least=0, nth=0):
        self.at_least, self.nth, self.seen = int(at_least), int(nth), None

    def requests(self):
        return device_alloc_requests()

    def __enter__(self):
        device_alloc_refuse(self.at_least, self.nth)
        return self

    def __exit__(self, *a):
        self.seen = device_alloc_requests()
        device_alloc_refuse(0, 0)


def files_packed_bytes(paths):
    """commet_files_packed_bytes: (reads, bases, packed_bytes) of the set ReadSet.from_fasta would make of these files, counted on the
    host — what a residency planner needs before any set is parsed"""
    lib = _l.load()
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    r, b, p = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    if lib.commet_files_packed_bytes(arr, len(paths), C.byref(r), C.byref(b), C.byref(p)) != 0:
        raise CommetError(_err(lib))
    return int(r.value), int(b.value), int(p.value)


def hits_to_tags(ctx, hits, file_reads=None, t_first=1, n_t=1, want_shared=True):
    """Context.hits_to_tags: tags_at for every t in t_first .. t_first + n_t - 1 and the per-file counts, on ctx's device"""
    return ctx.hits_to_tags(hits, file_reads, t_first, n_t, want_shared)


class Context:
    """commet_ctx: device, k, t, the 4-lane Bloom filter in HBM."""

    def __init__(self, k, t=2, device=0):
        self._lib = _l.load()
        self._h = self._lib.commet_create(int(device), int(k), int(t))
        if not self._h:
            raise CommetError(_err(self._lib))
        self.k = int(k)
        self.t = self._lib.commet_min_hits(self._h)
        self.device = int(device)
        self._readsets = weakref.WeakSet()

    def close(self):
        if getattr(self, "_h", None):
            for rs in list(self._readsets):      # read sets die with their context
                rs.close()
            self._lib.commet_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CommetError(_err(self._lib))

    @property
    def max_kmer(self):
        return int(self._lib.commet_max_kmer(self._h))

    def set_option(self, name, value):
        self._check(self._lib.commet_set_option(self._h, name.encode(), int(value)))

    def synchronize(self):
        self._check(self._lib.commet_synchronize(self._h))

    def device_memory(self):
        """commet_device_memory: (free, total) bytes of the context's device; blocks the library keeps for reuse count as free"""
        f, t = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.commet_device_memory(self._h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def filter_reset(self):
        self._check(self._lib.commet_filter_reset(self._h))

    def index_reads(self, rs, first=0, count=None, select_bits=None, want_kmers=True):
        n = rs.num_reads
        if count is None:
            count = n - first
        sel = _as_bits(select_bits, n, "select_bits")
        fed = C.c_uint64(0)
        self._check(self._lib.commet_index_reads(self._h, rs._h, first, count, _ptr(sel),
                                                 C.byref(fed) if want_kmers else None))
        return int(fed.value) if want_kmers else None

    def search_reads(self, rs, active_bits=None):
        n = rs.num_reads
        act = _as_bits(active_bits, n, "active_bits")
        found = np.zeros(bits_nbytes(n), dtype=np.uint8)
        scanned = C.c_uint64(0)
        nfound = C.c_uint64(0)
        self._check(self._lib.commet_search_reads(self._h, rs._h, _ptr(act), _ptr(found), C.byref(scanned),
                                                  C.byref(nfound)))
        return found, int(scanned.value), int(nfound.value)

    def index_and_search(self, index_rs, search_sets, index_select=None, search_selects=None):
        """The chunk loop on resident sets.  Returns (tags, stats, info):
        tags[i] = BooleanVector bytes of search set i, stats[i] = dict(indexed,
        searched, shared) — the numbers of the reference's log line."""
        ns = len(search_sets)
        isel = _as_bits(index_select, index_rs.num_reads, "index_select")
        ssel = _selections(search_selects, search_sets, "search_select")
        tags = [np.zeros(bits_nbytes(rs.num_reads), dtype=np.uint8) for rs in search_sets]
        stats = (_l.PairStats * max(ns, 1))()
        info = _l.JobInfo()
        self._check(self._lib.commet_index_and_search(self._h, index_rs._h, _ptr(isel), ns, _handles(search_sets), _ptrs(ssel), _ptrs(tags),
                                                      stats, C.byref(info)))
        return tags, _stats_list(stats, ns), _info_dict(info)

    def index_many_and_search(self, index_sets, search_rs, index_selects=None, search_select=None):
        """commet_index_many_and_search: job j indexes index_sets[j] (restricted to index_selects[j]) and searches search_rs; the jobs
        share passes over the search set where the library can arrange it.  Returns (tags, stats, info): tags[j], stats[j] as
        index_and_search(index_sets[j], [search_rs], ...) gives them for job j alone."""
        nj = len(index_sets)
        isel = _selections(index_selects, index_sets, "index_select")
        ssel = _as_bits(search_select, search_rs.num_reads, "search_select")
        tags = [np.zeros(bits_nbytes(search_rs.num_reads), dtype=np.uint8) for _ in range(nj)]
        stats = (_l.PairStats * max(nj, 1))()
        info = _l.JobInfo()
        self._check(self._lib.commet_index_many_and_search(self._h, nj, _handles(index_sets), _ptrs(isel), search_rs._h, _ptr(ssel), _ptrs(tags),
                                                           stats, C.byref(info)))
        return tags, _stats_list(stats, nj), _info_dict(info)

    def index_and_profile(self, index_rs, search_sets, index_select=None, search_selects=None, max_hits=8):
        """commet_index_and_profile: the chunk loop with a search that does not stop at t.  Returns (hits, info): hits[i] = np.uint8
        per read of search set i, min(max_hits, the read's greedy non-overlapping full hits on its better strand, in its best chunk);
        tags_at(hits[i], t) is the BooleanVector index_and_search gives on a context of this k and that t, for every t in 1..max_hits.
        The chunk filters are searched in groups of up to set_option("chunk_group", 1..8) per pass over a search set (default 8; 1: one
        filter per pass); the bytes do not depend on it, info["search_launches"] counts the passes.
        set_option("profile_wide", 2) takes the wide bit-sliced rows instead where 12 <= k <= 24 (jobs of many small chunks: every chunk
        filter of a pass side by side in one table set, one hits_wide_kernel launch per search set and pass; "slice_wide_words" caps the
        rows); 1 = never; 0 = auto: jobs of more than 256 chunk filters whose search sets hold no read of more than 300 bases (the shape it
        was measured faster at).  The bytes do not depend on it either.
        set_option("profile_slice", 2) takes the narrow bit-sliced tables where the wide rows do not take the call and 12 <= k <= 24: 32 x
        "slice_words" chunk filters (up to 256) per pass in one table set, one hits_sliced_kernel launch per search set and pass; 1 = never;
        0 = auto, which is never for now.  The bytes do not depend on it.
        set_option("profile_tiled", 2) sends every pass of one or two chunk filters over a set with 25 <= k <= 34 and at most 255 windows per
        read through the tiled probe (tq_probe_kernel, then tq_hits_replay_kernel) on the set's query list of (k, t = 1), which is cached with
        the set (ReadSet.cache_bytes counts it; the search's own list on a context of t = 1); 1 = never; 0 = auto: sets of 2^20 reads or more whose list (8 bytes per k-mer, estimated)
        stays within "query_list_max_mb".
        Independent of "tiled_search"; the bytes do not depend on it."""
        ns = len(search_sets)
        isel = _as_bits(index_select, index_rs.num_reads, "index_select")
        ssel = _selections(search_selects, search_sets, "search_select")
        hits = [np.zeros(rs.num_reads, dtype=np.uint8) for rs in search_sets]
        info = _l.JobInfo()
        self._check(self._lib.commet_index_and_profile(self._h, index_rs._h, _ptr(isel), ns, _handles(search_sets), _ptrs(ssel), int(max_hits),
                                                       _ptrs(hits), C.byref(info)))
        return hits, _info_dict(info)

    def index_many_and_profile(self, index_sets, search_rs, index_selects=None, search_select=None, max_hits=8):
        """commet_index_many_and_profile: job j indexes index_sets[j] (restricted to index_selects[j]) and profiles search_rs (under
        search_select, the same for every job) with a cap of its own: max_hits is an int or a list with one entry per job.  The jobs
        share hits passes over the search set where the library can arrange it (up to eight chunk filters a pass, a job never split;
        set_option("multi_job", 1): job by job; 2: a search set of long reads, which takes a wave per read ("long_search"), shares
        hits passes too — by default its jobs run one by one).  The same read set may appear in several jobs under different selections.
        Returns (hits, info): hits[j] = np.uint8 per read of search_rs, byte for byte what
        index_and_profile(index_sets[j], [search_rs], index_selects[j], [search_select], max_hits[j]) gives for job j alone; info sums
        over the jobs (search_launches = the passes)."""
        nj = len(index_sets)
        caps = [int(max_hits)] * nj if np.isscalar(max_hits) else [int(x) for x in max_hits]
        if len(caps) != nj:
            raise CommetError(f"max_hits: need one entry per job ({nj}), got {len(caps)}")
        isel = _selections(index_selects, index_sets, "index_select")
        ssel = _as_bits(search_select, search_rs.num_reads, "search_select")
        hits = [np.zeros(search_rs.num_reads, dtype=np.uint8) for _ in range(nj)]
        cap_arr = (C.c_int * max(nj, 1))(*caps)
        info = _l.JobInfo()
        self._check(self._lib.commet_index_many_and_profile(self._h, nj, _handles(index_sets), _ptrs(isel), search_rs._h, _ptr(ssel), cap_arr,
                                                            _ptrs(hits), C.byref(info)))
        return hits, _info_dict(info)

    def hits_to_tags(self, hits, file_reads=None, t_first=1, n_t=1, want_shared=True, fill=0):
        """commet_hits_to_tags: hits_tags_kernel on host bytes.  Returns (tags, shared): tags[ti] = tags_at(hits, t_first + ti), made
        on the device; shared[ti][f] = the reads of file f (file_reads: the read counts of contiguous files, default one file) with at
        least that many hits (None when want_shared is false).  fill (tests): the byte the output buffers hold before the call."""
        h = np.ascontiguousarray(hits, dtype=np.uint8)
        fr = np.ascontiguousarray([h.size] if file_reads is None else file_reads, dtype=np.uint64)
        tags = [np.full(bits_nbytes(h.size), fill, dtype=np.uint8) for _ in range(int(n_t))]
        shared = np.full((int(n_t), fr.size), fill * 0x0101010101010101, dtype=np.uint64) if want_shared else None
        self._check(self._lib.commet_hits_to_tags(self._h, _ptr(h) if h.size else None, h.size, fr.size, fr.ctypes.data_as(_l.u64p), int(t_first),
                                                  int(n_t), _ptrs(tags), _ptr(shared)))
        return tags, shared

    def index_and_thresholds(self, index_rs, search_sets, index_select=None, search_selects=None, max_t=8):
        """commet_index_and_thresholds: index_and_profile with max_hits = max_t, thresholded on the device.  Returns (tags, shared,
        info): tags[s][t - 1] = the BooleanVector bytes index_and_search gives for search set s on a context of this k and that t,
        shared[s][t - 1] = np.uint64 per file of set s, its reads among them — for every t in 1..max_t, from one search."""
        ns, T = len(search_sets), int(max_t)
        isel = _as_bits(index_select, index_rs.num_reads, "index_select")
        ssel = _selections(search_selects, search_sets, "search_select")
        tags = [[np.zeros(bits_nbytes(rs.num_reads), dtype=np.uint8) for _ in range(T)] for rs in search_sets]
        shared = [[np.zeros(rs.num_files, dtype=np.uint64) for _ in range(T)] for rs in search_sets]
        info = _l.JobInfo()
        self._check(self._lib.commet_index_and_thresholds(self._h, index_rs._h, _ptr(isel), ns, _handles(search_sets), _ptrs(ssel), T,
                                                          _ptrs([a for row in tags for a in row]), _ptrs([a for row in shared for a in row]),
                                                          C.byref(info)))
        return tags, shared, _info_dict(info)

    def index_many_and_thresholds(self, index_sets, search_rs, index_selects=None, search_select=None, t=2):
        """commet_index_many_and_thresholds: index_many_and_profile with max_hits[j] = t[j] (an int or one entry per job), thresholded
        on the device: the many-job search with a threshold per job.  Returns (tags, shared, info): tags[j] = job j's BooleanVector
        bytes at t[j], shared[j] = np.uint64 per file of search_rs."""
        nj = len(index_sets)
        ts = [int(t)] * nj if np.isscalar(t) else [int(x) for x in t]
        if len(ts) != nj:
            raise CommetError(f"t: need one entry per job ({nj}), got {len(ts)}")
        isel = _selections(index_selects, index_sets, "index_select")
        ssel = _as_bits(search_select, search_rs.num_reads, "search_select")
        tags = [np.zeros(bits_nbytes(search_rs.num_reads), dtype=np.uint8) for _ in range(nj)]
        shared = [np.zeros(search_rs.num_files, dtype=np.uint64) for _ in range(nj)]
        info = _l.JobInfo()
        self._check(self._lib.commet_index_many_and_thresholds(self._h, nj, _handles(index_sets), _ptrs(isel), search_rs._h, _ptr(ssel),
                                                               (C.c_int * max(nj, 1))(*ts), _ptrs(tags), _ptrs(shared), C.byref(info)))
        return tags, shared, _info_dict(info)

    def index_and_search_relative(self, index_rs, search_sets, index_select=None, search_selects=None, percent=50, min_hits=1):
        """commet_index_and_search_relative: the chunk loop with a threshold per read, t_r = max(min_hits, ceil(percent / 100 x W_r)),
        W_r = len // k the most non-overlapping k-mers the read can hold (relative.thresholds is the rule in numpy).  A read is found
        when one chunk filter holds t_r of its non-overlapping k-mers on one strand; a read with t_r > W_r never is.  Returns (tags,
        shared, info): tags[s] = the BooleanVector bytes of search set s, shared[s] = np.uint64 per file of set s, both made on the
        device.  The context's own t is not used.  Where every read gets the same t_r the result is index_and_search's at that t."""
        ns = len(search_sets)
        isel = _as_bits(index_select, index_rs.num_reads, "index_select")
        ssel = _selections(search_selects, search_sets, "search_select")
        tags = [np.zeros(bits_nbytes(rs.num_reads), dtype=np.uint8) for rs in search_sets]
        shared = [np.zeros(rs.num_files, dtype=np.uint64) for rs in search_sets]
        info = _l.JobInfo()
        self._check(self._lib.commet_index_and_search_relative(self._h, index_rs._h, _ptr(isel), ns, _handles(search_sets), _ptrs(ssel),
                                                               int(percent), int(min_hits), _ptrs(tags), _ptrs(shared), C.byref(info)))
        return tags, shared, _info_dict(info)

    def poison(self, byte):
        """test hook: every bit array of the context (filter slots, interleaved A planes, bit-sliced planes and tables) filled with `byte`"""
        self.set_option("poison", byte)

    def export_filter_reference(self, slot=0):
        """the filter of `slot` in the reference's byte layout (a job leaves the chunk filters of its last groups in slots 0 .. g - 1)"""
        self.set_option("export_slot", slot)
        nbytes = int(2 ** (self.k - 1))
        out = np.zeros(max(nbytes, 1), dtype=np.uint8)
        self._check(self._lib.commet_filter_export_reference(self._h, _ptr(out), out.size))
        return out[:nbytes]

    def filter_set_bits(self, slot=0, cap=1 << 23):
        """test hook: the set bits of `slot` as stored, sorted np.uint64 words (plane << 56) | address within the plane (plane 0 = A at
        its psi_a address, 1..3 = B, C, D at the key) — exact at every k, where the byte export needs 2^(k-1) bytes of host memory.
        More than `cap` set bits: CommetError, which names the count."""
        self.set_option("export_slot", slot)
        out = np.zeros(max(int(cap), 1), dtype=np.uint64)
        n = C.c_uint64(0)
        self._check(self._lib.commet_filter_set_bits(self._h, _ptr(out), int(cap), C.byref(n)))
        if n.value > cap:
            raise CommetError(f"filter_set_bits: slot {slot} holds {n.value} set bits, cap = {cap}")
        return np.sort(out[:n.value])

    def last_kernel_ms(self):
        i = C.c_double(0)
        s = C.c_double(0)
        self._check(self._lib.commet_last_kernel_ms(self._h, C.byref(i), C.byref(s)))
        return i.value, s.value

    def kernel_times(self):
        """{kernel: (launches, total_ms)} since set_option("kernel_timing", 1)"""
        arr = (_l.KernelTime * 64)()
        n = C.c_int(0)
        self._check(self._lib.commet_kernel_times(self._h, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n.value, 64))}

    def cache_stats(self):
        """HBM held by the cached query lists of this context's read sets: dict(bytes, budget_bytes, evictions)"""
        b, g, e = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.commet_cache_stats(self._h, C.byref(b), C.byref(g), C.byref(e)))
        return dict(bytes=int(b.value), budget_bytes=int(g.value), evictions=int(e.value))

    def membench(self, atomic, table_bytes, n_access):
        ms = C.c_double(0)
        self._check(self._lib.commet_membench(self._h, int(atomic), int(table_bytes), int(n_access), C.byref(ms)))
        return ms.value

    def ldsbench(self, mode, n_words, n_access):
        ms = C.c_double(0)
        self._check(self._lib.commet_ldsbench(self._h, int(mode), int(n_words), int(n_access), C.byref(ms)))
        return ms.value


class ReadSet:
    """commet_readset: the reads of one set, packed and resident in HBM."""

    def __init__(self, ctx, max_reads, max_bases, _handle=None):
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = _handle if _handle is not None else self._lib.commet_readset_create(ctx._h, int(max_reads), int(max_bases))
        if not self._h:
            raise CommetError(_err(self._lib))
        ctx._readsets.add(self)

    @classmethod
    def from_fasta(cls, ctx, paths):
        """Maps the FASTA files of one set (host parser in the library), streams them to HBM, finalizes."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        h = ctx._lib.commet_readset_from_fasta(ctx._h, arr, len(paths))
        if not h:
            raise CommetError(_err(ctx._lib))
        rs = cls(ctx, 0, 0, _handle=h)
        rs.finalize()
        return rs

    def save(self, path):
        """Writes the packed image of the set (commet_readset_save)."""
        self._check(self._lib.commet_readset_save(self._h, os.fsencode(path)))

    @classmethod
    def load(cls, ctx, path):
        """Loads a packed image written by save() — no parsing; finalizes."""
        h = ctx._lib.commet_readset_load(ctx._h, os.fsencode(path))
        if not h:
            raise CommetError(_err(ctx._lib))
        rs = cls(ctx, 0, 0, _handle=h)
        rs.finalize()
        return rs

    def export(self):
        """Descriptor + HIP IPC handles of the set's device buffers (bytes): another process of the node imports the set
        from it, device to device, without a file.  This set must stay alive until every importer has returned."""
        n = C.c_uint64(0)
        self._check(self._lib.commet_readset_export(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self._check(self._lib.commet_readset_export(self._h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]

    @classmethod
    def import_(cls, ctx, blob):
        """A set exported by another process of the node (ReadSet.export), copied device to device; finalizes."""
        h = ctx._lib.commet_readset_import(ctx._h, blob, len(blob))
        if not h:
            raise CommetError(_err(ctx._lib))
        rs = cls(ctx, 0, 0, _handle=h)
        rs.finalize()
        return rs

    def filter(self, min_len=0, max_n=None, min_shannon=0.0, max_reads=None):
        """commet_readset_filter: the reads `filter_reads -l min_len -n max_n -e min_shannon -m max_reads` selects in each file of the
        set, decided on the device from the resident planes.  max_n None: any number of non-ACGT bases; max_reads None: no cap (it
        applies per file).  Returns (bits, stats): the set-wide selection (the form index_and_search takes as a select) and, per file,
        dict(reads, selected, removed_length, removed_n, removed_shannon) — the numbers the tool prints."""
        nf = self.num_files
        bits = np.zeros(bits_nbytes(self.num_reads), dtype=np.uint8)
        st = (_l.FilterStats * max(nf, 1))()
        self._check(self._lib.commet_readset_filter(self._ctx._h, self._h, int(min_len), -1 if max_n is None else int(max_n),
                                                    float(min_shannon), -1 if max_reads is None else int(max_reads), _ptr(bits), st))
        return bits, [{f: int(getattr(st[i], f)) for f, _ in _l.FilterStats._fields_} for i in range(nf)]

    def relative_thresholds(self, percent, min_hits=1):
        """commet_readset_relative_thresholds: np.uint16 per read, the threshold index_and_search_relative gives it under no selection
        (relative.thresholds is the same rule in numpy); 0 where the read cannot hold that many non-overlapping k-mers"""
        out = np.zeros(self.num_reads, dtype=np.uint16)
        self._check(self._lib.commet_readset_relative_thresholds(self._ctx._h, self._h, int(percent), int(min_hits), _ptr(out)))
        return out

    def file_reads(self):
        return [int(self._lib.commet_readset_file_reads(self._h, i)) for i in range(self.num_files)]

    @classmethod
    def from_files(cls, ctx, files):
        """files: list of (bases uint8[...], offsets uint64[n+1]) — one entry per file of the set."""
        nr = sum(len(o) - 1 for _, o in files)
        nb = sum(int(o[-1]) for _, o in files)
        rs = cls(ctx, nr, nb)
        for b, o in files:
            rs.add_file(b, o)
        rs.finalize()
        return rs

    @property
    def cache_bytes(self):
        """HBM held by data derived from the set and cached with it (the tiled search's query list and, beside it, the tiled hit profile's)"""
        return int(self._lib.commet_readset_cache_bytes(self._h))

    def drop_cache(self):
        self._lib.commet_readset_drop_cache(self._h)

    def cache_estimate(self):
        """bytes of the set's query list for its context's (k, t); 0 = the set does not qualify for the tiled search"""
        return int(self._lib.commet_readset_cache_estimate(self._ctx._h, self._h))

    def reserve_cache(self):
        """commet_readset_reserve_cache: asks the driver NOW (from the calling thread) for the memory the set's query list will need, so
        that a list above the cap can be built later without an allocation on a job's path"""
        self._ctx._check(self._lib.commet_readset_reserve_cache(self._ctx._h, self._h))

    def offload(self):
        """commet_readset_offload: the set leaves the device for pageable host memory of its own; refused while a job uses it"""
        self._check(self._lib.commet_readset_offload(self._h))

    def restore(self):
        """commet_readset_restore: the offloaded set comes back, indistinguishable from before"""
        self._check(self._lib.commet_readset_restore(self._h))

    @property
    def resident(self):
        return bool(self._lib.commet_readset_is_resident(self._h))

    @property
    def device_bytes(self):
        """bytes the set's own buffers hold on the device now (0 when offloaded)"""
        return int(self._lib.commet_readset_device_bytes(self._h))

    @property
    def packed_bytes(self):
        """bytes the set's own buffers hold when resident, whether or not it is resident now"""
        return int(self._lib.commet_readset_packed_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.commet_readset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CommetError(_err(self._lib))

    def add_file(self, bases, offsets):
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        if o.size < 1 or int(o[-1]) > b.size:
            raise CommetError("offsets do not match bases")
        self._check(self._lib.commet_readset_begin_file(self._h))
        self._check(self._lib.commet_readset_append(self._h, _ptr(b), _ptr(o), o.size - 1))

    def add_file_staged(self, bases, offsets):
        """The same through the pinned staging API (commet_readset_stage_acquire / _commit): the caller's parser writes
        ASCII bases straight into pinned buffers, the device packs them (pack_reads_kernel)."""
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        o = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = o.size - 1
        self._check(self._lib.commet_readset_begin_file(self._h))
        done = 0
        while done < n:
            hb, ho = _l.u8p(), _l.u64p()
            bcap, rcap = C.c_uint64(0), C.c_uint64(0)
            self._check(self._lib.commet_readset_stage_acquire(self._h, C.byref(hb), C.byref(bcap), C.byref(ho), C.byref(rcap)))
            b0 = int(o[done])
            take = 0
            while done + take < n and take < rcap.value and int(o[done + take + 1]) - b0 <= bcap.value:
                take += 1
            if take == 0:
                self._check(self._lib.commet_readset_stage_commit(self._h, 0))
                raise CommetError("a read does not fit the staging buffer")
            nb = int(o[done + take]) - b0
            C.memmove(hb, b[b0:b0 + nb].ctypes.data, nb)
            offs = (o[done:done + take + 1] - np.uint64(b0)).astype(np.uint64)
            C.memmove(ho, offs.ctypes.data, offs.size * 8)
            self._check(self._lib.commet_readset_stage_commit(self._h, take))
            done += take

    def finalize(self):
        self._check(self._lib.commet_readset_finalize(self._h))

    @property
    def num_reads(self):
        return int(self._lib.commet_readset_num_reads(self._h))

    @property
    def num_files(self):
        return int(self._lib.commet_readset_num_files(self._h))

    def kmer_counts(self):
        out = np.zeros(max(self.num_reads, 1), dtype=np.uint32)
        self._check(self._lib.commet_readset_kmer_counts(self._h, _ptr(out)))
        return out[:self.num_reads]
