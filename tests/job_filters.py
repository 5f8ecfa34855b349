"""What a job's chunk filters must hold, byte for byte (test_gpu_job_filter_bytes.py on the GPU, test_job_filters_cpu.py here):
no GPU, TEST INFRASTRUCTURE ONLY.

A job builds the filter of every chunk with `launch_index(fresh_filter = true, filter_zeroed = false)`: no memset, the bucketed build
defines all 2^(k+2) bits of the slot itself.  The checker gives the bytes each slot must then hold:

checker_run     the restated tool's run of the job with its chunk trace (ok_trace_begin / ok_trace_end): tags, log numbers, and per
                chunk (first, last, reads, k-mers) in set-wide read numbers
chunk_filter    ob.Bloom(k) fed with the selected reads of [first, last]: the reference's bytes of that chunk's filter
tile_census     the build's buckets of a chunk counted from the checker's keys: how many are empty (a tile written as zeros by a
                work item of its own), hold 1 .. 2^17 keys (one build workgroup stores the tile), or more (several workgroups OR
                into a tile that part_zero_split_kernel has cleared)
slot_chunks     which chunk run_slots built last into every filter slot
first_difference  where two filters differ, by tile, for an assertion's message"""
import ctypes as C
import collections
import os

import numpy as np

import oracle_binding as ob
import util

TILE_BITS = 19                    # index_part.hpp: a bucket is a tile of 2^19 bits of one plane
BUILD_CAP = 1 << 17               # keys per build workgroup: a bucket of more is split
POISONS = (0xFF, 0xA5)


def checker_run(d, k, t, index_reads, search_sets, max_kmer=0, index_select=None):
    """the checker's run of the job (checkers.checker_job, with an input filter on the index set and the chunk trace)
    -> dict(tags = bools per search set, stats = [dict(indexed, searched, shared, probes)], chunks, kmers,
            trace = [(first, last, reads, k-mers)] per chunk)"""
    d = str(d)
    os.makedirs(d, exist_ok=True)
    util.write_fasta(os.path.join(d, "I.fa"), index_reads)
    if index_select is not None:
        util.write_bv(os.path.join(d, "I.fa.bv"), "filter of I.fa", index_select)
    open(os.path.join(d, "i.txt"), "w").write("I:I.fa" + (",I.fa.bv" if index_select is not None else "") + "\n")
    for q, rs in enumerate(search_sets):
        util.write_fasta(os.path.join(d, f"Q{q:02d}.fa"), rs)
    open(os.path.join(d, "s.txt"), "w").write("".join(f"Q{q:02d}:Q{q:02d}.fa\n" for q in range(len(search_sets))))
    trace = np.zeros((4096, 4), dtype=np.uint64)
    lib = ob.load()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        lib.ok_trace_begin(trace.ctypes.data_as(C.c_void_p), len(trace))
        try:
            rc, res, chunks, kmers = ob.index_and_search("i.txt", "s.txt", f"out{t}", f"log{t}", k, t, max_kmer=max_kmer)
        finally:
            n_traced = int(lib.ok_trace_end())
    finally:
        os.chdir(cwd)
    assert rc == 0 and len(res) == len(search_sets) and n_traced == chunks <= len(trace)
    by_name = {r["name"]: r for r in res}
    tags, stats = [], []
    for q, rs in enumerate(search_sets):
        _, n, bits = util.read_bv(os.path.join(d, f"out{t}", f"Q{q:02d}.fa_in_I.bv"))
        assert n == len(rs)
        tags.append(util.bools_from_bits(bits, n))
        stats.append(by_name[f"Q{q:02d}"])
    return dict(tags=tags, stats=stats, chunks=chunks, kmers=kmers, trace=[tuple(int(v) for v in row) for row in trace[:chunks]])


def chunk_select(n_reads, row, index_select=None):
    """the job's indexed reads restricted to the chunk of trace row (first, last, reads, k-mers), as bools"""
    first, last, reads, _ = row
    sel = np.zeros(n_reads, dtype=bool)
    if reads:
        sel[first:last + 1] = True if index_select is None else np.asarray(index_select, dtype=bool)[first:last + 1]
        assert int(sel.sum()) == reads, (row, int(sel.sum()))
    return sel


def chunk_filter(k, index_reads, row, index_select=None):
    """the checker's filter bytes of one chunk of the job: 2^(k-1) bytes, reference layout"""
    sel = chunk_select(len(index_reads), row, index_select)
    bases, offs = util.to_batch(index_reads)
    f = ob.Bloom(k)
    fed = f.index(bases, offs, util.bits_from_bools(sel))
    assert fed == row[3], (row, fed)
    out = f.bytes()
    f.close()
    return out


def bucket_counts(k, reads):
    """keys per bucket of the bucketed build, bucket = (plane << (k - 19)) | (key >> 19) as in PartGeom: 2^(k-17) counts"""
    assert k >= TILE_BITS + 1
    shift = k - TILE_BITS
    counts = np.zeros(4 << shift, dtype=np.int64)
    for read, copies in collections.Counter(reads).items():
        keys, _ = ob.keys_of_read(read, k)
        for plane in range(4):
            counts += copies * np.bincount((plane << shift) | (keys[:, plane] >> np.uint64(TILE_BITS)).astype(np.int64), minlength=len(counts))
    return counts


def tile_census(k, index_reads, row, index_select=None):
    """-> dict(empty, single, split, keys) of the chunk of trace row: buckets without a key, of 1 .. 2^17 keys, of more"""
    sel = chunk_select(len(index_reads), row, index_select)
    counts = bucket_counts(k, [r for r, s in zip(index_reads, sel) if s])
    assert int(counts.sum()) == 4 * row[3]
    return dict(empty=int((counts == 0).sum()), single=int(((counts > 0) & (counts <= BUILD_CAP)).sum()), split=int((counts > BUILD_CAP).sum()),
                keys=int(counts.sum()))


def classes(census):
    """the bucket classes a chunk contains, as a set of names"""
    return {n for n in ("empty", "single", "split") if census[n]}


def slot_chunks(n_chunks, group):
    """run_slots (capi/job.hpp) takes the chunks in groups of `group` and builds the chunks of a group into slots 0, 1, ...  -> per
    slot 0 .. group - 1 the chunk built into it last (None: never).  Slots at or beyond the last group's size keep the chunk of the
    group before."""
    assert n_chunks >= 1 and group >= 1
    out = [None] * group
    for c0 in range(0, n_chunks, group):
        for i in range(min(group, n_chunks - c0)):
            out[i] = c0 + i
    return out


def effective_group(n_chunks, chunk_group):
    """the group size run_slots forms for search sets that qualify for groups of eight: one chunk goes alone, five to eight filters
    per pass only for jobs of more than four chunks"""
    if n_chunks < 2:
        return 1
    return chunk_group if chunk_group <= 4 or n_chunks > 4 else 4


def first_difference(got, want):
    """None when the filters are byte-equal, else a message: the first differing tile (byte offset >> 16), the bytes that differ in
    it and in all, the set bits that are extra / missing there, and the build's bucket (key >> 19 = byte offset >> 18) with the planes"""
    if got.shape != want.shape:
        return f"{got.size} bytes, expected {want.size}"
    step = 1 << 24
    first, total = None, 0
    for o in range(0, got.size, step):
        d = got[o:o + step] != want[o:o + step]
        n = int(np.count_nonzero(d))
        if n and first is None:
            first = o + int(np.argmax(d))
        total += n
    if first is None:
        return None
    tile = first >> 16
    g, w = got[tile << 16:(tile + 1) << 16], want[tile << 16:(tile + 1) << 16]
    extra = np.bitwise_and(g, np.bitwise_not(w))
    missing = np.bitwise_and(w, np.bitwise_not(g))
    either = int(np.bitwise_or.reduce(np.bitwise_xor(g, w)))
    planes = "".join(p for p, m in zip("abcd", (0x88, 0x44, 0x22, 0x11)) if either & m)
    return (f"first differing tile {tile} (byte {first}, bucket key >> 19 = {first >> 18}, planes {planes}): {int(np.count_nonzero(g != w))} bytes differ there "
            f"({int(np.unpackbits(extra).sum())} extra bits, {int(np.unpackbits(missing).sum())} missing), {total} bytes in all; "
            f"got 0x{int(got[first]):02x}, expected 0x{int(want[first]):02x}")


# ---- index sets with all three bucket classes ---------------------------------------------------------------------------------------
def three_class_reads(seed, k, n_random, n_chunks=1, hot=300):
    """random reads of 40-160 bases (few: most buckets stay empty), copies of A x 150 (every plane's bucket 0 gets more than 2^17
    equal keys per chunk: split tiles), `hot` (ACG)-repeat reads (hot buckets of one workgroup), shuffled"""
    rng = np.random.default_rng(seed)
    poly = (BUILD_CAP // (150 - k + 1) + 12) * n_chunks + 100 * (n_chunks - 1)
    reads = util.random_reads(rng, n_random, max(40, k), 160, n_rate=0.005) + [b"A" * 150] * poly + [(b"ACG" * 50)[:110 + i % 3] for i in range(hot)]
    return [reads[i] for i in rng.permutation(len(reads))]


def max_kmer_for(k, reads, n_chunks, select=None):
    """-> (max_kmer, chunks as the planner will cut them [(first, end)]) so that `reads` (restricted to `select`) make n_chunks chunks
    of about equal k-mer counts"""
    import oracle_pool
    bases, offs = util.to_batch(reads)
    kc = ob.kmer_counts(bases, offs, k).astype(np.int64)
    if select is not None:
        kc = kc[np.asarray(select, dtype=bool)]
    total = int(kc.sum())
    if n_chunks == 1:
        return total + 1, [(0, len(kc))]
    mk = total // n_chunks
    for _ in range(200):
        got = oracle_pool.chunks_from_counts(kc, mk)
        if len(got) == n_chunks and int(kc[got[-1][0]:got[-1][1]].sum()) * 2 > mk:
            return mk, got
        mk += (1 if len(got) > n_chunks else -1) * max(1, total // (200 * n_chunks))
    raise AssertionError(f"no max_kmer gives {n_chunks} chunks")
