"""A numpy model of hits_tags_kernel's contract (commet_amd/csrc/hits_tags.hpp) and the designed byte arrays its tests run on.
Shared by tests/test_matrix_sweep_cpu.py (the model against api.tags_at and matrix_io.popcount) and tests/test_gpu_thresholds.py
(the kernel against the model).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4099]
RANGES = [(1, 1), (1, 8), (3, 2), (1, 255), (255, 1)]           # (t_first, n_t)


def model(hits, file_reads, t_first, n_t):
    """-> (tags, shared): tags[ti] = n // 8 + 1 bytes, bit r % 64 of 64-bit word r // 64 = hits[r] >= t_first + ti, bits past n zero;
    shared[ti, f] = the reads of file f (contiguous runs of file_reads[f] reads) with at least that many hits.  Word by word and
    read by read: nothing of packbits / unpackbits, which the host code under comparison uses."""
    h = np.asarray(hits, dtype=np.uint8)
    n = h.size
    assert sum(int(c) for c in file_reads) == n
    ends = np.cumsum([int(c) for c in file_reads]).tolist()
    tags, shared = [], np.zeros((n_t, len(file_reads)), dtype=np.uint64)
    for ti in range(n_t):
        t = t_first + ti
        words = [0] * (n // 64 + 1)
        f = 0
        for r in range(n):
            while ends[f] <= r:
                f += 1
            if int(h[r]) >= t:
                words[r >> 6] |= 1 << (r & 63)
                shared[ti, f] += 1
        raw = b"".join(w.to_bytes(8, "little") for w in words)
        tags.append(np.frombuffer(raw, dtype=np.uint8)[:n // 8 + 1].copy())
    return tags, shared


def fast_model(hits, file_reads, t_first, n_t):
    """the same contract, vectorised (what the GPU test compares against at every size; checked against model() on the CPU)"""
    h = np.asarray(hits, dtype=np.uint8)
    n = h.size
    starts = np.concatenate([[0], np.cumsum(np.asarray(file_reads, dtype=np.int64))]).astype(np.int64)
    tags, shared = [], np.zeros((n_t, len(file_reads)), dtype=np.uint64)
    for ti in range(n_t):
        ge = np.zeros((n // 8 + 1) * 8, dtype=np.uint8)
        ge[:n] = h >= (t_first + ti)
        tags.append(np.packbits(ge, bitorder="little"))
        csum = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(ge[:n], dtype=np.int64)])
        shared[ti] = csum[starts[1:]] - csum[starts[:-1]]
    return tags, shared


def file_cuts(n):
    """{name: file_reads} — one file; a cut at a multiple of 64; a cut at 16 m + 5; two cuts inside one 64-read word; an empty first,
    middle and last file.  Cuts past n are clamped to n (small sizes: the files behind them are empty)"""
    def reads(cuts):
        c = [0] + [min(x, n) for x in cuts] + [n]
        return [b - a for a, b in zip(c[:-1], c[1:])]
    m64 = 64 * max(1, n // 128)
    m16 = 16 * (n // 32) + 5
    w = 64 * (n // 128)
    mid = n // 2
    return {"one": [n], "cut64": reads([m64]), "cut16m5": reads([m16]), "two_in_word": reads([w + 20, w + 41]),
            "empties": [0] + reads([mid, mid]) + [0]}


def boundaries(n, file_reads):
    """the reads either side of every boundary: first and last read, file cuts, the 16-byte piece of a lane, the 64-read word, the
    1024 reads of a wave, the 4096 reads of a tile"""
    at = {0, n}
    at.update(np.cumsum(file_reads).tolist())
    for step in (16, 64, 1024, 4096):
        at.update(range(0, n + 1, step))
    pos = sorted({p for b in at for p in (b - 1, b) if 0 <= p < n})
    return pos


def designed_bytes(n, file_reads, t_first, n_t, rotation):
    """n bytes: the values 0, t - 1, t, t + 1 and 255 for the first and the last threshold of the range, drawn at random everywhere and
    dealt out in turn (from `rotation` on) over boundaries()"""
    vals = []
    for t in (t_first, t_first + n_t - 1):
        vals += [0, t - 1, t, min(t + 1, 255), 255]
    rng = np.random.default_rng(1000 * n + 10 * t_first + n_t)
    h = rng.choice(np.array(vals, dtype=np.uint8), size=n) if n else np.zeros(0, dtype=np.uint8)
    for i, p in enumerate(boundaries(n, file_reads)):
        h[p] = vals[(i + rotation) % len(vals)]
    return h
