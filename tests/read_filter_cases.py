"""The cases of the read-filter tests (tests/test_read_filter_rule.py on the CPU, tests/test_gpu_read_filter.py on the GPU): read
files made from fixed seeds and the filter options that go with them.  A case is one read SET (one or more files); the tool runs
once per file with the case's options, the device filter once per set.

    Case.build(dir)       writes the files, returns their paths
    Case.tool_args(...)   the options as filter_reads takes them on its command line
    Case.api_kwargs()     the same options as ReadSet.filter takes them
"""
import math
import os

import numpy as np

import util


class Case:
    def __init__(self, name, files, l=None, n=None, e=None, m=None, extra=()):
        """files: [(file name, format, reads, write_reads keywords)]; e: the -e value AS TEXT (what the tool's atof reads);
        extra: tool-only options (-c)"""
        self.name, self.files, self.l, self.n, self.e, self.m, self.extra = name, files, l, n, e, m, list(extra)

    def build(self, d):
        os.makedirs(d, exist_ok=True)
        paths = []
        for fname, fmt, reads, kw in self.files:
            kw = dict(kw)
            if "rng_seed" in kw:
                kw["rng"] = np.random.default_rng(kw.pop("rng_seed"))
            p = os.path.join(d, fname)
            util.write_reads(p, reads, fmt, **kw)
            paths.append(p)
        return paths

    def tool_args(self, with_extra=True):
        a = []
        if self.l is not None:
            a += ["-l", str(self.l)]
        if self.n is not None:
            a += ["-n", str(self.n)]
        if self.e is not None:
            a += ["-e", self.e]
        if self.m is not None:
            a += ["-m", str(self.m)]
        return a + (self.extra if with_extra else [])

    def api_kwargs(self):
        return dict(min_len=self.l or 0, max_n=self.n, min_shannon=float(self.e) if self.e is not None else 0.0, max_reads=self.m)

    def __repr__(self):
        return self.name


def shannon_index(read):
    """the tool's index of a read (filter_reads.cpp:265-306) in its own number formats: float index, double terms"""
    s = read.upper()
    L = len(s)
    acgt = [s.count(c) for c in (b"A", b"C", b"G", b"T")]
    idx = np.float32(0)
    for c in acgt + [L - sum(acgt)]:
        f = np.float32(c) / np.float32(L)
        if f == 0:
            continue
        idx = np.float32(float(idx) + float(f) * math.log(float(f)) / math.log(2))
    return abs(idx)


def _host_tools_reads(seed, n=300):
    """tests/test_host_tools.py, _make_fasta"""
    rng = np.random.default_rng(seed)
    reads = util.random_reads(rng, n, 1, 120, n_rate=0.03, lower_rate=0.2, other_rate=0.01)
    reads[5] = b"A" * 80                      # Shannon 0
    reads[6] = b"AC" * 40                     # Shannon 1
    reads[7] = b"N" * 30
    return reads, dict(rng_seed=seed + 1000, multiline=(seed % 2 == 0))


def _shuffled(rng, counts):
    s = np.frombuffer(b"".join(bytes([c]) * k for c, k in zip(b"ACGT", counts)), dtype=np.uint8).copy()
    rng.shuffle(s)
    return s.tobytes()


def _cases():
    out = []
    # the twelve option sets of tests/test_host_tools.py, on its reads
    twelve = [(1, {}), (2, dict(l=50)), (3, dict(n=2)), (4, dict(e="1.9")), (5, dict(l=30, n=1, e="1.5")), (6, dict(m=40)), (7, dict(m=0)),
              (8, dict(l=64, e="1.95", m=25)), (9, dict(l=10, extra=["-c", "my comment"])), (10, dict(e="0")), (11, dict(m=300)),
              (12, dict(n=0, m=7))]
    for seed, o in twelve:
        reads, kw = _host_tools_reads(seed)
        out.append(Case(f"host_tools_{seed}", [("reads.fa", "fa", reads, kw)], **o))

    # one read length / ragged
    rng = np.random.default_rng(101)
    uni = util.random_reads(rng, 700, 100, 100, n_rate=0.01, lower_rate=0.1, other_rate=0.004)
    for i in range(0, 60, 3):                                    # low-complexity reads of the same length
        uni[i] = _shuffled(rng, [100 - 3 * (i // 3), i // 3, i // 3, i // 3])
    out.append(Case("uniform_100", [("u.fa", "fa", uni, {})], l=50, n=2, e="1.5"))
    rng = np.random.default_rng(102)
    out.append(Case("ragged_1_150", [("r.fa", "fa", util.random_reads(rng, 900, 1, 150, n_rate=0.02, lower_rate=0.15, other_rate=0.005), {})],
                    l=60, n=2, e="1.8"))
    # lower case, N, IUPAC, CRLF lines
    rng = np.random.default_rng(103)
    out.append(Case("crlf_iupac", [("c.fa", "fa", util.random_reads(rng, 400, 1, 150, n_rate=0.04, lower_rate=0.5, other_rate=0.03), dict(crlf=True))],
                    l=40, n=3, e="1.7"))
    # FASTQ, gzipped FASTA
    rng = np.random.default_rng(104)
    out.append(Case("fastq", [("q.fq", "fq", util.random_reads(rng, 500, 20, 150, n_rate=0.02, lower_rate=0.1, other_rate=0.005), {})], l=60, n=1, e="1.9"))
    out.append(Case("fastq_crlf", [("qc.fq", "fq", util.random_reads(rng, 300, 20, 150, n_rate=0.02, lower_rate=0.1, other_rate=0.005), dict(crlf=True))],
                    l=60, n=2, e="1.9"))
    out.append(Case("fasta_gz", [("z.fa.gz", "fa.gz", util.random_reads(rng, 500, 1, 150, n_rate=0.02, lower_rate=0.1, other_rate=0.005), {})], l=30, n=2, e="1.6"))
    # a set of three files; -m smaller than, equal to and larger than a file's reads, and 0
    rng = np.random.default_rng(105)
    three = [("a.fa", "fa", util.random_reads(rng, 40, 10, 150, n_rate=0.02), {}),
             ("b.fq", "fq", util.random_reads(rng, 64, 10, 150, n_rate=0.02), {}),
             ("c.fa", "fa", util.random_reads(rng, 130, 10, 150, n_rate=0.02), dict(rng_seed=7, multiline=True))]
    for m in (30, 64, 40, 200, 0):
        out.append(Case(f"three_files_m{m}", three, l=30, n=3, e="1.2", m=m))
    out.append(Case("three_files_m64_keep_all", three, m=64))     # every read kept: the cap is reached with a file's last read
    out.append(Case("three_files_no_m", three, l=30, n=3, e="1.2"))
    # an empty record in the middle of a file
    rng = np.random.default_rng(106)
    for fmt in ("fa", "fq"):
        reads = util.random_reads(rng, 200, 10, 150, n_rate=0.02)
        reads[77] = b""
        out.append(Case(f"empty_record_{fmt}", [("e." + fmt, fmt, reads, {})], l=40, e="1.5"))
        out.append(Case(f"empty_record_{fmt}_m50", [("e." + fmt, fmt, reads, {})], l=40, e="1.5", m=50))
        out.append(Case(f"empty_record_{fmt}_m150", [("e." + fmt, fmt, reads, {})], l=40, e="1.5", m=150))
    two = [("e0.fa", "fa", reads, {}), ("e1.fa", "fa", util.random_reads(rng, 90, 10, 150), {})]
    out.append(Case("empty_record_two_files", two, l=40, n=2, e="1.5", m=60))
    # reads longer than 1024 bases among short ones: both kernel mappings, and the reads the host decides
    rng = np.random.default_rng(107)
    mixed = util.random_reads(rng, 300, 30, 150, n_rate=0.02, lower_rate=0.1, other_rate=0.004)
    for i in range(0, 300, 9):
        mixed[i] = util.random_reads(rng, 1, 600, 3000, n_rate=0.003)[0]
    mixed[4] = b"AC" * 700                                       # index 1, longer than the table
    mixed[13] = b"A" * 1500                                      # index 0
    mixed[22] = _shuffled(rng, [1000, 500, 500, 0])              # index 1.5
    mixed[31] = _shuffled(rng, [300, 300, 300, 300])             # index 2
    mixed[40] = _shuffled(rng, [256, 256, 256, 256])             # 1024: the table's last row
    mixed[49] = _shuffled(rng, [257, 256, 256, 256])             # 1025: the first length the host decides
    mixed[58] = b"N" * 1100
    for e in ("1", "1.5", "2", "1.99"):
        out.append(Case(f"long_mixed_e{e}", [("long.fa", "fa", mixed, {})], l=60, n=5, e=e))
    out.append(Case("long_mixed_no_shannon", [("long.fa", "fa", mixed, {})], l=100, n=1))
    out.append(Case("long_mixed_fq_m", [("long.fq", "fq", mixed, {}), ("short.fa", "fa", mixed[1:4], {})], l=60, n=5, e="1.5", m=100))
    rng = np.random.default_rng(108)
    mid = util.random_reads(rng, 200, 30, 1024, n_rate=0.01, lower_rate=0.1)   # longest read > 512: a wave per read, the table covers all
    mid[3] = _shuffled(rng, [256, 256, 256, 256])
    mid[9] = b"AC" * 300
    out.append(Case("mid_600_1024", [("mid.fa", "fa", mid, {})], l=60, n=8, e="1.98"))
    # thresholds that sit exactly on reachable indices (the test is <: such a read is kept)
    rng = np.random.default_rng(109)
    th = util.random_reads(rng, 200, 80, 80, n_rate=0.0, lower_rate=0.0, other_rate=0.0)
    th[0] = b"AC" * 40                                           # index 1
    th[1] = _shuffled(rng, [20, 20, 20, 20])                     # index 2
    th[2] = _shuffled(rng, [40, 20, 20, 0])                      # index 1.5
    th[3] = _shuffled(rng, [0, 40, 20, 20])
    th[4] = b"ACGT" * 20
    th[5] = _shuffled(rng, [41, 39, 0, 0])                       # just below 1
    th[6] = _shuffled(rng, [21, 19, 20, 20])                     # just below 2
    for e in ("1", "2", "1.5"):
        out.append(Case(f"threshold_e{e}", [("th.fa", "fa", th, {})], e=e))
    # ... and the float index of a present read itself, with the digits a float needs
    rng = np.random.default_rng(110)
    own = util.random_reads(rng, 600, 100, 100, n_rate=0.01, lower_rate=0.1, other_rate=0.0)
    idx = sorted(shannon_index(r) for r in own)
    for q in (len(idx) // 2, len(idx) // 10):
        out.append(Case(f"threshold_own_index_{q}", [("own.fa", "fa", own, {})], e="%.9g" % float(idx[q])))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def verdict_bitmaps(case, paths):
    """numpy restatement of the per-read part of the rule over the case's files as written (paths = case.build(...); the records as
    util.parse_reads reads them: a '\\r' of a CRLF line is part of the read): set-wide keep / removed by length / removed by N bitmaps
    (64 reads per word), the set's empty reads, the files' (first, count)"""
    keep, by_len, by_n, empty, spans = [], [], [], [], []
    l, n, e = case.l or 0, case.n, np.float32(float(case.e)) if case.e is not None else np.float32(0)
    for p in paths:
        reads = util.parse_reads(p)
        spans.append((len(keep), len(reads)))
        for r in reads:
            s = r.upper()
            other = len(s) - sum(s.count(c) for c in (b"A", b"C", b"G", b"T"))
            v = [False, False, False]
            if len(s) == 0:
                empty.append(len(keep))
            elif len(s) < l:
                v[1] = True
            elif n is not None and other > n:
                v[2] = True
            elif not (e > 0 and shannon_index(r) < e):
                v[0] = True
            keep.append(v[0]), by_len.append(v[1]), by_n.append(v[2])

    def words(b):
        w = np.zeros(len(b) // 64 + 1, dtype=np.uint64)
        pk = np.packbits(np.asarray(b, dtype=bool), bitorder="little")
        w.view(np.uint8)[:pk.size] = pk
        return w
    return words(keep), words(by_len), words(by_n), np.array(empty, dtype=np.uint64), spans
