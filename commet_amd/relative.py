"""Search with a threshold per read, relative to its length: a read is shared when one chunk filter holds at least --percent of the
non-overlapping k-mers the read can hold.

    python -m commet_amd.relative -i index.txt -s search.txt -k K --percent P [-t MIN] -o OUT [--chunk-group G] [--device D]

-i / -s take the reference's set-config grammar as commet_amd.sweep does (one set per line; the index file holds exactly one set).
The rule, for a read of `len` bases (every character counts, ACGT or not):

    W_r = len // k                                    the most non-overlapping k-mers the read can hold
    t_r = max(MIN, (P * W_r + 99) // 100)             P in 1..100; MIN (-t, default 1) below 1 behaves as 1

A read is shared iff one chunk filter of the index set holds t_r non-overlapping k-mers of it on one strand (the greedy count of
`index_and_search`); a read with t_r > W_r never is.  One Context.index_and_search_relative call does the work; it writes

    OUT/<file>_in_<index>.bv   the BooleanVector of every search file, named and written as commet_amd.sweep writes its vectors;
                               on a set whose reads all get the same t_r it is byte for byte what `index_and_search -t t_r` writes
    OUT/relative.csv           set;file;reads;shared;min_t;max_t  (min_t / max_t: the smallest and largest t_r among the file's reads
                               that can be shared at all, 0 when there is none)

`thresholds(lengths, k, percent, min_hits)` is the rule in numpy."""
import argparse
import os
import sys

import numpy as np

from .sweep import _load, _write_files, read_sets


def thresholds(lengths, k, percent, min_hits=1):
    """-> t_r per read as np.int64: W_r = len // k, t_r = max(min_hits, (percent * W_r + 99) // 100), and 0 where t_r > W_r (such a read
    can never be found): what ReadSet.relative_thresholds gives, made on the host"""
    w = np.asarray(lengths, dtype=np.int64) // int(k)
    t = np.maximum(max(int(min_hits), 1), (int(percent) * w + 99) // 100)
    return np.where(t > w, 0, t)


def parser():
    p = argparse.ArgumentParser(prog="python -m commet_amd.relative", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-i", dest="index", required=True, help="set-config file of the index set")
    p.add_argument("-s", dest="search", required=True, help="set-config file of the search sets")
    p.add_argument("-k", dest="k", type=int, required=True, help="k-mer size")
    p.add_argument("--percent", dest="percent", type=int, required=True, help="share of the read's non-overlapping k-mers, in percent (1..100)")
    p.add_argument("-t", dest="min_hits", type=int, default=1, help="least threshold of any read (default 1)")
    p.add_argument("-o", dest="out", required=True, help="output directory")
    p.add_argument("--chunk-group", dest="chunk_group", type=int, default=None, help="chunk filters per search pass (1..8; default: the library's)")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None, api=None):
    ap = parser()
    a = ap.parse_args(argv)
    if not 1 <= a.percent <= 100:
        ap.error("--percent must be in 1..100")
    if a.k < 1:
        ap.error("-k must be positive")
    if a.chunk_group is not None and not 1 <= a.chunk_group <= 8:
        ap.error("--chunk-group must be in 1..8")
    for path in (a.index, a.search):
        if not os.path.isfile(path):
            ap.error(f"Cannot read file {path}")
    index_sets, search_sets = read_sets(a.index), read_sets(a.search)
    if len(index_sets) != 1:
        ap.error("Only one set of files is allowed for indexing")
    if api is None:
        import commet_amd as api
    index_tag, index_entries = index_sets[0]
    with api.Context(k=a.k, t=1, device=a.device) as ctx:
        irs, _, isel = _load(api, ctx, index_entries)
        loaded = [(tag, entries) + _load(api, ctx, entries) for tag, entries in search_sets]
        if a.chunk_group is not None:
            ctx.set_option("chunk_group", a.chunk_group)
        tags, _, info = ctx.index_and_search_relative(irs, [l[2] for l in loaded], isel, [l[4] for l in loaded], percent=a.percent,
                                                      min_hits=a.min_hits)
        os.makedirs(a.out, exist_ok=True)
        lines = []
        for l, bits in zip(loaded, tags):
            n = sum(l[3])
            found = np.unpackbits(bits, bitorder="little")[:n]      # a byte per read: _write_files thresholds bytes
            rows = []
            _write_files(api, a.out, 1, l, found, index_tag, rows, per_t=False)
            thr = l[2].relative_thresholds(a.percent, a.min_hits)
            pos = 0
            for _, tag, f, reads, shared in rows:
                mine = thr[pos:pos + reads]
                pos += reads
                mine = mine[mine > 0]
                lines.append((tag, f, reads, shared, int(mine.min()) if mine.size else 0, int(mine.max()) if mine.size else 0))
        with open(os.path.join(a.out, "relative.csv"), "w") as fh:
            fh.write("set;file;reads;shared;min_t;max_t\n")
            for r in lines:
                fh.write(";".join(str(x) for x in r) + "\n")
    print(f"relative: k={a.k} percent={a.percent} min_hits={max(a.min_hits, 1)}, {int(info['n_chunks'])} chunk filter(s), "
          f"{int(info['search_launches'])} search pass(es), {len(lines)} vectors under {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
