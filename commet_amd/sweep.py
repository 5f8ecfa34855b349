"""Threshold sweep: the `.bv` vectors of `index_and_search -t t` for every t in 1..T from ONE profile job.

    python -m commet_amd.sweep -i index.txt -s search.txt -k K --max-t T -o OUT [--chunk-group N] [--profile-wide {0,1,2}] [--profile-slice {0,1,2}] [--profile-tiled {0,1,2}]

-i / -s take the reference's set-config grammar (`name:file[,bv];file[,bv]...`, one set per line; the index file holds exactly one
set).  The sets are parsed and packed by the library's own ingest (ReadSet.from_fasta), one Context.index_and_profile(max_hits=T) gives a hit count per read, and

    OUT/t<t>/<file>_in_<index>.bv   for t = 1..T: byte for byte what `index_and_search -t t` writes for the same configs
    OUT/sweep.csv                   t;set;file;reads;shared  (shared = reads of the file with at least t hits)

The filters, which do not depend on t, are built once instead of T times, and every search set is walked once per GROUP of up to
--chunk-group chunk filters (1..8, the library's option "chunk_group"; default: the library's, 8); the closing line reports the
passes that took.  --profile-wide (the library's option "profile_wide") 2 takes the wide bit-sliced rows at 12 <= k <= 24 instead:
all chunk filters side by side, one pass per search set unless the rows are capped; 1 never, 0 the library's choice (default).
--profile-slice (the library's option "profile_slice") 2 takes the narrow bit-sliced tables at 12 <= k <= 24 where the wide rows do not
take the call: up to 256 chunk filters per pass; 1 never, 0 the library's choice (default: never).
--profile-tiled (the library's option "profile_tiled") 2 sends passes of one or two chunk filters at 25 <= k <= 34 through the tiled
probe; 1 never, 0 the library's choice (default: sets of 2^20 reads and more whose query list fits its cap).
No .log files are written: the reference's `searched`
figure is the read count of the LAST chunk pass, which depends on t through the tags of the earlier chunks, and one pass over the
chunks does not reproduce it."""
import argparse
import os
import sys

import numpy as np

from . import matrix_io


def read_sets(path):
    """the set-config grammar as the tools read it (csrc/host/set_config.hpp; include/set_parser.h:46-102 of the reference):
    [(tag, [(file, bv or None)])] ordered by tag; the tag is not trimmed, a line without ':' is SET<n>, a repeated tag replaces the
    earlier line, only ' ' is trimmed around files and bvs"""
    with open(path, "rb") as fh:
        lines = fh.read().decode(errors="surrogateescape").split("\n")
    sets, n = {}, 0
    for line in lines:
        if not line:
            continue
        n += 1
        tag, colon, rest = line.partition(":")
        if not colon:
            tag, rest = "SET%d" % n, line
        entries = []
        for item in rest.split(";"):
            item = item.strip(" ")
            f, comma, bv = item.partition(",")
            entries.append((f.strip(" "), bv.strip(" ") if comma else None))
        sets[tag] = entries
    return sorted(sets.items(), key=lambda kv: kv[0].encode(errors="surrogateescape"))


def _load(api, ctx, entries):
    """-> (resident set, per-file read counts, set-wide selection bits or None)"""
    rs = api.ReadSet.from_fasta(ctx, [f for f, _ in entries])
    counts = rs.file_reads()
    if not any(bv for _, bv in entries):
        return rs, counts, None
    parts = []
    for (f, bv), n in zip(entries, counts):
        if bv is None:
            bits = np.zeros(n // 8 + 1, dtype=np.uint8)
            bits[:(n + 7) // 8] = np.packbits(np.ones(n, dtype=bool), bitorder="little")
            parts.append((n, bits))
            continue
        nb, bits = matrix_io.read_bv(bv)
        if nb != n:
            raise SystemExit(f"Number of reads in {f} and boolean vector size are not equal -> quit")
        parts.append((n, bits))
    return rs, counts, matrix_io.concat_bits(parts)[1]


def parser():
    p = argparse.ArgumentParser(prog="python -m commet_amd.sweep", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("-i", dest="index", required=True, help="set-config file of the index set")
    p.add_argument("-s", dest="search", required=True, help="set-config file of the search sets")
    p.add_argument("-k", dest="k", type=int, required=True, help="k-mer size")
    p.add_argument("--max-t", dest="max_t", type=int, required=True, help="largest threshold T (1..255); OUT/t1 .. OUT/tT are written")
    p.add_argument("-o", dest="out", required=True, help="output directory")
    p.add_argument("--chunk-group", dest="chunk_group", type=int, default=None, help="chunk filters per search pass (1..8; default: the library's)")
    p.add_argument("--profile-wide", dest="profile_wide", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the wide bit-sliced rows (12 <= k <= 24): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--profile-slice", dest="profile_slice", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the narrow bit-sliced tables (12 <= k <= 24, up to 256 chunk filters a pass): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--profile-tiled", dest="profile_tiled", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the tiled probe (25 <= k <= 34, passes of one or two chunk filters): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if not 1 <= a.max_t <= 255:
        ap.error("--max-t must be in 1..255")
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
    import commet_amd as api
    index_tag, index_entries = index_sets[0]
    with api.Context(k=a.k, t=1, device=a.device) as ctx:
        irs, _, isel = _load(api, ctx, index_entries)
        loaded = [(tag, entries) + _load(api, ctx, entries) for tag, entries in search_sets]
        if a.chunk_group is not None:
            ctx.set_option("chunk_group", a.chunk_group)
        if a.profile_wide is not None:
            ctx.set_option("profile_wide", a.profile_wide)
        if a.profile_slice is not None:
            ctx.set_option("profile_slice", a.profile_slice)
        if a.profile_tiled is not None:
            ctx.set_option("profile_tiled", a.profile_tiled)
        hits, info = ctx.index_and_profile(irs, [l[2] for l in loaded], isel, [l[4] for l in loaded], max_hits=a.max_t)
        rows = []
        for t in range(1, a.max_t + 1):
            d = os.path.join(a.out, "t%d" % t)
            os.makedirs(d, exist_ok=True)
            for (tag, entries, _, counts, _), h in zip(loaded, hits):
                pos = 0
                for (f, _), n in zip(entries, counts):
                    bits = api.tags_at(h[pos:pos + n], t)
                    pos += n
                    matrix_io.write_bv(os.path.join(d, f[f.rfind("/") + 1:] + "_in_" + index_tag + ".bv"), f + " in " + index_tag, n, bits)
                    rows.append((t, tag, f, n, matrix_io.popcount(bits, n)))
        with open(os.path.join(a.out, "sweep.csv"), "w") as fh:
            fh.write("t;set;file;reads;shared\n")
            for r in rows:
                fh.write(";".join(str(x) for x in r) + "\n")
    print(f"sweep: k={a.k} t=1..{a.max_t}, {int(info['n_chunks'])} chunk filter(s) built once, {int(info['search_launches'])} search pass(es), "
          f"{len(rows)} vectors under {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
