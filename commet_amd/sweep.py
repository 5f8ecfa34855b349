"""Threshold sweep: the `.bv` vectors of `index_and_search -t t` for every t in 1..T from ONE profile job.

    python -m commet_amd.sweep -i index.txt -s search.txt -k K --max-t T -o OUT [--full] [--chunk-group N] [--multi-job {0,1,2}] [--profile-wide {0,1,2}] [--profile-slice {0,1,2}] [--profile-tiled {0,1,2}]

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
chunks does not reproduce it.

--full sweeps the SYMMETRIC comparison instead: the `.bv` files of `index_and_search -f -t t` for every t in 1..T.  As the tool does,
only the first search set is used (stderr says so when more are given).  With A = the index set and B = that search set:

    pass 1   one index_and_profile(A -> B), max_hits = T:                  T1(t) = hits >= t
    pass 2   one index_many_and_profile of T jobs: job t indexes B under T1(t), all search A under A's own selection,
             max_hits[t] = t: T2(t) = hits_t >= t                         -> OUT/t<t>/<A file>_in_<B tag>.bv
    pass 3   per t, index_and_profile(A under T2(t) -> B under T1(t), max_hits = t)   -> OUT/t<t>/<B file>_in_<A tag>.bv

The T jobs of pass 2 share hits passes over A (up to eight chunk filters a pass); only pass 3 stays one job per threshold, because its
search selection differs per t.  sweep.csv holds the rows of both directions.
--multi-job (the library's option "multi_job") decides how pass 2 shares: 0 the library's choice (default: shared passes, except
over a set A of long reads, which takes a wave per read and is walked once per job), 1 never, 2 always — a set of long reads
included (hits_jobs_wave_kernel: A is walked once per pass, not once per t)."""
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
    p.add_argument("--full", dest="full", action="store_true",
                   help="the symmetric comparison of `index_and_search -f` on the first search set: both directions for every t")
    p.add_argument("--chunk-group", dest="chunk_group", type=int, default=None, help="chunk filters per search pass (1..8; default: the library's)")
    p.add_argument("--multi-job", dest="multi_job", type=int, default=None, choices=(0, 1, 2),
                   help="--full: the jobs of pass 2 in shared hits passes: 0 the library's choice, 1 never, 2 always (sets of long reads too)")
    p.add_argument("--profile-wide", dest="profile_wide", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the wide bit-sliced rows (12 <= k <= 24): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--profile-slice", dest="profile_slice", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the narrow bit-sliced tables (12 <= k <= 24, up to 256 chunk filters a pass): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--profile-tiled", dest="profile_tiled", type=int, default=None, choices=(0, 1, 2),
                   help="the profile through the tiled probe (25 <= k <= 34, passes of one or two chunk filters): 0 the library's choice, 1 never, 2 always")
    p.add_argument("--device", type=int, default=0)
    return p


def _write_files(api, out, t, loaded_set, h, suffix, rows, per_t=True):
    """the vectors of one set at threshold t, file by file, as save_bv of the tool writes them: <file>_in_<suffix>.bv, under out/t<t>
    (per_t false, commet_amd.relative: under out itself)"""
    tag, entries, _, counts, _ = loaded_set
    d = os.path.join(out, "t%d" % t) if per_t else out
    os.makedirs(d, exist_ok=True)
    pos = 0
    for (f, _), n in zip(entries, counts):
        bits = api.tags_at(h[pos:pos + n], t)
        pos += n
        matrix_io.write_bv(os.path.join(d, f[f.rfind("/") + 1:] + "_in_" + suffix + ".bv"), f + " in " + suffix, n, bits)
        rows.append((t, tag, f, n, matrix_io.popcount(bits, n)))


def sweep_full(api, ctx, A, B, max_t, out):
    """the three passes of `index_and_search -f` for every t in 1..max_t; A, B = (tag, entries, read set, per-file reads, selection bits
    or None).  -> (rows of sweep.csv, [info of pass 1, of pass 2, of every pass 3])"""
    rows, infos = [], []
    h1, info = ctx.index_and_profile(A[2], [B[2]], A[4], [B[4]], max_hits=max_t)
    infos.append(info)
    ts = list(range(1, max_t + 1))
    t1 = [api.tags_at(h1[0], t) for t in ts]
    h2, info = ctx.index_many_and_profile([B[2]] * max_t, A[2], index_selects=t1, search_select=A[4], max_hits=ts)
    infos.append(info)
    for t, sel1, h in zip(ts, t1, h2):
        _write_files(api, out, t, A, h, B[0], rows)
        h3, info = ctx.index_and_profile(A[2], [B[2]], api.tags_at(h, t), [sel1], max_hits=t)
        infos.append(info)
        _write_files(api, out, t, B, h3[0], A[0], rows)
    return rows, infos


def main(argv=None, api=None):
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
    if api is None:
        import commet_amd as api
    index_tag, index_entries = index_sets[0]
    if a.full:
        if not search_sets:
            ap.error("no set to search")
        if len(search_sets) > 1:
            print(f"sweep: --full compares the index set with the first search set only ({search_sets[0][0]}); "
                  f"{len(search_sets) - 1} more set(s) ignored", file=sys.stderr)
        search_sets = search_sets[:1]
    with api.Context(k=a.k, t=1, device=a.device) as ctx:
        irs, _, isel = _load(api, ctx, index_entries)
        loaded = [(tag, entries) + _load(api, ctx, entries) for tag, entries in search_sets]
        if a.chunk_group is not None:
            ctx.set_option("chunk_group", a.chunk_group)
        if a.multi_job is not None:
            ctx.set_option("multi_job", a.multi_job)
        if a.profile_wide is not None:
            ctx.set_option("profile_wide", a.profile_wide)
        if a.profile_slice is not None:
            ctx.set_option("profile_slice", a.profile_slice)
        if a.profile_tiled is not None:
            ctx.set_option("profile_tiled", a.profile_tiled)
        rows = []
        if a.full:
            irs_counts = irs.file_reads()
            rows, infos = sweep_full(api, ctx, (index_tag, index_entries, irs, irs_counts, isel), loaded[0], a.max_t, a.out)
            info = {"n_chunks": sum(int(i["n_chunks"]) for i in infos), "search_launches": sum(int(i["search_launches"]) for i in infos)}
        else:
            hits, info = ctx.index_and_profile(irs, [l[2] for l in loaded], isel, [l[4] for l in loaded], max_hits=a.max_t)
            for t in range(1, a.max_t + 1):
                for l, h in zip(loaded, hits):
                    _write_files(api, a.out, t, l, h, index_tag, rows)
        with open(os.path.join(a.out, "sweep.csv"), "w") as fh:
            fh.write("t;set;file;reads;shared\n")
            for r in rows:
                fh.write(";".join(str(x) for x in r) + "\n")
    if a.full:
        print(f"sweep: k={a.k} t=1..{a.max_t}, both directions: {info['n_chunks']} chunk filter(s) built, {info['search_launches']} search pass(es) "
              f"({int(infos[1]['search_launches'])} for the {a.max_t} jobs of pass 2), {len(rows)} vectors under {a.out}")
        return 0
    print(f"sweep: k={a.k} t=1..{a.max_t}, {int(info['n_chunks'])} chunk filter(s) built once, {int(info['search_launches'])} search pass(es), "
          f"{len(rows)} vectors under {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
