"""relative_bench.py — what the length-relative search (commet_index_and_search_relative) costs beside the calls it stands between.
  python tools/relative_bench.py [--long ragged_1k_10k] [--short-reads 1000000] [-k 32] [--scale 1.0] [--lib-profile PATH]
Long reads: on a long-read workload of tools/long_read_bench.py (default: ragged, 1-10 kb), the relative call at --percent 10 and 50
against commet_index_and_profile with max_hits = 255, which walks every read to 255 hits where the relative call stops at t_r.  The
profile runs TWICE: the distance between its two runs is the run-to-run spread that the comparison has to be read against.
--lib-profile: the profile runs load that library file (a build of the parent commit) instead of the tree's.
Short reads: 2 x N x 100 bases, the relative call at 50 % (t_r = 2 everywhere) against commet_index_and_search at t = 2, which has
masks and the tiled probe where the relative call has neither; the tags of the two must be the same bytes.
Every measurement is a fresh child process under a time limit; the first that fails ends the run.  One JSON line per comparison."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CHILD_LIMIT_S = 300


def child(a):
    import commet_amd
    if a.lib:
        from commet_amd import lib as lib_
        lib_.LIB_PATH = a.lib                            # (loaded on first use: this file instead of the tree's library)
        for name in ("commet_readset_relative_thresholds", "commet_index_and_search_relative"):
            lib_.SIGNATURES.pop(name, None)              # (a build of the parent commit has neither; the profile run needs neither)
    offs = np.load(os.path.join(a.dir, f"{a.child}_offs.npy"))
    sets = [np.load(os.path.join(a.dir, f"{a.child}_{s}_bases.npy")) for s in range(2)]
    with commet_amd.Context(k=a.k, t=2) as ctx:
        irs = commet_amd.ReadSet.from_files(ctx, [(sets[0], offs)])
        qrs = commet_amd.ReadSet.from_files(ctx, [(sets[1], offs)])

        def call():
            if a.what == "profile":
                hits, info = ctx.index_and_profile(irs, [qrs], max_hits=255)
                return hits[0], info
            if a.what == "search":
                tags, _, info = ctx.index_and_search(irs, [qrs])
                return tags[0], info
            tags, _, info = ctx.index_and_search_relative(irs, [qrs], percent=a.percent, min_hits=1)
            return tags[0], info

        call()                                           # warm-up: allocations, first launches
        runs = [call() for _ in range(a.repeats)]
        out, info = runs[-1]
    ms = [round(i["search_ms"], 3) for _, i in runs]
    print(json.dumps({"what": a.what, "percent": a.percent, "search_ms": ms, "index_ms": round(info["index_kernel_ms"], 3), "chunks": info["n_chunks"],
                      "search_launches": info["search_launches"], "reads_scanned": info["reads_scanned"],
                      "found": int((out > 0).sum()) if a.what == "profile" else int(np.unpackbits(out).sum()),
                      "sha256": hashlib.sha256(out.tobytes()).hexdigest()}))


def run_child(a, d, name, what, percent=0, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--dir", d, "-k", str(a.k), "--what", what, "--percent", str(percent),
           "--repeats", str(a.repeats)] + (["--lib", lib] if lib else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit(f"{name}: the {what} run failed (rc {p.returncode})")
    return json.loads(p.stdout.strip().split("\n")[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", default="ragged_1k_10k", help="a workload name of tools/long_read_bench.py; '' skips the comparison")
    ap.add_argument("--short-reads", type=int, default=1_000_000, help="reads per set of the short-read comparison; 0 skips it")
    ap.add_argument("-k", type=int, default=32)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib-profile", default=None, help="the library file the profile runs load (a build of the parent commit)")
    ap.add_argument("--child", default=None)             # (internal) workload of a measuring process
    ap.add_argument("--dir", default=None)
    ap.add_argument("--what", default="relative")
    ap.add_argument("--percent", type=int, default=50)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import long_read_bench as lrb
    with tempfile.TemporaryDirectory(prefix="relbench") as d:
        if a.long:
            n, total = lrb.make_pair(a.long, a.scale, d)
            prof = [run_child(a, d, a.long, "profile", lib=a.lib_profile) for _ in range(2)]
            rel = {p: run_child(a, d, a.long, "relative", p) for p in (10, 50)}
            best = [min(r["search_ms"]) for r in prof]
            spread = abs(best[0] - best[1])
            out = {"workload": a.long, "reads_per_set": n, "bases_per_set": total, "k": a.k, "profile_lib": a.lib_profile or "this tree",
                   "profile_255": prof, "profile_spread_ms": round(spread, 3), "relative": rel,
                   "relative_at_or_below_profile": {p: min(r["search_ms"]) <= max(best) + spread for p, r in rel.items()}}
            print(json.dumps(out), flush=True)
            for f in os.listdir(d):
                os.remove(os.path.join(d, f))
        if a.short_reads:
            name = f"len100x{a.short_reads}"
            lrb.WORKLOADS[name] = (a.short_reads, lambda rng, n_: np.full(n_, 100, dtype=np.int64))
            n, total = lrb.make_pair(name, 1.0, d)
            srch = run_child(a, d, name, "search")
            rel = run_child(a, d, name, "relative", 50)
            out = {"workload": name, "reads_per_set": n, "k": a.k, "search_t2": srch, "relative_50": rel, "same_tags": srch["sha256"] == rel["sha256"],
                   "relative_over_search": round(min(rel["search_ms"]) / max(1e-9, min(srch["search_ms"])), 2)}
            print(json.dumps(out), flush=True)
            if not out["same_tags"]:
                raise SystemExit(f"{name}: the tags of the relative call and of the search differ")


if __name__ == "__main__":
    main()
