"""long_read_bench.py — one index_and_search job on sets of LONG reads, lane-per-read kernels (long_search = 1) against the wave-per-read
kernel (long_search = 2, search_long_kernel): 2 x N synthetic reads, a tenth of the second set copied from the first (1 % of the
copied bases substituted).  Workloads: reads of 450 bases (merged 2 x 250 pairs), ragged 1-10 kb, and a mixed set (99 % 100-300
bases, 1 % 5 kb).  Every run is a fresh process; A and B alternate; the tags of the two must be the same bytes.
  python tools/long_read_bench.py [--workloads len450 ragged_1k_10k mixed | len<N> | mixed<N> | ragged<A>_<B> | huge<N>x<L>] [--pairs 3] [-k 32] [-t 2] [--scale 1.0]
Prints one JSON line per workload: search ms (min-max over the pairs), bases/s, per-kernel times, the index's share of the job.
  python tools/long_read_bench.py --index-mode [--part-min-kmers N] ...
The same protocol on the INDEX side: A = index_mode 1 (index_kernel, a lane per read, atomic ORs), B = index_mode 2 (the bucketed
build through the item list, part_items_fill_kernel); index ms from the job's own events, the tags byte-compared, and B's launches
checked: more than one scatter1 piece, no index_kernel.  `huge<N>x<L>`: N reads of L bases per set.
  python tools/long_read_bench.py --jobs 8 [--lib-a PATH] ...
Several jobs on one long search set through commet_index_many_and_search: N index sets (set 0 of the workload cut into N parts,
alternately of two chunks and of one under the max_kmer the tool sets) against set 1.  A = the jobs alone (multi_job = 1), B = shared
passes of search_long_kernel (multi_job = 2), fresh processes, every job's tags byte-compared.  --lib-a: A loads that library file
instead (a build of another commit: its commet_index_many_and_search as it stands, no multi_job option set)."""
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

WORKLOADS = {   # name: (reads per set, lengths(rng, n))
    "len450": (1_000_000, lambda rng, n: np.full(n, 450, dtype=np.int64)),
    "ragged_1k_10k": (60_000, lambda rng, n: rng.integers(1000, 10001, size=n, dtype=np.int64)),
    "mixed": (1_000_000, lambda rng, n: np.where(rng.random(n) < 0.01, 5000, rng.integers(100, 301, size=n)).astype(np.int64)),
}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def workload(name):
    """the three named ones, and for threshold sweeps `len<N>` (every read N bases), `mixed<N>` (99 % 100-300 bases, 1 % N) and
    `ragged<A>_<B>` (uniform in A..B)"""
    if name in WORKLOADS:
        return WORKLOADS[name]
    if name.startswith("len"):
        L = int(name[3:])
        return max(20_000, 450_000_000 // L), lambda rng, n: np.full(n, L, dtype=np.int64)
    if name.startswith("mixed"):
        L = int(name[5:])
        return 1_000_000, lambda rng, n: np.where(rng.random(n) < 0.01, L, rng.integers(100, 301, size=n)).astype(np.int64)
    if name.startswith("huge"):
        n, L = (int(x) for x in name[4:].split("x"))
        return n, lambda rng, n_: np.full(n_, L, dtype=np.int64)
    if name.startswith("ragged"):
        lo, hi = (int(x) for x in name[6:].split("_"))
        return max(20_000, 660_000_000 // (lo + hi)), lambda rng, n: rng.integers(lo, hi + 1, size=n, dtype=np.int64)
    raise SystemExit(f"unknown workload {name}")


def make_pair(name, scale, d):
    """writes the two sets of a workload as .npy files (bases, offsets); both sets have the same read lengths"""
    n, lens_of = workload(name)
    n = max(1, int(n * scale)) if name.startswith("huge") else max(64, int(n * scale))
    lens = lens_of(np.random.default_rng(11), n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:].view(np.int64))
    total = int(offs[-1])
    sets = []
    for s in range(2):
        rng = np.random.default_rng(100 + s)
        codes = rng.integers(0, 4, size=total, dtype=np.uint8)
        if s == 1:                                   # the first tenth of the reads: copies of set 0's, one base in a hundred substituted
            cut = int(offs[n // 10])
            keep = rng.random(cut) < 0.01
            codes[:cut] = np.where(keep, codes[:cut], sets[0][:cut])
        sets.append(codes)
    for s in range(2):
        np.save(os.path.join(d, f"{name}_{s}_bases.npy"), ACGT[sets[s]])
    np.save(os.path.join(d, f"{name}_offs.npy"), offs)
    return n, total


def child(a):
    import commet_amd
    offs = np.load(os.path.join(a.dir, f"{a.child}_offs.npy"))
    sets = [np.load(os.path.join(a.dir, f"{a.child}_{s}_bases.npy")) for s in range(2)]
    with commet_amd.Context(k=a.k, t=a.t) as ctx:
        ctx.set_option("long_search", a.long_search)
        if a.index_mode:
            ctx.set_option("index_mode", a.child_index_mode)
            ctx.set_option("part_min_kmers", a.part_min_kmers)
        irs = commet_amd.ReadSet.from_files(ctx, [(sets[0], offs)])
        qrs = commet_amd.ReadSet.from_files(ctx, [(sets[1], offs)])
        ctx.index_and_search(irs, [qrs])             # warm-up: allocations, first launches
        ctx.set_option("kernel_timing", 1)
        tags, stats, info = ctx.index_and_search(irs, [qrs])
        kt = {k_: [c, round(ms, 3)] for k_, (c, ms) in ctx.kernel_times().items()}
        ctx.set_option("kernel_timing", 0)
        tags2, stats2, info2 = ctx.index_and_search(irs, [qrs])   # untimed kernels: the job's own event times
        irs_n = irs.num_reads
        if a.index_mode:     # a selection (every read but the last): the bucketed build's workspace cannot hold the item list from the job before
            bits = np.full(irs_n // 8 + 1, 0xFF, dtype=np.uint8)
            bits[(irs_n - 1) // 8] &= np.uint8(~(1 << ((irs_n - 1) % 8)) & 0xFF)
            ctx.index_and_search(irs, [qrs], bits)
            sel_info = ctx.index_and_search(irs, [qrs], bits)[2]
    sel_ms = round(sel_info["index_kernel_ms"], 3) if a.index_mode else None
    if a.index_mode and a.child_index_mode == 2:     # B must be the bucketed build, its scatter1 cut into more than one piece
        assert "index_kernel" not in kt and kt["part_scatter1_pieces"][0] > kt["part_scatter1_kernel"][0], kt
    print(json.dumps({"long_search": a.long_search, "index_mode": a.child_index_mode, "search_ms": round(info2["search_ms"], 3), "index_ms": round(info2["index_kernel_ms"], 3), "index_sel_ms": sel_ms,
                      "total_ms": round(info2["total_ms"], 3), "chunks": info["n_chunks"], "shared": stats[0]["shared"],
                      "kernels": kt, "tags_sha256": hashlib.sha256(tags[0].tobytes() + tags2[0].tobytes()).hexdigest()}))


def child_jobs(a):
    """N index sets against one search set in one commet_index_many_and_search call; prints search ms of the call and per job"""
    import commet_amd
    if a.lib:
        from commet_amd import lib as lib_
        lib_.LIB_PATH = a.lib                        # (loaded on first use: this file instead of the tree's library)
    offs = np.load(os.path.join(a.dir, f"{a.child}_offs.npy"))
    sets = [np.load(os.path.join(a.dir, f"{a.child}_{s}_bases.npy")) for s in range(2)]
    n = len(offs) - 1
    # parts of two shares and of one, alternating; with max_kmer at 1.5 shares the large ones are two chunks, the small ones one
    weights = [2 - (j & 1) for j in range(a.jobs)]
    cuts = [n * sum(weights[:j]) // sum(weights) for j in range(a.jobs + 1)]
    kmers = np.maximum(np.diff(offs.astype(np.int64)) - a.k + 1, 0)
    share = int(kmers.sum()) // sum(weights)
    with commet_amd.Context(k=a.k, t=a.t) as ctx:
        ctx.set_option("long_search", a.long_search)
        if a.multi_job >= 0:
            ctx.set_option("multi_job", a.multi_job)
        qrs = commet_amd.ReadSet.from_files(ctx, [(sets[1], offs)])
        irs = []
        for j in range(a.jobs):
            lo, hi = cuts[j], cuts[j + 1]
            b0, b1 = int(offs[lo]), int(offs[hi])
            irs.append(commet_amd.ReadSet.from_files(ctx, [(sets[0][b0:b1].copy(), (offs[lo:hi + 1] - offs[lo]).astype(np.uint64))]))
        ctx.set_option("max_kmer", share * 3 // 2)
        ctx.index_many_and_search(irs, qrs)          # warm-up: allocations, first launches
        ctx.set_option("kernel_timing", 1)
        tags, stats, info = ctx.index_many_and_search(irs, qrs)
        kt = {k_: [c, round(ms, 3)] for k_, (c, ms) in ctx.kernel_times().items()}
        ctx.set_option("kernel_timing", 0)
        tags2, stats2, info2 = ctx.index_many_and_search(irs, qrs)   # untimed kernels: the call's own event times
    print(json.dumps({"multi_job": a.multi_job, "lib": a.lib, "search_ms": round(info2["search_ms"], 3), "index_ms": round(info2["index_kernel_ms"], 3),
                      "total_ms": round(info2["total_ms"], 3), "chunks": info["n_chunks"], "search_launches": info2["search_launches"],
                      "job_search_ms": [round(s_["search_ms"], 3) for s_ in stats2], "shared": [s_["shared"] for s_ in stats],
                      "kernels": kt, "tags_sha256": hashlib.sha256(b"".join(t_.tobytes() for t_ in tags + tags2)).hexdigest()}))


def main_jobs(a, d):
    for name in a.workloads:
        n, total = make_pair(name, a.scale, d)
        runs = {"A": [], "B": []}
        for _ in range(a.pairs):
            for side in ("A", "B"):
                what = ["--jobs", str(a.jobs), "--long-search", str(a.long_search)]
                if side == "A":
                    what += ["--lib", a.lib_a, "--multi-job", "-1"] if a.lib_a else ["--multi-job", "1"]
                else:
                    what += ["--multi-job", "2"]
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--dir", d, "-k", str(a.k), "-t", str(a.t)] + what,
                                   capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-2000:])
                    raise SystemExit(f"{name}: run {side} failed (rc {p.returncode})")
                runs[side].append(json.loads(p.stdout.strip().split("\n")[-1]))
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        digests = {r["tags_sha256"] for side in runs for r in runs[side]}
        out = {"workload": name, "jobs": a.jobs, "reads_in_search_set": n, "bases_in_search_set": total, "k": a.k, "t": a.t, "same_tags": len(digests) == 1,
               "chunks": runs["B"][0]["chunks"], "baseline": a.lib_a or "multi_job = 1"}
        for side, key in (("A", "jobs_alone"), ("B", "shared_passes")):
            out[key] = {"search_ms": [r["search_ms"] for r in runs[side]], "search_launches": runs[side][-1]["search_launches"],
                        "job_search_ms": runs[side][-1]["job_search_ms"], "kernels": runs[side][-1]["kernels"]}
        out["shared_faster_in_every_pair"] = all(b["search_ms"] < a_["search_ms"] for a_, b in zip(runs["A"], runs["B"]))
        print(json.dumps(out), flush=True)
        if not out["same_tags"]:
            raise SystemExit(f"{name}: the tags of the shared passes and of the jobs alone differ")
        if runs["B"][0]["search_launches"] >= a.jobs:
            raise SystemExit(f"{name}: the jobs did not share a pass")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("-k", type=int, default=32)
    ap.add_argument("-t", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--child", default=None)         # (internal) workload of a measuring process
    ap.add_argument("--dir", default=None)
    ap.add_argument("--long-search", type=int, default=2)
    ap.add_argument("--index-mode", action="store_true", help="A/B of the index side: index_mode 1 against 2")
    ap.add_argument("--child-index-mode", type=int, default=0)   # (internal)
    ap.add_argument("--part-min-kmers", type=int, default=1)
    ap.add_argument("--jobs", type=int, default=0, help="N index sets against one long search set through commet_index_many_and_search: alone against shared passes")
    ap.add_argument("--lib-a", default=None, help="--jobs: the library file run A loads (a build of another commit)")
    ap.add_argument("--lib", default=None)           # (internal)
    ap.add_argument("--multi-job", type=int, default=-1)         # (internal) -1 = leave the option alone
    a = ap.parse_args()
    if a.child:
        return child_jobs(a) if a.jobs else child(a)
    with tempfile.TemporaryDirectory(prefix="longbench") as d:
        if a.jobs:
            return main_jobs(a, d)
        for name in a.workloads:
            n, total = make_pair(name, a.scale, d)
            runs = {1: [], 2: []}
            for _ in range(a.pairs):
                for mode in (1, 2):                  # A, B, A, B, ...
                    what = ["--index-mode", "--child-index-mode", str(mode), "--part-min-kmers", str(a.part_min_kmers), "--long-search", str(a.long_search)] \
                        if a.index_mode else ["--long-search", str(mode)]
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--dir", d, "-k", str(a.k), "-t", str(a.t)] + what,
                                       capture_output=True, text=True, timeout=600)
                    if p.returncode != 0:
                        sys.stderr.write(p.stderr[-2000:])
                        raise SystemExit(f"{name}: the run with {'index_mode' if a.index_mode else 'long_search'} = {mode} failed (rc {p.returncode})")
                    runs[mode].append(json.loads(p.stdout.strip().split("\n")[-1]))
            for f in os.listdir(d):
                os.remove(os.path.join(d, f))
            digests = {r["tags_sha256"] for m in runs for r in runs[m]}
            out = {"workload": name, "reads_per_set": n, "bases_per_set": total, "mean_len": round(total / n, 1), "k": a.k, "t": a.t,
                   "same_tags": len(digests) == 1, "shared": runs[1][0]["shared"], "chunks": runs[1][0]["chunks"]}
            if a.index_mode:
                for mode, key in ((1, "index_kernel"), (2, "bucketed")):
                    out[key] = {"index_ms": [r["index_ms"] for r in runs[mode]], "index_sel_ms": [r["index_sel_ms"] for r in runs[mode]], "search_ms": [r["search_ms"] for r in runs[mode]],
                                "kernels": runs[mode][-1]["kernels"]}
                out["bucketed_faster_in_every_pair"] = all(b["index_ms"] < a_["index_ms"] and b["index_sel_ms"] < a_["index_sel_ms"] for a_, b in zip(runs[1], runs[2]))
                print(json.dumps(out), flush=True)
                if not out["same_tags"]:
                    raise SystemExit(f"{name}: the tags of the two index constructions differ")
                continue
            for mode, key in ((1, "lane_per_read"), (2, "wave_per_read")):
                ms = [r["search_ms"] for r in runs[mode]]
                out[key] = {"search_ms": ms, "search_ms_min_max": [min(ms), max(ms)], "bases_per_s": round(total / (min(ms) * 1e-3)) if min(ms) > 0 else None,
                            "index_ms": [r["index_ms"] for r in runs[mode]],
                            "index_share": round(min(r["index_ms"] for r in runs[mode]) / max(1e-9, min(r["index_ms"] + r["search_ms"] for r in runs[mode])), 3),
                            "kernels": runs[mode][-1]["kernels"]}
            out["wave_faster_in_every_pair"] = all(b["search_ms"] < a_["search_ms"] for a_, b in zip(runs[1], runs[2]))
            print(json.dumps(out), flush=True)
            if not out["same_tags"]:
                raise SystemExit(f"{name}: the tags of the two kernels differ")


if __name__ == "__main__":
    main()
