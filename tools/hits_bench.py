"""hits_bench.py — does one profile job beat a job per threshold?  On the configs[1] shape (2 x 10 M x 100 bp, k = 32, sets generated as
bench.py does):
  (a) one Context.index_and_profile(max_hits = T)                       -> the tags of t = 1..T
  (b) the T Context.index_and_search jobs at t = 1..T, one context each -> the same tags, the way there was before
The T tag vectors of (a) and (b) are byte-compared.  Every figure comes from a fresh child process under its own time limit, (a) and
(b) alternating over `--rounds`; a child warms up once, times `--reps` calls with a host clock around the whole call (it ends in a
stream synchronise and the copy back) and then runs once more with option kernel_timing for the per-kernel split.
  --jobs-lib PATH   the library (b) runs on (a build of the commit before the profile existed); default: the one in the tree
  --many-chunks     also one profile job of a few hundred chunks (configs[4]'s k = 21, 150 bp, scaled down)
  --groups          ONLY the chunk_group leg: per shape (configs[1]'s; with --many-chunks the many-chunk one as well) the profile at
                    chunk_group = 1, at the default and, with --jobs-lib, on that library (the parent commit's build), in fresh child
                    processes alternating over `--rounds`; the hit bytes of the three are compared, medians and spreads reported,
                    and one job at t = 5 of the many-chunk shape gives the break-even T
  --wide            ONLY the profile_wide leg (needs --many-chunks): on the many-chunk shape (2 x 600 000 x 150 bp, k = 21, 313 chunks) and,
                    when --many-reads is given more than once, on every further read count (2 000 000 reads cross 1 024 chunks), the
                    profile on --jobs-lib (the parent commit's build), at profile_wide = 1 and at profile_wide = 2, fresh child processes
                    alternating over `--rounds`, the three hit arrays byte-compared; one job at t = 5 gives the break-even T
  --sliced          ONLY the profile_slice leg (needs --many-chunks): on every read count of --many-reads (k = 21, 150 bp; 200 000 and 450 000
                    reads cross about 107 and about 240 chunk filters, one pass of the narrow tables) the profile at profile_slice = 1 (the
                    slot loop) and at profile_slice = 2 (hits_sliced_kernel), fresh child processes alternating over `--rounds`, the hit
                    arrays byte-compared, the per-kernel times of both legs reported
  --tiled           ONLY the profile_tiled leg, on the configs[1] shape (--reads, --read-len, -k): the profile on --jobs-lib (the parent
                    commit's build), at profile_tiled = 1 (the slot loop), at profile_tiled = 2 (tq_probe_kernel + tq_hits_replay_kernel) and at the
                    default (auto),
                    fresh child processes alternating over `--rounds`, the hit arrays byte-compared; the timed calls find the (k, 1) query
                    list cached, `first_call` is the warm-up call that builds it (tq_count / tq_fill and the allocation)
  --parent-tiled    with --tiled and --jobs-lib: one more leg, `parent_tiled2`, --jobs-lib at profile_tiled = 2 (a parent that has the
                    option: the like-for-like partner of `tiled2` when the tiled kernels themselves changed)
  --jobs N          ONLY the many-job leg (measured at --reads 5000000: 2 x 5 M x 100 bp, k = 32, the shape the tiled profile was measured
                    on): N jobs, each indexing a disjoint N-th of set 0 by selection, all searching set 1 with max_hits = --max-t;
                    (a) `alone`: the jobs one by one through commet_index_and_profile at its own auto choices, (b) `shared`: ONE
                    commet_index_many_and_profile call; fresh child processes alternating over `--rounds`, the N byte arrays compared
                    first, then per leg the median over the rounds of the per-process median wall time of the N jobs, and its spread
  --long            with --jobs N: the many-job leg on search sets of LONG reads, which take a wave per read — the two sets of
                    tools/long_read_bench.py's workloads `ragged_1k_10k` and `len5500` (--long-workloads, --scale), one result line
                    each; both legs are ONE commet_index_many_and_profile call, (a) `alone` under multi_job = 1 (the jobs one by one
                    through hits_wave_kernel), (b) `shared` under multi_job = 2 (hits_jobs_wave_kernel); the protocol is --jobs' own
  --thresholds      with --jobs N: the step behind the search.  Job j has the threshold 1 + j % --max-t; (a) `bytes`, the way there was before:
                    ONE commet_index_many_and_profile call, then api.tags_at and matrix_io.popcount per job on the host; (b) `tags`: ONE
                    commet_index_many_and_thresholds call (hits_tags_kernel: only bits come down).  Tags and counts of the two are
                    compared; per leg the wall time of the whole step, the event-timed device time of the searches and the rest (host)
  python tools/hits_bench.py [--reads 10000000] [--read-len 100] [-k 32] [--max-t 8] [--rounds 2] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sets(work, tag):
    return [(np.load(os.path.join(work, f"{tag}{i}_b.npy")), np.load(os.path.join(work, f"{tag}{i}_o.npy"))) for i in (0, 1)]


def _kernels(ctx):
    return {name: [cnt, round(ms, 3)] for name, (cnt, ms) in sorted(ctx.kernel_times().items(), key=lambda kv: -kv[1][1])}


def child_profile(a):
    if a.jobs_lib:                                                               # (the groups leg: the profile on another build)
        from commet_amd import lib
        lib.LIB_PATH = a.jobs_lib
    import commet_amd
    (b0, o0), (b1, o1) = _sets(a.work, a.tag)
    out = {}
    with commet_amd.Context(k=a.k, t=2) as ctx:
        if a.max_kmer:
            ctx.set_option("max_kmer", a.max_kmer)
        if a.chunk_group:
            ctx.set_option("chunk_group", a.chunk_group)
        if a.profile_wide:
            ctx.set_option("profile_wide", a.profile_wide)
        if a.profile_tiled:
            ctx.set_option("profile_tiled", a.profile_tiled)
        if a.profile_slice:
            ctx.set_option("profile_slice", a.profile_slice)
        irs = commet_amd.ReadSet.from_files(ctx, [(b0, o0)])
        qrs = commet_amd.ReadSet.from_files(ctx, [(b1, o1)])
        _, first = ctx.index_and_profile(irs, [qrs], max_hits=a.max_t)           # warm-up (workspaces; the tiled leg's query list)
        out["first_call"] = {f: round(first[f], 3) for f in ("total_ms", "index_ms", "search_ms")}
        out["cache_bytes"] = int(qrs.cache_bytes)
        calls = []
        for _ in range(a.reps):
            hits, info = ctx.index_and_profile(irs, [qrs], max_hits=a.max_t)
            calls.append(info)
        ctx.set_option("kernel_timing", 1)
        ctx.index_and_profile(irs, [qrs], max_hits=a.max_t)
        out["kernels_ms"] = _kernels(ctx)
        ctx.set_option("kernel_timing", 0)
        out["total_ms"] = [round(i["total_ms"], 3) for i in calls]
        out["index_ms"] = [round(i["index_ms"], 3) for i in calls]
        out["search_ms"] = [round(i["search_ms"], 3) for i in calls]
        out["chunks"], out["reads_walked"] = int(calls[-1]["n_chunks"]), int(calls[-1]["reads_scanned"])
        out["search_launches"] = int(calls[-1]["search_launches"])
        out["windows"] = int(qrs.kmer_counts().astype(np.uint64).sum())          # complete windows of the search set: one plane-A request each at most
        out["histogram"] = np.bincount(hits[0], minlength=a.max_t + 1).tolist()
        if a.ceiling:
            acc = 1 << 30
            out["gather_ceiling_per_s"] = acc / (ctx.membench(0, (4 << a.k) // 8, acc) * 1e-3)
        if a.hits_name:
            np.save(os.path.join(a.work, a.hits_name), hits[0])
        np.save(os.path.join(a.work, f"{a.tag}_profile_tags.npy"), np.stack([commet_amd.tags_at(hits[0], t) for t in range(1, a.max_t + 1)]))
    print("RESULT " + json.dumps(out), flush=True)


def child_jobs(a):
    from commet_amd import lib
    if a.jobs_lib:
        lib.LIB_PATH = a.jobs_lib
        import ctypes
        if not hasattr(ctypes.CDLL(a.jobs_lib), "commet_index_and_profile"):
            lib.SIGNATURES.pop("commet_index_and_profile")                      # (a library from before the profile)
    import commet_amd
    (b0, o0), (b1, o1) = _sets(a.work, a.tag)
    out = {"lib": lib.LIB_PATH, "per_t": {}}
    tags_all = []
    for t in a.ts:
        with commet_amd.Context(k=a.k, t=t) as ctx:
            if a.max_kmer:
                ctx.set_option("max_kmer", a.max_kmer)
            irs = commet_amd.ReadSet.from_files(ctx, [(b0, o0)])
            qrs = commet_amd.ReadSet.from_files(ctx, [(b1, o1)])
            ctx.index_and_search(irs, [qrs])                                     # warm-up (query lists, workspaces)
            calls = []
            for _ in range(a.reps):
                tags, stats, info = ctx.index_and_search(irs, [qrs])
                calls.append(info)
            ctx.set_option("kernel_timing", 1)
            ctx.index_and_search(irs, [qrs])
            out["per_t"][str(t)] = {"total_ms": [round(i["total_ms"], 3) for i in calls], "index_ms": [round(i["index_ms"], 3) for i in calls],
                                    "search_ms": [round(i["search_ms"], 3) for i in calls], "shared": stats[0]["shared"], "kernels_ms": _kernels(ctx)}
            tags_all.append(tags[0].copy())
    np.save(os.path.join(a.work, f"{a.tag}_job_tags.npy"), np.stack(tags_all))
    print("RESULT " + json.dumps(out), flush=True)


def child_many(a):
    """the --jobs leg: a.n_jobs jobs on disjoint parts of set 0, all searching set 1; a.share: one many-job call, else one call per job"""
    import time
    import commet_amd
    (b0, o0), (b1, o1) = _sets(a.work, a.tag)
    out = {}
    with commet_amd.Context(k=a.k, t=2) as ctx:
        if a.multi_job >= 0:
            ctx.set_option("multi_job", a.multi_job)
        irs = commet_amd.ReadSet.from_files(ctx, [(b0, o0)])
        qrs = commet_amd.ReadSet.from_files(ctx, [(b1, o1)])
        n = irs.num_reads
        part = np.arange(n) * a.n_jobs // n                                      # read r belongs to job r * N // n
        sels = []
        for j in range(a.n_jobs):
            bits = np.zeros(n // 8 + 1, dtype=np.uint8)
            packed = np.packbits(part == j, bitorder="little")
            bits[:packed.size] = packed
            sels.append(bits)

        ts = [1 + j % a.max_t for j in range(a.n_jobs)]

        def call():
            """-> (hits per job, summed info, wall ms); every library call ends in a stream synchronise and the copy back"""
            t0 = time.perf_counter()
            if a.leave == "bytes":                                               # (--thresholds: -> (tags, counts) per job in place of the hits)
                from commet_amd.matrix_io import popcount
                hits, info = ctx.index_many_and_profile([irs] * a.n_jobs, qrs, index_selects=sels, max_hits=ts)
                tags = [commet_amd.tags_at(h, t) for h, t in zip(hits, ts)]
                hits = (tags, [popcount(tg, qrs.num_reads) for tg in tags])
            elif a.leave == "tags":
                tags, shared, info = ctx.index_many_and_thresholds([irs] * a.n_jobs, qrs, index_selects=sels, t=ts)
                hits = (tags, [int(sh.sum()) for sh in shared])
            elif a.share:
                hits, info = ctx.index_many_and_profile([irs] * a.n_jobs, qrs, index_selects=sels, max_hits=a.max_t)
            else:
                hits, info = [], {}
                for sel in sels:
                    h, i = ctx.index_and_profile(irs, [qrs], index_select=sel, max_hits=a.max_t)
                    hits.append(h[0])
                    info = {f: info.get(f, 0) + i[f] for f in i}
            return hits, info, (time.perf_counter() - t0) * 1e3

        _, first, first_ms = call()                                              # warm-up (slots, workspaces, the query list of a tiled pass)
        out["first_call_ms"] = round(first_ms, 3)
        calls = [call() for _ in range(a.reps)]
        hits, info, _ = calls[-1]
        ctx.set_option("kernel_timing", 1)
        call()
        out["kernels_ms"] = _kernels(ctx)
        ctx.set_option("kernel_timing", 0)
        out["wall_ms"] = [round(c[2], 3) for c in calls]
        out["index_ms"] = [round(c[1]["index_ms"], 3) for c in calls]
        out["search_ms"] = [round(c[1]["search_ms"], 3) for c in calls]
        out["chunks"], out["search_launches"], out["reads_walked"] = int(info["n_chunks"]), int(info["search_launches"]), int(info["reads_scanned"])
        if a.leave:
            out["found_per_job"] = hits[1]
            np.save(os.path.join(a.work, a.hits_name), np.stack(hits[0]))
        else:
            out["found_per_job"] = [int((h > 0).sum()) for h in hits]
            np.save(os.path.join(a.work, a.hits_name), np.stack(hits))
    print("RESULT " + json.dumps(out), flush=True)


def many_leg(a):
    legs = [("alone", ["--n-jobs", str(a.jobs)]), ("shared", ["--n-jobs", str(a.jobs), "--share"])]
    if a.long:                                                                   # one many-job call either way: the option decides
        legs = [("alone", ["--n-jobs", str(a.jobs), "--share", "--multi-job", "1"]), ("shared", ["--n-jobs", str(a.jobs), "--share", "--multi-job", "2"])]
    runs = {name: [] for name, _ in legs}
    equal = []
    for r in range(a.rounds):
        for name, extra in legs:
            runs[name].append(run_child(a, "many", "c1", a.limit, extra + ["--hits-name", f"many_{name}.npy"]))
            print(f"round {r} {name}: wall ms {runs[name][-1]['wall_ms']}", file=sys.stderr, flush=True)
        equal.append(bool(np.array_equal(np.load(os.path.join(a.work, "many_alone.npy")), np.load(os.path.join(a.work, "many_shared.npy")))))
    out = {"hits_equal": all(equal), "runs": runs}
    for name, _ in legs:
        per = [med(c["wall_ms"]) for c in runs[name]]
        out[name] = {"wall_ms": round(med(per), 3), "rounds_wall_ms": per, "wall_ms_spread": round((max(per) - min(per)) / med(per), 4),
                     "index_ms": round(med([med(c["index_ms"]) for c in runs[name]]), 3), "search_ms": round(med([med(c["search_ms"]) for c in runs[name]]), 3),
                     "first_call_ms": round(med([c["first_call_ms"] for c in runs[name]]), 3), "chunks": runs[name][0]["chunks"],
                     "search_launches": runs[name][0]["search_launches"], "reads_walked": runs[name][0]["reads_walked"], "kernels_ms": runs[name][0]["kernels_ms"]}
    out["shared_over_alone"] = round(out["shared"]["wall_ms"] / out["alone"]["wall_ms"], 4)
    out["found_per_job"] = runs["shared"][0]["found_per_job"]
    return out


def thresholds_leg(a):
    """--thresholds: bytes + host thresholding against the thresholds call, fresh processes alternated"""
    legs = [("bytes", ["--n-jobs", str(a.jobs), "--leave", "bytes"]), ("tags", ["--n-jobs", str(a.jobs), "--leave", "tags"])]
    runs = {name: [] for name, _ in legs}
    equal = []
    for r in range(a.rounds):
        for name, extra in legs:
            runs[name].append(run_child(a, "many", "c1", a.limit, extra + ["--hits-name", f"thr_{name}.npy"]))
            print(f"round {r} {name}: wall ms {runs[name][-1]['wall_ms']}", file=sys.stderr, flush=True)
        equal.append(bool(np.array_equal(np.load(os.path.join(a.work, "thr_bytes.npy")), np.load(os.path.join(a.work, "thr_tags.npy")))
                          and runs["bytes"][-1]["found_per_job"] == runs["tags"][-1]["found_per_job"]))
    out = {"outputs_equal": all(equal), "runs": runs}
    for name, _ in legs:
        per = [med(c["wall_ms"]) for c in runs[name]]
        dev = med([med(c["index_ms"]) + med(c["search_ms"]) for c in runs[name]])
        k = runs[name][0]["kernels_ms"]
        out[name] = {"wall_ms": round(med(per), 3), "rounds_wall_ms": per, "wall_ms_spread": round((max(per) - min(per)) / med(per), 4),
                     "search_device_ms": round(dev, 3), "hits_tags_kernel": k.get("hits_tags_kernel"),
                     "host_ms": round(med(per) - dev - (k.get("hits_tags_kernel") or [0, 0.0])[1], 3), "kernels_ms": k}
    out["tags_over_bytes"] = round(out["tags"]["wall_ms"] / out["bytes"]["wall_ms"], 4)
    # the kernel's traffic: every job's n bytes read once, n / 8 bytes of its one tag vector written
    n, launches, ms = a.reads, *(out["tags"]["hits_tags_kernel"] or [0, 0.0])
    if ms:
        out["hits_tags_bytes_per_s"] = launches * (n + n / 8) / (ms * 1e-3)
        out["hits_tags_share_of_8TBs"] = round(out["hits_tags_bytes_per_s"] / 8e12, 4)
    out["found_per_job"] = runs["tags"][0]["found_per_job"]
    return out


def long_jobs(a):
    """the --jobs leg on long-read sets: per workload of long_read_bench.py its two sets (made by that tool's own generator), then many_leg"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import long_read_bench as lrb
    res = {"shapes": []}
    for name in a.long_workloads:
        n, total = lrb.make_pair(name, a.scale, a.work)
        offs = np.load(os.path.join(a.work, f"{name}_offs.npy"))
        for i in (0, 1):                                                         # (as _sets reads them)
            os.replace(os.path.join(a.work, f"{name}_{i}_bases.npy"), os.path.join(a.work, f"c1{i}_b.npy"))
            np.save(os.path.join(a.work, f"c1{i}_o.npy"), offs)
        os.remove(os.path.join(a.work, f"{name}_offs.npy"))
        m = many_leg(a)
        shape = {"workload": f"{name}: 2 x {n} reads, {total} bases a set, longest {int(np.diff(offs.astype(np.int64)).max())}, k={a.k}, {a.jobs} jobs on disjoint parts "
                             f"of set 0, max_hits={a.max_t}; alone: multi_job = 1, shared: multi_job = 2", "many": m}
        res["shapes"].append(shape)
        print(json.dumps({"workload": shape["workload"], "hits_equal": m["hits_equal"], "shared_over_alone": m["shared_over_alone"],
                          "found_per_job": m["found_per_job"], "alone": m["alone"], "shared": m["shared"]}), flush=True)
        if not m["hits_equal"]:
            raise SystemExit(f"{name}: the bytes of the shared passes and of the jobs alone differ")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res) + "\n")


def run_child(a, mode, tag, limit, extra=()):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--work", a.work, "--tag", tag, "-k", str(a.k if tag == "c1" else 21),
           "--max-t", str(a.max_t), "--reps", str(a.reps)] + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise SystemExit(f"child {mode} ({tag}) ended with status {p.returncode}; nothing more is started\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
    return json.loads([ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])


def med(x):
    return float(np.median(x))


def groups_leg(a, tag, lib_args, legs=None):
    """the profile of one shape on the parent's library (if given), at chunk_group = 1 and at the default (or the given legs): fresh
    processes, alternated"""
    if legs is None:
        legs = ([("parent", lib_args)] if lib_args else []) + [("group1", ["--chunk-group", "1"]), ("default", [])]
    runs = {name: [] for name, _ in legs}
    equal = []
    for r in range(a.rounds):
        for name, extra in legs:
            runs[name].append(run_child(a, "profile", tag, a.limit, extra + ["--hits-name", f"{tag}_{name}.npy"] + (["--ceiling"] if r == 0 and name == "default" else [])))
        h = [np.load(os.path.join(a.work, f"{tag}_{name}.npy")) for name, _ in legs]
        equal.append(all(np.array_equal(h[0], x) for x in h[1:]))
    out = {"hits_equal": all(equal), "runs": runs}
    for name, _ in legs:
        per = {f: [med(c[f]) for c in runs[name]] for f in ("total_ms", "index_ms", "search_ms")}
        out[name] = {f: round(med(v), 3) for f, v in per.items()}
        out[name]["total_ms_spread"] = round((max(per["total_ms"]) - min(per["total_ms"])) / med(per["total_ms"]), 4)
        out[name]["first_call_total_ms"] = round(med([c["first_call"]["total_ms"] for c in runs[name]]), 3)
        out[name]["cache_bytes"] = runs[name][0].get("cache_bytes")
        out[name].update(reads_walked=runs[name][0]["reads_walked"], search_launches=runs[name][0].get("search_launches"), chunks=runs[name][0]["chunks"],
                         kernels_ms=runs[name][0]["kernels_ms"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("-k", type=int, default=32)
    ap.add_argument("--max-t", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--jobs-lib", default=None)
    ap.add_argument("--many-chunks", action="store_true")
    ap.add_argument("--groups", action="store_true")
    ap.add_argument("--chunk-group", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--hits-name", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--profile-wide", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--sliced", action="store_true")
    ap.add_argument("--profile-slice", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--tiled", action="store_true")
    ap.add_argument("--profile-tiled", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--parent-tiled", action="store_true")
    ap.add_argument("--jobs", type=int, default=0, help="N jobs on disjoint N-ths of set 0, all searching set 1: one by one against one many-job call")
    ap.add_argument("--n-jobs", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--share", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--thresholds", action="store_true", help="with --jobs: many-job profile + host thresholding against the thresholds call")
    ap.add_argument("--leave", default=None, choices=["bytes", "tags"], help=argparse.SUPPRESS)
    ap.add_argument("--long", action="store_true", help="with --jobs: on long-read search sets, multi_job = 1 against multi_job = 2")
    ap.add_argument("--long-workloads", nargs="+", default=["ragged_1k_10k", "len5500"], help="--long: workloads of tools/long_read_bench.py")
    ap.add_argument("--scale", type=float, default=1.0, help="--long: reads per set, as a share of the workload's")
    ap.add_argument("--multi-job", type=int, default=-1, help=argparse.SUPPRESS)     # (-1 = leave the option alone)
    ap.add_argument("--many-reads", type=int, nargs="+", default=[600_000])
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tag", default="c1", help=argparse.SUPPRESS)
    ap.add_argument("--ts", type=int, nargs="+", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--max-kmer", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--ceiling", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.ts is None:
        a.ts = list(range(1, a.max_t + 1))
    if a.child:
        return {"profile": child_profile, "jobs": child_jobs, "many": child_many}[a.child](a)
    if a.jobs_lib:
        a.jobs_lib = os.path.abspath(a.jobs_lib)
    from commet_amd import synth
    if a.long and a.jobs < 2:
        raise SystemExit("--long measures the many-job leg: give --jobs N, N >= 2")
    a.work = tempfile.mkdtemp(prefix="hits_bench_")
    try:
        if a.long:
            return long_jobs(a)
        for i in (0, 1) if not (a.wide or a.sliced) else ():                     # (the wide and sliced legs have shapes of their own)
            b, o = synth.synth_set(i, a.reads, a.read_len, base_set=0)
            np.save(os.path.join(a.work, f"c1{i}_b.npy"), b), np.save(os.path.join(a.work, f"c1{i}_o.npy"), o)
        res = {"workload": f"2 x {a.reads} x {a.read_len} bp, k={a.k}, t=1..{a.max_t}", "profile": [], "jobs": []}
        lib_args = ["--jobs-lib", a.jobs_lib] if a.jobs_lib else []
        if a.wide:
            if not a.many_chunks:
                raise SystemExit("--wide measures the many-chunk shapes: give --many-chunks")
            legs = ([("parent", lib_args)] if lib_args else []) + [("wide1", ["--profile-wide", "1"]), ("wide2", ["--profile-wide", "2"])]
            res = {"shapes": []}
            for n in a.many_reads:
                L = 150
                for i in (0, 1):
                    b, o = synth.synth_set(i, n, L, base_set=0)
                    np.save(os.path.join(a.work, f"c4{i}_b.npy"), b), np.save(os.path.join(a.work, f"c4{i}_o.npy"), o)
                shape = {"workload": f"2 x {n} x {L} bp, k=21, T={a.max_t}", "wide": groups_leg(a, "c4", lib_args, legs),
                         "job_t5": run_child(a, "jobs", "c4", a.limit, lib_args + ["--ts", "5"])}
                res["shapes"].append(shape)
                w = shape["wide"]
                print(json.dumps({"workload": shape["workload"], "hits_equal": w["hits_equal"], "job_t5_ms": shape["job_t5"]["per_t"]["5"]["total_ms"],
                                  **{name: {f: w[name][f] for f in ("total_ms", "index_ms", "search_ms", "total_ms_spread", "search_launches", "reads_walked", "chunks")}
                                     for name, _ in legs}}), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                open(a.out, "w").write(json.dumps(res) + "\n")
            return
        if a.sliced:
            if not a.many_chunks:
                raise SystemExit("--sliced measures the many-chunk shapes: give --many-chunks")
            legs = [("slice1", ["--profile-slice", "1"]), ("slice2", ["--profile-slice", "2"])]
            res = {"shapes": []}
            for n in a.many_reads:
                L = 150
                for i in (0, 1):
                    b, o = synth.synth_set(i, n, L, base_set=0)
                    np.save(os.path.join(a.work, f"c4{i}_b.npy"), b), np.save(os.path.join(a.work, f"c4{i}_o.npy"), o)
                shape = {"workload": f"2 x {n} x {L} bp, k=21, T={a.max_t}", "sliced": groups_leg(a, "c4", [], legs)}
                res["shapes"].append(shape)
                w = shape["sliced"]
                print(json.dumps({"workload": shape["workload"], "hits_equal": w["hits_equal"],
                                  "slice2_over_slice1": round(w["slice2"]["total_ms"] / w["slice1"]["total_ms"], 4),
                                  **{name: {f: w[name][f] for f in ("total_ms", "index_ms", "search_ms", "total_ms_spread", "search_launches", "reads_walked", "chunks",
                                                                    "kernels_ms")} for name, _ in legs},
                                  "rounds_total_ms": {name: [med(c["total_ms"]) for c in w["runs"][name]] for name, _ in legs}}), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                open(a.out, "w").write(json.dumps(res) + "\n")
            return
        a.many_reads = a.many_reads[0]
        if a.jobs:
            if a.jobs < 2:
                raise SystemExit("--jobs needs at least two jobs")
            if a.thresholds:
                m = thresholds_leg(a)
                res = {"workload": f"2 x {a.reads} x {a.read_len} bp, k={a.k}, {a.jobs} jobs on disjoint parts of set 0, job j at t = 1 + j % {a.max_t}", "thresholds": m}
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    open(a.out, "w").write(json.dumps(res) + "\n")
                print(json.dumps({"workload": res["workload"], **{f: v for f, v in m.items() if f != "runs"}}), flush=True)
                if not m["outputs_equal"]:
                    raise SystemExit("the tags or counts of the two legs differ")
                return
            m = many_leg(a)
            res = {"workload": f"2 x {a.reads} x {a.read_len} bp, k={a.k}, {a.jobs} jobs on disjoint parts of set 0, max_hits={a.max_t}", "many": m}
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                open(a.out, "w").write(json.dumps(res) + "\n")
            print(json.dumps({"workload": res["workload"], "hits_equal": m["hits_equal"], "shared_over_alone": m["shared_over_alone"],
                              "found_per_job": m["found_per_job"], "alone": m["alone"], "shared": m["shared"]}), flush=True)
            return
        if a.tiled:
            legs = ([("parent", lib_args)] if lib_args else []) + ([("parent_tiled2", lib_args + ["--profile-tiled", "2"])] if a.parent_tiled else []) + \
                   [("tiled1", ["--profile-tiled", "1"]), ("tiled2", ["--profile-tiled", "2"]), ("auto", [])]
            t = groups_leg(a, "c1", lib_args, legs)
            res = {"workload": res["workload"], "tiled": t}
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                open(a.out, "w").write(json.dumps(res) + "\n")
            print(json.dumps({"workload": res["workload"], "hits_equal": t["hits_equal"],
                              **{name: {f: t[name][f] for f in ("total_ms", "index_ms", "search_ms", "total_ms_spread", "first_call_total_ms", "cache_bytes",
                                                                "search_launches", "reads_walked", "kernels_ms")} for name, _ in legs}}), flush=True)
            return
        if a.groups:
            res = {"workload": res["workload"], "groups": groups_leg(a, "c1", lib_args)}
            if a.many_chunks:
                n, L = a.many_reads, 150
                for i in (0, 1):
                    b, o = synth.synth_set(i, n, L, base_set=0)
                    np.save(os.path.join(a.work, f"c4{i}_b.npy"), b), np.save(os.path.join(a.work, f"c4{i}_o.npy"), o)
                res["many_chunks"] = {"workload": f"2 x {n} x {L} bp, k=21", "groups": groups_leg(a, "c4", lib_args),
                                      "job_t5": run_child(a, "jobs", "c4", a.limit, lib_args + ["--ts", "5"])}
            text = json.dumps(res)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                open(a.out, "w").write(text + "\n")
            for shape in (res, res.get("many_chunks")):
                if shape:
                    g = shape["groups"]
                    print(json.dumps({"workload": shape["workload"], "hits_equal": g["hits_equal"],
                                      **{name: {f: g[name][f] for f in ("total_ms", "index_ms", "search_ms", "total_ms_spread", "search_launches", "reads_walked")}
                                         for name in ("parent", "group1", "default") if name in g}}))
            if "many_chunks" in res:
                print(json.dumps({"job_t5_ms": res["many_chunks"]["job_t5"]["per_t"]["5"]["total_ms"]}))
            return
        for r in range(a.rounds):                                                # (a) and (b) alternate
            res["profile"].append(run_child(a, "profile", "c1", a.limit, ["--ceiling"] if r == 0 else []))
            res["jobs"].append(run_child(a, "jobs", "c1", a.limit, lib_args))
            pt, jt = np.load(os.path.join(a.work, "c1_profile_tags.npy")), np.load(os.path.join(a.work, "c1_job_tags.npy"))
            res.setdefault("tags_equal", []).append(bool(pt.shape == jt.shape and (pt == jt).all()))
        prof = med([med(p["total_ms"]) for p in res["profile"]])
        jobs = sum(med([med(j["per_t"][str(t)]["total_ms"]) for j in res["jobs"]]) for t in range(1, a.max_t + 1))
        p0 = res["profile"][0]
        hk = p0["kernels_ms"].get("hits_kernel", [0, 0.0])
        res["summary"] = {"profile_ms": round(prof, 3), "jobs_sum_ms": round(jobs, 3), "profile_over_jobs": round(prof / jobs, 4) if jobs else None,
                          "tags_equal": all(res["tags_equal"]), "hits_kernel_ms": hk[1], "hits_kernel_launches": hk[0],
                          "plane_a_requests_per_s_at_most": (p0["windows"] * hk[0] / (hk[1] * 1e-3)) if hk[1] else None,
                          "gather_ceiling_per_s": p0.get("gather_ceiling_per_s")}
        if a.many_chunks:
            n, L = a.many_reads, 150
            for i in (0, 1):
                b, o = synth.synth_set(i, n, L, base_set=0)
                np.save(os.path.join(a.work, f"c4{i}_b.npy"), b), np.save(os.path.join(a.work, f"c4{i}_o.npy"), o)
            res["many_chunks"] = {"workload": f"2 x {n} x {L} bp, k=21", "profile": run_child(a, "profile", "c4", a.limit),
                                  "job_t5": run_child(a, "jobs", "c4", a.limit, lib_args + ["--ts", "5"])}
    finally:
        shutil.rmtree(a.work, ignore_errors=True)
    text = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps(res["summary"]))
    if "many_chunks" in res:
        m = res["many_chunks"]
        print(json.dumps({"many_chunks": m["workload"], "chunks": m["profile"]["chunks"], "profile_ms": m["profile"]["total_ms"],
                          "job_t5_ms": m["job_t5"]["per_t"]["5"]["total_ms"]}))


if __name__ == "__main__":
    main()
