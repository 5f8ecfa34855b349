#!/usr/bin/env python3
"""residency_bench.py — what a set budget costs: the configs[2]-size matrix (10 sets x 10 M reads of 100 bp, k = 32, t = 2) through
commet_amd.matrix unconstrained and under budgets that hold 5 and 3 sets, each run in a fresh child process under its own time limit;
the first failure ends the script.  Per run: total_s, jobs_s, reload_s, set_wait_s, set_reloads, j1_builds (one JSON line each).

    python tools/residency_bench.py [--sets 10] [--reads 10000000] [--len 100] [--work DIR] [--limit-s 240]

The question it answers (MEASUREMENTS.md): do the reloads hide behind the jobs?  set_wait_s is the time the job thread stood waiting for
a set; reload_s the time the loader thread spent in commet_readset_restore."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
from commet_amd import matrix
budget = float(sys.argv[4]) if sys.argv[4] != "none" else None
res = matrix.run(sys.argv[2], sys.argv[3], k=32, t=2, verbose=False, set_budget_gb=budget)
prof = res["rank0_profile"]
out = {f: res.get(f) for f in ("total_s", "jobs_s", "load_s", "set_wait_s", "reload_s", "set_loads", "set_reloads", "set_offloads",
                               "peak_set_bytes", "set_budget_bytes", "set_sizing_s")}
out["j1_builds"] = prof["j1_builds"]
out["jobs"] = prof["jobs"]
print("RESULT " + json.dumps(out), flush=True)
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=10)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=100, dest="read_len")
    ap.add_argument("--work", default=None)
    ap.add_argument("--limit-s", type=int, default=240, help="time limit of each child run")
    ap.add_argument("--hold", default="5,3", help="budgets, in sets held")
    a = ap.parse_args()
    from multiprocessing import get_context
    from commet_amd import synth
    import commet_amd
    work = a.work or tempfile.mkdtemp(prefix="commet_resid_")
    os.makedirs(work, exist_ok=True)
    t0 = time.perf_counter()
    jobs = [(s, a.reads, a.read_len, os.path.join(work, f"set{s}.fa")) for s in range(a.sets)]
    with get_context("spawn").Pool(min(a.sets, 8)) as pool:
        pool.map(synth.write_set_fasta, jobs)
    sets_txt = os.path.join(work, "sets.txt")
    with open(sets_txt, "w") as fh:
        fh.write("".join(f"set{s}: {p}\n" for s, _, _, p in jobs))
    one = commet_amd.files_packed_bytes([jobs[0][3]])[2]              # (a host-side count: this process never opens the GPU)
    print(f"{a.sets} sets of {a.reads} reads written in {time.perf_counter() - t0:.1f} s; one set packs to {one} bytes", flush=True)
    runs = [("unconstrained", "none")] + [(f"holds_{h}", repr((int(h) * one + 0.5) / 2**30)) for h in a.hold.split(",") if h]
    for label, budget in runs:
        out_dir = os.path.join(work, "out_" + label)
        cmd = ["timeout", "-k", "10", str(a.limit_s), sys.executable, "-c", CHILD, ROOT, sets_txt, out_dir, budget]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = next((ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")), None)
        if p.returncode != 0 or line is None:
            print(f"{label}: exit code {p.returncode}\n{p.stdout[-3000:]}", flush=True)
            return p.returncode or 1                                  # nothing more is started on the device after a failure
        print(json.dumps(dict(run=label, **json.loads(line[7:]))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
