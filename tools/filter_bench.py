"""What the read filter costs: the filter_reads tool (a second pass over the text on the CPU) against commet_readset_filter on the
resident set, and the N x N driver with filter options on either path.

  python tools/filter_bench.py set [--reads 10000000] [--len 100]
      one synthetic FASTA set and its FASTQ twin, -l 50 -n 2 -e 1.5: wall time of commet_amd/bin/filter_reads at its default threads,
      wall time of commet_readset_filter, its kernel time (option kernel_timing), and the bytes the kernel reads over that time
      against the streaming ceiling commet_membench mode 4 (a device-to-device copy) reports in the same run.
  python tools/filter_bench.py matrix [--sets 10] [--reads 10000000] [--tool]
      the matrix of synthetic sets with the same options; --tool: COMMET_MATRIX_FILTER_TOOL=1, the filter_reads processes.

Every result is one JSON line on stdout."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = dict(l=50, n=2, e=1.5)


def scratch():
    root = os.environ.get("COMMET_SCRATCH") or ("/dev/shm" if os.access("/dev/shm", os.W_OK) else tempfile.gettempdir())
    return tempfile.mkdtemp(prefix="commet_filter_bench_", dir=root)


def write_fastq_fast(path, bases, n, L):
    """the FASTQ twin of synth.write_fasta_fast: '@%09d', the read, '+', a quality line of 'I'"""
    rec = 11 + (L + 1) + 2 + (L + 1)
    view = np.asarray(bases, dtype=np.uint8).reshape(n, L)
    block = 1 << 20
    with open(path, "wb") as fh:
        for r0 in range(0, n, block):
            m = min(block, n - r0)
            buf = np.full((m, rec), ord("I"), dtype=np.uint8)
            buf[:, 0] = ord("@")
            idx = np.arange(r0, r0 + m, dtype=np.int64)
            for d in range(9):
                buf[:, 9 - d] = (idx % 10 + ord("0")).astype(np.uint8)
                idx //= 10
            buf[:, 10] = ord("\n")
            buf[:, 11:11 + L] = view[r0:r0 + m]
            buf[:, 11 + L] = ord("\n")
            buf[:, 12 + L] = ord("+")
            buf[:, 13 + L] = ord("\n")
            buf[:, -1] = ord("\n")
            fh.write(buf.data)


def bench_set(a):
    import commet_amd
    from commet_amd import matrix, synth
    work = scratch()
    try:
        n, L = a.reads, a.len
        bases, _ = synth.synth_set_skewed(0, n, L)                # a tenth of the reads low-complexity: the Shannon test has work
        fa, fq = os.path.join(work, "s.fa"), os.path.join(work, "s.fq")
        synth.write_fasta_fast(fa, bases, n, L)
        write_fastq_fast(fq, bases, n, L)
        del bases
        tool = os.path.join(ROOT, "commet_amd", "bin", "filter_reads")
        args = ["-l", str(OPTS["l"]), "-n", str(OPTS["n"]), "-e", str(OPTS["e"])]
        out = dict(reads=n, read_len=L, options=OPTS)
        with commet_amd.Context(k=32, t=2, device=0) as ctx:
            # the streaming ceiling, in the same run: a device-to-device copy reads and writes its bytes once each
            nbytes = 1 << 30
            ms = min(ctx.membench(4, nbytes, 0) for _ in range(3))
            ceiling = 2 * nbytes / ms / 1e6
            out["copy_ceiling_GBps"] = round(ceiling, 1)
            for tag, path in (("fasta", fa), ("fastq", fq)):
                t0 = time.perf_counter()
                subprocess.run([tool, path] + args + ["-o", path + ".bv"], check=True, stdout=subprocess.DEVNULL)
                tool_s = time.perf_counter() - t0
                t0 = time.perf_counter()
                rs = commet_amd.ReadSet.from_fasta(ctx, [path])
                parse_s = time.perf_counter() - t0
                rs.filter(min_len=OPTS["l"], max_n=OPTS["n"], min_shannon=OPTS["e"])          # (first call: table, scratch)
                ctx.set_option("kernel_timing", 1)
                walls = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    bits, st = rs.filter(min_len=OPTS["l"], max_n=OPTS["n"], min_shannon=OPTS["e"])
                    walls.append(time.perf_counter() - t0)
                kt = ctx.kernel_times()
                ctx.set_option("kernel_timing", 0)
                (kname, (launches, total_ms)), = [(k_, v) for k_, v in kt.items() if k_.startswith("read_filter")]
                kernel_ms = total_ms / launches
                read_bytes = (n * L // 32 + n) * 12                # the planes: 12 bytes per word triple
                nb, want = matrix.read_bv(path + ".bv")
                out[tag] = dict(file_bytes=os.path.getsize(path), tool_wall_s=round(tool_s, 3), parse_upload_s=round(parse_s, 3),
                                device_wall_ms=round(1e3 * min(walls), 3), device_wall_ms_all=[round(1e3 * w, 3) for w in walls],
                                kernel=kname, kernel_ms=round(kernel_ms, 4), plane_bytes=read_bytes,
                                kernel_GBps=round(read_bytes / kernel_ms / 1e6, 1), of_copy_ceiling=round(read_bytes / kernel_ms / 1e6 / ceiling, 3),
                                selected=st[0]["selected"], removed=[st[0]["removed_length"], st[0]["removed_n"], st[0]["removed_shannon"]],
                                same_bits_as_tool=bool(nb == n and np.array_equal(bits, want)))
                rs.close()
        print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def bench_matrix(a):
    from commet_amd import matrix, synth
    import multiprocessing as mp
    work = scratch()
    os.environ["COMMET_SCRATCH"] = work
    if a.tool:
        os.environ["COMMET_MATRIX_FILTER_TOOL"] = "1"
    else:
        os.environ.pop("COMMET_MATRIX_FILTER_TOOL", None)
    try:
        t0 = time.perf_counter()
        jobs = [(s, a.reads, a.len, os.path.join(work, f"set{s}.fa")) for s in range(a.sets)]
        with mp.get_context("spawn").Pool(min(a.sets, 8)) as pool:
            pool.map(synth.write_set_fasta, jobs, chunksize=1)
        with open(os.path.join(work, "sets.txt"), "w") as fh:
            for s in range(a.sets):
                fh.write(f"S{s}: {work}/set{s}.fa\n")
        gen_s = time.perf_counter() - t0
        res = matrix.run(os.path.join(work, "sets.txt"), os.path.join(work, "out") + "/", k=32, t=2, verbose=False, **OPTS)
        keep = ("filter_s", "load_s", "jobs_s", "set_wait_s", "total_s", "reads_searched", "considered")
        print(json.dumps(dict(path="filter_reads processes" if a.tool else "device filter", sets=a.sets, reads=a.reads, read_len=a.len, options=OPTS,
                              generate_s=round(gen_s, 2), **{f: (round(res[f], 4) if isinstance(res[f], float) else res[f]) for f in keep})), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["set", "matrix"])
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--sets", type=int, default=10)
    ap.add_argument("--tool", action="store_true")
    a = ap.parse_args()
    (bench_set if a.what == "set" else bench_matrix)(a)
