"""The N x N matrix at every threshold t in 1..T from one run — `python -m commet_amd.matrix sets.txt -k K --max-t T -o OUT/`.

To see how the similarity matrix moves with t, Commet.py (and `matrix -t t`) is run T times; every run parses, loads and filters the
sets again and rebuilds every J1 index.  All three stages of the job DAG can share one search over the thresholds:

    J1(ref)             the filters do not depend on t: ONE profile job answers every t (commet_index_and_thresholds);
    J2(ref, i, t)       for all i and t: they index S_i under J1's tags at t and all search S_ref under S_ref's own filter bits — jobs
                        of one search set with one search selection, a threshold per job (commet_index_many_and_thresholds);
    J3(ref, i, t)       for all ref < i and all t: they search S_i under S_i's own filter bits (Commet.py:230-233) — the same, one
                        call per target, kept back until the target's last reference set is through J2 (as matrix._schedule does).

Tags and the per-file counts of the matrix cells are made on the device (hits_tags_kernel): no host code here thresholds bytes or
counts bits.  OUT/t<t>/ holds, for every t, the `_in_` .bv files and the three csv matrices, byte for byte what
`python -m commet_amd.matrix sets.txt -k K -t t` writes with the same filter options; the filter .bv files go to OUT/ once.  No .log
files: their `searched` figure depends on t (a job at t skips the reads an earlier chunk has tagged at t), as sweep.py says.

One rank, every set resident: no --gpus, no launcher's ranks, no --set-budget-gb.  -l must be 0: Commet.py raises a non-zero -l to
k * t, so the filter itself would depend on t."""
import os
import time
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

from . import matrix
from .matrix_io import split_bits, write_bv, write_matrices


def refusal(max_t, gpus=1, set_budget_gb=None, l=0, world=1):
    """why --max-t cannot run with these options (None: it can)"""
    if not 1 <= max_t <= 255:
        return f"--max-t must be in 1..255 (got {max_t}): a read's hits are counted in a byte"
    if gpus > 1 or world > 1:
        return f"--max-t runs on one rank ({max(gpus, world)} asked for): the threshold sweep keeps every set resident on one GPU"
    if set_budget_gb is not None:
        return "--max-t with --set-budget-gb: the threshold sweep keeps every set resident"
    if l != 0:
        return f"--max-t with -l {l}: Commet.py raises a non-zero -l to k * t, so the filter itself would depend on t"
    return None


class SweepJobs:
    """the library calls of the sweep, the files they leave under OUT/t<t>/, what they add to the matrices"""

    def __init__(self, eng, cfg, T, sets, sel, counts, prof):
        self.eng, self.cfg, self.T, self.sets, self.sel, self.counts, self.prof = eng, cfg, T, sets, sel, counts, prof
        self.shared = {t: {} for t in range(1, T + 1)}             # t -> (from set, in set) -> reads of `from` found in `in`
        self.writer, self.written = ThreadPoolExecutor(2), []
        self.kernel_times = getattr(eng, "kernel_times", lambda: None)

    def acc(self, inf, n):
        self.prof["calls"] += 1
        self.prof["jobs"] += n
        self.prof["call_ms"] += inf["total_ms"]
        self.prof["device_ms"] += inf["index_ms"] + inf["search_ms"]

    def j1(self, ref, targets):
        """J1 of a reference set at every t: tags[s][t - 1] of each target"""
        sets, sel = self.sets, self.sel
        tags, _shared, inf = self.eng.index_and_thresholds(sets[ref], [sets[i] for i in targets], sel[ref], [sel[i] for i in targets], self.T)
        self.acc(inf, 1)
        return tags

    def on_one_search_set(self, jobs, search_id, selections):
        """jobs = [(index set, t)] that all search one set under its own filter bits -> [tags] in their order; their files, their cells"""
        if not jobs:
            return []
        sets = self.sets
        tags, shared, inf = self.eng.index_many_and_thresholds([sets[x] for x, _ in jobs], sets[search_id], selections, self.sel[search_id],
                                                               [t for _, t in jobs])
        self.acc(inf, len(jobs))
        for (x, t), tg, sh in zip(jobs, tags, shared):
            self.leave(search_id, x, t, tg, sh)
        return tags

    def leave(self, search, index, t, tags, per_file):
        """<file of `search`>_in_<index>.bv under t<t>/ (a J3 job's replaces nothing there: J1's tags are never written), and the cell"""
        cfg = self.cfg
        d = f"{cfg.out_dir}t{t}/"
        for f, c, b in zip(cfg.files[search], self.counts[search], split_bits(tags, self.counts[search])):
            self.written.append(self.writer.submit(write_bv, d + os.path.basename(f) + "_in_" + cfg.names[index] + ".bv", f + " in " + cfg.names[index], c, b))
        self.shared[t][(search, index)] = int(sum(int(v) for v in per_file))

    def finish(self):
        self.eng.synchronize()
        for f in self.written:
            f.result()
        self.writer.shutdown()
        return time.perf_counter()


def _schedule(N, T, jobs, note):
    """per reference set: J1 once, the J2 jobs (i, t) of all its targets and thresholds in one call; the J3 jobs (ref, t) of a target in
    one call as soon as its last reference set is through J2"""
    kept = {}                                                      # (ref, i, t) -> J2's tags, the index selection of J3(ref, i, t)
    thresholds = range(1, T + 1)
    for ref in range(N - 1):
        targets = list(range(ref + 1, N))
        tags1 = jobs.j1(ref, targets)
        j2 = [(i, t) for i in targets for t in thresholds]
        for (i, t), tg in zip(j2, jobs.on_one_search_set(j2, ref, [tags1[s][t - 1] for s in range(len(targets)) for t in thresholds])):
            kept[(ref, i, t)] = tg
        note(f"J1 and J2 jobs of set {ref} done at {T} thresholds ({jobs.prof['jobs']} jobs so far)")
        i = ref + 1                                                # the one target whose reference sets are all through now
        j3 = [(r, t) for r in range(i) for t in thresholds]
        jobs.on_one_search_set(j3, i, [kept.pop((r, i, t)) for r, t in j3])
        note(f"J3 jobs of set {i} done")
    assert not kept


def run(input_file, out_dir, k=33, max_t=4, l=0, n=-1, e=0.0, m=-1, bin_dir=None, verbose=True, engine_factory=None, progress=None):
    """-> dict(names, considered, matrices={t: N x N}, total_s, load_s, filter_s, jobs_s, ...); raises ValueError where refusal() says why"""
    t_start = time.perf_counter()
    why = refusal(int(max_t), l=l, world=int(os.environ.get("WORLD_SIZE", "1")))
    if why:
        raise ValueError(why)
    T = int(max_t)
    cfg = matrix._setup(input_file, out_dir, k, 1, 0, bin_dir, 0, verbose, progress)
    N, say, note = cfg.N, cfg.say, cfg.note
    for t in range(1, T + 1):
        os.makedirs(f"{cfg.out_dir}t{t}", exist_ok=True)
    eng = (engine_factory or matrix.HipEngine)(k, 1, 0)            # (the thresholds calls do not use the context's own t)
    lacking = [a for a in ("index_and_thresholds", "index_many_and_thresholds") if not hasattr(eng, a)]
    filters, jobs = None, None
    try:
        if lacking:
            raise RuntimeError(f"the threshold sweep needs an engine with the thresholds calls: {type(eng).__name__} has no " + " / ".join(lacking))
        filters = matrix.Filters(cfg.files, cfg.bvs, cfg.out_dir, cfg.bin_dir, 0, n, e, m, eng)
        if filters.tool:
            filters.start_tool(range(N), SimpleNamespace(barrier=lambda: None), say)
            filters.done()
        # ---- every set resident, its filter files in OUT/ once
        w0 = time.perf_counter()
        sets, counts, considered, sel = {}, {}, {}, {}
        for s in range(N):
            sets[s] = eng.parse(cfg.files[s])
            filters.leave(s, sets[s])
            counts[s], considered[s], sel[s] = filters.selection(s, sets[s])
            note(f"set {s} resident")
        load_s = time.perf_counter() - w0
        prof = dict(calls=0, jobs=0, call_ms=0.0, device_ms=0.0)
        jobs = SweepJobs(eng, cfg, T, sets, sel, counts, prof)
        t_jobs = time.perf_counter()
        _schedule(N, T, jobs, note)
        jobs_s = jobs.finish() - t_jobs
        # ---- the three matrices of every t
        considered_all = [considered[s] for s in range(N)]
        matrices = {}
        for t in range(1, T + 1):
            mat = [[0] * N for _ in range(N)]
            for (a, b), v in jobs.shared[t].items():
                mat[a][b] = v
            for s in range(N):
                mat[s][s] = considered_all[s]
            write_matrices(f"{cfg.out_dir}t{t}/", cfg.names, considered_all, mat)
            matrices[t] = mat
        total_s = time.perf_counter() - t_start
        res = dict(names=cfg.names, considered=considered_all, matrices=matrices, max_t=T, world=1, filter_s=filters.seconds, load_s=load_s,
                   jobs_s=jobs_s, total_s=total_s, jobs=prof["jobs"], calls=prof["calls"], call_ms=round(prof["call_ms"], 3),
                   device_ms=round(prof["device_ms"], 3))
        if jobs.kernel_times() is not None:
            res["kernel_ms"] = jobs.kernel_times()
        say(f"{prof['jobs']} jobs at {T} thresholds in {prof['calls']} calls, {jobs_s:.3f} s of jobs (load {load_s:.2f} s, total {total_s:.2f} s)")
        say("\t Output csv matrices are in: " + ", ".join(f"{cfg.out_dir}t{t}/" for t in range(1, T + 1)))
        for rs in sets.values():
            eng.release(rs)
        return res
    finally:
        if jobs is not None:
            jobs.writer.shutdown(wait=False, cancel_futures=True)
        if filters is not None:
            filters.shutdown()
        eng.close()
