"""N x N comparison driver with set residency — the MI355X counterpart of Commet.py's
local mode (reference: Commet.py:438-598), SURVEY 8f-2 / 8e.

Commet.py runs N^2-1 `index_and_search` processes one after the other; every one re-parses
its FASTA files and re-creates its filter, which on a GPU means a HIP start-up, a re-upload
and a 16 GB scratch allocation per job.  Here the job DAG runs in-process through the C ABI
on sets that stay packed in HBM:

    for ref < i :   J1  index S_ref                          search S_i      -> T1
                    J2  index S_i   restricted to T1         search S_ref    -> <G>_in_<S_i>.bv
                    J3  index S_ref restricted to J2's bits  search S_i      -> <F>_in_<S_ref>.bv

Order on a rank: per reference set J1 (one call: its index built once for all its targets), then the J2 jobs of those targets in ONE
call — they all search S_ref, and commet_index_many_and_search lets the chunk filters of up to four of them share a pass over it —
and, once every reference set is through, the J3 jobs target by target (they all search S_i) the same way.  What a job writes does
not depend on when it runs.

One process per GPU.  The path has no exchange step, so ranks share nothing but small files
and three host-side gathers (sharding.Ranks: a TCP store of rank 0, no torch in the ranks):
  * every set is PARSED ONCE on the node (set s by rank s % world; left-over sets by the ranks with
    the cheapest pairs), by a rank which exports the set's
    device buffers (commet_readset_export: HIP IPC handles, a 264-byte descriptor in a scratch
    directory); the other ranks that need the set copy it device to device
    (commet_readset_import: xGMI between GPUs) — no file, no parsing.  Where that is not to be
    had (the probe or the canary below fail, COMMET_MATRIX_IPC=0) the set travels as a packed
    image in /dev/shm (commet_readset_save / _load);
  * the row-major list of (ref, i) pairs is cut into contiguous runs of equal cost, one per
    rank: a rank works on few reference sets, builds J1's index of S_ref once for all its
    targets (as Commet.py's J1 does), and loads only the sets its pairs touch;
  * a rank that fails exits non-zero at once (the launcher then ends the group).

Same inputs and outputs as Commet.py: the set file `name: file[,bv]; file…`, the filter
step (`filter_reads`, skipped when bvs are given), `OUT/<file>_in_<set>.bv`,
`OUT/<s>_in_<i>.log`, `matrix_plain.csv`, `matrix_percentage.csv`, `matrix_normalized.csv`.

  python -m commet_amd.matrix sets.txt -k 32 -t 2 -o out/            (1 GPU)
  python -m commet_amd.matrix sets.txt -k 32 -t 2 -o out/ --gpus 8   (8 GPUs: starts its own ranks)
  python -m torch.distributed.run --nproc-per-node 8 -m commet_amd.matrix sets.txt …   (any launcher that sets RANK / WORLD_SIZE / MASTER_*)
  python -m commet_amd.matrix sets.txt -k 32 --max-t 4 -o out/       (1 GPU: the matrix at every t = 1..4 from one run, out/t<t>/: matrix_sweep.py)
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import threading
import time
import traceback
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from . import residency, sharding
from .handover import Handover, wait_file
from .matrix_io import (_log, c_atoi, concat_bits, default_filter_bv, filter_command, filter_comment, parse_set_file,  # noqa: F401 (re-exported)
                        popcount, read_bv, split_bits, write_bv, write_filter_bv, write_matrices)

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the engine: where the reads live and the jobs run ------------------------------------------------
class HipEngine:
    """The product engine: read sets packed in HBM, jobs through libcommet_hip.so (commet_amd.api).
    There is no other engine in the package; tests inject a CPU checker through `engine_factory` to run
    the multi-rank host logic without a GPU."""

    def __init__(self, k, t, local_rank):
        import commet_amd
        self._alloc0 = commet_amd.device_alloc_stats(-1)          # (before the context: its filter and workspaces count as this run's)
        # LOCAL_RANK modulo the devices this process sees (a launcher may give every rank one visible device);
        # COMMET_FORCE_DEVICE: debugging aid to run several ranks on one GPU (never set by the driver)
        self._api = commet_amd
        self.ctx = commet_amd.Context(k=k, t=t, device=sharding.pick_device(local_rank, commet_amd.device_count()))
        self._kernel_times = os.environ.get("COMMET_MATRIX_KERNEL_TIMES", "0") == "1"
        if self._kernel_times:
            self.ctx.set_option("kernel_timing", 1)
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if "COMMET_FORCE_DEVICE" in os.environ and world > 1:
            # several ranks on ONE device (a rehearsal): the cached query lists of all of them must fit it together — no rank can
            # take memory back from another one's cache
            self.ctx.set_option("query_list_budget_mb", (64 << 10) // world)

    def parse(self, files):
        return self._api.ReadSet.from_fasta(self.ctx, files)

    def save(self, rs, path):
        rs.save(path)

    def load(self, path):
        return self._api.ReadSet.load(self.ctx, path)

    def parse_probe(self):
        """a tiny set of this rank's own, for the hand-over probe"""
        b = np.frombuffer(b"ACGTTGCAACGTACGTTTGACCAGTACGATCGATCGGCTA" * 4, dtype=np.uint8)
        o = np.arange(5, dtype=np.uint64) * np.uint64(40)
        return self._api.ReadSet.from_files(self.ctx, [(b, o)])

    def export_set(self, rs):
        """bytes another rank imports the set from, device to device (HIP IPC); rs must outlive every import"""
        return rs.export()

    def import_set(self, blob):
        return self._api.ReadSet.import_(self.ctx, blob)

    def canary_argv(self, scratch, candidates):
        """the command of the fresh child process that imports the first real set before this process does (ipc_canary.py)"""
        # (by path, not `-m`: the child's working directory need not be one from which the package can be imported)
        return [sys.executable, os.path.join(HERE, "ipc_canary.py"), str(self.ctx.device), str(self.ctx.k), str(self.ctx.t), scratch,
                ",".join(str(c) for c in candidates)]

    def same_set(self, a, b):
        """the packed images of two resident sets are the same bytes (the hand-over probe: what came over is what was sent)"""
        d = tempfile.mkdtemp(prefix="commet_probe_", dir=_scratch_root())
        try:
            a.save(os.path.join(d, "a.pk"))
            b.save(os.path.join(d, "b.pk"))
            with open(os.path.join(d, "a.pk"), "rb") as fa, open(os.path.join(d, "b.pk"), "rb") as fb:
                return fa.read() == fb.read()
        finally:
            shutil.rmtree(d, ignore_errors=True)

    def file_reads(self, rs):
        return rs.file_reads()

    def filter_set(self, rs, l, n, e, m_per_file):
        """The selection `filter_reads -l l [-n n] -e e [-m m_per_file]` makes in every file of the resident set (n < 0: no -n,
        m_per_file < 0: no -m), on the device (commet_readset_filter) -> (set-wide bits, per-file counters)"""
        return rs.filter(min_len=l, max_n=None if n < 0 else n, min_shannon=e, max_reads=None if m_per_file < 0 else m_per_file)

    def release(self, rs):
        rs.close()

    # a set leaves the device and comes back (--set-budget-gb: commet_readset_offload / _restore)
    def packed_bytes(self, files):
        """bytes the set of these files holds on the device when resident, from a count of their records on the host"""
        return self._api.files_packed_bytes(files)[2]

    def set_bytes(self, rs):
        return rs.packed_bytes

    def offload(self, rs):
        rs.offload()

    def restore(self, rs):
        rs.restore()

    def index_and_search(self, index, searches, isel, ssels):
        return self.ctx.index_and_search(index, searches, isel, ssels)

    def index_many_and_search(self, indexes, search, isels, ssel):
        return self.ctx.index_many_and_search(indexes, search, isels, ssel)

    # the threshold sweep (matrix_sweep.py): tags of every t and per-file counts, made on the device
    def index_and_thresholds(self, index, searches, isel, ssels, max_t):
        return self.ctx.index_and_thresholds(index, searches, isel, ssels, max_t)

    def index_many_and_thresholds(self, indexes, search, isels, ssel, ts):
        return self.ctx.index_many_and_thresholds(indexes, search, isels, ssel, ts)

    def list_estimate(self, rs):
        return rs.cache_estimate()

    def reserve_list(self, rs):
        rs.reserve_cache()

    def device_total(self):
        return self.ctx.device_memory()[1]

    def alloc_stats(self):
        """what this run has asked the DRIVER for so far (commet_device_alloc_stats; blocks reused from the library's own cache do
        not count): host ms inside hipMalloc, bytes, calls — a box that charges a process for its first use of device memory
        (15-30 ms per GiB on some of the pool's) shows here, between the kernels, not in any kernel's time"""
        now = self._api.device_alloc_stats(-1)
        return {f: now[f] - self._alloc0[f] for f in now}

    def kernel_times(self):
        """COMMET_MATRIX_KERNEL_TIMES=1: {kernel: [launches, ms]} of this rank's jobs (a hipEvent pair around every launch; the chunks
        of a group are then built one after the other, so the figures add up but the run is a little slower) — else None"""
        return {k: [c, round(ms, 3)] for k, (c, ms) in self.ctx.kernel_times().items()} if self._kernel_times else None

    def synchronize(self):
        self.ctx.synchronize()

    def close(self):
        self.ctx.close()

    def mismatch_error(self, msg):
        return self._api.CommetError(msg)


def _scratch_root():
    root = os.environ.get("COMMET_SCRATCH")
    if root:
        return root
    return "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()


# ---- the filter step (Commet.py:103-121) ----------------------------------------------------------------
class Filters:
    """The filter vectors of the sets, for both drivers: which way they come about (given in the set file / all ones / made on the
    device / one filter_reads per file), the per-set cache of the device's selections, the seconds the step took (`seconds`).
    leave(s, rs) writes the .bv files of a set this rank has parsed; selection(s, rs) is what the jobs need of set s."""

    def __init__(self, files, bvs, out_dir, bin_dir, l, n, e, m, eng):
        self.files, self.bin_dir, self.l, self.n, self.e, self.m, self.eng = files, bin_dir, l, n, e, m, eng
        tool = os.environ.get("COMMET_MATRIX_FILTER_TOOL", "0") == "1"
        self.given = bvs is not None
        # Commet.py's default options (-l 0 -e 0, no -n, no -m) remove no read: the filter vectors are then all ones over each file's
        # reads and are written from the parser's record counts by the set's owner (default_filter_bv: the tool's bytes, tested), every
        # rank derives the same selection from the counts of the set it holds — no second pass over the files, nothing to wait for.
        # COMMET_MATRIX_FILTER_TOOL=1 runs filter_reads all the same.
        self.synth = not self.given and l == 0 and e == 0 and n < 0 and m < 0 and not tool
        # Any other options: every read's length and base counts are in the resident set's planes, so the selection is made on the device
        # from the copy each rank holds (filter_set: commet_readset_filter, the tool's bits) — no filter_reads process re-reads the text,
        # nothing to wait for; the set's owner leaves the tool's .bv files.  Engines without filter_set and COMMET_MATRIX_FILTER_TOOL=1
        # run filter_reads as before.
        self.device = not self.given and not self.synth and not tool and hasattr(eng, "filter_set")
        self.tool = not (self.given or self.synth or self.device)
        self.bvs = bvs if self.given else [[out_dir + os.path.basename(f) + ".bv" for f in fl] for fl in files]
        self.seconds = 0.0
        self.device_sel = {}                                      # set -> its per-file (count, bits), made on the device
        self.pool, self.jobs, self.err = None, [], []             # the filter_reads processes of this rank; what one of them raised
        self.t0 = self.end = time.perf_counter()
        self.wait = None

    def start_tool(self, owned, ranks, say, wait=None):
        """One filter_reads per file of the sets in `owned` (the set's parser filters its files, too: one producer per set):
        independent processes (each one multi-threaded over its file), a few at a time — and beside the parsing of the sets.  A
        filter's .bv is written under another name and renamed into place, so the file appears complete or not at all: whoever needs
        set s (any rank) waits for ITS files only (selection), not for every filter of the node — `wait` = (stop_ev, prof) of a
        driver that loads beside them; one that calls done() before it loads passes none."""
        self.t0 = self.end = time.perf_counter()
        cmds = []
        for s in owned:
            for f, b in zip(self.files[s], self.bvs[s]):
                cmds.append(filter_command(self.bin_dir, f, b, self.l, self.n, self.e, self.m, len(self.files[s])))
                say("Filtering command: " + " ".join(cmds[-1]))
        for c in cmds:                                             # what an earlier run left in this directory must not be read as this run's
            for stale in (c[-1], c[-1] + ".part"):
                try:
                    os.remove(stale)
                except OSError:
                    pass
        ranks.barrier()                                            # (every rank's stale files are gone before anybody looks for new ones)
        self.ranks, self.wait = ranks, wait
        self.pool = ThreadPoolExecutor(max_workers=int(os.environ.get("COMMET_FILTER_JOBS", "3")))
        # (the sets are loaded last set first: so are their filters)
        self.jobs = [self.pool.submit(self._run_tool, c) for c in reversed(cmds)]
        for j in self.jobs:
            j.add_done_callback(self._tool_over)

    @staticmethod
    def _run_tool(cmd):
        subprocess.run(cmd[:-1] + [cmd[-1] + ".part"], check=True, stdout=subprocess.DEVNULL)
        os.rename(cmd[-1] + ".part", cmd[-1])

    def _tool_over(self, f):
        self.end = max(self.end, time.perf_counter())             # when the last of them was done
        if not f.cancelled() and f.exception() is not None:
            self.err.append(f.exception())                        # whoever waits for a set is told at once

    def done(self):
        """this rank's filter processes are through (raises what a filter_reads process raised)"""
        if self.pool is not None:
            try:
                for j in self.jobs:
                    j.result()
            finally:
                self.pool.shutdown(wait=True)
            self.seconds = (self.end if self.jobs else time.perf_counter()) - self.t0

    def shutdown(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)

    def _device(self, s, rs):
        """the selection of set s from the resident copy this rank holds; the per-file cap is what the tool's atoi makes of the
        `-m` the driver passes it (str(m / files of the set))"""
        if s not in self.device_sel:
            w0 = time.perf_counter()
            bits, _ = self.eng.filter_set(rs, self.l, self.n, self.e, c_atoi(str(self.m / len(self.files[s]))) if self.m >= 0 else -1)
            cs = self.eng.file_reads(rs)
            self.device_sel[s] = list(zip(cs, split_bits(bits, cs)))
            self.seconds += time.perf_counter() - w0
        return self.device_sel[s]

    def leave(self, s, rs):
        """the filter files of a set this rank has just parsed: from its record counts (default options), or the device's selection"""
        if self.synth:
            for c_, f_, b_ in zip(self.eng.file_reads(rs), self.files[s], self.bvs[s]):
                default_filter_bv(b_, f_, c_)
        elif self.device:
            parts = self._device(s, rs)
            w0 = time.perf_counter()
            for (c_, bits_), f_, b_ in zip(parts, self.files[s], self.bvs[s]):
                write_filter_bv(b_, f_, c_, bits_, self.l, self.n, self.e)
            self.seconds += time.perf_counter() - w0

    def selection(self, s, rs):
        """set s is resident; once its filter files are there (written by whichever rank filtered them): its per-file read counts,
        the number of reads it was asked about (the matrix's diagonal), its input selection -> (counts, considered, sel);
        None: this rank is stopping"""
        counts = self.eng.file_reads(rs)
        if self.wait is not None:
            for b in self.bvs[s]:
                if not wait_file(b, f"the filter of set {s}", os.path.dirname(b), self.wait[0], self.err, self.ranks, self.wait[1]):
                    return None
        if self.synth:                                            # all ones (the set's owner has left the files: leave)
            parts = [(c, default_filter_bv(None, f, c)) for c, f in zip(counts, self.files[s])]
        elif self.device:                                         # from the copy this rank holds (its owner has left the files, too)
            parts = self._device(s, rs)
        else:
            parts = [read_bv(b) for b in self.bvs[s]]
        considered = sum(popcount(b, nb) for nb, b in parts)
        for (nb, _), c, f in zip(parts, counts, self.files[s]):
            if nb != c:
                raise self.eng.mismatch_error(f"Number of reads in {f} and boolean vector size are not equal -> quit")
        _, sel = concat_bits(parts)
        if considered == sum(counts) and os.environ.get("COMMET_MATRIX_KEEP_SEL", "0") != "1":
            sel = None                                            # every read selected (the default filters): no bitmap to upload, dense plans
        return counts, considered, sel


# ---- the jobs of a rank: library calls, the files they leave, what they add to the matrix --------------------------
class Jobs:
    """Runs jobs on resident sets (sets, sel, counts, considered: filled by the loader as the sets arrive) and leaves their files.
    shared: (from set, in set) -> reads of `from` found in `in`.  Which job runs when is the driver's business."""

    def __init__(self, eng, sets, sel, counts, considered, prof, names, files, out_dir):
        self.eng, self.sets, self.sel, self.counts, self.considered, self.prof = eng, sets, sel, counts, considered, prof
        self.names, self.files, self.out_dir = names, files, out_dir
        self.shared = {}
        self.reads_searched = 0
        self.call_log = os.environ.get("COMMET_MATRIX_CALL_LOG")   # one line per library call: jobs, wall, event-timed device time, python clock
        self.job_log = prof.setdefault("job_log", [])   # one row per library call: [kind, search set or reference, [the other sets], index ms, search ms, call ms]
        #                                                 (what tools/schedule_sim.py replays on the pair cut of N ranks)
        # the .bv and .log files of a job are written by two helper threads while the next job runs (6 MB per 50 M-read file: 3-4 ms
        # of a job's ~6 ms of host time at configs[3]); all of them are on disk before the jobs' clock stops
        self.writer, self.written = ThreadPoolExecutor(2), []

    def acc(self, inf, n=1, what=None):
        prof = self.prof
        prof["jobs"] += n
        prof["call_ms"] += inf["total_ms"]
        prof["device_ms"] += inf["index_ms"] + inf["search_ms"]
        if what is not None:
            self.job_log.append([what[0], what[1], list(what[2]), round(inf["index_ms"], 3), round(inf["search_ms"], 3), round(inf["total_ms"], 3)])
        if self.call_log:
            with open(self.call_log, "a") as fh:
                fh.write(f"{prof['rank']} {n} {inf['total_ms']:.3f} {inf['index_ms']:.3f} {inf['search_ms']:.3f} {time.perf_counter():.6f}\n")

    def on_one_search_set(self, index_ids, search_id, selections, kind="J2"):
        """Jobs that search the SAME set — the J2 jobs of a reference set, the J3 jobs of a target (Commet.py:220, 233) — in one call
        where the engine has one (commet_index_many_and_search: their chunk filters share passes over the search set: the lane-a
        gathers of its reads, two thirds of such a job's memory requests, are made once per pass instead of once per job);
        -> [(tags, stats, index_ms)] in the jobs' order, bit for bit what the jobs give one by one."""
        eng, sets, sel = self.eng, self.sets, self.sel
        if not index_ids:
            return []
        if hasattr(eng, "index_many_and_search") and len(index_ids) > 1:
            tags, st, inf = eng.index_many_and_search([sets[x] for x in index_ids], sets[search_id], selections, sel[search_id])
            self.acc(inf, len(index_ids), (kind, search_id, index_ids))
            return [(tags[j], st[j], inf["index_ms"] / len(index_ids)) for j in range(len(index_ids))]
        out = []
        for x, sl in zip(index_ids, selections):
            tags, st, inf = eng.index_and_search(sets[x], [sets[search_id]], sl, [sel[search_id]])
            self.acc(inf, 1, (kind, search_id, [x]))
            out.append((tags[0], st[0], inf["index_ms"]))
        return out

    def j1(self, ref, targets):
        """J1 of a reference set: its index built once for all these targets -> the tags of each target"""
        sets, sel = self.sets, self.sel
        tags, _st, inf = self.eng.index_and_search(sets[ref], [sets[i] for i in targets], sel[ref], [sel[i] for i in targets])
        self.prof["j1_builds"] += 1
        self.reads_searched += sum(self.considered[i] for i in targets)
        self.acc(inf, 1, ("J1", ref, targets))
        return tags

    def leave(self, search, index, tags, st, index_ms, w0):
        """the files of one J2 / J3 job: <file of `search`>_in_<index>.bv, <search>_in_<index>.log; its entry of the matrix"""
        names, out_dir = self.names, self.out_dir
        for f, c, b in zip(self.files[search], self.counts[search], split_bits(tags, self.counts[search])):
            self.written.append(self.writer.submit(write_bv, out_dir + os.path.basename(f) + "_in_" + names[index] + ".bv", f + " in " + names[index], c, b))
        self.written.append(self.writer.submit(_log, out_dir, names[search], names[index], st, index_ms, time.perf_counter() - w0))
        self.shared[(search, index)] = st["shared"]
        self.reads_searched += self.considered[search]

    def finish(self):
        """every job is through and every file on disk (what a writer raised is raised here) -> the clock's reading then;
        the rank's allocation figures and, where they were asked for, its kernel times go into the profile"""
        eng, prof = self.eng, self.prof
        eng.synchronize()
        for f in self.written:
            f.result()
        self.writer.shutdown()
        end = time.perf_counter()
        if hasattr(eng, "alloc_stats"):
            a_ = eng.alloc_stats()
            prof["alloc_wait_ms"], prof["fresh_device_bytes"], prof["alloc_calls"] = round(a_["wait_ms"], 1), a_["fresh_bytes"], a_["calls"]
        if hasattr(eng, "kernel_times") and eng.kernel_times() is not None:
            prof["kernel_ms"] = eng.kernel_times()
        return end

    def cancel(self):
        """a failing run: what has not been written yet is not waited for"""
        self.writer.shutdown(wait=False, cancel_futures=True)


# ---- residency without a budget: parse my sets once, publish them, take the others I need ---------------------------------
class Loader:
    """Makes the sets of this rank's pairs resident and fills sets / counts / sel / considered: everything first (load_first), or on
    a second thread in the order the jobs want them while the job thread runs them (start; wait_for, there, wait_any are the job
    thread's side of it)."""

    def __init__(self, eng, cfg, cut, filters, hand, ranks, prof, stop_ev):
        self.eng, self.files, self.note, self.cut, self.filters, self.hand, self.ranks, self.prof = eng, cfg.files, cfg.note, cut, filters, hand, ranks, prof
        self.sets, self.counts, self.sel, self.considered = {}, {}, {}, {}
        self.stop_ev = stop_ev                                    # set when this rank is through (or has failed): ends every wait
        self.jobs_done = threading.Event()
        self.thread, self.ready, self.order, self.own_first, self.solo = None, None, [], [], False
        self.err = []                                             # what the loading thread raised: handed to the job thread
        self.t0 = self.load_end = time.perf_counter()
        self.loaded_all = False
        self.set_wait = 0.0

    def parse(self, s):
        w0 = time.perf_counter()
        rs = self.eng.parse(self.files[s])
        self.prof["parse_s"] += time.perf_counter() - w0
        self.prof.setdefault("parse_log", []).append([s, round(time.perf_counter() - w0, 4)])
        self.prof["sets_parsed"] += 1
        self.filters.leave(s, rs)
        return rs

    def parse_own(self, s):
        """one of this rank's sets: parsed here and nowhere else; published for the ranks that need it"""
        rs = self.parse(s)
        if s in self.cut.needed_by_others:
            self.hand.publish(s, rs)
        if s in self.cut.needed:
            self.sets[s] = rs
        elif self.hand is None or s not in self.hand.exported:
            self.eng.release(rs)

    def fetch(self, s):
        rs = self.hand.fetch(s)
        if rs is not None:
            self.sets[s] = rs
        return rs is not None

    def prepare(self, s):
        got = self.filters.selection(s, self.sets[s])
        if got is not None:
            self.counts[s], self.considered[s], self.sel[s] = got
        return got is not None

    def load_first(self):
        """COMMET_MATRIX_PIPELINE=0: every set resident before the first job"""
        cut = self.cut
        for s in cut.owned:
            if s in cut.needed or s in cut.needed_by_others:
                self.parse_own(s)
        self.ranks.barrier()                                      # every image is in place
        for s in cut.needed:
            if s not in self.sets:
                self.fetch(s)                                     # (its owner's descriptor / image is in place behind the barrier)
        for s in cut.needed:
            self.prepare(s)
        self.load_end = time.perf_counter()

    def start(self, refs):
        """A second host thread makes the sets resident in the order the jobs want them (read sets are made on a stream
        of their own, include/commet_hip.h) while this one runs the jobs of a reference set as soon as it and its
        targets are there: the host-bound loading hides behind the device-bound jobs.  One rank: the thread parses
        the files, last set first, and ref = N-2, N-3, ... need the sets ref .. N-1.  Several ranks: the thread parses
        this rank's own sets and publishes them, then takes the others' as they appear (no barrier in between)."""
        cut, N = self.cut, len(self.files)
        self.ready = [threading.Event() for _ in range(N)]
        self.solo = cut.world == 1                                # (then the loading thread parses, too)
        if self.solo:
            self.order = list(range(N - 1, -1, -1))
        else:
            for ref in refs:
                for s in [ref] + [i for (r, i) in cut.mine if r == ref]:
                    if s not in self.order:
                        self.order.append(s)
            # Several ranks: nobody waits at a barrier for every set of the node to be parsed.  This rank parses its own
            # sets first — the ones most ranks wait for first — and publishes their images; then it takes the other
            # ranks' images, in the order its jobs want them, as soon as each file appears.  Its first job starts when
            # the two sets of that job are there, whatever the other ranks are still parsing.
            wanted_by = {s_: sum(1 for r in range(cut.world) if any(s_ in cut.pairs[c] for c in cut.runs[r])) for s_ in cut.owned}
            self.own_first = sorted((s_ for s_ in cut.owned if s_ in cut.needed or s_ in cut.needed_by_others), key=lambda s_: (-wanted_by[s_], s_))
            # (simulated and NOT adopted in round 6: parsing first the sets some rank cannot start without — in every pair of its run —
            # helps the ranks that wait for those and delays the one with the longest run: configs[3] at eight ranks 2.50 against 2.58 s
            # with one run's fitted costs, 2.65 against 2.53 s with another's: tools/schedule_sim.py, blocking_first)
        self.thread = threading.Thread(target=self.load_all, name="commet-set-loader", daemon=True)
        self.thread.start()

    def reserve_lists(self):
        """COMMET_MATRIX_LARGE_LISTS=1 (off by default): query lists above the library's cap (a 50 M-read set's is 11 GB; it saves
        ~12 ms of every J2 / J3 job that searches the set) for the sets this rank searches three times or more; their memory is asked
        from the driver HERE, by the loader thread once every set is resident, and a set whose memory waits in the library's device
        cache gets its list at its next eligible scan but one.  Measured on configs[3] (profiles/r05_large_lists): 11.0 s against
        11.8 s on a box whose device memory had been used before (the driver's 110 GiB take no time there), 13.4 s on a fresh box —
        there hipMalloc costs 15-30 ms per GiB (3.4 s), and while one thread is inside hipMalloc the HIP calls of every other thread
        of the process wait, so the job thread stands still with it.  Hence opt-in: for long-lived hosts."""
        eng, sets = self.eng, self.sets
        if os.environ.get("COMMET_MATRIX_LARGE_LISTS", "0") != "1" or not hasattr(eng, "list_estimate"):
            return
        scans = {}
        for (r_, i_) in self.cut.mine:                            # J2 searches the reference set, J3 the target (Commet.py:220, 233)
            scans[r_] = scans.get(r_, 0) + 1
            scans[i_] = scans.get(i_, 0) + 1
        want = [s_ for s_ in sorted(scans, key=lambda s_: -scans[s_]) if scans[s_] >= 3 and s_ in sets]
        est = {s_: eng.list_estimate(sets[s_]) for s_ in want}
        want = [s_ for s_ in want if est[s_] > (4 << 30)]          # (smaller lists are the library's default already)
        budget = 0.4 * eng.device_total()
        got = 0
        for s_ in want:
            if self.stop_ev.is_set() or self.jobs_done.is_set() or sum(est[x] for x in want[:want.index(s_) + 1]) > budget:
                break
            eng.reserve_list(sets[s_])
            got += 1
        self.prof["lists_reserved"] = got
        if got:
            self.note(f"memory of {got} large query lists set aside ({sum(est[x] for x in want[:got]) / 2**30:.0f} GiB)")

    def load_all(self):
        try:
            for s in self.own_first:
                if self.stop_ev.is_set():
                    return
                self.parse_own(s)
            for s in self.order:
                if self.stop_ev.is_set():                         # the job thread has failed
                    break
                if self.solo:
                    self.sets[s] = self.parse(s)
                elif s not in self.sets and not self.fetch(s):
                    break
                if not self.prepare(s):
                    break
                self.ready[s].set()
                self.note(f"set {s} resident")
            self.load_end = time.perf_counter()
            self.loaded_all = True
            self.reserve_lists()
        except BaseException as ex:          # handed to the job thread, which is waiting for a set
            self.err.append(ex)
            for ev in self.ready:
                ev.set()
        finally:
            if not self.loaded_all:
                self.load_end = time.perf_counter()

    def there(self, s):
        return self.thread is None or self.ready[s].is_set()

    def _wait(self, there, every):
        """the job thread waits for the loading thread; errors of the filters / the loader / another rank end the wait"""
        w0 = time.perf_counter()
        polls = 0
        while not there():
            if self.filters.err:                                  # a filter_reads process of this rank failed
                raise self.filters.err[0]
            if self.err:
                raise self.err[0]
            polls += 1
            if self.cut.world > 1 and polls % every == 0 and hasattr(self.ranks, "check"):
                self.ranks.check()                                # (has a rank given up?  Its sets will never come)
        self.set_wait += time.perf_counter() - w0
        if self.err:
            raise self.err[0]

    def wait_for(self, s):
        """set s is resident (raises what the loader raised, if it did)"""
        if self.thread is not None:
            self._wait(lambda: self.ready[s].wait(0.05), 5)

    def wait_any(self, left):
        """nothing can start: until some reference set of `left` is there with one of its targets"""
        self._wait(lambda: any(self.there(r_) and any(self.there(i) for i in left[r_]) for r_ in left) or time.sleep(0.002), 125)

    def finish(self):
        """every set is loaded (one rank: a set no pair needs is still loaded and counted) -> seconds the loading took"""
        if self.thread is not None:
            for s in self.order:
                self.wait_for(s)
            self.thread.join()
        return self.load_end - self.t0

    def join(self, failed):
        """-> the loading thread is stuck in a HIP call that does not return: the process is on its way out"""
        if self.thread is not None and self.thread.is_alive():    # (an error in the job thread)
            self.thread.join(timeout=5.0 if failed else None)
        return self.thread is not None and self.thread.is_alive()


# ---- what both drivers begin and end with ---------------------------------------------------------------------------------
def _setup(input_file, out_dir, k, t, l, bin_dir, rank, verbose, progress):
    if out_dir[-1] != "/":
        out_dir += "/"
    os.makedirs(out_dir, exist_ok=True)
    names, files, bvs = parse_set_file(input_file)
    if l < k * t and l != 0:                                      # Commet.py:509-513 (l stays 0 by default)
        l = k * t
    return SimpleNamespace(out_dir=out_dir, bin_dir=bin_dir or os.path.join(HERE, "bin"), names=names, files=files, bvs=bvs, N=len(names), l=l,
                           say=print if (verbose and rank == 0) else (lambda *a, **kw: None),
                           note=progress if progress is not None else (lambda msg: None))


def _profile(rank, pairs, handover, ranks, share):
    return dict(rank=rank, pairs=pairs, sets_parsed=0, sets_loaded=0, j1_builds=0, parse_s=0.0, save_s=0.0, load_s=0.0,
                jobs=0, call_ms=0.0, device_ms=0.0, handover=handover, backend=getattr(ranks, "backend", None),
                torch_loaded="torch" in sys.modules, predicted_share=share)


def _matrices(cfg, everyone):
    """the three matrices from every rank's (shared, profile, considered) -> the head of the report"""
    N = cfg.N
    mat = [[0] * N for _ in range(N)]
    diag = {}
    for d, _, cons in everyone:
        diag.update(cons)                                         # (every set is in some rank's pairs)
        for (a, b), v in d.items():
            mat[a][b] = v
    considered_all = [diag[s] for s in range(N)]
    for s in range(N):
        mat[s][s] = considered_all[s]
    write_matrices(cfg.out_dir, cfg.names, considered_all, mat)
    cfg.say("All Commet work is done")
    cfg.say("\t Output csv matrices are in:")
    for f in ("matrix_plain.csv", "matrix_percentage.csv", "matrix_normalized.csv"):
        cfg.say("\t\t" + cfg.out_dir + f)
    return dict(names=cfg.names, considered=considered_all, matrix=mat)


def _report(result, everyone, filter_s, load_s, filter_overlaps_load, load_overlaps_jobs, jobs_s, total_s, searched, world):
    """the times and rates of a run, in the report of rank 0
    (the filter processes run beside the parsing: filter_s and load_s overlap, total_s is the wall time of it all)"""
    prof = everyone[0][1]
    result.update(filter_s=filter_s, load_s=load_s, filter_overlaps_load=filter_overlaps_load, load_overlaps_jobs=load_overlaps_jobs,
                  set_wait_s=prof.get("set_wait_s", 0.0), jobs_s=jobs_s, total_s=total_s, reads_searched=searched, world=world,
                  rank0_profile=prof, per_rank=[p for _, p, _c in everyone],
                  reads_per_s=searched / jobs_s if jobs_s > 0 else 0.0,
                  reads_per_s_incl_load_and_filter=searched / total_s if total_s > 0 else 0.0)
    return result


def run(input_file, out_dir, k=33, t=2, l=0, n=-1, e=0.0, m=-1, bin_dir=None, ranks=None, verbose=True,
        engine_factory=None, progress=None, fatal_hook=None, set_budget_gb=None):
    """set_budget_gb (also COMMET_MATRIX_SET_BUDGET_GB, --set-budget-gb; fractions allowed): the most device memory the packed sets may
    hold together, in GiB — sets leave the device and come back as residency.plan says (one rank only); None: every set stays resident.
    progress: optional callable(str), called on every rank at the stages of the run (a caller that keeps stdout for itself —
    bench.py — shows a long run is alive with it).
    fatal_hook: optional callable(str), called from a watchdog thread right before this process is ended with os._exit because a
    HIP call of it does not return (an import of another rank's set): the caller's last chance to say what it has to say"""
    t_start = time.perf_counter()
    own_ranks = ranks is None
    if ranks is None:
        ranks = sharding.Ranks()
    if set_budget_gb is None and os.environ.get("COMMET_MATRIX_SET_BUDGET_GB"):
        set_budget_gb = float(os.environ["COMMET_MATRIX_SET_BUDGET_GB"])
    if set_budget_gb is not None and ranks.world > 1:
        raise ValueError(f"--set-budget-gb with {ranks.world} ranks: a set budget is kept by one rank only (run without --gpus / a launcher, "
                         "or without the budget)")
    try:
        cfg = _setup(input_file, out_dir, k, t, l, bin_dir, ranks.rank, verbose, progress)
        make_engine = engine_factory or HipEngine
        if set_budget_gb is not None:
            return _run_under_budget(cfg, k, t, n, e, m, ranks, make_engine, int(float(set_budget_gb) * (1 << 30)), t_start)
        return _run_resident(cfg, k, t, n, e, m, ranks, make_engine, fatal_hook, t_start)
    finally:
        if own_ranks and sys.exc_info()[0] is None:
            ranks.close()


# ---- every set resident: the pairs of a rank, grouped by reference set ---------------------------------------------------------
def _cut(files, world, rank):
    """who does what: pairs in contiguous runs of equal cost, every set parsed by one rank (sharding.assign_owners)"""
    N = len(files)
    pairs = [(ref, i) for ref in range(N - 1) for i in range(ref + 1, N)]
    size = [float(sum(os.path.getsize(f) for f in fl)) for fl in files]   # cost proxy known before any parsing
    pair_cost = [size[a] + size[b] for a, b in pairs]
    runs = sharding.assign_pairs_contiguous(pair_cost, world)
    mine = [pairs[c] for c in runs[rank]]
    owner = sharding.assign_owners(N, world, [sum(pair_cost[c] for c in runs[r]) for r in range(world)])
    return SimpleNamespace(world=world, pairs=pairs, runs=runs, mine=mine, owner=owner, needed=sorted({s for p in mine for s in p}),
                           owned=[s for s in range(N) if owner[s] == rank],
                           needed_by_others={s for r in range(world) if r != rank for c in runs[r] for s in pairs[c]},
                           # what the static cut expects of this rank
                           share=round(sum(pair_cost[c] for c in runs[rank]) / max(sum(pair_cost), 1e-9), 4))


def _foreign(cut, r):
    """the sets rank r takes from others"""
    return sorted({s for c in cut.runs[r] for s in cut.pairs[c] if cut.owner[s] != r})


def _schedule(cut, refs, loader, jobs, note):
    """Order of a rank's jobs: per reference set J1 (its index built once for all its targets), then the J2 jobs of its targets
    together (they all search S_ref); the J3 jobs — (ref, i) searches S_i — are kept back and run target by target at the end, so
    that the J3 jobs of a target share passes as well.  The files a job writes do not depend on when it runs."""
    mine, prof = cut.mine, jobs.prof
    kept_T2 = {}                   # (ref, i) -> J2's result, the index selection of J3(ref, i); freed as J3 consumes it
    refs_left = {}                 # target -> reference sets of this rank's pairs that have not been through J2 yet
    for (r_, i_) in mine:
        refs_left[i_] = refs_left.get(i_, 0) + 1

    def j3_of(i):
        """J3 of every pair of target i: S_i in (S_ref restricted to J2's result) — overwrites J1's <F>_in_<S_ref>.bv (Commet.py:233)"""
        w0 = time.perf_counter()
        loader.wait_for(i)
        of_i = [r for (r, t_) in mine if t_ == i]
        for ref, (T3, st3, index_ms) in zip(of_i, jobs.on_one_search_set(of_i, i, [kept_T2.pop((r, i)) for r in of_i], "J3")):
            jobs.leave(i, ref, T3, st3, index_ms, w0)
        note(f"J3 jobs of set {i} done ({prof['jobs']} so far)")

    # Which reference set next (round 6): the first of the rank's list that is resident TOGETHER with one of its targets — a rank of a
    # node starts on whatever pair has arrived instead of waiting for the first reference set of its list (tools/schedule_sim.py on
    # configs[3]: 2.69 -> 2.53 s at eight ranks, 4.24 -> 3.97 s at four).  A reference set some of whose targets are still on their way
    # is taken up again later (one more index build of S_ref instead of an idle GPU, as before).  One rank, or everything loaded
    # first: the list's own order.
    there = loader.there
    left = {ref: [i for (r, i) in mine if r == ref] for ref in refs}
    while left:
        ref = next((r_ for r_ in refs if r_ in left and there(r_) and any(there(i) for i in left[r_])), None)
        if ref is None:
            loader.wait_any(left)
            continue
        targets = [i for i in left[ref] if there(i)]
        left[ref] = [i for i in left[ref] if i not in targets]
        for s_need in [ref] + targets:
            loader.wait_for(s_need)                                  # (resident: raises what the loader raised, if it did)
        w0 = time.perf_counter()
        tags1 = jobs.j1(ref, targets)
        # J2 of every target: X_i = S_i restricted to (S_i in S_ref); S_ref in X_i
        for i, (T2, st2, index_ms) in zip(targets, jobs.on_one_search_set(targets, ref, list(tags1))):
            jobs.leave(ref, i, T2, st2, index_ms, w0)
            kept_T2[(ref, i)] = T2
        if not left[ref]:
            del left[ref]
            note(f"J1 and J2 jobs of set {ref} done ({prof['jobs']} so far)")
        # The J3 jobs — (ref, i) searches S_i — are kept back so that the J3 jobs of a target share passes as well, but no longer than
        # needed: a target's batch runs as soon as the last of its reference sets on this rank has been through J2 (its J2 bitmaps are
        # freed with it, its files are on disk: a late failure loses little).  The files a job writes do not depend on when it runs.
        for i in targets:
            refs_left[i] -= 1
        for i in sorted(targets):
            if refs_left[i] == 0:
                j3_of(i)
    assert not any(refs_left.values()) and not kept_T2            # (every target's references are in `refs`: no J3 is left over)


def _tell_the_others(ranks, ex):
    """a failing rank of several: tell the others at once (their waits end with an error naming this rank) instead of leaving them
    in a gather until the timeout"""
    if not isinstance(ex, RuntimeError) or "rendezvous" not in str(ex):
        try:                                                      # what this rank ran into may only be the wake of another rank's failure
            ranks.check()                                         # (scratch gone under its feet): then THAT is the error to report
        except RuntimeError as first:
            raise first from ex
    ranks.abort(f"{type(ex).__name__}: {ex}")


def _run_resident(cfg, k, t, n, e, m, ranks, make_engine, fatal_hook, t_start):
    """The matrix with every set of a rank's pairs resident, on one rank or several."""
    world, rank = ranks.world, ranks.rank
    N, say, note = cfg.N, cfg.say, cfg.note
    cut = _cut(cfg.files, world, rank)
    stop_ev = threading.Event()                                   # set when this rank is through (or has failed): ends every wait
    prof = _profile(rank, len(cut.mine), "image", ranks, cut.share)
    # ---- filter step (Commet.py:103-121): one filter_reads per file, run by the rank that parses the set ---------
    eng = make_engine(k, t, ranks.local_rank)
    filters = Filters(cfg.files, cfg.bvs, cfg.out_dir, cfg.bin_dir, cfg.l, n, e, m, eng)
    if filters.tool:
        filters.start_tool(cut.owned, ranks, say, wait=(stop_ev, prof))
    hand = None
    if world > 1:
        # rank 0 makes the directory (mkdtemp: a fresh name, mode 0700 — the scratch root is shared with other users)
        scratch = ranks.broadcast_object(tempfile.mkdtemp(prefix="commet_pk_", dir=_scratch_root()) if rank == 0 else None)
        hand = Handover(eng, ranks, scratch, cut.owned, prof, note, fatal_hook, stop_ev, filters.err)
        if hand.probe(say):
            prof["handover"] = "ipc"
    # sets are made resident by a second thread while the jobs run (COMMET_MATRIX_PIPELINE=0: everything first)
    pipelined = N >= 2 and os.environ.get("COMMET_MATRIX_PIPELINE", "1") != "0"
    note(f"{N} sets, {len(cut.mine)} of {len(cut.pairs)} pairs on this rank; sets are handed over "
         + ("device to device" if prof["handover"] == "ipc" else "as packed images" if world > 1 else "nowhere (one rank)"))
    if hand is not None:
        canary_rank = next((r for r in range(world) if _foreign(cut, r)), None)
        hand.start_canary(canary_rank, _foreign(cut, rank))
    loader = Loader(eng, cfg, cut, filters, hand, ranks, prof, stop_ev)
    try:
        if hand is not None and hand.use_ipc and any(s in cut.needed_by_others for s in cut.owned):
            hand.start_server()
        refs = sorted({p[0] for p in cut.mine}, reverse=pipelined)    # pipelined: last reference set first
        if pipelined:
            loader.start(refs)
        else:
            loader.load_first()
            say(f"loaded {N} sets in {loader.load_end - loader.t0:.2f} s (rank 0: {prof['sets_parsed']} parsed, {prof['sets_loaded']} from packed images)")
        jobs = Jobs(eng, loader.sets, loader.sel, loader.counts, loader.considered, prof, cfg.names, cfg.files, cfg.out_dir)
        t_jobs = time.perf_counter()
        try:
            _schedule(cut, refs, loader, jobs, note)
        except BaseException:
            jobs.cancel()
            raise
        loader.jobs_done.set()                                    # (no list memory is set aside for jobs that are over)
        jobs_s = jobs.finish() - t_jobs - loader.set_wait         # (pipelined: without the waits for sets still being loaded)
        prof["jobs_s"], prof["set_wait_s"] = jobs_s, loader.set_wait
        load_s = loader.finish()
        filters.done()                                            # (this rank's filter processes: what one of them raised is raised here)
        # ---- matrices on rank 0 -----------------------------------------------------------------------------
        everyone = ranks.gather_objects((jobs.shared, prof, loader.considered))   # (every rank is through its jobs: nobody asks for a set any more)
        if hand is not None:
            hand.stop()
        result = _matrices(cfg, everyone) if rank == 0 else None
        slowest = ranks.max_seconds(jobs_s)
        slowest_load = ranks.max_seconds(load_s)
        slowest_filter = ranks.max_seconds(filters.seconds)
        total_searched = ranks.sum_int(jobs.reads_searched)
        total_s = ranks.max_seconds(time.perf_counter() - t_start)
        if result is not None:
            _report(result, everyone, slowest_filter, slowest_load, filters.pool is not None, pipelined, slowest, total_s, total_searched, world)
            say(f"{total_searched} reads searched in {slowest:.3f} s of jobs on {world} GPU(s): {result['reads_per_s'] / 1e6:.1f} M reads/s "
                f"({result['reads_per_s_incl_load_and_filter'] / 1e6:.1f} M reads/s with filter {slowest_filter:.2f} s + load {slowest_load:.2f} s)")
        if hand is not None:
            hand.release_exported(loader.sets)
        for rs in loader.sets.values():
            eng.release(rs)
        return result
    except BaseException as ex:
        if world > 1 and hasattr(ranks, "abort"):
            _tell_the_others(ranks, ex)
        raise
    finally:
        failed = sys.exc_info()[0] is not None
        stop_ev.set()
        if failed and hand is not None:
            hand.linger()
        stuck = loader.join(failed)
        if hand is not None:
            hand.stop()
        filters.shutdown()
        if not stuck:
            eng.close()                                           # (never under a thread that is still inside the library)
        if hand is not None:
            hand.cleanup(failed or getattr(ranks, "failed", False))


# ---- a set budget: the plan's loads and evicts on one thread, its jobs on another --------------------------------------------------
class PlanLoader:
    """The loader thread of a run under a set budget: the plan's "load" and "evict" steps.  It parses a set at its first "load" (its
    filter runs then, while the set is resident), offloads it at an "evict" it will come back from (releases it at its last one) and
    restores it at a later "load" — as far ahead of the job thread as the budget allows, one load past a pending evict at most.
    The job thread waits for a load (wait_load) and says how far it is (advance)."""

    def __init__(self, eng, cfg, filters, steps, sizes, budget_bytes, prof, res, stop):
        self.eng, self.files, self.names, self.note, self.filters = eng, cfg.files, cfg.names, cfg.note, filters
        self.steps, self.sizes, self.budget_bytes, self.prof, self.res, self.stop = steps, sizes, budget_bytes, prof, res, stop
        self.sets, self.counts, self.sel, self.considered = {}, {}, {}, {}
        self.cv = threading.Condition()
        self.done = [False] * len(steps)                          # "load" steps carried out
        self.progress, self.resident, self.err = 0, 0, None       # progress: the job thread is through every step before it
        self.t0 = self.load_end = time.perf_counter()
        self.set_wait = 0.0
        self.last_use = {}
        for idx, st in enumerate(steps):
            for s in ([st[1]] if st[0] in ("load", "evict") else [st[1]] + (list(st[2]) if st[0] == "j1" else [st[2]])):
                self.last_use[s] = idx
        self.thread = threading.Thread(target=self.load_all, name="commet-set-loader", daemon=True)

    def first_load(self, s):
        eng, prof = self.eng, self.prof
        w0 = time.perf_counter()
        rs = eng.parse(self.files[s])
        prof["parse_s"] += time.perf_counter() - w0
        prof["sets_parsed"] += 1
        if hasattr(eng, "set_bytes") and eng.set_bytes(rs) > self.sizes[s]:
            raise RuntimeError(f"set {self.names[s]} holds {eng.set_bytes(rs)} bytes on the device, {self.sizes[s]} were planned")
        self.sets[s] = rs
        self.filters.leave(s, rs)                                 # (while the set is resident, before its first offload)
        self.counts[s], self.considered[s], self.sel[s] = self.filters.selection(s, rs)

    def do_load(self, idx):
        s, res = self.steps[idx][1], self.res
        assert self.resident + self.sizes[s] <= self.budget_bytes
        self.resident += self.sizes[s]                            # (counted before the memory is asked for)
        res["peak_set_bytes"] = max(res["peak_set_bytes"], self.resident)
        if s not in self.sets:
            self.first_load(s)
        else:
            w0 = time.perf_counter()
            self.eng.restore(self.sets[s])
            res["reload_s"] += time.perf_counter() - w0
            res["set_reloads"] += 1
        res["set_loads"] += 1
        self.load_end = time.perf_counter()
        with self.cv:
            self.done[idx] = True
            self.cv.notify_all()
        self.note(f"set {s} resident")

    def load_all(self):
        steps, sizes, cv = self.steps, self.sizes, self.cv
        try:
            for idx, st in enumerate(steps):
                if self.stop.is_set():
                    return
                if st[0] == "load" and not self.done[idx]:
                    self.do_load(idx)
                elif st[0] == "evict":
                    s = st[1]
                    while True:
                        with cv:
                            if self.progress >= idx or self.stop.is_set():
                                break
                            nxt = idx + 1                         # one load ahead of the evict, where the budget has the room
                            ahead = (nxt < len(steps) and steps[nxt][0] == "load" and not self.done[nxt]
                                     and self.resident + sizes[steps[nxt][1]] <= self.budget_bytes)
                            if not ahead:
                                cv.wait(0.05)
                                continue
                        self.do_load(nxt)
                    if self.stop.is_set():
                        return
                    if self.last_use[s] > idx:
                        self.eng.offload(self.sets[s])
                        self.res["set_offloads"] += 1
                    else:
                        self.eng.release(self.sets.pop(s))
                    self.resident -= sizes[s]
        except BaseException as ex:
            with cv:
                self.err = ex
                cv.notify_all()

    def wait_load(self, p):
        """the job thread: step p, a load, is carried out (raises what the loader raised)"""
        w0 = time.perf_counter()
        with self.cv:
            while not self.done[p] and self.err is None:
                self.cv.wait(0.05)
            if self.err is not None:
                raise self.err
        self.set_wait += time.perf_counter() - w0

    def advance(self, p):
        with self.cv:
            self.progress = p
            self.cv.notify_all()

    def join(self, failed):
        """-> the thread is stuck inside the library"""
        if self.thread.is_alive():
            self.thread.join(timeout=5.0 if failed else None)
        return self.thread.is_alive()


def _plan_jobs(steps, loader, jobs):
    """the job thread of a run under a set budget: the plan's jobs, in its order"""
    sel, considered, prof = jobs.sel, jobs.considered, jobs.prof
    T1 = {}                                                       # (ref, i) -> J1's tags of S_i, until the pair's J2 takes them
    p = 0
    while p < len(steps):
        st = steps[p]
        if st[0] == "load":
            loader.wait_load(p)
            p += 1
        elif st[0] == "evict":
            p += 1
        elif st[0] == "j1":
            _, ref, targets = st
            q = p + 1                                             # J1 of several reference sets against ONE streamed target: they all search it
            while len(targets) == 1 and q < len(steps) and steps[q][0] == "j1" and steps[q][2] == targets:
                q += 1
            if q - p > 1:
                i, of_i = targets[0], [r_ for _, r_, _t in steps[p:q]]
                for r_, (tg, _st1, _ms) in zip(of_i, jobs.on_one_search_set(of_i, i, [sel[r_] for r_ in of_i], "J1")):
                    T1[(r_, i)] = tg
                prof["j1_builds"] += len(of_i)
                jobs.reads_searched += considered[i] * len(of_i)
            else:
                for i, tg in zip(targets, jobs.j1(ref, targets)):
                    T1[(ref, i)] = tg
            p = q
        else:
            q = p
            while q < len(steps) and steps[q][0] == "pair":
                q += 1
            run_ = [(r_, i_) for _, r_, i_ in steps[p:q]]
            w0 = time.perf_counter()
            T2 = {}
            a = 0
            while a < len(run_):                                  # J2: consecutive pairs of one reference set search it together
                b = a
                while b < len(run_) and run_[b][0] == run_[a][0]:
                    b += 1
                ref, targets = run_[a][0], [i_ for _, i_ in run_[a:b]]
                for i, (tg, st2, index_ms) in zip(targets, jobs.on_one_search_set(targets, ref, [T1.pop((ref, i)) for i in targets], "J2")):
                    jobs.leave(ref, i, tg, st2, index_ms, w0)
                    T2[(ref, i)] = tg
                a = b
            for i in dict.fromkeys(i_ for _, i_ in run_):         # J3: the pairs of one target search it together
                of_i = [r_ for r_, i_ in run_ if i_ == i]
                for ref, (tg, st3, index_ms) in zip(of_i, jobs.on_one_search_set(of_i, i, [T2.pop((r_, i)) for r_ in of_i], "J3")):
                    jobs.leave(i, ref, tg, st3, index_ms, w0)
            p = q
        loader.advance(p)


def _run_under_budget(cfg, k, t, n, e, m, ranks, make_engine, budget_bytes, t_start):
    """The matrix of one rank when the packed sets may hold at most budget_bytes of device memory together (--set-budget-gb).

    The reference runs one job at a time from disk and so finishes whatever N is (Commet.py:186-240); here residency.plan orders the
    pair chains block by block, and two threads follow it: the loader (PlanLoader) and the job thread, which runs the plan's jobs in
    order (_plan_jobs).  J2 jobs that search one reference set and J3 jobs that search one target, their sets loaded together, still
    share passes (Jobs.on_one_search_set).  Every file written is what the unconstrained run writes: a job's result does not
    depend on when it runs, nor on how J1 of its reference set was split (residency.py)."""
    N, names, files, say, note = cfg.N, cfg.names, cfg.files, cfg.say, cfg.note
    eng = make_engine(k, t, ranks.local_rank)
    jobs, loader, filters = None, None, None
    stop = threading.Event()
    try:
        lacking = [a for a in ("packed_bytes", "offload", "restore") if not hasattr(eng, a)]
        if lacking:
            raise RuntimeError(f"a set budget needs an engine whose sets can leave the device and come back: {type(eng).__name__} has no "
                               + " / ".join(lacking))
        # what every set will hold, before any is parsed: the plan needs all of them (HipEngine: a count of the files' records on the
        # host, i.e. every file is read once more than without a budget — its time is reported as set_sizing_s, inside total_s)
        w0 = time.perf_counter()
        sizes = [int(eng.packed_bytes(fl)) for fl in files]
        sizing_s = time.perf_counter() - w0
        try:
            steps = residency.plan(sizes, budget_bytes)           # (raises before any job when two sets cannot meet)
        except ValueError as ex:
            big = sorted(range(N), key=lambda s: (-sizes[s], s))[:2]
            raise ValueError(f"{ex} [{', '.join(names[s] for s in big)}]") from None
        note(f"{N} sets of {sum(sizes) / 2**30:.2f} GiB under a set budget of {budget_bytes / 2**30:.2f} GiB: "
             f"{sum(1 for st in steps if st[0] == 'load')} loads planned")
        # ---- filters (Commet.py:103-121): filter_reads, where it is the way, is through before the first load
        filters = Filters(files, cfg.bvs, cfg.out_dir, cfg.bin_dir, cfg.l, n, e, m, eng)
        if filters.tool:
            filters.start_tool(range(N), ranks, say)
            filters.done()
        prof = _profile(0, N * (N - 1) // 2, "none", ranks, 1.0)
        res = dict(set_budget_bytes=int(budget_bytes), set_sizing_s=sizing_s, set_loads=0, set_reloads=0, set_offloads=0, peak_set_bytes=0, reload_s=0.0)
        loader = PlanLoader(eng, cfg, filters, steps, sizes, budget_bytes, prof, res, stop)
        loader.thread.start()
        jobs = Jobs(eng, loader.sets, loader.sel, loader.counts, loader.considered, prof, names, files, cfg.out_dir)
        t_jobs = time.perf_counter()
        _plan_jobs(steps, loader, jobs)
        jobs_s = jobs.finish() - t_jobs - loader.set_wait
        loader.thread.join()
        if loader.err is not None:
            raise loader.err
        prof["jobs_s"], prof["set_wait_s"] = jobs_s, loader.set_wait
        everyone = [(jobs.shared, prof, loader.considered)]
        res.update(_matrices(cfg, everyone))
        total_s = time.perf_counter() - t_start
        _report(res, everyone, filters.seconds, loader.load_end - loader.t0, False, True, jobs_s, total_s, jobs.reads_searched, 1)
        res.update(j1_builds=prof["j1_builds"], reload_s=round(res["reload_s"], 6))
        say(f"{jobs.reads_searched} reads searched in {jobs_s:.3f} s of jobs; {res['set_loads']} set loads ({res['set_reloads']} reloads, "
            f"{res['reload_s']:.3f} s), at most {res['peak_set_bytes'] / 2**30:.2f} of {budget_bytes / 2**30:.2f} GiB of sets resident")
        for rs in loader.sets.values():
            eng.release(rs)
        return res
    finally:
        stop.set()
        if jobs is not None:
            jobs.cancel()
        if filters is not None:
            filters.shutdown()
        if not (loader is not None and loader.join(sys.exc_info()[0] is not None)):
            eng.close()                                           # (never under a thread that is still inside the library)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Filtering and full N x N intersections of read sets on MI355X GPUs")
    ap.add_argument("input_file")
    ap.add_argument("-b", "--binaries_directory", dest="bin_dir", default=None)
    ap.add_argument("-o", "--output_directory", dest="directory", default="output_commet/")
    ap.add_argument("-k", type=int, default=33)
    ap.add_argument("-t", type=int, default=2)
    ap.add_argument("-l", type=int, default=0)
    ap.add_argument("-n", type=int, default=-1)
    ap.add_argument("-e", type=float, default=0)
    ap.add_argument("-m", type=int, default=-1)
    ap.add_argument("--set-budget-gb", dest="set_budget_gb", type=float, default=None,
                    help="most device memory the packed read sets may hold together, in GiB (fractions allowed): sets leave the device and "
                         "come back so that a matrix larger than the device finishes; one rank only")
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks to start on this node, one per GPU (ignored under a launcher that has set WORLD_SIZE)")
    ap.add_argument("--max-t", dest="max_t", type=int, default=None,
                    help="the matrix at every threshold t in 1..MAX_T from one run (commet_amd.matrix_sweep): OUT/t<t>/ holds what -t t "
                         "writes; one rank, every set resident, -l 0; -t is not used")
    a = ap.parse_args(argv)
    if a.max_t is not None:
        from . import matrix_sweep
        budget = a.set_budget_gb if a.set_budget_gb is not None else os.environ.get("COMMET_MATRIX_SET_BUDGET_GB")
        why = matrix_sweep.refusal(a.max_t, gpus=a.gpus, set_budget_gb=budget, l=a.l, world=int(os.environ.get("WORLD_SIZE", "1")))
        if why:
            ap.error(why)
        try:
            res = matrix_sweep.run(a.input_file, a.directory, k=a.k, max_t=a.max_t, n=a.n, e=a.e, m=a.m, bin_dir=a.bin_dir)
            if os.environ.get("COMMET_MATRIX_REPORT"):
                import json
                with open(os.environ["COMMET_MATRIX_REPORT"], "w") as fh:
                    json.dump(res, fh)
        except BaseException:
            traceback.print_exc()
            sys.stderr.flush()
            os._exit(1)
        return 0
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # this process never touches the GPU: it starts the ranks as plain child processes and leaves with their exit code
        return sharding.spawn_ranks(a.gpus, [sys.executable, "-m", "commet_amd.matrix"] + list(sys.argv[1:] if argv is None else argv))
    try:
        res = run(a.input_file, a.directory, k=a.k, t=a.t, l=a.l, n=a.n, e=a.e, m=a.m, bin_dir=a.bin_dir, set_budget_gb=a.set_budget_gb)
        if res is not None and os.environ.get("COMMET_MATRIX_REPORT"):   # rank 0: times and per-rank profile, as JSON
            import json
            with open(os.environ["COMMET_MATRIX_REPORT"], "w") as fh:
                json.dump({f: v for f, v in res.items() if f != "rank0_profile"}, fh)
    except BaseException:
        # a rank that fails must not leave its peers in a barrier: report and leave at once, skipping the process
        # group's shutdown handshake; torch.distributed.run then terminates the other ranks and exits non-zero
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
