"""How a set parsed by one rank of the N x N driver (commet_amd.matrix) reaches the others: device to device over HIP IPC (the owner
exports its buffers, the others copy them over xGMI: no file, tens of ms for a 50 M-read set) when every rank can import a probe set
of its neighbour and of rank 0; else as a packed image in the scratch directory (0.5 s to write, 0.2 s to read).  Matters with
several ranks only: a run of one rank never makes a Handover.

The files of the scratch directory — `set<s>.ipc`, `set<s>.pk`, `set<s>.want.<rank>`, `canary.ok`, `canary.fail`, `import.lock` — are
what the ranks (and ipc_canary.py) tell each other; every one of them is renamed into place: complete or absent."""
import os
import shutil
import subprocess
import sys
import threading
import time


def wait_file(path, what, where, stop_ev, errors, ranks, prof):
    """a file another rank publishes (renamed into place: complete or absent): there once its owner has got that far
    (or never, if that rank died: the launcher then ends this process; the deadline only bounds a stray wait).
    False: stop_ev was set, this rank is stopping; what a filter process raised (errors) is raised here"""
    deadline = time.perf_counter() + float(os.environ.get("COMMET_DIST_TIMEOUT_S", "600"))
    w0 = time.perf_counter()
    polls = 0
    while not os.path.exists(path):
        if errors:
            raise errors[0]
        if stop_ev.is_set():
            return False
        polls += 1
        if polls % 128 == 0 and hasattr(ranks, "check"):   # (every quarter of a second: has the rank that is to publish it given up?)
            ranks.check()
        if time.perf_counter() > deadline:
            raise RuntimeError(f"{what} did not appear in {where}")
        time.sleep(0.002)
    prof["image_wait_s"] = prof.get("image_wait_s", 0.0) + time.perf_counter() - w0
    return True


class Handover:
    """The hand-over of one rank: `exported` are the sets it keeps alive for the others' imports, `use_ipc` what the probe of all ranks
    found (the owners publish descriptors), `ipc` whether THIS rank still imports (no more once the canary has failed)."""

    def __init__(self, eng, ranks, scratch, owned, prof, note, fatal_hook, stop_ev, errors):
        self.eng, self.ranks, self.scratch, self.owned, self.prof, self.note = eng, ranks, scratch, owned, prof, note
        self.fatal_hook, self.stop_ev, self.errors = fatal_hook, stop_ev, errors
        self.use_ipc = self.ipc = False
        self.exported = {}
        self.canary, self.canary_rank, self.verdict = None, None, None
        self.server, self.serve_stop = None, threading.Event()

    def _path(self, s, ext):
        return os.path.join(self.scratch, f"set{s}.{ext}")

    def _remove_own(self):
        for s in self.owned:
            for ext in ("pk", "ipc"):
                try:
                    os.remove(self._path(s, ext))
                except OSError:
                    pass

    def _give_up(self, limit):
        rank = self.ranks.rank
        msg = f"commet_amd.matrix, rank {rank}: commet_readset_import did not return within {limit:.0f} s; leaving"
        print(msg, file=sys.stderr, flush=True)
        if self.fatal_hook is not None:
            try:
                self.fatal_hook(msg)
            except Exception:
                pass
        self._remove_own()
        os._exit(4)

    def import_guarded(self, blob, limit_s=None):
        """eng.import_set with a deadline: a HIP call that hangs cannot be cancelled from inside the process, so a rank whose
        import does not return leaves (non-zero; the launcher ends the job) rather than keep its peers waiting for good.
        COMMET_IPC_LOCK=1 also takes a lock file of the node around the import (one import at a time on the node: a round-3
        precaution against two processes attaching to each other's buffers at the same moment, never needed without torch)."""
        limit = float(limit_s if limit_s is not None else os.environ.get("COMMET_IPC_IMPORT_LIMIT_S", "120"))
        watch = threading.Timer(limit, self._give_up, (limit,))
        watch.daemon = True
        watch.start()
        try:
            if os.environ.get("COMMET_IPC_LOCK", "0") == "1":
                import fcntl
                with open(os.path.join(self.scratch, "import.lock"), "a+") as lf:
                    fcntl.flock(lf, fcntl.LOCK_EX)
                    try:
                        return self.eng.import_set(blob)
                    finally:
                        fcntl.flock(lf, fcntl.LOCK_UN)
            return self.eng.import_set(blob)
        finally:
            watch.cancel()

    # The default since round 4 (COMMET_MATRIX_IPC=0: packed images).  Round 3 had to make it opt-in: an import of a 50 M-read set
    # did not return when the rank process had imported torch (for the gloo barrier) — two ROCm runtimes in one process.  The ranks
    # meet over sharding's TCP store now and hold one runtime.  Two nets stay under the large imports, which the probe below (a
    # four-read set) says nothing about: the first REAL set is imported by a fresh child process first (the canary: killed when it
    # does not come back, and every rank then asks the owners for packed images), and an import of this process that does not
    # return within COMMET_IPC_IMPORT_LIMIT_S ends the rank non-zero instead of leaving the job hung.
    def probe(self, say):
        """every rank imports a probe set of its neighbour and of rank 0 -> use_ipc, the same on every rank (two collective calls,
        made by every rank whatever happens to it: gather_objects, sum_int)"""
        eng, ranks = self.eng, self.ranks
        world, rank = ranks.world, ranks.rank
        if os.environ.get("COMMET_MATRIX_IPC", "1") == "0" or not hasattr(eng, "export_set"):
            return False
        probe = blob = None
        try:
            probe = eng.parse_probe()
            blob = eng.export_set(probe)
        except Exception as ex:
            say(f"device-to-device hand-over of sets not available ({ex}): packed images instead")
        blobs = ranks.gather_objects(blob)                        # (every rank, whatever happened above)
        ok = int(blob is not None)
        if ok:
            try:
                for src in sorted({0, (rank + 1) % world} - {rank}):
                    if blobs[src] is None:
                        ok = 0
                    else:
                        got = self.import_guarded(blobs[src], os.environ.get("COMMET_IPC_PROBE_LIMIT_S", "30"))   # (four reads: seconds are generous) every rank's probe set holds the same reads:
                        if hasattr(eng, "same_set") and not eng.same_set(got, probe):   # a copy that arrives damaged counts as no hand-over
                            say("device-to-device hand-over of sets: the probe set did not arrive intact: packed images instead")
                            ok = 0
                        eng.release(got)
            except Exception as ex:
                say(f"device-to-device hand-over of sets not available ({ex}): packed images instead")
                ok = 0
        self.use_ipc = self.ipc = ranks.sum_int(ok) == world      # (also: every import of the probes is done)
        if probe is not None:
            eng.release(probe)
        return self.use_ipc

    def start_canary(self, canary_rank, candidates):
        """the canary: of the ranks that take sets from others, the first one (canary_rank) starts a fresh child process that imports
        the first real set to appear, one of `candidates` (tests/engines without a child command: no canary)"""
        self.canary_rank = canary_rank if self.use_ipc else None
        if (self.use_ipc and self.ranks.rank == canary_rank and hasattr(self.eng, "canary_argv")
                and os.environ.get("COMMET_IPC_CANARY", "1") != "0"):
            self.canary = subprocess.Popen(self.eng.canary_argv(self.scratch, candidates), stdout=subprocess.DEVNULL)

    def canary_verdict(self):
        """Did the fresh child process of `canary_rank` get the first real set across?  That rank waits for its child (and
        kills it by its pid when it does not answer in COMMET_IPC_CANARY_S), says so in the scratch directory, the others
        read it there.  True: this process imports, too."""
        if self.verdict is None:
            ok_path, fail_path = os.path.join(self.scratch, "canary.ok"), os.path.join(self.scratch, "canary.fail")
            if self.ranks.rank == self.canary_rank:
                verdict = "passed"
                if self.canary is not None:
                    limit = float(os.environ.get("COMMET_IPC_CANARY_S", "30"))
                    try:
                        rc = self.canary.wait(timeout=limit)
                        verdict = "passed" if rc == 0 else f"failed (exit code {rc})"
                    except subprocess.TimeoutExpired:
                        self.canary.kill()
                        try:
                            self.canary.wait(timeout=5)
                        except subprocess.TimeoutExpired:
                            pass
                        verdict = f"failed (no answer within {limit:.0f} s: killed)"
                path = ok_path if verdict == "passed" else fail_path
                with open(path + ".tmp", "w") as fh:
                    fh.write(verdict)
                os.rename(path + ".tmp", path)
            else:
                deadline = time.perf_counter() + float(os.environ.get("COMMET_DIST_TIMEOUT_S", "600"))
                while not (os.path.exists(ok_path) or os.path.exists(fail_path)):
                    if self.stop_ev.is_set() or time.perf_counter() > deadline:
                        break
                    time.sleep(0.002)
                verdict = "passed" if os.path.exists(ok_path) else (open(fail_path).read() if os.path.exists(fail_path) else "failed (no verdict)")
            self.verdict = verdict
            self.prof["ipc_canary"] = verdict
        return self.verdict == "passed"

    def wait_file(self, path, what):
        return wait_file(path, what, self.scratch, self.stop_ev, self.errors, self.ranks, self.prof)

    def publish(self, s, rs):
        """a set this rank has parsed and others need: its descriptor (a small file; the set stays alive for the importers) or its
        packed image (commet_readset_save writes a .tmp and renames it: the file appears complete or not at all)"""
        w0 = time.perf_counter()
        if self.use_ipc:
            path = self._path(s, "ipc")
            with open(path + ".tmp", "wb") as fh:
                fh.write(self.eng.export_set(rs))
            os.rename(path + ".tmp", path)
            self.exported[s] = rs
        else:
            self.eng.save(rs, self._path(s, "pk"))
        self.prof["save_s"] += time.perf_counter() - w0

    def fetch(self, s):
        """another rank's set: from its owner's device buffers, or from its packed image; None: this rank is stopping"""
        ipc_path, pk_path = self._path(s, "ipc"), self._path(s, "pk")
        if hasattr(self.ranks, "check"):
            self.ranks.check()                                    # (no import from a job that has lost a rank: its owner may be leaving)
        if self.ipc:
            if not self.wait_file(ipc_path, f"the descriptor of set {s}"):
                return None
            if not self.canary_verdict():                         # (the first set only)
                self.ipc = False
                self.prof["handover"] = "image"
                self.note(f"device-to-device hand-over given up (canary {self.verdict}): packed images from here on")
        if self.ipc:
            w0 = time.perf_counter()
            with open(ipc_path, "rb") as fh:
                rs = self.import_guarded(fh.read())
        else:
            if self.use_ipc:                                      # the owners published descriptors only: ask for the image
                open(os.path.join(self.scratch, f"set{s}.want.{self.ranks.rank}"), "w").close()
            if not self.wait_file(pk_path, f"the packed image of set {s}"):
                return None
            w0 = time.perf_counter()
            rs = self.eng.load(pk_path)
        self.prof["load_s"] += time.perf_counter() - w0
        self.prof["sets_loaded"] += 1
        return rs

    def serve_images(self):
        """the way back: a rank that gave the device-to-device hand-over up asks for `set<s>.pk`; its owner, which keeps
        every exported set alive, writes it"""
        served = set()
        while not self.serve_stop.wait(0.005):
            for s in list(self.exported):
                if s not in served and any(f.startswith(f"set{s}.want.") for f in os.listdir(self.scratch)):
                    w0 = time.perf_counter()
                    self.eng.save(self.exported[s], self._path(s, "pk"))
                    self.prof["save_s"] += time.perf_counter() - w0
                    served.add(s)

    def start_server(self):
        self.server = threading.Thread(target=self.serve_images, name="commet-image-server", daemon=True)
        self.server.start()

    def release_exported(self, sets):
        """(after a gather of all ranks that comes after every rank's loading: no import of an exported set is still under way)"""
        for s, rs in self.exported.items():
            if s not in sets:
                self.eng.release(rs)

    def linger(self):
        """A failing rank that has exported sets: the other ranks may be in the middle of importing a set of this one: they notice the
        abort within a quarter of a second and start no new import; what is under way takes tens of ms.  An exporter that left at once
        would leave them in a HIP call that never returns (seen: 120 s until their own watchdog)."""
        if self.exported:
            time.sleep(float(os.environ.get("COMMET_ABORT_LINGER_S", "2")))

    def stop(self):
        """the image server (after the gather that says nobody asks for a set any more), and a canary nobody asked about (this rank
        failed first)"""
        if self.server is not None and self.server.is_alive():
            self.serve_stop.set()
            self.server.join()
        if self.canary is not None and self.canary.poll() is None:
            self.canary.kill()

    def cleanup(self, failed):
        """rank 0 removes the scratch directory once everybody is through (a barrier); a failing rank removes its own images"""
        if not failed:
            self.ranks.barrier()
            if self.ranks.rank == 0:
                shutil.rmtree(self.scratch, ignore_errors=True)
        else:
            self._remove_own()
