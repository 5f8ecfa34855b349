"""The reference's compiled tools (oracle/_ref), live or replayed, for the tests that compare against them.

Where oracle/_ref/<name> exists (build() compiles it where the reference sources are at hand) a call runs it.  Elsewhere the
call is replayed from tests/golden/ref_runs/: the exit code, stdout, stderr and the files that very call wrote, recorded from
the binary on the same inputs (every test input is made from fixed seeds).  A replay writes those files back where the binary
would have written them, so the test reads them as it reads a live run's.

    COMMET_REF_RECORD=1 python -m pytest tests/test_host_tools.py tests/test_oracle_vs_ref.py     (oracle/_ref built)

rewrites the records of the tests it runs: one gzipped JSON file per test, a list of its calls in order."""
import base64
import gzip
import hashlib
import json
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STORE = os.path.join(HERE, "golden", "ref_runs")

_calls = {}          # test id -> calls made so far in this session


def ref_tool(name):
    p = os.path.join(ROOT, "oracle", "_ref", name)
    return p if os.path.exists(p) else None


def _test_id():
    cur = os.environ.get("PYTEST_CURRENT_TEST")
    assert cur, "refrun.run is called from inside a test"
    return cur.rsplit(" ", 1)[0]


def _record_path(test_id):
    mod, _, name = test_id.partition("::")
    return os.path.join(STORE, os.path.splitext(os.path.basename(mod))[0], re.sub(r"[^A-Za-z0-9_.\[\]-]", "_", name) + ".json.gz")


def _digests(d):
    """relative path -> sha256 of every file under d (nothing when d does not exist yet)"""
    out = {}
    for base, _, files in os.walk(d):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, d)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def run(name, args, cwd, watch=None):
    """oracle/_ref/<name> with args in cwd -> subprocess.CompletedProcess (stdout and stderr as bytes).  watch: the directories
    the call writes into (default [cwd]); the record keeps the files of them the call created or changed."""
    watch = [cwd] if watch is None else list(watch)
    test_id = _test_id()
    i = _calls.get(test_id, 0)
    _calls[test_id] = i + 1
    path = _record_path(test_id)
    tool = ref_tool(name)
    if tool:
        before = [_digests(d) for d in watch]
        p = subprocess.run([tool] + list(args), cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if os.environ.get("COMMET_REF_RECORD") == "1":
            files = []
            for w, (d, old) in enumerate(zip(watch, before)):
                for rel, h in sorted(_digests(d).items()):
                    if old.get(rel) != h:
                        files.append([w, rel, base64.b64encode(open(os.path.join(d, rel), "rb").read()).decode()])
            calls = json.loads(gzip.decompress(open(path, "rb").read())) if i > 0 and os.path.exists(path) else []
            calls = calls[:i] + [{"tool": name, "args": list(args), "returncode": p.returncode,
                                  "stdout": base64.b64encode(p.stdout).decode(), "stderr": base64.b64encode(p.stderr).decode(),
                                  "files": files}]
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as fh:
                fh.write(gzip.compress(json.dumps(calls, sort_keys=True).encode(), mtime=0))
        return p
    if not os.path.exists(path):
        pytest.fail(f"oracle/_ref/{name} is not built and {os.path.relpath(path, ROOT)} holds no stored run of it "
                    f"(record one with COMMET_REF_RECORD=1 where oracle/_ref is built)")
    calls = json.loads(gzip.decompress(open(path, "rb").read()))
    assert i < len(calls), f"{test_id}: call {i + 1} of the reference's {name}, {len(calls)} stored"
    c = calls[i]
    assert (c["tool"], c["args"]) == (name, list(args)), f"{test_id}: call {i + 1} stored as {c['tool']} {c['args']}"
    for w, rel, data in c["files"]:
        p = os.path.join(watch[w], rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "wb") as fh:
            fh.write(base64.b64decode(data))
    return subprocess.CompletedProcess([name] + list(args), c["returncode"], base64.b64decode(c["stdout"]), base64.b64decode(c["stderr"]))
