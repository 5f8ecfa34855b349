"""The device-memory cache (commet_amd/csrc/host/devmem.hpp: size classes, filed blocks and their reuse, the per-device cap, trim and
retry, the exact-size last attempt, pooled and shareable blocks, the refusal hook, blocks set aside, five threads on one cache) on the
CPU, through host/devmem_check.cpp: the cache over a fake driver that logs every call.  The program is built plain, with
-fsanitize=address,undefined and with -fsanitize=thread, and each build runs as a child process of its own — with the cache on, with
COMMET_DEVMEM_CACHE=0, and with stream-ordered blocks (COMMET_DEVMEM_POOL=1); a failed expectation or a sanitizer report ends the
child with a status that is not 0.  (The library runs the same header over the HIP runtime: capi/state.hpp.)"""
import os
import subprocess

import pytest

from conftest import ROOT

HOST = os.path.join(ROOT, "commet_amd", "csrc", "host")
SRC = os.path.join(HOST, "devmem_check.cpp")
SAN = os.path.join(ROOT, "commet_amd", "_san")
BUILDS = {
    "plain": (os.path.join(ROOT, "commet_amd", "bin", "devmem_check"), ["-O2"]),
    "asan_ubsan": (os.path.join(SAN, "asan", "bin", "devmem_check"),
                   ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
    "tsan": (os.path.join(SAN, "tsan", "bin", "devmem_check"), ["-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=thread"]),
}
MODES = {
    "cache_on": {},
    "cache_off": {"COMMET_DEVMEM_CACHE": "0"},
    "pooled": {"COMMET_DEVMEM_POOL": "1", "COMMET_DEVMEM_POOL_MIN_MB": "8"},
}
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")


@pytest.fixture(scope="module")
def built():
    deps = [SRC, os.path.join(HOST, "devmem.hpp")]
    jobs = []
    for exe, flags in BUILDS.values():
        if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
            continue
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        jobs.append(subprocess.Popen(["g++", "-std=c++17", "-Wall", "-pthread"] + flags + ["-o", exe, SRC],
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for j in jobs:
        out = j.communicate()[0].decode()
        assert j.returncode == 0, out[-3000:]
    return {name: exe for name, (exe, _) in BUILDS.items()}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("build", list(BUILDS))
def test_devmem_check(built, build, mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("COMMET_DEVMEM_")}
    p = subprocess.run([built[build]], env=dict(env, **SAN_ENV, **MODES[mode]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    lines = out.split("\n")
    assert "ok threads" in lines and "ok size classes" in lines and not any(ln.startswith("FAIL") for ln in lines), out[-3000:]
    assert ("ok cache off" in lines) == (mode == "cache_off") and ("ok reuse" in lines) == (mode != "cache_off"), out[-3000:]
    assert ("ok make shareable" in lines) == (mode == "pooled"), out[-3000:]
