"""The read filter's rule (commet_amd/csrc/host/filter_rule.hpp), on the CPU: the filter_reads tool built on it against the
reference's tool for every case of tests/read_filter_cases.py (tests/refrun.py: live where oracle/_ref is built, else the stored
runs), the host half of the device filter — the Shannon table and the finishing function, through libcommet_plan.so — against the
tool, and the N x N driver's .bv writer against the tool's bytes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import refrun
import util
from conftest import ROOT
from read_filter_cases import CASES, verdict_bitmaps

BIN = os.environ.get("COMMET_BIN_DIR") or os.path.join(ROOT, "commet_amd", "bin")
HOST = os.path.join(ROOT, "commet_amd", "csrc", "host")
PLAN_LIB = os.environ.get("COMMET_PLAN_LIB") or os.path.join(ROOT, "commet_amd", "libcommet_plan.so")


def _newer(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


@pytest.fixture(scope="module")
def filter_reads():
    tool = os.path.join(BIN, "filter_reads")
    srcs = [os.path.join(HOST, f) for f in ("filter_reads.cpp", "filter_rule.hpp", "fasta_source.hpp", "bv_file.hpp")]
    if not os.environ.get("COMMET_BIN_DIR") and _newer(tool, srcs):
        os.makedirs(BIN, exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", tool, srcs[0], "-lz"], check=True)
    return tool


@pytest.fixture(scope="module")
def plan():
    srcs = [os.path.join(HOST, "plan_capi.cpp"), os.path.join(HOST, "filter_rule.hpp"), os.path.join(ROOT, "commet_amd", "csrc", "read_iter.hpp")]
    if not os.environ.get("COMMET_PLAN_LIB") and _newer(PLAN_LIB, srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", PLAN_LIB, srcs[0]], check=True)
    lib = C.CDLL(PLAN_LIB)
    lib.commet_filter_shannon_table.restype = C.c_uint64
    lib.commet_filter_shannon_table.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p]
    lib.commet_filter_finish_file.restype = None
    lib.commet_filter_finish_file.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int64,
                                              C.c_void_p, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _strip_time(b):
    return re.sub(rb"Total  time : .* s", b"Total  time : T s", b)


def tool_counters(stdout):
    """(selected, removed by length, by N, by Shannon) from what the tool prints"""
    t = stdout.decode()
    g = lambda pat: int(re.search(pat, t).group(1))
    return (g(r"Number of selected reads = (\d+)"), g(r"Length filter \[[^\]]*\]: (\d+) reads removed"),
            g(r"Number of N filter \[[^\]]*\]: (\d+) reads removed"), g(r"Shannon filter \[[^\]]*\]: (\d+) reads removed"))


def run_tool(tool, case, paths, out_dir, with_extra=True):
    """the tool on every file of the case -> [(stdout, bv path)]"""
    os.makedirs(out_dir, exist_ok=True)
    out = []
    for i, p in enumerate(paths):
        bv = os.path.join(out_dir, f"f{i}.bv")
        r = subprocess.run([tool, p] + case.tool_args(with_extra) + ["-o", bv], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        out.append((r.stdout, bv))
    return out


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_tool_matches_reference(tmp_path, filter_reads, case):
    for d in ("ours", "ref"):
        case.build(str(tmp_path / d))
    for i, (fname, _, _, _) in enumerate(case.files):
        args = [fname] + case.tool_args() + ["-o", f"out{i}.bv"]
        a = subprocess.run([filter_reads] + args, cwd=str(tmp_path / "ours"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        b = refrun.run("filter_reads", args, str(tmp_path / "ref"))
        assert a.returncode == b.returncode == 0
        assert _strip_time(a.stdout) == _strip_time(b.stdout)
        assert open(tmp_path / "ours" / f"out{i}.bv", "rb").read() == open(tmp_path / "ref" / f"out{i}.bv", "rb").read()


def test_shannon_table_holds_the_tools_terms(plan):
    for lo, hi in ((100, 100), (1, 150), (37, 1024)):
        n = plan.commet_filter_shannon_table(lo, hi, None)
        assert n == sum(L + 1 for L in range(lo, hi + 1))
        tab = np.full(n, np.nan)
        assert plan.commet_filter_shannon_table(lo, hi, _p(tab)) == n
        at = 0
        for L in range(lo, hi + 1):
            row = tab[at:at + L + 1]
            at += L + 1
            assert row[0] == 0
            for c in (1, 2, L // 3, L // 2, L - 1, L):
                if 1 <= c <= L:
                    f = float(np.float32(c) / np.float32(L))
                    assert row[c] == f * math.log(f) / math.log(2), (L, c)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_finish_file_reproduces_the_tool(tmp_path, filter_reads, plan, case):
    """verdict bitmaps computed in numpy from the case's reads -> the finishing function -> the tool's bits and its four counters"""
    paths = case.build(str(tmp_path / "in"))
    runs = run_tool(filter_reads, case, paths, str(tmp_path / "out"))
    keep, by_len, by_n, empty, spans = verdict_bitmaps(case, paths)
    out = np.zeros_like(keep)
    want_bits = []
    for (first, count), (stdout, bv) in zip(spans, runs):
        counts = np.zeros(4, dtype=np.uint64)
        plan.commet_filter_finish_file(_p(keep), _p(by_len), _p(by_n), first, count, _p(empty), len(empty), -1 if case.m is None else case.m,
                                       _p(out), _p(counts))
        _, nb, bits = util.read_bv(bv)
        assert nb == count
        assert tuple(int(x) for x in counts) == tool_counters(stdout)
        want_bits.append(util.bools_from_bits(bits, nb))
    total = sum(c for _, c in spans)
    got = np.unpackbits(out.view(np.uint8), bitorder="little")
    assert np.array_equal(got[:total].astype(bool), np.concatenate(want_bits))
    assert not got[total:].any()                                  # padding bits stay zero


def test_finish_file_walks_word_boundaries(plan):
    """the cap reached at every position around a word boundary, files that start and end inside a word, against the read-by-read loop"""
    rng = np.random.default_rng(5)
    n = 64 * 5 + 17
    for trial in range(200):
        v = rng.integers(0, 4, size=n)                            # 0 keep, 1 length, 2 N, 3 Shannon
        if trial % 3 == 0:
            v[:] = 0
        first = int(rng.integers(0, 130))
        count = int(rng.integers(0, n - first + 1))
        empty = np.array(sorted(set(int(x) for x in rng.integers(0, n, size=int(rng.integers(0, 3))))), dtype=np.uint64)
        m = int(rng.integers(-1, count + 3))
        words = lambda b: np.frombuffer(np.packbits(np.concatenate([b, np.zeros(64 - n % 64, dtype=bool)]), bitorder="little").tobytes(), dtype=np.uint64).copy()
        keep, by_len, by_n = words(v == 0), words(v == 1), words(v == 2)
        out = rng.integers(0, 2**63, size=keep.size, dtype=np.uint64)
        before = np.unpackbits(out.view(np.uint8), bitorder="little").astype(bool)
        counts = np.zeros(4, dtype=np.uint64)
        plan.commet_filter_finish_file(_p(keep), _p(by_len), _p(by_n), first, count, _p(empty), len(empty), m, _p(out), _p(counts))
        # the loop of filter_reads.cpp:186-205
        cap = count if m < 0 else m
        bits, sel, rm, pos = np.ones(count, dtype=bool), 0, [0, 0, 0, 0], 0
        while pos < count and sel < cap and (first + pos) not in empty:
            if v[first + pos] == 0:
                sel += 1
            else:
                bits[pos] = False
                rm[v[first + pos]] += 1
            pos += 1
        if sel >= cap:
            bits[pos:] = False
        assert [int(x) for x in counts] == [sel, rm[1], rm[2], rm[3]], (trial, first, count, m)
        after = np.unpackbits(out.view(np.uint8), bitorder="little").astype(bool)
        assert np.array_equal(after[first:first + count], bits), (trial, first, count, m)
        assert np.array_equal(after[:first], before[:first]) and np.array_equal(after[first + count:], before[first + count:])


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_driver_bv_writer_gives_the_tools_bytes(tmp_path, filter_reads, case):
    """commet_amd.matrix.write_filter_bv, fed the tool's bits, writes the tool's file: comment block, size line, bits"""
    from commet_amd import matrix
    paths = case.build(str(tmp_path / "in"))
    runs = run_tool(filter_reads, case, paths, str(tmp_path / "out"), with_extra=False)   # (the driver never passes -c)
    for p, (_, bv) in zip(paths, runs):
        nb, bits = matrix.read_bv(bv)
        mine = str(tmp_path / "mine.bv")
        matrix.write_filter_bv(mine, p, nb, bits, case.l or 0, -1 if case.n is None else case.n, float(case.e) if case.e is not None else 0.0)
        assert open(mine, "rb").read() == open(bv, "rb").read()
        assert not os.path.exists(mine + ".part")


def test_driver_cap_is_what_atoi_makes_of_the_quotient():
    from commet_amd import matrix
    for m, nfiles in ((5000, 1), (5000, 3), (7, 2), (0, 4), (10**17, 1), (1, 3)):
        text = str(m / nfiles)
        want = int(re.match(r"\d*", text).group(0) or 0)
        assert matrix.c_atoi(text) == want
    assert matrix.c_atoi("  -12x") == -12 and matrix.c_atoi("+7.9") == 7 and matrix.c_atoi("x") == 0 and matrix.c_atoi("1e+16") == 1
