"""commet_readset_filter (read_filter.hpp, capi/filter.hpp) on the MI355X against the filter_reads tool, bit for bit: every case of
tests/read_filter_cases.py through ReadSet.filter — also after a save / load round trip and at another k —, the selection fed to
commet_index_and_search, and the N x N driver with filter options on the device against the same run with filter_reads processes."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import util
from conftest import ROOT
from read_filter_cases import CASES

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
TOOL = os.path.join(ROOT, "commet_amd", "bin", "filter_reads")


@pytest.fixture(scope="module", autouse=True)
def _tools():
    from commet_amd import build
    build.build_lib()
    build.build_tools()


def _tool(case, paths, out_dir):
    """the tool on every file of the case -> (set-wide bools, per-file counters as ReadSet.filter reports them, the .bv paths)"""
    os.makedirs(out_dir, exist_ok=True)
    bools, stats, bvs = [], [], []
    for i, p in enumerate(paths):
        bv = os.path.join(out_dir, f"f{i}.bv")
        r = subprocess.run([TOOL, p] + case.tool_args() + ["-o", bv], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, r.stderr.decode()
        t = r.stdout.decode()
        g = lambda pat: int(re.search(pat, t).group(1))
        _, nb, bits = util.read_bv(bv)
        bools.append(util.bools_from_bits(bits, nb))
        stats.append(dict(reads=nb, selected=g(r"Number of selected reads = (\d+)"), removed_length=g(r"Length filter \[[^\]]*\]: (\d+) reads removed"),
                          removed_n=g(r"Number of N filter \[[^\]]*\]: (\d+) reads removed"),
                          removed_shannon=g(r"Shannon filter \[[^\]]*\]: (\d+) reads removed")))
        bvs.append(bv)
    return np.concatenate(bools), stats, bvs


def _check(rs, case, want_bools, want_stats):
    bits, stats = rs.filter(**case.api_kwargs())
    n = rs.num_reads
    assert n == want_bools.size and bits.size == n // 8 + 1
    got = np.unpackbits(bits, bitorder="little")
    assert np.array_equal(got[:n].astype(bool), want_bools)
    assert not got[n:].any()                                      # padding bits are zero
    assert stats == want_stats
    return bits


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_filter_matches_the_tool(tmp_path, case):
    """the resident set, its image loaded into a context of another k, and the first context again: the tool's bits and counters"""
    import commet_amd
    paths = case.build(str(tmp_path / "in"))
    want_bools, want_stats, _ = _tool(case, paths, str(tmp_path / "tool"))
    with commet_amd.Context(k=20, t=2, device=0) as ctx, commet_amd.Context(k=33, t=2, device=0) as ctx2:
        rs = commet_amd.ReadSet.from_fasta(ctx, paths)
        first = _check(rs, case, want_bools, want_stats)
        rs.save(str(tmp_path / "set.pk"))
        rs2 = commet_amd.ReadSet.load(ctx2, str(tmp_path / "set.pk"))          # the filter does not depend on k
        assert np.array_equal(_check(rs2, case, want_bools, want_stats), first)
        rs3 = commet_amd.ReadSet.load(ctx, str(tmp_path / "set.pk"))
        assert np.array_equal(_check(rs3, case, want_bools, want_stats), first)
        assert np.array_equal(_check(rs, case, want_bools, want_stats), first)  # (a second call: the kept table and scratch)


@pytest.mark.parametrize("name", ["ragged_1_150", "three_files_m40", "long_mixed_e1.5", "uniform_100"])
def test_selection_drives_index_and_search_like_the_tools_bv(tmp_path, name):
    """commet_index_and_search with the returned bits as index_select and search_select = the same job with the tool's .bv files"""
    import commet_amd
    from commet_amd import matrix
    case = next(c for c in CASES if c.name == name)
    other = next(c for c in CASES if c.name == "crlf_iupac")
    with commet_amd.Context(k=12, t=2, device=0) as ctx:
        sets, dev, tool = [], [], []
        for tag, c in (("a", case), ("b", other)):
            paths = c.build(str(tmp_path / tag))
            _, _, bvs = _tool(c, paths, str(tmp_path / (tag + "_tool")))
            rs = commet_amd.ReadSet.from_fasta(ctx, paths)
            sets.append(rs)
            dev.append(rs.filter(**c.api_kwargs())[0])
            tool.append(matrix.concat_bits([matrix.read_bv(b) for b in bvs])[1])
        for i, s in ((0, 1), (1, 0)):
            t_dev, st_dev, _ = ctx.index_and_search(sets[i], [sets[s]], dev[i], [dev[s]])
            t_tool, st_tool, _ = ctx.index_and_search(sets[i], [sets[s]], tool[i], [tool[s]])
            assert np.array_equal(t_dev[0], t_tool[0])
            assert {f: st_dev[0][f] for f in ("indexed", "searched", "shared")} == {f: st_tool[0][f] for f in ("indexed", "searched", "shared")}
            assert st_dev[0]["searched"] > 0


@pytest.fixture()
def abcde(tmp_path):
    os.makedirs(tmp_path / "ABCDE_bench")
    for f, copies in (("A", "A"), ("B", "BD"), ("C", "CE")):
        data = gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read()
        for c in copies:
            open(tmp_path / "ABCDE_bench" / (c + ".fa"), "wb").write(data)
    open(tmp_path / "sets.txt", "w").write(open(os.path.join(GOLD, "abcde", "commet_py", "five_sets", "sets.txt")).read())
    return tmp_path


def _same_files(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    n_bv = 0
    for f in fa:
        x, y = open(os.path.join(a, f), "rb").read(), open(os.path.join(b, f), "rb").read()
        if f.endswith(".log"):                                    # times differ; the counts do not
            x, y = x.split(b"\n")[-2], y.split(b"\n")[-2]
        assert x == y, f
        n_bv += f.endswith(".bv")
    return n_bv


def test_matrix_with_filter_options_device_against_tool(abcde, monkeypatch):
    """ABCDE with -l 60 -n 2 -e 1.8 -m 5000: the device filter, the filter_reads processes (COMMET_MATRIX_FILTER_TOOL=1) and a 2-rank
    run on one GPU leave byte-identical directories — filter .bv, result .bv, the three CSVs; logs apart from their times"""
    from commet_amd import matrix
    monkeypatch.chdir(abcde)
    opts = dict(k=32, t=2, l=60, n=2, e=1.8, m=5000, verbose=False)
    started = []
    real_run = subprocess.run

    def watch(cmd, *a, **kw):
        started.append(cmd)
        return real_run(cmd, *a, **kw)

    monkeypatch.setattr(subprocess, "run", watch)
    monkeypatch.delenv("COMMET_MATRIX_FILTER_TOOL", raising=False)
    res_dev = matrix.run("sets.txt", "out_dev/", **opts)
    assert not any("filter_reads" in str(c) for c in started)     # no filter_reads process unless asked for
    monkeypatch.setenv("COMMET_MATRIX_FILTER_TOOL", "1")
    res_tool = matrix.run("sets.txt", "out_tool/", **opts)
    assert sum("filter_reads" in str(c) for c in started) == 5
    monkeypatch.delenv("COMMET_MATRIX_FILTER_TOOL")
    assert _same_files("out_dev", "out_tool") == 5 + 20            # 5 filter vectors, 5 x 4 results
    assert res_dev["matrix"] == res_tool["matrix"] and res_dev["considered"] == res_tool["considered"]
    assert all(0 < c <= 5000 for c in res_dev["considered"]) and res_dev["filter_s"] > 0
    # two ranks on one GPU
    env = {k_: v for k_, v in os.environ.items() if k_ not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(COMMET_FORCE_DEVICE="0", COMMET_SCRATCH=str(abcde), PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
    p = real_run([sys.executable, "-m", "commet_amd.matrix", "sets.txt", "-k", "32", "-t", "2", "-l", "60", "-n", "2", "-e", "1.8", "-m", "5000",
                  "-o", "out_two/", "--gpus", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert _same_files("out_dev", "out_two") == 25
