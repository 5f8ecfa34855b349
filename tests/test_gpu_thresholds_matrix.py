"""`python -m commet_amd.matrix --max-t T` on the GPU (commet_amd/matrix_sweep.py): OUT/t<t>/ against the reference's own golden files of
ABCDE_bench at t = 2 (tests/golden/abcde/commet_py/three_sets, k = 32), and against one run of the single-t driver per t on the four
synthetic sets (k = 20): .bv files and csv matrices byte for byte."""
import gzip
import os

import pytest

from conftest import ROOT
from sweep_sets import four_sets

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module", autouse=True)
def _tools():
    from commet_amd import build
    build.build_lib()
    build.build_tools()


def _is_result(f):
    return f.endswith(".csv") or (f.endswith(".bv") and "_in_" in f)


def test_sweep_reproduces_commet_py_at_t2(tmp_path, monkeypatch):
    from commet_amd import matrix_sweep
    gold = os.path.join(GOLD, "abcde", "commet_py", "three_sets")
    os.makedirs(tmp_path / "ABCDE_bench")
    for f, copies in (("A", "A"), ("B", "BD"), ("C", "CE")):
        data = gzip.open(os.path.join(GOLD, "abcde", f + ".fa.gz")).read()
        for c in copies:
            open(tmp_path / "ABCDE_bench" / (c + ".fa"), "wb").write(data)
    monkeypatch.chdir(tmp_path)
    open("sets.txt", "w").write(open(os.path.join(gold, "sets.txt")).read())
    res = matrix_sweep.run("sets.txt", "out/", k=32, max_t=3, verbose=False)
    want = sorted(f for f in os.listdir(gold) if f.endswith((".csv", ".bv")))
    assert sum(map(_is_result, want)) >= 3 + 6
    for f in want:
        got = os.path.join("out", "t2", f) if _is_result(f) else os.path.join("out", f)      # (filter .bv files: in OUT/ once)
        assert open(got, "rb").read() == open(os.path.join(gold, f), "rb").read(), f
    for t in (1, 2, 3):
        assert sorted(os.listdir(f"out/t{t}")) == sorted(f for f in want if _is_result(f))
    assert res["matrices"][2][0][0] == 12000 and not [f for f in os.listdir("out") if f.endswith(".log")]

def test_sweep_equals_one_run_per_threshold(tmp_path, monkeypatch):
    from commet_amd import matrix, matrix_sweep
    monkeypatch.chdir(tmp_path)
    four_sets()
    res = matrix_sweep.run("sets.txt", "out/", k=20, max_t=3, verbose=False)
    assert res["calls"] == 3 * 3 and res["jobs"] == 3 + 2 * 6 * 3
    for t in (1, 2, 3):
        one = matrix.run("sets.txt", f"one{t}/", k=20, t=t, verbose=False)
        want = sorted(f for f in os.listdir(f"one{t}") if _is_result(f))
        assert len(want) == 3 + 5 * 3 and sorted(os.listdir(f"out/t{t}")) == want
        for f in want:
            assert open(f"out/t{t}/{f}", "rb").read() == open(f"one{t}/{f}", "rb").read(), (t, f)
        assert res["matrices"][t] == one["matrix"]
