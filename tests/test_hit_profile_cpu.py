"""The host side of the hit profile that needs no GPU: tags_at's packing, the sweep command's argument errors and its set-config
reader, and the entry point's refusal to run without a device (there is no CPU fallback)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from conftest import ROOT


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1000])
def test_tags_at_packs_like_a_boolean_vector(n):
    import commet_amd
    from commet_amd import api
    rng = np.random.default_rng(n)
    hits = rng.integers(0, 6, size=n).astype(np.uint8)
    for t in (1, 3, 5, 6):
        got = commet_amd.tags_at(hits, t)
        assert got.dtype == np.uint8 and got.size == api.bits_nbytes(n) == n // 8 + 1
        assert got.tobytes() == util.bits_from_bools(hits >= t).tobytes()
        assert np.array_equal(util.bools_from_bits(got, n), hits >= t)
        assert not np.unpackbits(got, bitorder="little")[n:].any()          # padding bits are zero
    assert not commet_amd.tags_at(hits, 6).any() and commet_amd.tags_at(hits, 0).tobytes() == util.bits_from_bools(np.ones(n, bool)).tobytes()


def _sweep(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "commet_amd.sweep"] + args, cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_sweep_argument_errors(tmp_path):
    open(tmp_path / "i.txt", "w").write("A:a.fa\n")
    open(tmp_path / "two.txt", "w").write("A:a.fa\nB:b.fa\n")
    open(tmp_path / "s.txt", "w").write("B:b.fa\n")
    ok = ["-i", "i.txt", "-s", "s.txt", "-k", "32", "-o", "out"]
    for args, msg in ((ok, b"--max-t"), (ok + ["--max-t", "0"], b"1..255"), (ok + ["--max-t", "256"], b"1..255"),
                      (ok[2:] + ["--max-t", "4"], b"-i"), (["-i", "none.txt"] + ok[2:] + ["--max-t", "4"], b"Cannot read file none.txt"),
                      (["-i", "two.txt"] + ok[2:] + ["--max-t", "4"], b"Only one set of files is allowed for indexing"),
                      (ok[:4] + ["-k", "0", "-o", "out", "--max-t", "4"], b"-k")):
        r = _sweep(args, tmp_path)
        assert r.returncode == 2 and msg in r.stderr, (args, r.stderr)
        assert not os.path.exists(tmp_path / "out")
    r = _sweep(["--help"], tmp_path)
    assert r.returncode == 0 and b"No .log files" in r.stdout and b"sweep.csv" in r.stdout


def test_sweep_reads_the_set_config_grammar(tmp_path):
    from commet_amd import sweep
    open(tmp_path / "s.txt", "w").write("zed: a.fa , a.bv ;b.fa\n\nno_colon.fa;x.fa,y.bv\nB:c.fa\nzed:d.fa\n")
    assert sweep.read_sets(str(tmp_path / "s.txt")) == [("B", [("c.fa", None)]), ("SET2", [("no_colon.fa", None), ("x.fa", "y.bv")]),
                                                        ("zed", [("d.fa", None)])]


def test_profile_needs_a_device():
    import commet_amd
    from commet_amd import lib
    h = lib.load()
    assert hasattr(h, "commet_index_and_profile") and "commet_index_and_profile" in lib.SIGNATURES
    if h.commet_device_count() == 0:
        with pytest.raises(commet_amd.CommetError, match="no HIP device|no CPU fallback"):
            with commet_amd.Context(k=32) as ctx:
                ctx.index_and_profile(None, [])
