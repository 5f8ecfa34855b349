"""The CPU restatement (oracle/) against the compiled reference (oracle/_ref), on randomised scenarios: live where the
reference was built, else against its stored runs on the same scenarios (tests/refrun.py, tests/golden/ref_runs)."""
import os

import pytest

import refrun
from scenarios import Scenario, compare_runs, run_oracle


def _reference(scn, out, log):
    """the reference's index_and_search on the scenario (paths relative to its directory: the stored runs hold the arguments)"""
    rel = lambda p: os.path.relpath(p, scn.dir)          # noqa: E731
    return refrun.run("index_and_search", ["-i", scn.index_cfg, "-s", scn.search_cfg, "-o", rel(out), "-l", rel(log),
                                           "-k", str(scn.k), "-t", str(scn.t)], scn.dir, watch=[out, log])


@pytest.mark.parametrize("seed", range(40))
def test_oracle_matches_reference(tmp_path, seed):
    scn = Scenario(str(tmp_path / "scn"), seed)
    out_r, log_r = str(tmp_path / "out_ref"), str(tmp_path / "log_ref")
    out_o, log_o = str(tmp_path / "out_orc"), str(tmp_path / "log_orc")
    p = _reference(scn, out_r, log_r)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    rc, res, chunks, kmers = run_oracle(scn, out_o, log_o)
    assert rc == 0
    compare_runs(out_r, log_r, out_o, log_o, scn)


@pytest.mark.parametrize("seed", range(500, 530))
def test_oracle_matches_reference_fastq_and_gzip(tmp_path, seed):
    """FASTQ and gzip inputs, format chosen per file"""
    scn = Scenario(str(tmp_path / "scn"), seed, formats=("fa", "fq", "fa.gz", "fq.gz"), crlf=False)
    out_r, log_r = str(tmp_path / "out_ref"), str(tmp_path / "log_ref")
    out_o, log_o = str(tmp_path / "out_orc"), str(tmp_path / "log_orc")
    p = _reference(scn, out_r, log_r)
    assert p.returncode == 0, p.stderr.decode()[-500:]
    rc, res, chunks, kmers = run_oracle(scn, out_o, log_o)
    assert rc == 0
    compare_runs(out_r, log_r, out_o, log_o, scn)
