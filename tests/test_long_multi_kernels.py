"""search_long_kernel's instantiations in the built library (no GPU): the sixteen of one job, under the names they have always had,
and the two with the filters of several jobs in a pass (long_search.hpp, JOBS) — nothing else of that name."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def kernel_symbols():
    from commet_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build_lib()
    out = subprocess.run(["nm", "-C", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"commet::(?:__device_stub__)?(\w+_kernel(?:<[^(]*>)?)\(", out))


def test_search_long_kernel_instantiations(kernel_symbols):
    got = {s for s in kernel_symbols if s.startswith("search_long_kernel<")}
    one_job = {f"search_long_kernel<{w}, {nf}, {c}>" for w in ("unsigned int", "unsigned long") for nf in (1, 2, 4, 8) for c in ("false", "true")}
    jobs = {f"search_long_kernel<{w}, 8, false, true>" for w in ("unsigned int", "unsigned long")}
    assert got == one_job | jobs


def test_the_kernel_body_is_one_text():
    """both kernel templates include the one body; the body names no kernel of its own"""
    from conftest import ROOT
    src = open(os.path.join(ROOT, "commet_amd", "csrc", "long_search.hpp")).read()
    assert src.count('#include "long_search_body.hpp"') == 2
    assert "__global__" not in open(os.path.join(ROOT, "commet_amd", "csrc", "long_search_body.hpp")).read()
