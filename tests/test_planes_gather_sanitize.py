"""The element gather's host code under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/planes_gather_fuzz.cpp, a stand-alone program, with the library's host sources
(gh_core.cpp holds gh_pgather_plan; csrc/gh_planes_gather.hpp is the text the kernels compile
too) with -fsanitize=address,undefined and no recovery.  The program plans random tensor lists
and element ranges in heap blocks of exact size against a naive recomputation and every refusal,
then runs the range join's per-lane text over every lane of those ranges, with the staging
buffer, the stored arena and the destination in heap blocks of exact size, against the scalar
rule.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cse375-finalproj-huffman-decoding_amd")
ASAN = os.path.join(PKG, "build", "asan")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def asan_build():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(os.path.join(ASAN, "planes_gather_fuzz"))
    return ASAN


def test_planes_gather_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "planes_gather_fuzz"), "2000", "23"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
