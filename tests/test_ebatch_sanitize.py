"""The batched encode's host layout under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/ebatch_fuzz.cpp, a stand-alone program, with the library's host sources
(gh_core.cpp holds gh::ebatch_in_plan and gh::ebatch_out_plan) with
-fsanitize=address,undefined and no recovery.  The program lays out random batches (empty
inputs, inputs at the lane edges and at the work-unit edges n = unit - 1, unit, unit + 1),
checks every extent against a naive recomputation, 16-byte alignment, that padded extents
never overlap, the unit prefix, and that the limits are refused.
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
    assert os.path.exists(os.path.join(ASAN, "ebatch_fuzz"))
    return ASAN


def test_ebatch_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "ebatch_fuzz"), "20000", "17"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
