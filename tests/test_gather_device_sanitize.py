"""The device gather plan's arithmetic under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/gather_device_fuzz.cpp, a stand-alone program, with the library's host
sources with -fsanitize=address,undefined and no recovery.  The program runs the functions
of csrc/gh_gather_range.hpp -- the text the planning kernels compile -- on the CPU: locate
over random ranges, a serial scan, emit into a piece buffer of exactly
gh_gather_piece_bound pieces, over random valid index images, and checks the pieces, their
count and the byte total against gh_gather_plan.
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
    assert os.path.exists(os.path.join(ASAN, "gather_device_fuzz"))
    return ASAN


def test_gather_device_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "gather_device_fuzz"), "20000", "17"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
