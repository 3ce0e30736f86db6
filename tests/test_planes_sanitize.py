"""The byte planes' host code under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/planes_fuzz.cpp, a stand-alone program, with the library's host sources
(gh_core.cpp holds gh_planes_layout, the host twins and the container's writer and parser;
csrc/gh_planes.hpp is the text the kernels compile too) with -fsanitize=address,undefined and
no recovery.  The program lays out random tensor lists and checks them against a naive
recomputation and every refusal; runs the twins with the tensor and every plane in heap
blocks of exact size against the scalar rule, and the vector rule on random groups; writes
containers and parses the valid image, truncations of it and bit-flipped copies, reading
every view a successful parse returns.
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
    assert os.path.exists(os.path.join(ASAN, "planes_fuzz"))
    return ASAN


def test_planes_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "planes_fuzz"), "400", "17"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
