"""The level-by-level package-merge under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/pm_flat_fuzz.cpp, a stand-alone program, with the library's host sources
(gh_core.cpp holds gh_package_merge and gh_package_merge_flat) and csrc/gh_pm_flat.hpp, the
header the batched encoder's code kernel compiles for the device, with
-fsanitize=address,undefined and no recovery.  The program compares the two forms' lengths
over random histograms, drives the levels item by item as the kernel's threads do (every
position filled exactly once, no level longer than 2n - 2 items, sorted lists), checks a Kraft
sum of exactly 1 and the canonical entries against build_canon.
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
    assert os.path.exists(os.path.join(ASAN, "pm_flat_fuzz"))
    return ASAN


def test_pm_flat_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "pm_flat_fuzz"), "4000", "17"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
