"""The batched gather plan's arithmetic under AddressSanitizer + UBSan (CPU only).

`make asan` (cse375-finalproj-huffman-decoding_amd/Makefile) builds
tests/sanitize/batch_gather_fuzz.cpp, a stand-alone program, with the library's host
sources with -fsanitize=address,undefined and no recovery.  The program runs the functions
of csrc/gh_batch_range.hpp -- the text the planning kernels compile -- on the CPU, item by
item as the kernels' threads do: locate per range, a serial scan, emit per piece into a
piece buffer of exactly gh_gather_piece_bound pieces, over random batches, and checks the
pieces, their count, the byte total and the flagged-range count against gh_batchdec_plan.
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
    assert os.path.exists(os.path.join(ASAN, "batch_gather_fuzz"))
    return ASAN


def test_batch_gather_fuzz_under_asan(asan_build):
    r = subprocess.run([os.path.join(asan_build, "batch_gather_fuzz"), "20000", "17"], capture_output=True,
                       text=True, timeout=600, env=ENV)
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]
    assert r.returncode == 0 and "iterations ok" in r.stdout, text[-2000:]
