"""Batched encode without a GPU: the new entry points in the header / EXPORTED / the library /
the ctypes table, the unit size, the kernel names, and the loud failure of BatchEncoder (and
BatchDecoder) without a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EBATCH_NAMES = ("gh_ebatch_create", "gh_ebatch_destroy", "gh_ebatch_load", "gh_ebatch_load_device",
                "gh_ebatch_plan", "gh_ebatch_plan_of", "gh_ebatch_encode", "gh_ebatch_wait", "gh_ebatch_sizes",
                "gh_ebatch_download", "gh_ebatch_items", "gh_ebatch_kernel_shape", "gh_ebatch_kernel_shapes")


def _header():
    return open(os.path.join(ROOT, "include", "gaphuff.h")).read()


def test_ebatch_names_declared_and_exported(gh):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in EBATCH_NAMES:
        assert name in declared and name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert {n for n in declared if n.startswith("gh_ebatch_")} == set(EBATCH_NAMES)
    for t in ("gh_ebatch_item", "gh_ebatch_report", "gh_ebatch"):
        assert re.search(r"\b%s;" % t, src), t
    assert ctypes.sizeof(gh.gh_ebatch_item) == 16 and ctypes.sizeof(gh.gh_ebatch_report) == 40


def test_unit_bytes_matches_header(gh):
    m = re.search(r"#define\s+GH_EBATCH_UNIT_BYTES\s+(\d+)", _header())
    assert m and int(m.group(1)) == gh.GH_EBATCH_UNIT_BYTES == 1024


def test_ebatch_kernel_shapes(gh):
    names = gh.ebatch_kernel_shapes()
    assert names and len(set(names)) == len(names)
    assert all(n.startswith("ebatch<") for n in names)
    assert not set(names) & set(gh.kernel_shapes())
    assert not set(names) & set(gh.enc_kernel_shapes())
    assert not set(names) & set(gh.batch_kernel_shapes())


def test_no_gpu_ebatch_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(gh.GapHuffError) as e:
        gh.BatchEncoder(0)
    assert e.value.code == -5
    with pytest.raises(gh.GapHuffError) as e:
        gh.BatchDecoder(0)
    assert e.value.code == -5
    with pytest.raises(gh.GapHuffError):
        gh.encode_batch([gh.generate(1, 0.5, 1000)])
