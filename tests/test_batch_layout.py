"""Batched decode without a GPU: the output layout (gh_batch_layout against a numpy
restatement), its refusals, the new entry points in the header / EXPORTED / the library, the
loud failure of BatchDecoder without a device, and the batch kernel names."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_ARG = -1
BATCH_NAMES = ("gh_batch_create", "gh_batch_destroy", "gh_batch_layout", "gh_batch_load", "gh_batch_load_device",
               "gh_batch_decode", "gh_batch_wait", "gh_batch_status", "gh_batch_output", "gh_batch_offsets",
               "gh_batch_download", "gh_batch_kernel_shape", "gh_batch_kernel_shapes")


def _layout(ns):
    """out_off[i] = sum_{j<i} round_up(n_j, 16); out_off[len] = the arena size."""
    n = np.asarray(ns, dtype=np.uint64)
    padded = (n + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(padded, dtype=np.uint64)])


@pytest.mark.parametrize("ns", [[], [0], [1], [16], [17, 0, 15, 16]], ids=str)
def test_layout_small(gh, ns):
    got = gh.batch_layout(ns)
    assert got.dtype == np.uint64 and np.array_equal(got, _layout(ns))
    assert (got % 16 == 0).all()


def test_layout_random(gh):
    rng = np.random.default_rng(375)
    ns = np.where(rng.random(1000) < 0.1, 0, rng.integers(0, 1 << 20, 1000)).astype(np.uint64)
    ns[::97] = rng.integers(1 << 33, 1 << 40, ns[::97].size)  # past 32 bits
    got = gh.batch_layout(ns)
    assert np.array_equal(got, _layout(ns))
    assert (np.diff(got) >= ns).all() and (np.diff(got) - ns < 16).all()


def test_layout_refusals(gh):
    L = gh.lib()
    off = np.zeros(4, dtype=np.uint64)
    n = np.asarray([1, 2, 3], dtype=np.uint64)
    assert L.gh_batch_layout(None, 3, off.ctypes.data) == GH_E_ARG
    assert L.gh_batch_layout(n.ctypes.data, 3, None) == GH_E_ARG
    assert L.gh_batch_layout(None, 0, None) == GH_E_ARG
    assert L.gh_batch_layout(None, 0, off.ctypes.data) == 0 and off[0] == 0
    # a single size whose rounding overflows, and a sum that does
    for bad in ([(1 << 64) - 1], [(1 << 64) - 15], [1 << 63, 1 << 63], [(1 << 64) - 32, 8, 17]):
        with pytest.raises(gh.GapHuffError) as e:
            gh.batch_layout(np.asarray(bad, dtype=np.uint64))
        assert e.value.code == GH_E_ARG
    # the largest arena that fits
    assert int(gh.batch_layout([(1 << 64) - 32, 16])[-1]) == (1 << 64) - 16


def test_batch_names_declared_and_exported(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in BATCH_NAMES:
        assert name in declared and name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert {n for n in declared if n.startswith("gh_batch_")} == set(BATCH_NAMES)
    for t in ("gh_batch_item", "gh_batch_report", "gh_batch"):
        assert re.search(r"\b%s;" % t, src), t
    assert ctypes.sizeof(gh.gh_batch_item) == 56 and ctypes.sizeof(gh.gh_batch_report) == 32


def test_no_gpu_batch_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(gh.GapHuffError) as e:
        gh.BatchDecoder(0)
    assert e.value.code == -5
    with pytest.raises(gh.GapHuffError):
        gh.decode_batch([gh.encode(gh.generate(1, 0.5, 1000))])


def test_batch_kernel_shapes(gh):
    names = gh.batch_kernel_shapes()
    assert names and len(set(names)) == len(names)
    assert not set(names) & set(gh.kernel_shapes())
    assert not set(names) & set(gh.enc_kernel_shapes())
