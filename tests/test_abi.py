"""The C-ABI library loads and exports every entry point include/gaphuff.h
declares; without a GPU the decoder fails loudly (no CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared():
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src)))


def test_header_lists_expected_entry_points(gh):
    assert set(declared()) == set(gh.EXPORTED)


def test_library_exports_all(gh):
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in declared():
        assert hasattr(lib, name), name


def test_shape_and_sync_queries_declared_and_exported(gh):
    """The encoder's kernel-shape queries and the sync LUT width: in the header, in
    gh.EXPORTED, in the library and in the ctypes table (no device needed)."""
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in ("gh_ectx_kernel_shape", "gh_enc_kernel_shapes", "gh_enc_kernel_shape_for", "gh_sync_lut_bits"):
        assert name in declared() and name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert len(gh.enc_kernel_shapes()) == 14
    assert 1 <= gh.sync_lut_bits() <= 16


def test_version_and_error_strings(gh):
    assert b"gfx950" in gh.lib().gh_version()
    assert isinstance(gh.lib().gh_last_error(), bytes)


def test_no_gpu_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(gh.GapHuffError) as e:
        gh.Decoder(0)
    assert e.value.code == -5
    img = gh.encode(gh.generate(1, 0.5, 1000))
    with pytest.raises(gh.GapHuffError):
        gh.decode(img)


def test_no_gpu_encoder_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(gh.GapHuffError) as e:
        gh.Encoder(0)
    assert e.value.code == -5
    with pytest.raises(gh.GapHuffError):
        gh.encode_gpu(gh.generate(1, 0.5, 1000))
