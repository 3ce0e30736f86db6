"""Sliced encode on the device: gh_ectx_counts / gh_ectx_encode_slice /
gh_ectx_download_slice (gh_enc_write_kernel<NSW, SLICE = true>) and the one-shot
gh_encode_sharded.  The oracle is the host encoder (gh_encode_slice, gh_encode_write):
every slice's words and gap words word for word, every merged image byte for byte.
"""
import os
import subprocess

import numpy as np
import pytest

import slice_cases as sc
from test_encode_slices import shifted_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def enc(gpu):
    with gpu.Encoder(0) as e:
        yield e


def _same(got, want, what):
    assert got.size == want.size, what
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: "
                             f"{int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}")


# ---- 1. parity with the host: the matrix of tests/test_encode_slices.py
@pytest.mark.parametrize("name,label", sc.CASES)
def test_slices_equal_host(gpu, enc, name, label):
    data, plan, start, image = sc.case_input(gpu, name)
    b = sc.case_bounds(name, label, data.size)
    parts = []
    for i, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
        base, bits = int(start[lo]), int(start[hi] - start[lo])
        enc.load(data[lo:hi])
        s, ms = enc.encode_slice(plan, base)
        words, gapw = enc.download_slice()
        sc.check_extents_and_edges(gpu, s, words, gapw, base, bits)
        hs, hw, hg = gpu.encode_slice(data[lo:hi], plan, base)
        _same(words, hw, f"slice {i} [{lo}, {hi}) words")
        _same(gapw, hg, f"slice {i} [{lo}, {hi}) gap words")
        parts.append((s, words, gapw))
    order = np.random.default_rng(len(b)).permutation(len(parts))
    _same(gpu.merge_slices(plan, [parts[i] for i in order]), image, "merged image")


# ---- 2. shift invariance: base_bit >= 2^32
def test_shift_invariance_past_2_32(gpu, enc):
    data, plan, far, near = shifted_case(gpu)
    enc.load(data)
    for base in (far, near):
        s, _ = enc.encode_slice(plan, base)
        words, gapw = enc.download_slice()
        hs, hw, hg = gpu.encode_slice(data, plan, base)
        assert bytes(memoryview(s)) == bytes(memoryview(hs))
        _same(words, hw, f"words at base {base}")
        _same(gapw, hg, f"gap words at base {base}")


# ---- 3. the write kernel's persistent loop: more chunks than workgroups
def test_persistent_loop_two_large_slices(gpu, enc):
    n = 32 << 20  # 4096 chunks of 8 KiB a slice
    data = gpu.generate(91, 0.1, 2 * n)
    plan = gpu.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    base1 = int(lens[data[:n]].sum(dtype=np.uint64))
    parts = []
    for lo, base in ((0, 0), (n, base1)):
        enc.load(data[lo:lo + n])
        s, _ = enc.encode_slice(plan, base)
        parts.append((s,) + enc.download_slice())
    assert parts[0][0].bits == base1 and base1 + parts[1][0].bits == plan.bits
    _same(gpu.merge_slices(plan, parts), gpu.encode(data), "merged image")


def test_slice_longer_than_a_scan_block(gpu, enc):
    """The chunk offsets are scanned in blocks of 8192 chunks (64 MiB of input): a slice of
    two blocks at a non-zero base, so the base is carried into the second block's offset."""
    lo, n = (1 << 20) + 5, (65 << 20) + 17
    data = gpu.generate(92, 0.9, lo + n)
    plan = gpu.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    base = int(lens[data[:lo]].sum(dtype=np.uint64))
    parts = []
    for a, b, bb in ((0, lo, 0), (lo, lo + n, base)):
        enc.load(data[a:b])
        s, _ = enc.encode_slice(plan, bb)
        parts.append((s,) + enc.download_slice())
    hs, hw, hg = gpu.encode_slice(data[lo:], plan, base)
    _same(parts[1][1], hw, "words")
    _same(parts[1][2], hg, "gap words")
    _same(gpu.merge_slices(plan, parts), gpu.encode(data), "merged image")


# ---- 4. context reuse and state
def test_context_reuse_and_state(gpu):
    data = gpu.generate(17, 0.5, 300_001)
    host = gpu.encode(data)
    plan = gpu.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    lo = 100_003
    base = int(lens[data[:lo]].sum(dtype=np.uint64))
    with gpu.Encoder(0) as e:
        e.load(data)
        with pytest.raises(gpu.GapHuffError) as err:
            e.download_slice()  # nothing encoded yet
        assert err.value.code == -8
        e.make_plan()
        e.encode()
        _same(e.download(), host, "whole image, first")
        with pytest.raises(gpu.GapHuffError) as err:
            e.download_slice()  # the last encode was a whole one
        assert err.value.code == -8
        # a slice at a non-zero base
        e.load(data[lo:])
        assert np.array_equal(e.counts(), np.bincount(data[lo:], minlength=256).astype(np.uint64))
        with pytest.raises(gpu.GapHuffError) as err:
            e.encode()  # counts make no plan
        assert err.value.code == -8
        s, _ = e.encode_slice(plan, base)
        words, gapw = e.download_slice()
        hs, hw, hg = gpu.encode_slice(data[lo:], plan, base)
        _same(words, hw, "slice words")
        _same(gapw, hg, "slice gap words")
        e.plan = plan  # (Encoder.download sizes its buffer from it)
        for call in (e.download, e.index):
            with pytest.raises(gpu.GapHuffError) as err:
                call()
            assert err.value.code == -8
        # errors as the host's
        with pytest.raises(gpu.GapHuffError) as err:
            e.encode_slice(plan, base + 1)
        assert err.value.code == -1
        with pytest.raises(gpu.GapHuffError) as err:
            e.download_slice()  # the failed encode left no slice
        assert err.value.code == -8
        other = gpu.encode_plan(data[data != data[lo]])
        with pytest.raises(gpu.GapHuffError) as err:
            e.encode_slice(other, 0)
        assert err.value.code == -3
        # whole encode again, after a fresh plan
        e.load(data)
        e.make_plan()
        e.encode()
        _same(e.download(), host, "whole image, again")
        img, _ = e.index(8)
        assert np.array_equal(img, gpu.encode_index(data, 8))


# ---- 5. one-shot, CLI, roundtrip
@pytest.mark.parametrize("k", [1, 2, 5])
def test_encode_sharded_one_device(gpu, k):
    data, plan, start, image = sc.case_input(gpu, "gen")
    img, ms = gpu.encode_sharded(data, k, devices=[0] * k, return_ms=True)
    _same(img, image, f"{k} slices")
    assert ms > 0.0
    if k == 5:
        assert np.array_equal(gpu.decode(img), data)


def test_encode_sharded_edges(gpu):
    for data in (np.zeros(0, dtype=np.uint8), np.array([9], dtype=np.uint8), np.arange(5, dtype=np.uint8)):
        _same(gpu.encode_sharded(data, 3), gpu.encode(data), f"n = {data.size}")  # (empty slices)
    data = sc.case_input(gpu, "gen")[0]
    L = gpu.lib()
    import ctypes
    plan = gpu.gh_encode_plan()
    out = np.zeros(64, dtype=np.uint8)
    rc = L.gh_encode_sharded(data.ctypes.data, data.size, None, 2, 0, out.ctypes.data, out.size, ctypes.byref(plan), None)
    assert rc == -9 and plan.file_bytes == gpu.encode_plan(data).file_bytes  # the plan is filled first


def test_cli_slices(tmp_path, gpu):
    data = gpu.generate(4243, 0.9, 1_000_017)
    data.tofile(tmp_path / "in.bin")
    enc_bin = os.path.join(ROOT, "bin", "encoder")
    for out, extra in (("host.huff", []), ("sl.huff", ["--gpu", "0", "--slices", "3", "--write-index", str(tmp_path / "sl.idx")])):
        r = subprocess.run([enc_bin, str(tmp_path / "in.bin"), str(tmp_path / out)] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "sl.huff").read_bytes() == (tmp_path / "host.huff").read_bytes()
    assert np.array_equal(np.fromfile(tmp_path / "sl.idx", dtype=np.uint8), gpu.encode_index(data, 8))


# ---- 6. several devices
def test_encode_sharded_several_devices(gpu):
    nd = min(gpu.device_count(), 4)
    if nd < 2:
        pytest.skip("one device visible")
    data, plan, start, image = sc.case_input(gpu, "long")
    for k in (nd, 2 * nd + 1):
        _same(gpu.encode_sharded(data, k, devices=list(range(nd))), image, f"{k} slices on {nd} devices")
