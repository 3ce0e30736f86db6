"""The seek index of a sliced stream on the device: gh_ectx_index_slice
(gh_enc_index_kernel<SLICE = true>), the one-shot gh_encode_sharded_index and the CLI.  The
oracle is the host (gh_encode_index_slice entry for entry, gh_encode_index byte for byte),
itself checked against numpy in tests/test_index_slices.py.
"""
import os
import subprocess

import numpy as np
import pytest

import slice_cases as sc
from test_index_slices import big_origin_case, owned, straddled, whole_index

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = os.path.join(ROOT, "bin", "encoder")
GH_E_ARG, GH_E_STATE, GH_E_SMALL = -1, -8, -9
STRIDES = (8, 9, 12)


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    monkeypatch.delenv("GH_ENC_INDEX_GRID", raising=False)


@pytest.fixture(scope="module")
def enc(gpu):
    with gpu.Encoder(0) as e:
        yield e


def _same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: "
                             f"{int(got[bad[0]])} for {int(want[bad[0]])}")


def device_slices(gpu, enc, data, plan, start, bounds, strides=STRIDES, counts=True):
    """{k: [(entries, k0)]}: every slice loaded, encoded and indexed on the device at every
    stride, each against the host's gh_encode_index_slice."""
    parts = {k: [] for k in strides}
    for i, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        base = int(start[lo])
        enc.load(data[lo:hi])
        if counts:
            enc.counts()
        enc.encode_slice(plan, base)
        for k in strides:
            ent, k0, ms = enc.index_slice(lo, k)
            hent, hk0 = gpu.encode_index_slice(data[lo:hi], plan, base, lo, k)
            assert k0 == hk0, (i, k)
            _same(ent, hent, f"slice {i} [{lo}, {hi}) stride 2^{k}")
            parts[k].append((ent, k0))
    return parts


def merged(gpu, plan, k, parts, seed=0):
    order = np.random.default_rng(seed).permutation(len(parts))
    return gpu.merge_index_slices(plan, k, [parts[i] for i in order])


# ---- 1. the host matrix on the device
@pytest.mark.parametrize("name,label", sc.CASES)
def test_slices_equal_host(gpu, enc, name, label):
    data, plan, start, image = sc.case_input(gpu, name)
    b = sc.case_bounds(name, label, data.size)
    parts = device_slices(gpu, enc, data, plan, start, b)
    for k in STRIDES:
        _same(merged(gpu, plan, k, parts[k], len(b)), whole_index(gpu, name, k), f"merged index, stride 2^{k}")


def test_seams_on_boundaries(gpu, enc):
    data, plan, start, image = sc.case_input(gpu, "flat")
    b = [0, 4096, 4096, 4097, 8191, 8192, 12304, data.size]
    parts = device_slices(gpu, enc, data, plan, start, b)
    assert [(k0, e.tolist()) for e, k0 in parts[8]] == [(0, [0]), (1, []), (1, [4096]), (2, []), (2, []),
                                                        (2, [8192, 12288]), (4, [])]
    for k in STRIDES:
        _same(merged(gpu, plan, k, parts[k]), gpu.encode_index(data, k), f"stride 2^{k}")


@pytest.mark.parametrize("shift", [0, 1])
def test_boundaries_inside_codewords(gpu, enc, shift):
    data, plan, start, image = sc.case_input(gpu, "long")
    ks, offs = straddled(gpu)
    b = [0] + [o - shift for o in offs] + [data.size]
    parts = device_slices(gpu, enc, data, plan, start, b, strides=(8,))[8]
    for i, (j, o) in enumerate(zip(ks, offs)):
        ent, k0 = parts[i + shift]
        if shift == 0:
            assert k0 + ent.size - 1 == j and int(ent[-1]) == o  # the slice's sym_base + n
        else:
            assert k0 == j and int(ent[0]) == o                  # its sym_base + 1
    _same(merged(gpu, plan, 8, parts), whole_index(gpu, "long", 8), "merged index")


def test_origins_past_2_32(gpu, enc):
    data, plan, base, sym, start = big_origin_case(gpu)
    enc.load(data)
    enc.encode_slice(plan, base)
    for k in STRIDES:
        ent, k0, _ = enc.index_slice(sym, k)
        wk0, want = owned(start, 0, data.size, sym, k)
        assert k0 == wk0
        _same(ent, want, f"stride 2^{k}")
    assert enc.index_slice(sym, 8)[0].size >= 2


# ---- 2. slice lengths around one thread (16 bytes) and one chunk (8192 bytes)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 8191, 8192, 8193, 16385])
def test_slice_lengths(gpu, enc, n):
    data, plan, start, image = sc.case_input(gpu, "gen")
    b = [0, 70001, 70001 + n, data.size]
    assert int(start[70001]) % 1024 and int(start[70001]) % 32  # an unaligned non-zero base_bit
    parts = device_slices(gpu, enc, data, plan, start, b, counts=False)
    for k in STRIDES:
        _same(merged(gpu, plan, k, parts[k]), gpu.encode_index(data, k), f"stride 2^{k}")


# ---- 3. few workgroups, many chunks each
@pytest.mark.parametrize("grid", ["1", "2"])
def test_few_workgroups(gpu, monkeypatch, grid):
    data = gpu.generate(55, 0.5, 50_003 + 40 * 8192)
    plan = gpu.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    start = np.concatenate([[0], np.cumsum(lens[data], dtype=np.uint64)]).astype(np.uint64)
    monkeypatch.setenv("GH_ENC_INDEX_GRID", grid)
    with gpu.Encoder(0) as e:
        parts = device_slices(gpu, e, data, plan, start, [0, 50_003, data.size])
    for k in STRIDES:
        _same(merged(gpu, plan, k, parts[k]), gpu.encode_index(data, k), (grid, k))


# ---- 4. the slice crosses a scan block (8192 chunks) on top of base_bit
def test_second_slice_crosses_a_scan_block(gpu, enc):
    lo, n = (1 << 20) + 5, (64 << 20) + 12345  # 8193 chunks
    data = gpu.generate(92, 0.9, lo + n)
    plan = gpu.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    base = int(lens[data[:lo]].sum(dtype=np.uint64))
    parts = {8: [], 12: []}
    for a, b, bb in ((0, lo, 0), (lo, lo + n, base)):
        enc.load(data[a:b])
        enc.encode_slice(plan, bb)
        for k in parts:
            ent, k0, _ = enc.index_slice(a, k)
            hent, hk0 = gpu.encode_index_slice(data[a:b], plan, bb, a, k)
            assert k0 == hk0
            _same(ent, hent, f"slice at {a}, stride 2^{k}")
            parts[k].append((ent, k0))
    for k in parts:
        _same(merged(gpu, plan, k, parts[k]), gpu.encode_index(data, k), f"merged, stride 2^{k}")


# ---- 5. state
def test_state(gpu):
    data, plan, start, image = sc.case_input(gpu, "gen")
    lo = 100_003
    base = int(start[lo])

    def refused(e, code=GH_E_STATE):
        with pytest.raises(gpu.GapHuffError) as err:
            e.index_slice(lo, 8)
        assert err.value.code == code

    with gpu.Encoder(0) as e:
        refused(e)  # fresh
        e.load(data[lo:])
        refused(e)  # loaded
        e.counts()
        refused(e)  # counted
        e.encode_slice(plan, base)
        words, gapw = e.download_slice()
        # two strides after one slice encode, repeated
        for k in (8, 12, 8):
            ent, k0, ms = e.index_slice(lo, k)
            hent, hk0 = gpu.encode_index_slice(data[lo:], plan, base, lo, k)
            assert k0 == hk0 and ms >= 0.0
            _same(ent, hent, f"stride 2^{k}")
        # the slice's words are untouched by the index
        w2, g2 = e.download_slice()
        assert np.array_equal(w2, words) and np.array_equal(g2, gapw)
        # the whole-stream index stays refused after a slice encode
        e.plan = plan
        with pytest.raises(gpu.GapHuffError) as err:
            e.index(8)
        assert err.value.code == GH_E_STATE
        # a short buffer: the extents all the same
        import ctypes
        k0, nk = ctypes.c_uint64(), ctypes.c_uint64()
        L = gpu.lib()
        assert L.gh_ectx_index_slice(e._h, lo, 8, None, 0, ctypes.byref(k0), ctypes.byref(nk), None) == GH_E_SMALL
        assert (k0.value, nk.value) == gpu.index_slice_extent(base, plan.bits - base, 8)
        for k in (7, 21):
            assert L.gh_ectx_index_slice(e._h, lo, k, None, 0, ctypes.byref(k0), ctypes.byref(nk), None) == GH_E_ARG
        e.load(data[lo:])
        refused(e)  # reloaded
        e.load(data)
        e.make_plan()
        refused(e)  # planned
        e.encode()
        refused(e)  # a whole encode is no slice encode
        assert np.array_equal(e.index(8)[0], whole_index(gpu, "gen", 8))
    # an empty slice owns nothing and launches nothing
    with gpu.Encoder(0) as e:
        e.load(data[:0])
        e.encode_slice(plan, base)
        ent, k0, ms = e.index_slice(lo, 8)
        assert ent.size == 0 and k0 == -(-base // (128 << 8))


# ---- 6. one call
@pytest.mark.parametrize("K", [1, 3, 7])
def test_encode_sharded_with_index(gpu, K):
    data, plan, start, image = sc.case_input(gpu, "gen")
    for k in (8, 9):
        img, idx = gpu.encode_sharded(data, K, index_log2_stride=k)
        _same(img, image, f"{K} slices: image")
        _same(idx, whole_index(gpu, "gen", k), f"{K} slices: index, stride 2^{k}")
    img, ms, idx = gpu.encode_sharded(data, K, return_ms=True, index_log2_stride=12)
    assert ms > 0.0
    _same(idx, gpu.encode_index(data, 12), "stride 2^12")
    # without a stride: what it returned before
    assert isinstance(gpu.encode_sharded(data, K), np.ndarray)
    with pytest.raises(gpu.GapHuffError) as err:
        gpu.encode_sharded(data, K, index_log2_stride=21)
    assert err.value.code == GH_E_ARG


def test_encode_sharded_with_index_edges(gpu):
    for data in (np.zeros(0, dtype=np.uint8), np.array([9], dtype=np.uint8), np.arange(5, dtype=np.uint8)):
        img, idx = gpu.encode_sharded(data, 3, index_log2_stride=8)
        _same(img, gpu.encode(data), f"n = {data.size}")
        _same(idx, gpu.encode_index(data, 8), f"n = {data.size}: index")
    data = sc.case_input(gpu, "gen")[0]
    import ctypes
    L = gpu.lib()
    plan = gpu.gh_encode_plan()
    out = np.zeros(int(L.gh_encode_bound(data.size)), dtype=np.uint8)
    idx = np.zeros(48, dtype=np.uint8)
    rc = L.gh_encode_sharded_index(data.ctypes.data, data.size, None, 2, 0, out.ctypes.data, out.size,
                                   ctypes.byref(plan), None, 8, idx.ctypes.data, idx.size, None)
    assert rc == GH_E_SMALL and plan.g == gpu.encode_plan(data).g and not idx.any()


def test_encode_sharded_with_index_two_devices(gpu):
    if gpu.device_count() < 2:
        pytest.skip("one device visible")
    data, plan, start, image = sc.case_input(gpu, "long")
    for K in (2, 5):
        img, idx = gpu.encode_sharded(data, K, devices=[0, 1], index_log2_stride=8)
        _same(img, image, f"{K} slices on 2 devices")
        _same(idx, whole_index(gpu, "long", 8), f"{K} slices on 2 devices: index")


# ---- 7. the CLI
def test_cli_slices_write_index(gpu, tmp_path):
    data = gpu.generate(4243, 0.9, 3_000_017)
    src, out, idx = tmp_path / "in.bin", tmp_path / "c.huff", tmp_path / "c.ghidx"
    data.tofile(src)
    r = subprocess.run([ENCODER, str(src), str(out), "--gpu", "0", "--slices", "3", "--write-index", str(idx),
                        "--index-stride", "9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Original size: 3000017 bytes" in r.stdout
    want = gpu.encode_index(data, 9)
    assert f"Index: {(want.size - 40) // 8} entries, stride 2^9, {want.size} bytes" in r.stdout
    assert [l.split(":")[0] for l in r.stdout.splitlines()] == [
        "Input file", "Original size", "Compressed size", "Encode kernel time", "Total encode time", "Throughput", "Index"]
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), gpu.encode(data))
    assert np.array_equal(np.fromfile(idx, dtype=np.uint8), want)
    bad = subprocess.run([ENCODER, str(src), str(out), "--gpu", "0", "--slices", "3", "--write-index", str(idx),
                          "--index-stride", "21"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "stride" in bad.stderr
