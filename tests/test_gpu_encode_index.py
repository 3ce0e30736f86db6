"""The seek index from the GPU encoder: gh_ectx_index (gh_enc_index_kernel).

Encoder.index is compared byte for byte with the host's gh.encode_index (itself checked
against the data in test_encode_index), with Decoder.build_index of the encoded image,
and, for the streams whose expected offsets are cheap to compute, with the data: code
lengths from the image's symbol list, an exclusive cumsum, searchsorted "left", N.

Sizes at the kernel's edges (a thread holds 16 bytes, a chunk 8192): N around one
thread, one chunk and two chunks; uniform 256-symbol data (8-bit code: every chunk start
and every thread start is a boundary candidate); the 1..16-bit ladder; the one-symbol code
(1 bit per byte: fewer than one boundary per chunk, the skip path); one and two
workgroups over 40 chunks; a stream that crosses a scan block of 8192 chunks; and (slow)
bit positions past 2^32."""
import os
import subprocess

import numpy as np
import pytest

from test_encode_index import CODES, GEN, STREAMS, _coded, _expected, _make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = os.path.join(ROOT, "bin", "encoder")
STRIDES = (8, 9, 12, 20)
GH_E_ARG, GH_E_STATE, GH_E_SMALL = -1, -8, -9
ENV_KNOBS = ("GH_ENC_INDEX_GRID", "GH_INDEX_GRID", "GH_MODE")

_cache = {}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture
def case(gpu, request):
    """(name, data), made once."""
    name = request.param
    if name not in _cache:
        data = _make(gpu, name)
        data.setflags(write=False)
        _cache[name] = (name, data)
    return _cache[name]


def _encoded(gh, e, data, force_version=0):
    e.load(data)
    e.make_plan(force_version)
    e.encode()


def _same(got, want, what):
    assert got.size == want.size, what
    if not np.array_equal(got, want):
        a, b = got[40:].view("<u8"), want[40:].view("<u8")
        bad = np.nonzero(a != b)[0]
        raise AssertionError(f"{what}: header equal {np.array_equal(got[:40], want[:40])}, {bad.size} of {a.size} "
                             f"entries differ, first {bad[:4]}: {a[bad[:4]]} != {b[bad[:4]]}")


# ---- the index ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_index_equals_the_host_index(gpu, case):
    name, data = case
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        for k in STRIDES:
            image, ms = e.index(k)
            _same(image, gpu.encode_index(data, k), (name, k))
            gpu.parse_index(image)
            assert ms >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", [*GEN, *CODES], indirect=True)
def test_index_equals_build_index(gpu, case):
    name, data = case
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        image, _ = e.index(8)
        img = e.download()
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        _same(image, d.build_index(8)[0], name)
    assert np.array_equal(gpu.parse_index(image).offsets, _expected(gpu, data, img, 8))


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0.1, 0.9])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 8191, 8192, 8193, 16385, 65549])
def test_edge_sizes(gpu, r, n):
    data = gpu.generate(4000 + n, r, n)
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        for k in (8, 9):
            _same(e.index(k)[0], gpu.encode_index(data, k), (n, r, k))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [1, 4, 9])
def test_uniform_bytes_every_thread_start_is_a_boundary_candidate(gpu, chunks):
    """256 symbols, each as often as the others: an 8-bit code, so thread t of chunk c
    starts at bit 65536 c + 128 t and every boundary is a thread's first bit (count 0)."""
    n = 8192 * chunks
    data = np.random.default_rng(chunks).permutation(np.arange(n, dtype=np.int64) % 256).astype(np.uint8)
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        assert {l for _, l in gpu.parse(e.download()).symbols} == {8}
        for k in (8, 9, 10):
            image, _ = e.index(k)
            _same(image, gpu.encode_index(data, k), (chunks, k))
            off = gpu.parse_index(image).offsets
            assert np.array_equal(off[:-1], np.arange(off.size - 1, dtype=np.uint64) * (16 << k))


@pytest.mark.gpu
def test_boundaries_per_chunk(gpu):
    """A ladder with 128 symbols of 16 bits (lengths 1..9 and 128 x 16; at N = 2^23 they
    occur 16384 times), its 16-bit symbols gathered into two whole chunks: 131072 bits each,
    four to five boundaries of stride 2^8 per chunk.  And the one-symbol code: a boundary
    every fourth chunk."""
    data, lens = _coded({**{l: 1 for l in range(1, 10)}, 16: 128}, 1 << 23, seed=3)
    is16 = np.asarray([lens.get(v, 0) == 16 for v in range(256)])[data]
    rest, run = data[~is16], data[is16]
    assert run.size == 2 * 8192
    heavy = np.concatenate([rest[:100 * 8192], run, rest[100 * 8192:]])
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, heavy)
        assert dict(gpu.parse(e.download()).symbols) == lens
        image, _ = e.index(8)
        _same(image, gpu.encode_index(heavy, 8), "ladder, 16-bit chunks")
        # chunks 100 and 101 hold 4 x 32768 bits each: 4 boundaries, 5 when the first bit is one
        length_of = np.asarray([lens.get(v, 0) for v in range(256)])
        assert (length_of[heavy[100 * 8192: 102 * 8192]] == 16).all()
        o100 = int(length_of[heavy[:100 * 8192]].sum())
        assert -(-(o100 + 131072) // 32768) - -(-o100 // 32768) in (4, 5)
        one = np.full(40 * 8192, 65, dtype=np.uint8)
        _encoded(gpu, e, one)
        for k in (8, 10):
            image, _ = e.index(k)
            _same(image, gpu.encode_index(one, k), ("one symbol", k))
        off = gpu.parse_index(e.index(8)[0]).offsets
        assert np.array_equal(off[:-1], np.arange(off.size - 1, dtype=np.uint64) * 32768)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", ["1", "2"])
def test_few_workgroups(gpu, monkeypatch, grid):
    """One and two workgroups walk 41 chunks (each scans many chunks, skipped ones between
    them at stride 2^12)."""
    data = gpu.generate(55, 0.5, 40 * 8192 + 77)
    monkeypatch.setenv("GH_ENC_INDEX_GRID", grid)
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        for k in (8, 9, 12):
            _same(e.index(k)[0], gpu.encode_index(data, k), (grid, k))


@pytest.mark.gpu
def test_crosses_a_scan_block(gpu):
    """N = 64 MiB + 12 345: 8193 chunks, so the last chunk's offset is the second scan
    block's (non-zero) offset plus its local one."""
    data = gpu.generate(64, 0.5, (64 << 20) + 12_345)
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        for k in (8, 11):
            _same(e.index(k)[0], gpu.encode_index(data, k), k)


@pytest.mark.gpu
@pytest.mark.slow
def test_bit_positions_past_2_32(gpu):
    """N = 2^29 + 2^20 at r = 0.0 (about 8 bits per byte): payload bit positions pass 2^32.
    Compared with the decoder's index of the encoded image, on the device."""
    data = gpu.generate(29, 0.0, (1 << 29) + (1 << 20))
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        assert e.plan.bits > 1 << 32
        img = e.download()
        got = {k: e.index(k)[0] for k in (8, 12)}
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for k, image in got.items():
            _same(image, d.build_index(k)[0], k)


# ---- state ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_state(gpu):
    a = gpu.generate(1, 0.5, 100_003)
    b = gpu.generate(2, 0.9, 250_001)
    with gpu.Encoder(0) as e:
        for step in ("fresh", "loaded", "planned"):
            with pytest.raises(gpu.GapHuffError) as err:
                e.index(8)
            assert err.value.code == GH_E_STATE, step
            if step == "fresh":
                e.load(a)
            elif step == "loaded":
                e.make_plan()
        e.encode()
        img = e.download()
        # two strides after one encode, and the download is unchanged
        _same(e.index(8)[0], gpu.encode_index(a, 8), "a, 2^8")
        _same(e.index(10)[0], gpu.encode_index(a, 10), "a, 2^10")
        _same(e.index(8)[0], gpu.encode_index(a, 8), "a, 2^8 again")
        assert np.array_equal(e.download(), img) and np.array_equal(img, gpu.encode(a))
        # refusals leave the state as it was
        need = int(gpu.lib().gh_index_bytes(e.plan.g, 8))
        buf = np.zeros(need, dtype=np.uint8)
        for k in (7, 21):
            assert gpu.lib().gh_ectx_index(e._h, k, buf.ctypes.data, buf.size, None) == GH_E_ARG
        assert gpu.lib().gh_ectx_index(e._h, 8, buf.ctypes.data, need - 1, None) == GH_E_SMALL
        assert gpu.lib().gh_ectx_index(e._h, 8, None, need, None) == GH_E_ARG
        assert gpu.lib().gh_ectx_index(e._h, 8, buf.ctypes.data, need, None) == 0
        _same(buf, gpu.encode_index(a, 8), "a, raw call")
        # a reload invalidates it, and so does a new plan
        e.load(b)
        with pytest.raises(gpu.GapHuffError) as err:
            e.index(8)
        assert err.value.code == GH_E_STATE
        e.make_plan()
        with pytest.raises(gpu.GapHuffError) as err:
            e.index(8)
        assert err.value.code == GH_E_STATE
        # encode -> index -> encode of another input -> index
        e.encode()
        _same(e.index(9)[0], gpu.encode_index(b, 9), "b, 2^9")
        assert np.array_equal(e.download(), gpu.encode(b))
        _encoded(gpu, e, a, force_version=2)
        _same(e.index(8)[0], gpu.encode_index(a, 8), "a again, v2 header")


@pytest.mark.gpu
def test_empty_input(gpu):
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, np.zeros(0, dtype=np.uint8))
        image, ms = e.index(8)
        assert gpu.parse_index(image).offsets.tolist() == [0]
        _same(image, gpu.encode_index(b"", 8), "empty")


# ---- round trip -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_gather_through_the_encoders_index(gpu):
    data = gpu.generate(12, 0.5, 1_000_003)
    with gpu.Encoder(0) as e:
        _encoded(gpu, e, data)
        img, index = e.download(), e.index(8)[0]
    rng = np.random.default_rng(8)
    lo = rng.integers(0, data.size, size=300)
    ranges = [(int(a), int(min(a + rng.integers(0, 5000), data.size))) for a in lo]
    ranges += [(0, 0), (0, 1), (data.size - 1, data.size), (data.size, data.size)]
    got = gpu.decode_ranges(img, index, ranges)
    assert len(got) == len(ranges)
    for (a, b), g in zip(ranges, got):
        assert np.array_equal(g, data[a:b]), (a, b)


# ---- the CLI ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_gpu_write_index(gpu, tmp_path):
    data = gpu.generate(4243, 0.9, 3_000_017)
    src, out, idx = tmp_path / "in.bin", tmp_path / "c.huff", tmp_path / "c.ghidx"
    data.tofile(src)
    r = subprocess.run([ENCODER, str(src), str(out), "--gpu", "0", "--write-index", str(idx), "--index-stride", "9"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Original size: 3000017 bytes" in r.stdout
    want = gpu.encode_index(data, 9)
    assert f"Index: {(want.size - 40) // 8} entries, stride 2^9, {want.size} bytes" in r.stdout
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), gpu.encode(data))
    assert np.array_equal(np.fromfile(idx, dtype=np.uint8), want)
    bad = subprocess.run([ENCODER, str(src), str(out), "--gpu", "0", "--write-index", str(idx), "--index-stride", "21"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "stride" in bad.stderr
