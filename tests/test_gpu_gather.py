"""Batched range gather on the GPU: gh_ctx_gather / Decoder.gather / decode_ranges and
the decoder CLI's --ranges.

Every gather is compared with np.concatenate([data[lo:hi] ...]) of the original bytes.
The streams are those of tests/test_gpu_index.py (its small helpers are copied here):
gh_generate at r = 0.1 / 0.5 / 0.9; prescribed codes (a 1..16-bit ladder: a 1-bit
codeword, 16-bit codewords, the canonical fallback, up to 143 symbols in a segment; the
one-symbol code, which is incomplete; a grouped 4/8-bit code; a 2..7-bit ladder); three
goldens (G = 1 twice, exactly one full index block); one stream with G = 256 k + 1.
Strides: 2^8 (one wave block per index block) and 2^10 (the running position across four
wave blocks, the count-only skip and the early exit)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DECODER = os.path.join(ROOT, "bin", "decoder")
N_GEN = 300_000
N_CODE = 1 << 18
ENV_KNOBS = ("GH_MODE", "GH_TILE_GRID", "GH_TILE_SCAP", "GH_TILE_SCAPF", "GH_WS_K", "GH_WS_KC", "GH_WS_NS",
             "GH_WS_GRID", "GH_WS_STAGE", "GH_WS_LGC", "GH_MT_KC", "GH_MT_CLGR", "GH_LUT_BITS", "GH_LGR",
             "GH_TILE_IDLE", "GH_INDEX_GRID", "GH_GATHER_GRID")
GH_E_ARG, GH_E_STATE, GH_E_SMALL = -1, -8, -9


# ---- prescribed codes (the dyadic construction of test_gpu_shapes._stream) ------------
def _ladder(lo, hi, first=1):
    code = {lo: first}
    for l in range(lo + 1, hi):
        code[l] = 1
    left = 1.0 - sum(c * 2.0 ** -l for l, c in code.items())
    code[hi] = round(left * 2 ** hi)
    return code


def _coded(code, n, seed):
    """n bytes whose histogram forces `code` ({length: symbols}): symbol i occurs
    m * 2^(maxlen - len_i) times, shuffled."""
    lens = np.asarray([l for l in sorted(code) for _ in range(code[l])])
    vals = ((np.arange(len(lens)) * 37 + 11) % 256).astype(np.uint8)
    if len(lens) == 1:
        return np.repeat(vals, n), dict(zip(vals.tolist(), lens.tolist()))
    assert sum(2.0 ** -l for l in lens) == 1.0
    m, rem = divmod(n, 1 << int(lens.max()))
    assert m >= 1 and rem == 0
    data = np.random.default_rng(seed).permutation(np.repeat(vals, m * (1 << (int(lens.max()) - lens))))
    return data, dict(zip(vals.tolist(), lens.tolist()))


CODES = {
    "ladder_1_16": _ladder(1, 16),
    "one_symbol": {1: 1},
    "grouped_4_8": {4: 2, 8: 224},
    "ladder_2_7": _ladder(2, 7, 3),
}
GOLDENS = ("gen_r0.9_n1", "gen_r0.5_n7", "uniform256_exact_segments")
GEN = {"gen_r0.1": 0.1, "gen_r0.5": 0.5, "gen_r0.9": 0.9}
STREAMS = (*GEN, *CODES, *GOLDENS, "g_256k_plus_1")

_cache = {}


def _lengths(gh, img):
    length_of = np.zeros(256, dtype=np.int64)
    for sym, l in gh.parse(img).symbols:
        length_of[sym] = l
    return length_of


def _make(gh, name):
    if name in GEN:
        data = gh.generate(375 + int(GEN[name] * 10), GEN[name], N_GEN)
        return data, gh.encode(data)
    if name in CODES:
        data, want = _coded(CODES[name], N_CODE, seed=len(name))
        img = gh.encode(data)
        assert dict(gh.parse(img).symbols) == want, "package-merge did not return the prescribed lengths"
        return data, img
    if name in GOLDENS:
        return (np.fromfile(os.path.join(GOLDEN, name + ".bin"), dtype=np.uint8),
                np.fromfile(os.path.join(GOLDEN, name + ".huff"), dtype=np.uint8))
    # G = 256 k + 1: cut a generated stream where its bits fill 256 k + 1 segments
    data = gh.generate(77, 0.5, 100_000)
    bits = _lengths(gh, gh.encode(data))[data]
    g = -(-int(bits.sum()) // 128)
    target = (g - 1) // 256 * 256 + 1
    n = int(np.searchsorted(np.cumsum(bits), 128 * target, "right"))
    data = data[:n].copy()
    img = gh.encode(data)
    assert gh.parse(img).g == target and target % 256 == 1 and target > 256
    return data, img


def _expected(gh, data, img, log2_stride):
    s = gh.parse(img)
    bits = _lengths(gh, img)[data]
    assert data.size == s.n and bits.min(initial=1) >= 1
    starts = np.cumsum(bits) - bits
    nblocks = -(-s.g // (1 << log2_stride))
    off = np.searchsorted(starts, 128 * (1 << log2_stride) * np.arange(nblocks, dtype=np.int64), "left")
    return np.append(off, s.n).astype(np.uint64)


def _index_image(offsets, g, log2_stride):
    """The sidecar image of these offsets (include/gaphuff.h), made here: the gather is
    tested against indexes computed from the data, not against the index build."""
    off = np.asarray(offsets, dtype="<u8")
    hdr = np.asarray([0x0000315844494847, log2_stride, off[-1], g, off.size], dtype="<u8")
    return np.concatenate([hdr, off]).view(np.uint8)


@pytest.fixture
def case(gpu, monkeypatch, request):
    """(name, data, image, {log2_stride: parsed index}), made once per stream."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    name = request.param
    if name not in _cache:
        data, img = _make(gpu, name)
        data.setflags(write=False)
        g = gpu.parse(img).g
        ixs = {k: gpu.parse_index(_index_image(_expected(gpu, data, img, k), g, k)) for k in (8, 10)}
        _cache[name] = (name, data, img, ixs)
    return _cache[name]


def _batch(off, n, seed):
    """About 300 ranges (fewer for the one-block goldens): random ones of 0..5000 bytes, the
    whole stream, the last byte, single bytes at every offsets[k] - 1 and offsets[k], one
    range of exactly one index block, duplicates; then the batch reversed."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(40):
        lo = int(rng.integers(0, n + 1))
        out.append((lo, min(lo + int(rng.integers(0, 5001)), n)))
    out += [(0, n), (n - 1, n), (0, 0), (n, n)]
    ent = [int(v) for v in off]
    for e in ent:
        if 1 <= e <= n:
            out.append((e - 1, e))
        if e < n:
            out.append((e, e + 1))
    k = (len(ent) - 1) // 2
    out.append((ent[k], ent[k + 1]))
    out += out[3:12]  # duplicates
    return out + out[::-1]


def _want(data, ranges):
    return np.concatenate([data[lo:hi] for lo, hi in ranges] + [np.zeros(0, dtype=np.uint8)])


def _assert_same(got, want, ranges):
    assert got.size == want.size
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        ends = np.cumsum([hi - lo for lo, hi in ranges])
        i = int(np.searchsorted(ends, at, "right"))
        raise AssertionError(f"first difference at output byte {at}: range {i} = {ranges[i]}")


# ---- the gather ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_gather_matches_slices(gpu, case):
    name, data, img, ixs = case
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for k, ix in ixs.items():
            ranges = _batch(ix.offsets, data.size, seed=k + len(name))
            got, ms = d.gather(ix, ranges)
            _assert_same(got, _want(data, ranges), ranges)
            assert ms >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5", "ladder_1_16", "g_256k_plus_1"], indirect=True)
def test_gather_one_workgroup(gpu, monkeypatch, case):
    """GH_GATHER_GRID=1: one workgroup's four waves take every piece in turn."""
    name, data, img, ixs = case
    monkeypatch.setenv("GH_GATHER_GRID", "1")
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for k, ix in ixs.items():
            ranges = _batch(ix.offsets, data.size, seed=3 * k)
            got, _ = d.gather(ix, ranges)
            _assert_same(got, _want(data, ranges), ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ladder_2_7"], indirect=True)
@pytest.mark.parametrize("kc", (7, 10, 13))
def test_gather_count_table_widths(gpu, monkeypatch, case, kc):
    """Four, three and two lookups per window shift (count tables of 7, 10 and 13 bits)."""
    name, data, img, ixs = case
    monkeypatch.setenv("GH_WS_KC", str(kc))
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        ranges = _batch(ixs[10].offsets, data.size, seed=kc)
        got, _ = d.gather(ixs[10], ranges)
        _assert_same(got, _want(data, ranges), ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.9"], indirect=True)
def test_gather_into_device_memory(gpu, case):
    """The bytes land in a device buffer; the bytes past their total stay as they were."""
    name, data, img, ixs = case
    ranges = _batch(ixs[8].offsets, data.size, seed=21)[:50]
    want = _want(data, ranges)
    tail = 4096
    with gpu.Decoder(0) as d, gpu.DeviceBuffer(want.size + tail) as buf:
        d.load(gpu.parse(img))
        buf.upload(np.full(want.size + tail, 0xA5, dtype=np.uint8))
        total, _ = d.gather(ixs[8], ranges, dst_ptr=buf.addr, dst_len=want.size + tail)
        assert total == want.size
        got = buf.download(np.zeros(want.size + tail, dtype=np.uint8))
        _assert_same(got[: want.size], want, ranges)
        assert (got[want.size:] == 0xA5).all()
        # an exact fit, and one byte short
        d.gather(ixs[8], ranges, dst_ptr=buf.addr, dst_len=want.size)
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(ixs[8], ranges, dst_ptr=buf.addr, dst_len=want.size - 1)
        assert e.value.code == GH_E_SMALL


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.1"], indirect=True)
def test_gather_tables_follow_the_load(gpu, case):
    """Gather, decode, gather again on one context; then a reload of another stream (another
    code: the cached tables must go) and a gather of that one; then back."""
    name, data, img, ixs = case
    other, oimg = _make(gpu, "ladder_1_16")
    oix = gpu.parse_index(_index_image(_expected(gpu, other, oimg, 8), gpu.parse(oimg).g, 8))
    ranges = _batch(ixs[8].offsets, data.size, seed=1)[:80]
    oranges = _batch(oix.offsets, other.size, seed=2)[:80]
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        _assert_same(d.gather(ixs[8], ranges)[0], _want(data, ranges), ranges)
        d.decode()
        assert d.report().status == 0 and np.array_equal(d.download(data.size), data)
        _assert_same(d.gather(ixs[10], ranges)[0], _want(data, ranges), ranges)
        d.load(gpu.parse(oimg))
        _assert_same(d.gather(oix, oranges)[0], _want(other, oranges), oranges)
        d.load(gpu.parse(img))
        _assert_same(d.gather(ixs[8], ranges[::-1])[0], _want(data, ranges[::-1]), ranges[::-1])
        assert np.array_equal(d.gather(ixs[8], [])[0], np.zeros(0, dtype=np.uint8))
        assert d.gather(ixs[8], [(5, 5), (data.size, data.size)])[0].size == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_gather_errors(gpu, case):
    name, data, img, ixs = case
    s = gpu.parse(img)
    ix = ixs[8]
    other = gpu.encode(data[: data.size // 2])
    so = gpu.parse(other)
    oix = gpu.parse_index(_index_image(_expected(gpu, data[: data.size // 2], other, 8), so.g, 8))
    with gpu.Decoder(0) as d:
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(ix, [(0, 10)])
        assert e.value.code == GH_E_STATE
        d.load(s, 0, s.g // 2)
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(ix, [(0, 10)])
        assert e.value.code == GH_E_ARG
        d.load(s)
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(oix, [(0, 10)])
        assert e.value.code == GH_E_ARG
        for bad in ([(0, s.n + 1)], [(9, 8)]):
            with pytest.raises(gpu.GapHuffError) as e:
                d.gather(ix, bad)
            assert e.value.code == GH_E_ARG
        out = np.zeros(10, dtype=np.uint8)
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(ix, [(0, 10)], dst_ptr=out.ctypes.data, dst_len=9)
        assert e.value.code == GH_E_SMALL
        d.gather(ix, [(0, 10)], dst_ptr=out.ctypes.data, dst_len=10)  # host memory
        assert np.array_equal(out, data[:10])


@pytest.mark.gpu
def test_gather_empty_stream(gpu):
    img = gpu.encode(np.zeros(0, dtype=np.uint8))
    s = gpu.parse(img)
    assert s.n == 0
    ix = gpu.parse_index(_index_image([0] * (-(-s.g // 256) + 1), s.g, 8))
    with gpu.Decoder(0) as d:
        d.load(s)
        assert d.gather(ix, [(0, 0), (0, 0)])[0].size == 0
        with pytest.raises(gpu.GapHuffError) as e:
            d.gather(ix, [(0, 1)])
        assert e.value.code == GH_E_ARG


# ---- decode_ranges and the CLI ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5", "one_symbol"], indirect=True)
def test_decode_ranges_from_path_and_bytes(gpu, case, tmp_path):
    name, data, img, ixs = case
    path = tmp_path / "stream.huff"
    np.asarray(img).tofile(path)
    ranges = _batch(ixs[8].offsets, data.size, seed=8)[:60]
    for src, ix in ((str(path), ixs[8]), (path, ixs[10].raw), (img, ixs[8].raw), (gpu.parse(img), ixs[10])):
        got = gpu.decode_ranges(src, ix, ranges)
        assert len(got) == len(ranges)
        for (lo, hi), g in zip(ranges, got):
            assert g.size == hi - lo and np.array_equal(g, data[lo:hi]), (lo, hi)
    assert gpu.decode_ranges(img, ixs[8], []) == []


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5", "gen_r0.9_n1"], indirect=True)
def test_cli_ranges(gpu, case, tmp_path):
    name, data, img, ixs = case
    huff, idx, out, rfile = tmp_path / "s.huff", tmp_path / "s.ghidx", tmp_path / "out.bin", tmp_path / "r.txt"
    np.asarray(img).tofile(huff)
    ixs[8].raw.tofile(idx)
    ranges = _batch(ixs[8].offsets, data.size, seed=4)[:70]
    rfile.write_text("".join(f"{lo}:{hi}\n" for lo, hi in ranges) + "\n")
    r = subprocess.run([DECODER, str(huff), str(out), "--index", str(idx), "--ranges", str(rfile)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    _assert_same(np.fromfile(out, dtype=np.uint8), _want(data, ranges), ranges)
    # usage errors: exit code 2
    for extra in (["--range", "0:1"], ["--write-index", str(tmp_path / "x.ghidx")]):
        bad = subprocess.run([DECODER, str(huff), str(out), "--index", str(idx), "--ranges", str(rfile), *extra],
                             capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2, bad.stderr
    bad = subprocess.run([DECODER, str(huff), str(out), "--ranges", str(rfile)], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 2
    # a range past N is refused
    rfile.write_text(f"0:{data.size + 1}\n")
    bad = subprocess.run([DECODER, str(huff), str(out), "--index", str(idx), "--ranges", str(rfile)],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode not in (0, 2)
