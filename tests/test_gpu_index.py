"""Random access on the GPU: gh_ctx_build_index and decode_range.

The expected index comes from the data, not from the library: with bits[i] the code
length of data[i] (from the file's symbol list) and starts = exclusive cumsum(bits),
offsets[k] = number of codewords that start before payload bit 128 * stride * k
(searchsorted), then N.  `symbols` must equal the CPU oracle's count over all segments.
decode_range is compared with data[lo:hi] through an in-memory Stream, a file path and
the decoder CLI (--write-index, then --index --range).

Streams: gh_generate at r = 0.1 / 0.5 / 0.9 (the single-pass tile kernel twice, the
two-pass tile kernel); prescribed codes built as in test_gpu_shapes (a 1..16-bit ladder:
a 1-bit codeword, 16-bit codewords, the canonical fallback; the one-symbol code, which is
incomplete; a grouped 4/8-bit code; a 2..7-bit ladder for the narrow count tables); three
goldens (G = 1 twice, exactly one full index block); one stream with G = 256 k + 1."""
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
             "GH_TILE_IDLE", "GH_INDEX_GRID")
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
# forced decode structures per stream, where the code allows them (tile: grouped and
# minlen-3 codes; mtile: complete codes; wsplit: every code)
FORCED = {
    "grouped_4_8": ("tile", "mtile", "wsplit"),
    "gen_r0.5": ("tile", "mtile", "wsplit"),
    "ladder_1_16": ("mtile", "wsplit"),
    "one_symbol": ("wsplit",),
}

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


@pytest.fixture
def case(gpu, orc, monkeypatch, request):
    """(name, data, image, oracle total, expected offsets at stride 2^8), made once."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    name = request.param
    if name not in _cache:
        data, img = _make(gpu, name)
        ref, total = orc.decode(img)
        assert np.array_equal(ref, data), "the oracle does not return the input"
        data.setflags(write=False)
        _cache[name] = (name, data, img, total, _expected(gpu, data, img, 8))
    return _cache[name]


def _ranges(off, n, seed):
    """(0,0), (0,1), (N-1,N), (0,N); lo and hi on both sides of several entries; 20
    random ranges."""
    out = [(0, 0), (0, 1), (n - 1, n), (0, n)]
    inner = off[1:-1]
    for e in sorted({int(inner[i]) for i in (0, len(inner) // 2, len(inner) - 1)} if len(inner) else ()):
        for v in (e - 1, e, e + 1):
            if 0 <= v <= n:
                out += [(v, min(v + 777, n)), (max(v - 777, 0), v)]
    rng = np.random.default_rng(seed)
    for _ in range(20):
        out.append(tuple(sorted(rng.integers(0, n + 1, size=2).tolist())))
    return out


def _check_ranges(gh, src, ix, data, ranges):
    for lo, hi in ranges:
        got = gh.decode_range(src, ix, lo, hi)
        assert got.size == hi - lo and np.array_equal(got, data[lo:hi]), (lo, hi)


# ---- the index ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_index_is_exact(gpu, monkeypatch, case):
    """Strides 2^8, 2^9 and 2^12 (more than G for the small streams: two entries), each
    with the default grid and with one and two workgroups (a wave walks many index
    blocks); a full decode of the same context afterwards is still bit-exact."""
    name, data, img, total, _ = case
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        for grid in (None, "1", "2"):
            if grid is None:
                monkeypatch.delenv("GH_INDEX_GRID", raising=False)
            else:
                monkeypatch.setenv("GH_INDEX_GRID", grid)
            for k in (8, 9, 12):
                image, symbols, ms = d.build_index(k)
                ix = gpu.parse_index(image)
                assert (ix.log2_stride, ix.n, ix.g) == (k, s.n, s.g)
                want = _expected(gpu, data, img, k)
                assert ix.offsets.size == -(-s.g // (1 << k)) + 1
                assert np.array_equal(ix.offsets, want), (name, grid, k, np.nonzero(ix.offsets != want)[0][:4])
                assert symbols == total
                assert ms >= 0
        d.decode()
        rep = d.report()
        assert rep.status == 0 and rep.symbols == total
        assert np.array_equal(d.download(s.n), data)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ladder_2_7"], indirect=True)
@pytest.mark.parametrize("kc", (7, 10, 13))
def test_index_count_table_widths(gpu, monkeypatch, case, kc):
    """Four, three and two lookups per window shift (count tables of 7, 10 and 13 bits)."""
    name, data, img, total, want = case
    monkeypatch.setenv("GH_WS_KC", str(kc))
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for grid in (None, "1"):
            if grid:
                monkeypatch.setenv("GH_INDEX_GRID", grid)
            image, symbols, _ = d.build_index(8)
            assert np.array_equal(gpu.parse_index(image).offsets, want) and symbols == total


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_build_index_errors(gpu, case):
    name, data, img, total, _ = case
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        with pytest.raises(gpu.GapHuffError) as e:
            d.build_index(8)
        assert e.value.code == GH_E_STATE
        d.load(s, 0, s.g // 2)
        with pytest.raises(gpu.GapHuffError) as e:
            d.build_index(8)
        assert e.value.code == GH_E_ARG
        d.load(s)
        for k in (7, 21):
            buf = np.zeros(1 << 16, dtype=np.uint8)
            assert gpu.lib().gh_ctx_build_index(d._h, k, buf.ctypes.data, buf.size, None, None) == GH_E_ARG
        need = int(gpu.lib().gh_index_bytes(s.g, 8))
        buf = np.zeros(need, dtype=np.uint8)
        assert gpu.lib().gh_ctx_build_index(d._h, 8, buf.ctypes.data, need - 1, None, None) == GH_E_SMALL
        assert gpu.lib().gh_ctx_build_index(d._h, 8, buf.ctypes.data, need, None, None) == 0
        assert np.array_equal(gpu.parse_index(buf).offsets, case[4])


# ---- byte ranges ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_decode_range_from_stream(gpu, case):
    name, data, img, total, off = case
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        ix = gpu.parse_index(d.build_index(8)[0])
        ix9 = gpu.parse_index(d.build_index(9)[0])
    ranges = _ranges(off, s.n, seed=len(name))
    _check_ranges(gpu, s, ix, data, ranges)
    _check_ranges(gpu, img, ix9.raw, data, ranges[:10])  # file bytes and a sidecar image, stride 2^9


@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_decode_range_from_path(gpu, case, tmp_path):
    name, data, img, total, off = case
    path = tmp_path / "stream.huff"
    np.asarray(img).tofile(path)
    with gpu.Decoder(0) as d:
        info = d.load_file(str(path))
        assert (info.n, info.g) == (data.size, gpu.parse(img).g)
        ix = gpu.parse_index(d.build_index(8)[0])  # (a file load covers [0, G) too)
    assert np.array_equal(ix.offsets, off)
    _check_ranges(gpu, str(path), ix, data, _ranges(off, data.size, seed=5)[:14])
    _check_ranges(gpu, path, ix, data, [(data.size // 3, data.size // 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [n for n in STREAMS if n in FORCED], indirect=True)
def test_decode_range_forced_structures(gpu, monkeypatch, case):
    """The sub-range loads through each decode structure the code allows."""
    name, data, img, total, off = case
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        ix = gpu.parse_index(d.build_index(8)[0])
    ranges = _ranges(off, s.n, seed=11)
    ranges = ranges[:4] + ranges[6:10] + ranges[-3:]
    for mode in FORCED[name]:
        monkeypatch.setenv("GH_MODE", mode)
        lo, hi = s.n // 4, s.n // 2
        b, e, skip = ix.locate(lo, hi)
        with gpu.Decoder(0) as d:  # the structure that ran is the forced one
            d.load(s, b, e, skip + hi - lo)
            d.decode()
            assert gpu.MODE_NAMES[d.report().mode] == {"wsplit": "split"}.get(mode, mode)
        _check_ranges(gpu, s, ix, data, ranges)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_decode_range_refuses_another_streams_index(gpu, case, tmp_path):
    name, data, img, total, off = case
    other = gpu.encode(data[: data.size // 2])
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(other))
        ix = gpu.parse_index(d.build_index(8)[0])
    path = tmp_path / "stream.huff"
    np.asarray(img).tofile(path)
    for src in (gpu.parse(img), img, str(path)):
        with pytest.raises(gpu.GapHuffError) as e:
            gpu.decode_range(src, ix, 10, 20)
        assert e.value.code == GH_E_ARG


# ---- the CLI ------------------------------------------------------------------------------
def _run(*args):
    r = subprocess.run([DECODER, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    return r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5", "gen_r0.9_n1"], indirect=True)
def test_cli_write_index_then_range(gpu, case, tmp_path):
    name, data, img, total, off = case
    huff, idx, out = tmp_path / "s.huff", tmp_path / "s.ghidx", tmp_path / "out.bin"
    np.asarray(img).tofile(huff)
    text = _run(huff, out, "--write-index", idx, "--index-stride", 8)
    assert "Original size: %d bytes" % data.size in text  # the existing lines stay
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), data)
    ix = gpu.parse_index(np.fromfile(idx, dtype=np.uint8))
    assert np.array_equal(ix.offsets, off)
    n = data.size
    mid = int(off[len(off) // 2])
    for lo, hi in {(0, n), (max(mid - 1, 0), min(mid + 4097, n)), (n - 1, n)}:
        _run(huff, out, "--index", idx, "--range", f"{lo}:{hi}")
        assert np.array_equal(np.fromfile(out, dtype=np.uint8), data[lo:hi]), (lo, hi)
    # the Python path reads the CLI's sidecar too
    assert np.array_equal(gpu.decode_range(str(huff), np.fromfile(idx, dtype=np.uint8), 1 % n, n), data[1 % n:])
    bad = subprocess.run([DECODER, str(huff), str(out), "--index", str(idx), "--range", f"0:{n + 1}"],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0
