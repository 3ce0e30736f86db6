"""Device-planned gather on the GPU: gh_ctx_set_index / gh_ctx_gather_device /
gh_ctx_gather_wait / gh_ctx_gather_pieces (Decoder.set_index, gather_device, gather_wait,
gather_pieces).

The ranges and the destination lie in device memory and the plan is built by kernels, so
every gather is compared three ways: with np.concatenate([data[lo:hi] ...]) of the original
bytes, with Decoder.gather of the same batch, and piece by piece with Index.plan
(gh_gather_plan).  Every destination carries a sentinel: the bytes past the batch's total,
and the whole buffer after a refusal, must stay as they were.  The streams and their
indexes (computed from the data) are those of tests/test_gpu_gather.py, whose small helpers
are copied here."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_GEN = 300_000
N_CODE = 1 << 18
N_TILE = 1 << 20     # the r = 0.1 stream of the ordering test: a few dozen tiles of the tile kernel
SCAN_CHUNK = 2048    # ranges per chunk of the plan's single-workgroup scan (GP_SCAN_CHUNK, gh_gather_plan.hip)
SENTINEL = 0xA5
TAIL = 256
ENV_KNOBS = ("GH_MODE", "GH_TILE_GRID", "GH_TILE_SCAP", "GH_TILE_SCAPF", "GH_WS_K", "GH_WS_KC", "GH_WS_NS",
             "GH_WS_GRID", "GH_WS_STAGE", "GH_WS_LGC", "GH_MT_KC", "GH_MT_CLGR", "GH_LUT_BITS", "GH_LGR",
             "GH_TILE_IDLE", "GH_INDEX_GRID", "GH_GATHER_GRID")
GH_E_ARG, GH_E_CORRUPT, GH_E_STATE, GH_E_SMALL = -1, -7, -8, -9


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
    whole stream, the last byte, empty ranges, single bytes at every offsets[k] - 1 and
    offsets[k], one range of exactly one index block, duplicates, overlaps; then the batch
    reversed."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(40):
        lo = int(rng.integers(0, n + 1))
        out.append((lo, min(lo + int(rng.integers(0, 5001)), n)))
    out += [(0, n), (n - 1, n), (0, 0), (n, n), (n // 2, n // 2)]
    ent = [int(v) for v in off]
    for e in ent:
        if 1 <= e <= n:
            out.append((e - 1, e))
        if e < n:
            out.append((e, e + 1))
    k = (len(ent) - 1) // 2
    out.append((ent[k], ent[k + 1]))
    out += out[3:12]  # duplicates
    out += [(lo + (hi - lo) // 2, hi) for lo, hi in out[:8]]  # overlaps
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


def _ranges_array(ranges):
    return np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))


class _Dev:
    """A batch's ranges and a sentinel-filled destination of total + TAIL bytes in device
    memory; dst_len defaults to the exact total."""

    def __init__(self, gpu, ranges, total, dst_len=None):
        r = _ranges_array(ranges)
        self.n, self.total = r.shape[0], total
        self.dst_len = total if dst_len is None else dst_len
        self.rbuf = gpu.DeviceBuffer(max(r.nbytes, 16))
        self.dbuf = gpu.DeviceBuffer(total + TAIL)
        self.rbuf.upload(r)
        self.dbuf.upload(np.full(total + TAIL, SENTINEL, dtype=np.uint8))

    def enqueue(self, d, hip_stream=0):
        d.gather_device(self.rbuf.addr, self.n, self.dbuf.addr, self.dst_len, hip_stream)

    def bytes(self):
        """The gathered bytes; the tail past them must be untouched."""
        got = self.dbuf.download(np.zeros(self.total + TAIL, dtype=np.uint8))
        assert (got[self.total:] == SENTINEL).all(), "bytes past the batch's total were written"
        return got[: self.total]

    def untouched(self):
        return bool((self.dbuf.download(np.zeros(self.total + TAIL, dtype=np.uint8)) == SENTINEL).all())

    def close(self):
        self.rbuf.close()
        self.dbuf.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _gather_and_check(gpu, d, ix, data, ranges, host_gather=True):
    """One device-planned gather of `ranges` on d (index already resident): the bytes
    against the data and Decoder.gather, the pieces and the report against Index.plan."""
    want = _want(data, ranges)
    pieces, total = ix.plan(ranges)
    assert total == want.size
    with _Dev(gpu, ranges, total) as b:
        b.enqueue(d)
        rep = d.gather_wait()
        got = b.bytes()
    _assert_same(got, want, ranges)
    if host_gather:
        _assert_same(d.gather(ix, ranges)[0], want, ranges)
    assert rep.status == 0 and rep.out_bytes == total and rep.npieces == pieces.size and rep.kernel_ms >= 0
    dev_pieces = d.gather_pieces()
    assert dev_pieces.dtype == pieces.dtype and dev_pieces.size == pieces.size
    if not np.array_equal(dev_pieces, pieces):
        at = int(np.nonzero(dev_pieces != pieces)[0][0])
        raise AssertionError(f"piece {at}: device {dev_pieces[at]}, gh_gather_plan {pieces[at]}")
    assert pieces.size <= gpu.gather_piece_bound(len(ranges), total, ix.log2_stride)
    return rep


# ---- 1, 2: bytes and pieces ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_device_gather_matches_slices_host_gather_and_plan(gpu, case):
    name, data, img, ixs = case
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for k, ix in ixs.items():
            d.set_index(ix)  # (replaces the other stride's)
            ranges = _batch(ix.offsets, data.size, seed=k + len(name))
            _gather_and_check(gpu, d, ix, data, ranges)


# ---- 3: more ranges than one chunk of the scan ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
@pytest.mark.parametrize("one_workgroup", (False, True))
def test_many_short_ranges_pass_the_scan_chunk(gpu, monkeypatch, case, one_workgroup):
    name, data, img, ixs = case
    nr = 5000
    assert nr > 2 * SCAN_CHUNK and nr % SCAN_CHUNK  # three chunks, the last one partial: two carries
    if one_workgroup:
        monkeypatch.setenv("GH_GATHER_GRID", "1")
    rng = np.random.default_rng(33)
    lo = rng.integers(0, data.size - 3, size=nr)
    ranges = [(int(a), int(a + b)) for a, b in zip(lo, rng.integers(1, 4, size=nr))]
    ranges[SCAN_CHUNK - 1] = (0, 4000)  # a longer range as the last of a chunk and the first of the next
    ranges[SCAN_CHUNK] = (100, 9000)
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        d.set_index(ixs[8])
        _gather_and_check(gpu, d, ixs[8], data, ranges, host_gather=not one_workgroup)


# ---- 4: one long range among short ones -------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.1", "gen_r0.9"], indirect=True)
def test_whole_stream_between_short_ranges(gpu, case):
    name, data, img, ixs = case
    n = data.size
    rng = np.random.default_rng(4)
    lo = rng.integers(0, n - 40, size=200)
    short = [(int(a), int(a + b)) for a, b in zip(lo, rng.integers(0, 40, size=200))]
    ranges = short[:100] + [(0, n)] + short[100:]
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        for k in (8, 10):
            d.set_index(ixs[k])
            rep = _gather_and_check(gpu, d, ixs[k], data, ranges)
            if k == 8:  # the long range emits every block's piece
                assert rep.npieces >= ixs[8].offsets.size - 1 >= 25


# ---- 5: every gather kernel shape with a device piece count --------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,kc", [("ladder_2_7", 7), ("ladder_2_7", 10), ("ladder_2_7", 13),
                                     ("ladder_1_16", None), ("one_symbol", None)], indirect=["case"])
def test_count_table_widths_and_fallback(gpu, monkeypatch, case, kc):
    """Four, three and two lookups per window shift (count tables of 7, 10 and 13 bits), and
    the canonical fallback (16-bit codewords; an incomplete code)."""
    name, data, img, ixs = case
    if kc is not None:
        monkeypatch.setenv("GH_WS_KC", str(kc))
    with gpu.Decoder(0) as d:
        d.load(gpu.parse(img))
        d.set_index(ixs[10])
        _gather_and_check(gpu, d, ixs[10], data, _batch(ixs[10].offsets, data.size, seed=kc or 5)[:120])


# ---- 6, 7: untouched memory and refusals ---------------------------------------------------
def _corrupting_index(gpu, s, log2_stride=8):
    """An index that parses for (N, G) but is no real stream's: steps of one symbol, far
    below 8 * stride, then steps large enough to reach N."""
    nblocks = -(-s.g // (1 << log2_stride))
    big = -(-s.n // 30_000) + 1  # blocks of about 30 000 symbols (at most 143 * 256)
    small = nblocks - big
    assert small >= 30
    off = np.concatenate([np.arange(small, dtype=np.int64),
                          np.linspace(small, s.n, big + 1).astype(np.int64)])
    assert off.size == nblocks + 1 and np.diff(off).max() <= 143 << log2_stride and (np.diff(off) >= 0).all()
    return gpu.parse_index(_index_image(off, s.g, log2_stride)), small


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_device_refusals_leave_the_destination_untouched(gpu, case):
    name, data, img, ixs = case
    s = gpu.parse(img)
    ix = ixs[8]
    good = _batch(ix.offsets, data.size, seed=2)[:60]
    total = sum(hi - lo for lo, hi in good)
    mid = len(good) // 2

    def refused(d, ranges, code, dst_len=None, tot=None):
        tot = total if tot is None else tot
        with _Dev(gpu, ranges, tot, dst_len=dst_len) as b:
            b.enqueue(d)
            with pytest.raises(gpu.GapHuffError) as e:
                d.gather_wait()
            assert e.value.code == code, e.value
            assert e.value.report.npieces == 0 and e.value.report.status != 0
            assert b.untouched(), "a refused gather wrote to its destination"
            assert d.gather_pieces().size == 0

    with gpu.Decoder(0) as d:
        d.load(s)
        d.set_index(ix)
        refused(d, good[:mid] + [(9, 8)] + good[mid:], GH_E_ARG)
        refused(d, good[:mid] + [(s.n - 1, s.n + 1)] + good[mid:], GH_E_ARG)
        refused(d, good, GH_E_SMALL, dst_len=total - 1)
        # the same batch is fine afterwards: an exact fit
        _gather_and_check(gpu, d, ix, data, good)
        # an index that parses but belongs to no real stream: the plan exceeds the piece buffer
        bad_ix, small = _corrupting_index(gpu, s)
        d.set_index(bad_ix)
        spans = [(0, small)] * 50
        assert bad_ix.plan(spans)[0].size > gpu.gather_piece_bound(len(spans), 50 * small, 8)
        refused(d, spans, GH_E_CORRUPT, tot=50 * small)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_host_side_refusals(gpu, case):
    name, data, img, ixs = case
    s = gpu.parse(img)
    ix = ixs[8]
    half = data[: data.size // 2]
    other = gpu.encode(half)
    oix = gpu.parse_index(_index_image(_expected(gpu, half, other, 8), gpu.parse(other).g, 8))

    def state(fn, code=GH_E_STATE):
        with pytest.raises(gpu.GapHuffError) as e:
            fn()
        assert e.value.code == code, e.value

    with gpu.Decoder(0) as d, _Dev(gpu, [(0, 10)], 10) as b:
        state(lambda: b.enqueue(d))       # before a load
        state(lambda: d.set_index(ix))
        state(d.gather_wait)
        d.load(s)
        state(lambda: b.enqueue(d))       # before set_index
        state(d.gather_wait)              # nothing enqueued
        state(lambda: d.set_index(oix), GH_E_ARG)  # another stream's (N, G)
        d.set_index(ix)
        d.gather_device(0, 0, 0, 0)       # no range: fine, nothing launched
        state(d.gather_wait)
        state(lambda: d.gather_device(0, 1, b.dbuf.addr, 10), GH_E_ARG)  # null pointers
        state(lambda: d.gather_device(b.rbuf.addr, 1, 0, 10), GH_E_ARG)
        state(lambda: d.gather_device(b.rbuf.addr, gpu.GH_GATHER_MAX_RANGES + 1, b.dbuf.addr, 10), GH_E_ARG)
        b.enqueue(d)
        assert d.gather_wait().out_bytes == 10 and np.array_equal(b.bytes(), data[:10])
        d.load(s)                         # a reload drops the index
        state(lambda: b.enqueue(d))
        state(d.gather_wait)
        d.load(s, 0, s.g // 2)            # a partial load takes no index
        state(lambda: d.set_index(ix), GH_E_ARG)


@pytest.mark.gpu
def test_empty_stream(gpu):
    img = gpu.encode(np.zeros(0, dtype=np.uint8))
    s = gpu.parse(img)
    ix = gpu.parse_index(_index_image([0] * (-(-s.g // 256) + 1), s.g, 8))
    with gpu.Decoder(0) as d:
        d.load(s)
        d.set_index(ix)
        with _Dev(gpu, [(0, 0), (0, 0)], 0) as b:
            b.enqueue(d)
            rep = d.gather_wait()
            assert rep.out_bytes == 0 and rep.npieces == 0 and b.untouched()
        with _Dev(gpu, [(0, 1)], 1) as b:
            b.enqueue(d)
            with pytest.raises(gpu.GapHuffError) as e:
                d.gather_wait()
            assert e.value.code == GH_E_ARG and b.untouched()


# ---- 8: ordering with decodes (the device chain) -----------------------------------------
@pytest.mark.gpu
def test_gathers_between_tile_decodes(gpu, monkeypatch):
    """gather, decode, gather on one context, nothing waited for in between; then the decode
    on a second context of the same device.  The load picks a tile kernel, whose workgroups
    wait for each other: the gathers are members of the device's decode chain."""
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    data = gpu.generate(376, 0.1, N_TILE)
    img = gpu.encode(data)
    s = gpu.parse(img)
    ix = gpu.parse_index(_index_image(_expected(gpu, data, img, 8), s.g, 8))
    r1 = _batch(ix.offsets, data.size, seed=1)[:150]
    r2 = _batch(ix.offsets, data.size, seed=2)[100:250]
    t1, t2 = (sum(hi - lo for lo, hi in r) for r in (r1, r2))
    with gpu.Decoder(0) as d, gpu.Decoder(0) as d2:
        d.load(s)
        d2.load(s)
        assert d.kernel_shape().startswith("tile<") and d2.kernel_shape().startswith("tile<")
        d.set_index(ix)
        for dec in (d, d2):
            with _Dev(gpu, r1, t1) as b1, _Dev(gpu, r2, t2) as b2:
                b1.enqueue(d)
                dec.decode(timed=False)
                b2.enqueue(d)
                rep = d.gather_wait()
                drep = dec.report()
                assert rep.status == 0 and rep.out_bytes == t2
                assert drep.status == 0 and np.array_equal(dec.download(s.n), data)
                _assert_same(b1.bytes(), _want(data, r1), r1)
                _assert_same(b2.bytes(), _want(data, r2), r2)


# ---- 9: torch interop -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_torch_rows_on_the_current_stream(gpu, case):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    name, data, img, ixs = case
    dev = torch.device("cuda:0")
    # a stream of torch's own as the current one: its handle is not NULL, which the C ABI
    # reads as "the context's stream"
    with gpu.Decoder(0) as d, torch.cuda.stream(torch.cuda.Stream(device=dev)):
        d.load(gpu.parse(img))
        d.set_index(ixs[8])
        for rb in (64, 4096):
            rows = data.size // rb
            table = torch.from_numpy(data[: rows * rb].copy()).view(rows, rb)
            ids = torch.randint(0, rows, (300,), device=dev, generator=torch.Generator(device=dev).manual_seed(rb))
            ranges = torch.stack([ids * rb, ids * rb + rb], 1).contiguous()
            assert ranges.dtype == torch.int64 and ranges.shape == (300, 2)
            out = torch.full((300, rb), SENTINEL, dtype=torch.uint8, device=dev)
            handle = torch.cuda.current_stream().cuda_stream
            assert handle != 0
            d.gather_device(ranges.data_ptr(), 300, out.data_ptr(), out.numel(), handle)
            got = out.cpu()  # (a copy on the current stream: ordered behind the gather)
            rep = d.gather_wait()
            assert rep.status == 0 and rep.out_bytes == 300 * rb
            assert torch.equal(got, table[ids.cpu()])
