"""Foreign and incomplete code tables through every decode path on the GPU.

The streams are the images of tests/foreign_codes.py: tables gh.encode never writes
(incomplete ones with holes behind valid codewords, empty lengths, 16-bit codewords beside a
1-bit one, table symbols the data never uses) under data that sits on the table's longest or
shortest codeword.  Every result is compared with the data and with the CPU oracle's
bit-serial decode of the same image (made once per case); no GPU path is another's reference.
Batch decodes and gathers go into 0xA5-filled caller buffers with a guard; a Decoder decodes
into its own output of capacity N.

The wave split's fb=1 kernels are asserted by name under multi-symbol incomplete codes
(FORCED_WS; test_forced_rows_name_every_fb1_wave_split_kernel), and so are batch<fb=1>,
batchraw<fb=1> and bgather<fb=1>.  The paired negative case (a kept codeword overwritten by
a pattern outside the code) shows that "stray lookups never flag" is not met by never
flagging."""
import re

import numpy as np
import pytest

import foreign_codes as fc

GH_E_ARG, GH_E_CORRUPT = -1, -7
GUARD = 4096
FILL = 0xA5
ENV_KNOBS = ("GH_MODE", "GH_TILE_GRID", "GH_TILE_SCAP", "GH_TILE_SCAPF", "GH_WS_K", "GH_WS_KC", "GH_WS_NS",
             "GH_WS_GRID", "GH_WS_STAGE", "GH_WS_LGC", "GH_MT_KC", "GH_MT_CLGR", "GH_LUT_BITS", "GH_LGR",
             "GH_TILE_IDLE", "GH_INDEX_GRID", "GH_GATHER_GRID", "GH_BATCH_GRID")
ALL_CASES = fc.CASES + [(e, None) for e in fc.EDGE]
WS_FB1 = re.compile(r"ws_count<4,256,2,fb=1>\+ws_write<2,512,2,[23468],fb=1>")
FORCED_WS = [(code, ns) for code in ("holes16", "k3") for ns in (2, 3, 4, 6, 8)]
RANGE_CASES = [("holes16", "uniform"), ("flat8_200", "uniform"), ("cfg4like", "long")]


def _ws_fb1(ns):
    return f"ws_count<4,256,2,fb=1>+ws_write<2,512,2,{ns},fb=1>"


@pytest.fixture
def env(gpu, monkeypatch):
    """Every launcher knob cleared; env(**knobs) sets some."""
    def setenv(**knobs):
        for k in ENV_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in knobs.items():
            monkeypatch.setenv(k, str(v))
    setenv()
    return setenv


_refs = {}


def _case(orc, code, profile=None):
    """(Case, the oracle's symbol total): the oracle decodes each image once and must return
    the data."""
    key = (code, profile)
    if key not in _refs:
        c = fc.case(orc, code, profile)
        ref, total = orc.decode(c.image)
        assert np.array_equal(ref, c.data), "the oracle does not return the data"
        _refs[key] = (c, total)
    return _refs[key]


def _assert_same(got, want, what):
    assert got.size == want.size, what
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} wrong bytes of {want.size}, first at {bad[0]}")


def _decode_one(gpu, c, total):
    """One Decoder, one shard: (kernel shape, report); exact output, status 0, the oracle's
    symbol total (the last segment's padding codewords included)."""
    s = gpu.parse(c.image)
    with gpu.Decoder(0) as d:
        d.load(s)
        shape = d.kernel_shape()
        d.decode()
        rep = d.report()
        out = d.download(s.n)
    print(f"{shape}: grid {rep.grid}, tiles {rep.tiles}, G {s.g}")
    assert rep.status == 0, (shape, rep.status)
    assert rep.symbols == total and rep.out_bytes == s.n, (shape, rep.symbols, total)
    _assert_same(out, c.data, shape)
    return shape, rep


def _seg_first(c):
    """First symbol of every segment, then n: a segment owns the codewords that start in its
    128 bits (from the table's lengths, no decode)."""
    length_of = np.zeros(256, dtype=np.int64)
    for sym, l in c.symbols:
        length_of[sym] = l
    bits = length_of[c.data]
    starts = np.cumsum(bits) - bits
    g = -(-int(bits.sum()) // 128)
    first = np.searchsorted(starts, 128 * np.arange(g, dtype=np.int64), "left")
    return np.append(first, c.data.size).astype(np.int64)


def _edge_ranges(seg, n):
    """(lo, hi) pairs that start and end on, one before and one after a segment's first byte
    and an index block's (256 segments) first byte; empty ranges, single bytes, the whole."""
    out = [(0, 0), (n, n), (n // 2, n // 2), (0, n), (0, 1), (n - 1, n)]
    g = seg.size - 1
    points = {int(seg[g // 3]), int(seg[g - 1])} | {int(seg[k]) for k in range(256, g, 256)[:2]}
    points |= {int(seg[k]) for k in range(256, g, 256)[-1:]}
    for p in sorted(points):
        for a in (p - 1, p, p + 1):
            if 0 <= a <= n:
                out += [(a, min(a + 300, n)), (max(a - 300, 0), a), (a, a)]
    return out


def _index_image(offsets, g, log2_stride=8):
    """The sidecar image of these offsets (include/gaphuff.h), made here: the gathers are
    tested against an index computed from the data, not against the index build."""
    off = np.asarray(offsets, dtype="<u8")
    hdr = np.asarray([0x0000315844494847, log2_stride, off[-1], g, off.size], dtype="<u8")
    return np.concatenate([hdr, off]).view(np.uint8)


# ---- default pick -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("code,profile", ALL_CASES)
def test_default_pick(gpu, orc, env, code, profile):
    """What the launcher picks by itself: one shard, then three shards on one device."""
    c, total = _case(orc, code, profile)
    shape, _ = _decode_one(gpu, c, total)
    if fc.EDGE.get(code, (code,))[0] in fc.INCOMPLETE:
        assert WS_FB1.fullmatch(shape), shape
    _assert_same(gpu.decode(c.image, ngpus=3, devices=[0, 0, 0]), c.data, f"{shape}, three shards")


# ---- forced structures ----------------------------------------------------------------------
def test_forced_rows_name_every_fb1_wave_split_kernel(gh):
    """The names test_forced_wsplit asserts are all the fb=1 names the wave split's pickers
    can return.  Needs no GPU."""
    want = {k for _, ns in FORCED_WS for k in _ws_fb1(ns).split("+")}
    have = {k for k in gh.kernel_shapes() if k.startswith("ws_") and k.endswith("fb=1>")}
    assert want == have and len(have) == 6
    assert all(WS_FB1.fullmatch(_ws_fb1(ns)) for _, ns in FORCED_WS)


@pytest.mark.gpu
@pytest.mark.parametrize("code,ns", FORCED_WS)
def test_forced_wsplit(gpu, orc, env, code, ns):
    """Every store shape of ws_write<..., fb=1> under a multi-symbol incomplete code."""
    env(GH_MODE="wsplit", GH_WS_NS=ns)
    for profile in fc.PROFILES:
        c, total = _case(orc, code, profile)
        shape, rep = _decode_one(gpu, c, total)
        assert shape == _ws_fb1(ns) and gpu.MODE_NAMES[rep.mode] == "split"


@pytest.mark.gpu
@pytest.mark.parametrize("grid3", (False, True))
@pytest.mark.parametrize("profile", fc.PROFILES)
@pytest.mark.parametrize("code,mode", [("cfg4like", "tile"), ("minlen3", "tile"), ("ladder_1_16", "mtile")])
def test_forced_tile_kernels(gpu, orc, env, code, mode, profile, grid3):
    """The tile kernels on codes made for them and data that was not: segments full of the
    longest or of the shortest codeword, with the default grid and with three workgroups."""
    env(GH_MODE=mode, **({"GH_TILE_GRID": 3} if grid3 else {}))
    c, total = _case(orc, code, profile)
    shape, rep = _decode_one(gpu, c, total)
    assert shape.startswith(mode + "<") and gpu.MODE_NAMES[rep.mode] == mode
    if grid3:
        assert rep.grid <= 3
        if profile != "short":  # (a tile is 2048 or 3072 segments: the short profiles' streams have 2 or 3)
            assert rep.grid == 3 < rep.tiles  # more tiles than workgroups: a workgroup walks several


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ("tile", "mtile"))
def test_tile_kernels_refuse_an_incomplete_code(gpu, orc, env, mode):
    env(GH_MODE=mode)
    c, _ = _case(orc, "k3", "uniform")
    with gpu.Decoder(0) as d:
        with pytest.raises(gpu.GapHuffError) as e:
            d.load(gpu.parse(c.image))
    assert e.value.code == GH_E_ARG


# ---- index and gathers ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("code,profile", RANGE_CASES)
def test_index_equals_the_oracles_running_sum(gpu, orc, env, code, profile):
    c, total = _case(orc, code, profile)
    s = gpu.parse(c.image)
    counts = np.asarray([orc.segment_count(c.image, i) for i in range(s.g)], dtype=np.int64)
    run = np.concatenate([[0], np.cumsum(counts)])
    assert run[-1] == total and np.array_equal(run[:-1], _seg_first(c)[:-1])
    with gpu.Decoder(0) as d:
        d.load(s)
        image, symbols, _ = d.build_index(8)
    ix = gpu.parse_index(image)
    assert (ix.log2_stride, ix.n, ix.g) == (8, s.n, s.g) and symbols == total
    assert ix.offsets.size == -(-s.g // 256) + 1 >= 3
    assert np.array_equal(ix.offsets[:-1], run[:-1][::256]) and ix.offsets[-1] == s.n


@pytest.mark.gpu
@pytest.mark.parametrize("code,profile", RANGE_CASES)
def test_ranges_through_decode_range_and_both_gathers(gpu, orc, env, code, profile):
    c, _ = _case(orc, code, profile)
    s = gpu.parse(c.image)
    seg = _seg_first(c)
    ix = gpu.parse_index(_index_image(np.append(seg[:-1][::256], s.n), s.g))
    ranges = _edge_ranges(seg, s.n)
    assert len(ranges) >= 40
    want = np.concatenate([c.data[lo:hi] for lo, hi in ranges])
    for lo, hi in ranges:
        _assert_same(gpu.decode_range(s, ix, lo, hi), c.data[lo:hi], (lo, hi))
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64))
    with gpu.Decoder(0) as d, gpu.DeviceBuffer(r.nbytes) as dr, gpu.DeviceBuffer(want.size + GUARD) as buf:
        d.load(s)
        # ranges on the host, the destination in device memory
        buf.upload(np.full(want.size + GUARD, FILL, dtype=np.uint8))
        assert d.gather(ix, ranges, dst_ptr=buf.addr, dst_len=want.size)[0] == want.size
        got = buf.download(np.zeros(want.size + GUARD, dtype=np.uint8))
        _assert_same(got[: want.size], want, "gather")
        assert (got[want.size:] == FILL).all(), "gather wrote past the ranges' total"
        # ranges in device memory, the plan built on the GPU
        d.set_index(ix)
        dr.upload(r)
        buf.upload(np.full(want.size + GUARD, FILL, dtype=np.uint8))
        d.gather_device(dr.addr, r.shape[0], buf.addr, want.size)
        rep = d.gather_wait()
        got = buf.download(np.zeros(want.size + GUARD, dtype=np.uint8))
        assert rep.status == 0 and rep.out_bytes == want.size
        _assert_same(got[: want.size], want, "gather_device")
        assert (got[want.size:] == FILL).all(), "gather_device wrote past the ranges' total"


# ---- batches ----------------------------------------------------------------------------------
def _batch(gpu, orc):
    """[(name, Case, the oracle's symbol total)] of the mixed batch, made once: every foreign
    image, profile by profile so that neighbours differ in their code, the G = 255 / 256 / 257
    cases and two encoder-made streams in between."""
    if "batch" not in _refs:
        out = [(f"{code}/{profile}", *_case(orc, code, profile)) for profile in fc.PROFILES for code in fc.CODES]
        for at, name in zip((3, 14, 27, 31), fc.EDGE):
            out.insert(at, (name, *_case(orc, name)))
        for at, (seed, r, n) in zip((8, 21), ((601, 0.5, 50_000), (602, 0.9, 30_001))):
            data = gpu.generate(seed, r, n)
            img = gpu.encode(data)
            ref, total = orc.decode(img)
            assert np.array_equal(ref, data)
            data.setflags(write=False)
            out.insert(at, (f"encoder_r{r}", fc.Case(gpu.parse(img).symbols, data, img), total))
        tables = [c.symbols for _, c, _ in out]
        assert all(tables[k] != tables[k - 1] for k in range(1, len(out))), "neighbours share a table"
        assert len(out) == len(ALL_CASES) + 2
        _refs["batch"] = out
    return _refs["batch"]


def _check_arena(got, off, datas, skip=()):
    for i, d in enumerate(datas):
        lo, hi = int(off[i]), int(off[i + 1])
        if i not in skip:
            _assert_same(got[lo: lo + d.size], d, f"stream {i}")
        assert (got[lo + d.size: hi] == FILL).all(), f"pad bytes after stream {i} were written"
    assert (got[int(off[-1]):] == FILL).all(), "guard bytes after the arena were written"


def _decode_into(gpu, b, datas):
    """Decode b's loaded batch into a 0xA5-filled caller buffer with a guard; check every
    stream, every pad byte, the guard, the status and the counts."""
    ns = [d.size for d in datas]
    off = gpu.batch_layout(ns)
    assert np.array_equal(b.offsets(), off)
    arena = int(off[-1])
    with gpu.DeviceBuffer(arena + GUARD) as buf:
        buf.upload(np.full(arena + GUARD, FILL, dtype=np.uint8))
        b.decode(buf.addr, arena)
        rep = b.wait()
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    assert rep.nstreams == len(datas) and rep.bad_streams == 0 and rep.status == 0
    assert rep.out_bytes == sum(ns) and rep.launches == 3
    _check_arena(got, off, datas)
    st, sy = b.status()
    assert not st.any()
    assert (sy >= np.asarray(ns, dtype=np.uint64)).all()
    return sy


def _batch_ranges(cases, seed):
    """(stream, lo, hi) triples: _edge_ranges of every stream, shuffled."""
    out = []
    for s, c in enumerate(cases):
        out += [(s, lo, hi) for lo, hi in _edge_ranges(_seg_first(c), c.data.size)]
    order = np.random.default_rng(seed).permutation(len(out))
    return [out[i] for i in order]


def _gather_checked(gpu, b, datas, ranges):
    """The ranges through BatchDecoder.gather, then from device memory through gather_device
    into a filled buffer with a guard."""
    for (s, lo, hi), got in zip(ranges, b.gather(ranges)):
        _assert_same(got, datas[s][lo:hi], (s, lo, hi))
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 3)
    total = int((r[:, 2] - r[:, 1]).sum())
    with gpu.DeviceBuffer(r.nbytes) as dr, gpu.DeviceBuffer(total + GUARD) as buf:
        dr.upload(r)
        buf.upload(np.full(total + GUARD, FILL, dtype=np.uint8))
        b.gather_device(dr.addr, r.shape[0], buf.addr, total)
        rep = b.gather_wait()
        got = buf.download(np.zeros(total + GUARD, dtype=np.uint8))
    assert rep.status == 0 and rep.bad_ranges == 0 and rep.out_bytes == total
    _assert_same(got[:total], np.concatenate([datas[s][lo:hi] for s, lo, hi in ranges]), "gather_device")
    assert (got[total:] == FILL).all(), "bytes after the ranges' total were written"


@pytest.mark.gpu
def test_mixed_batch(gpu, orc, env):
    cases = [c for _, c, _ in _batch(gpu, orc)]
    datas = [c.data for c in cases]
    with gpu.BatchDecoder(0) as b:
        b.load([c.image for c in cases])
        assert b.kernel_shape() == "batch<fb=1>"
        sy = _decode_into(gpu, b, datas)
        assert sy.tolist() == [total for _, _, total in _batch(gpu, orc)]  # (the padding's codewords included)


@pytest.mark.gpu
def test_mixed_batch_from_device_words(gpu, orc, env):
    """The same batch from device-resident words at 4-byte-aligned, not 16-byte-aligned
    addresses."""
    cases = [c for _, c, _ in _batch(gpu, orc)]
    bufs, items = [], []
    try:
        for k, c in enumerate(cases):
            s = gpu.parse(c.image)
            _, _, gaps, pay = fc.split(c.image)
            words = np.concatenate([gaps, pay]).astype(np.uint32)
            pad = 1 + k % 3  # 4, 8 or 12 bytes past a 16-byte boundary
            buf = gpu.DeviceBuffer(4 * (words.size + pad) + 16)
            bufs.append(buf)
            buf.upload(np.concatenate([np.zeros(pad, dtype=np.uint32), words]))
            gap_ptr = buf.addr + 4 * pad
            assert gap_ptr % 4 == 0 and gap_ptr % 16 != 0
            items.append((s, gap_ptr + 4 * gaps.size, gap_ptr))
        with gpu.BatchDecoder(0) as b:
            b.load_device(items)
            assert b.kernel_shape() == "batch<fb=1>"
            _decode_into(gpu, b, [c.data for c in cases])
    finally:
        for buf in bufs:
            buf.close()


@pytest.mark.gpu
def test_mixed_batch_index_and_gathers(gpu, orc, env):
    cases = [c for _, c, _ in _batch(gpu, orc)]
    ranges = _batch_ranges(cases, seed=5)
    assert len(ranges) > 40 * len(cases)
    with gpu.BatchDecoder(0) as b:
        b.load([c.image for c in cases])
        assert b.gather_kernel_shape() == "bgather<fb=1>"
        b.index()
        rep = b.wait()
        assert rep.bad_streams == 0 and rep.status == 0
        _gather_checked(gpu, b, [c.data for c in cases], ranges)


@pytest.mark.gpu
def test_batches_within_the_tables(gpu, orc, env):
    """Codes of at most 10 bits (the batch kernels' widest table): with the incomplete
    flat8_200 among them the batch still takes the fallback, for its hole alone; complete
    foreign codes alone do not."""
    short = [_case(orc, code, p)[0] for p in fc.PROFILES for code in ("cfg4like", "unused_syms")]
    flat = [_case(orc, "flat8_200", p)[0] for p in fc.PROFILES]
    assert all(c.symbols[-1][1] <= 10 for c in short + flat)
    assert all(fc.kraft(c.symbols) == 65536 for c in short) and all(fc.kraft(c.symbols) < 65536 for c in flat)
    mixed = [x for pair in zip(short, flat + flat) for x in pair]
    with gpu.BatchDecoder(0) as b:
        for cases, fb in ((mixed, 1), (short, 0)):
            b.load([c.image for c in cases])
            assert b.kernel_shape() == f"batch<fb={fb}>" and b.gather_kernel_shape() == f"bgather<fb={fb}>"
            _decode_into(gpu, b, [c.data for c in cases])
            _gather_checked(gpu, b, [c.data for c in cases], _batch_ranges(cases, seed=6 + fb))


@pytest.mark.gpu
def test_mixed_batch_raw(gpu, orc, env):
    """The same images without their gap words: the gap arrays the GPU builds equal each
    image's own and the oracle's, and the decode is exact."""
    cases = [c for _, c, _ in _batch(gpu, orc)]
    parts = [fc.split(c.image) for c in cases]
    with gpu.BatchDecoder(0) as b:
        b.load_raw([(syms, n, pay) for syms, n, _, pay in parts])
        assert b.raw_kernel_shape() == "batchraw<fb=1>" and b.kernel_shape() == "batch<fb=1>"
        assert b.raw_report().launches == 3
        for i, (c, (_, _, gaps, _)) in enumerate(zip(cases, parts)):
            got = b.raw_gaps(i)
            assert got.size == gaps.size and np.array_equal(got, gaps), f"stream {i}: gap words differ"
            assert np.array_equal(got, orc.raw_gaps(c.data, c.symbols)), f"stream {i}: not the oracle's"
        _decode_into(gpu, b, [c.data for c in cases])


# ---- the paired negative case ---------------------------------------------------------------
def _damaged(orc, code):
    """(Case, damaged image, first symbol of the damaged codeword's segment)."""
    c, _ = _case(orc, code, "uniform")
    bad, i = fc.damage(c.image, c.symbols, c.data)
    seg = _seg_first(c)
    return c, bad, int(seg[np.searchsorted(seg, i, "right") - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("code", ["k3", "holes16"])
def test_damaged_stream_is_flagged_by_the_wave_split(gpu, orc, env, code):
    """A handled error path: the walk is bounded by G, the stores are clipped at N (the
    output capacity, beyond which a download is refused)."""
    c, bad, safe = _damaged(orc, code)
    s = gpu.parse(bad)
    with gpu.Decoder(0) as d:
        d.load(s)
        assert WS_FB1.fullmatch(d.kernel_shape())
        d.decode()
        rep = d.report()
        out = d.download(s.n)
    assert rep.status == gpu.GH_ST_BADCODE and rep.out_bytes <= s.n
    _assert_same(out[:safe], c.data[:safe], "bytes before the damaged segment")
    with pytest.raises(gpu.GapHuffError) as e:
        gpu.decode(bad)
    assert e.value.code == GH_E_CORRUPT


@pytest.mark.gpu
@pytest.mark.parametrize("code", ["k3", "holes16"])
def test_damaged_stream_in_the_mixed_batch(gpu, orc, env, code):
    """Only the damaged stream is flagged; every other stream is exact, and nothing is written
    past any stream's N or into the guard."""
    batch = _batch(gpu, orc)
    k = [name for name, _, _ in batch].index(f"{code}/uniform")
    c, bad, safe = _damaged(orc, code)
    assert batch[k][1] is c
    datas = [x.data for _, x, _ in batch]
    imgs = [x.image for _, x, _ in batch]
    imgs[k] = bad
    off = gpu.batch_layout([d.size for d in datas])
    arena = int(off[-1])
    with gpu.BatchDecoder(0) as b, gpu.DeviceBuffer(arena + GUARD) as buf:
        b.load(imgs)
        assert b.kernel_shape() == "batch<fb=1>"
        buf.upload(np.full(arena + GUARD, FILL, dtype=np.uint8))
        b.decode(buf.addr, arena)
        with pytest.raises(gpu.GapHuffError) as e:
            b.wait()
        assert e.value.code == GH_E_CORRUPT
        assert e.value.report.bad_streams == 1 and e.value.report.status == gpu.GH_ST_BADCODE
        st, _ = b.status()
        assert st[k] == gpu.GH_ST_BADCODE and not np.delete(st, k).any()
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    _check_arena(got, off, datas, skip=(k,))
    lo = int(off[k])
    _assert_same(got[lo: lo + safe], c.data[:safe], "bytes before the damaged segment")
