"""Batched gap-less decode on the GPU: gh_batchraw_* / BatchDecoder.load_raw /
load_raw_device / raw_gaps / raw_report / decode_batch_raw and the decoder CLI's --batch on raw
containers.

All comparisons are bit-exact: the gap words the three kernels build equal the encoder's own
(a gap-array image minus its gap words is the raw stream, tests/test_sync.py), every decoded
byte equals the input.  The streams are the mixed batch of tests/test_gpu_batch.py with every
image stripped of its gap words (helpers copied from it); plus one stream of more units than a
chain step takes, 1 503 small streams through one workgroup, arbitrary words against the host
twin, a corrupt stream among good ones, device-resident sources and reloads."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cse375-finalproj-huffman-decoding_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
DECODER = os.path.join(ROOT, "bin", "decoder")
GH_E_ARG, GH_E_CORRUPT, GH_E_STATE, GH_E_SMALL = -1, -7, -8, -9
GUARD = 4096
ENV_KNOBS = ("GH_BATCH_GRID",)
RAW_MAGIC = 0x0000315741524847
CHAIN_STEP = 64  # aggregates one step of the chain kernel takes (one per lane)


# ---- prescribed codes and the mixed batch (copied from tests/test_gpu_batch.py) -----------
def _ladder(lo, hi, first=1):
    code = {lo: first}
    for l in range(lo + 1, hi):
        code[l] = 1
    left = 1.0 - sum(c * 2.0 ** -l for l, c in code.items())
    code[hi] = round(left * 2 ** hi)
    return code


def _coded(code, n, seed):
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
    "ladder_1_16": (_ladder(1, 16), 1 << 16),
    "one_symbol_128": ({1: 1}, 128),
    "one_symbol_129": ({1: 1}, 129),
    "grouped_4_8": ({4: 2, 8: 224}, 1 << 16),
    "ladder_2_7": (_ladder(2, 7, 3), 1 << 16),
}
GOLDENS = ("gen_r0.9_n1", "gen_r0.5_n7", "uniform256_exact_segments")
CUTS = [(r, g) for r in (0.1, 0.5, 0.9) for g in (255, 256, 257, 1023, 1024, 1025)]
SMALL = ("gen_r0.5_g1024", "gen_r0.1_g255", "ladder_2_7", "grouped_4_8", "uniform256_exact_segments", "gen_r0.5_n7",
         "empty")  # complete codes of at most 10 bits: no lookup can miss


def _cut(gh, r, target, seed):
    data = gh.generate(seed, r, 60_000)
    n = data.size
    for _ in range(12):
        img = gh.encode(data[:n])
        s = gh.parse(img)
        if s.g == target:
            return data[:n].copy(), img
        length_of = np.full(256, 16, dtype=np.int64)
        for sym, l in s.symbols:
            length_of[sym] = l
        n = int(np.searchsorted(np.cumsum(length_of[data]), 128 * target, "right"))
    raise AssertionError(f"no cut of r = {r} gives G = {target}")


_cache = {}


def _streams(gh):
    """[(name, data, image)] in the mixed batch's order, made once."""
    if "all" in _cache:
        return _cache["all"]
    out = [("empty", np.zeros(0, dtype=np.uint8), gh.encode(np.zeros(0, dtype=np.uint8))),
           ("n1", np.asarray([200], dtype=np.uint8), gh.encode(np.asarray([200], dtype=np.uint8)))]
    for name, (code, n) in CODES.items():
        data, want = _coded(code, n, seed=len(name))
        img = gh.encode(data)
        assert dict(gh.parse(img).symbols) == want, "package-merge did not return the prescribed lengths"
        out.append((name, data, img))
    for i, (r, g) in enumerate(CUTS):
        data, img = _cut(gh, r, g, seed=500 + i)
        out.append((f"gen_r{r}_g{g}", data, img))
    big = gh.generate(77, 0.5, 300_000)
    out.append(("gen_300k", big, gh.encode(big)))
    for name in GOLDENS:
        out.append((name, np.fromfile(os.path.join(GOLDEN, name + ".bin"), dtype=np.uint8),
                    np.fromfile(os.path.join(GOLDEN, name + ".huff"), dtype=np.uint8)))
    order = np.random.default_rng(3).permutation(len(out))
    out = [out[i] for i in order]
    tables = [tuple(gh.parse(img).symbols) for _, _, img in out]
    for k in range(1, len(out)):
        if tables[k] == tables[k - 1]:
            out.insert(0, out.pop(k))
            tables.insert(0, tables.pop(k))
    assert all(tables[k] != tables[k - 1] for k in range(1, len(out)))
    for _, data, _ in out:
        data.setflags(write=False)
    _cache["all"] = out
    return out


@pytest.fixture
def streams(gpu, monkeypatch):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    return _streams(gpu)


def _strip(gh, img):
    """An image without its gap words: ((symbols, n, payload words), its own gap words)."""
    s = gh.parse(img)
    nw = (s.g + 7) // 8
    assert s.g == -(-s.w // 4)
    gaps = s.raw[s.raw.size - 4 * (nw + s.w): s.raw.size - 4 * s.w].copy().view(np.uint32)
    pay = s.raw[s.raw.size - 4 * s.w:].copy().view(np.uint32)
    return (list(s.symbols), int(s.n), pay), gaps


def _container(raw):
    """The raw-stream container of a (symbols, n, units) triple (gaphuff.h, GH_RAW_MAGIC)."""
    symbols, n, units = raw
    head = np.asarray([RAW_MAGIC, len(symbols)], dtype="<u8").view(np.uint8)
    table = np.asarray(symbols, dtype=np.uint8).reshape(-1)
    sizes = np.asarray([n, units.size], dtype="<u8").view(np.uint8)
    return np.concatenate([head, table, sizes, np.asarray(units, dtype="<u4").view(np.uint8)])


def _check_arena(got, off, datas, skip=()):
    for i, d in enumerate(datas):
        lo, hi = int(off[i]), int(off[i + 1])
        if i not in skip:
            assert np.array_equal(got[lo: lo + d.size], d), f"stream {i} differs"
            assert (got[lo + d.size: hi] == 0xA5).all(), f"pad bytes after stream {i} were written"
    assert (got[int(off[-1]):] == 0xA5).all(), "guard bytes after the arena were written"


def _decode_into(gh, b, datas):
    """Decode b's loaded batch into a 0xA5-filled caller buffer with a guard; check every
    stream, every pad byte, the guard and the status."""
    ns = [d.size for d in datas]
    off = gh.batch_layout(ns)
    assert np.array_equal(b.offsets(), off)
    arena = int(off[-1])
    with gh.DeviceBuffer(arena + GUARD) as buf:
        buf.upload(np.full(arena + GUARD, 0xA5, dtype=np.uint8))
        b.decode(buf.addr, arena)
        rep = b.wait()
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    assert rep.nstreams == len(datas) and rep.bad_streams == 0 and rep.status == 0 and rep.launches == 3
    _check_arena(got, off, datas)
    st, sy = b.status()
    assert not st.any()
    return sy


def _check_gaps(b, gaps):
    for i, g in enumerate(gaps):
        got = b.raw_gaps(i)
        assert got.size == g.size and np.array_equal(got, g), f"stream {i}: gap words differ"


# ---- the batch --------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_batch_raw(gpu, streams):
    datas = [d for _, d, _ in streams]
    raws, gaps = zip(*[_strip(gpu, img) for _, _, img in streams])
    with gpu.BatchDecoder(0) as b, gpu.BatchDecoder(0) as ref:
        b.load_raw(raws)
        assert b.raw_kernel_shape() == "batchraw<fb=1>" and b.kernel_shape() == "batch<fb=1>"
        rep = b.raw_report()
        nunits = sum(-(-(-(-r[2].size // 4)) // 256) for r in raws)
        assert rep.launches == 3 and rep.gap_ms > 0 and rep.scratch_bytes == (8 * 256 + 8 + 4) * nunits
        _check_gaps(b, gaps)
        sy = _decode_into(gpu, b, datas)
        ref.load([img for _, _, img in streams])
        _check_gaps(ref, gaps)  # (raw_gaps after a gap-array load: the words it was given)
        ref.decode()
        ref.wait()
        assert np.array_equal(ref.status()[1], sy)
        with pytest.raises(gpu.GapHuffError) as e:
            ref.raw_report()
        assert e.value.code == GH_E_STATE


@pytest.mark.gpu
def test_stream_longer_than_a_chain_step(gpu):
    """One stream whose units - 1 aggregates need more than one step of the chain kernel: the
    scan inside a step, the step boundary and the 4-bit state carried between steps."""
    data = gpu.generate(91, 0.5, 400_000)
    img = gpu.encode(data)
    raw, gaps = _strip(gpu, img)
    units = -(-gpu.parse(img).g // 256)
    assert units - 1 > CHAIN_STEP and img.size < 400_000
    with gpu.BatchDecoder(0) as b:
        b.load_raw([raw])
        assert b.raw_report().launches == 3
        _check_gaps(b, [gaps])
        _decode_into(gpu, b, [data])


_ONE_WAVE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import gaphuff as gh
tiny = [gh.generate(40 + i, r, n) for i, (r, n) in enumerate([(0.1, 700), (0.5, 5000), (0.9, 9000), (0.5, 1), (0.0, 300)])]
tiny.append(np.full(2000, 7, dtype=np.uint8))  # the one-symbol code: fallback lookups
raws, gaps = [], []
for d in tiny:
    s = gh.parse(gh.encode(d))
    nw = (s.g + 7) // 8
    gaps.append(s.raw[s.raw.size - 4 * (nw + s.w): s.raw.size - 4 * s.w].copy().view(np.uint32))
    raws.append((list(s.symbols), int(s.n), s.raw[s.raw.size - 4 * s.w:].copy().view(np.uint32)))
order = np.random.default_rng(11).permutation(np.repeat(np.arange(5), 300))
order = np.concatenate([order, [5, 0, 5]])
with gh.BatchDecoder(0) as b:
    b.load_raw([raws[i] for i in order])
    assert b.raw_report().launches == 3
    for i, k in enumerate(order):
        assert np.array_equal(b.raw_gaps(i), gaps[k]), (i, k)
    b.decode()
    rep = b.wait()
    assert rep.bad_streams == 0 and rep.nstreams == order.size == 1503
    for k, got in zip(order, b.download_all()):
        assert np.array_equal(got, tiny[k]), k
    print("one-wave ok", b.raw_kernel_shape())
"""


@pytest.mark.gpu
def test_one_workgroup_walks_many_raw_streams(gpu):
    """GH_BATCH_GRID=1: one workgroup's four waves build the gap words of 1503 streams of six
    codes, reloading their tables again and again; the launch count stays 3."""
    r = subprocess.run([sys.executable, "-c", _ONE_WAVE, PKG], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, GH_BATCH_GRID="1"))
    assert r.returncode == 0 and "one-wave ok batchraw<fb=1>" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape", [("ladder_2_7", "batchraw<fb=0>"), ("ladder_1_16", "batchraw<fb=1>")])
def test_arbitrary_words_equal_the_host_twin(gpu, streams, name, shape):
    """Random u32 words, no valid stream: the device's gap words equal gh_batchraw_gaps_host's
    on the same words, under a complete code of at most 10 bits (no lookup misses) and under
    the 1..16-bit ladder (the canonical fallback).  Nothing is claimed about a decode."""
    symbols = list(gpu.parse({s[0]: s for s in streams}[name][2]).symbols)
    rng = np.random.default_rng(len(name))
    raws = [(symbols, 1, rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32))
            for w in (1, 5, 1023, 1024, 1025, 3 * 1024 + 2, 67 * 1024 + 3)]
    with gpu.BatchDecoder(0) as b:
        b.load_raw(raws)
        assert b.raw_kernel_shape() == shape
        _check_gaps(b, [gpu.raw_gaps_host(u, symbols) for _, _, u in raws])


@pytest.mark.gpu
def test_both_shapes_are_listed(gpu):
    """Each name of batchraw_kernel_shapes() is asserted through raw_kernel_shape() above."""
    assert sorted(gpu.batchraw_kernel_shapes()) == ["batchraw<fb=0>", "batchraw<fb=1>"]


@pytest.mark.gpu
def test_one_corrupt_stream_among_good_ones(gpu, streams):
    """The one-symbol code with a 1 bit in its payload (a pattern outside the code): the raw
    load succeeds, the decode flags that stream alone, every other stream's bytes and gap
    words are exact.  A handled error path: the walks advance maxlen bits and stay in bounds."""
    names = [n for n, _, _ in streams]
    k = names.index("one_symbol_129")
    datas = [d for _, d, _ in streams]
    raws, gaps = map(list, zip(*[_strip(gpu, img) for _, _, img in streams]))
    bad = raws[k][2].copy()
    assert not bad.any()
    bad[1] |= 1 << 9
    raws[k] = (raws[k][0], raws[k][1], bad)
    off = gpu.batch_layout([d.size for d in datas])
    arena = int(off[-1])
    with gpu.BatchDecoder(0) as b, gpu.DeviceBuffer(arena + GUARD) as buf:
        b.load_raw(raws)
        _check_gaps(b, gaps)  # (the bad stream's too: one-bit steps keep every entry 0)
        buf.upload(np.full(arena + GUARD, 0xA5, dtype=np.uint8))
        b.decode(buf.addr, arena)
        with pytest.raises(gpu.GapHuffError) as e:
            b.wait()
        assert e.value.code == GH_E_CORRUPT
        assert e.value.report.bad_streams == 1 and e.value.report.status == gpu.GH_ST_BADCODE
        st, _ = b.status()
        assert st[k] == gpu.GH_ST_BADCODE and not np.delete(st, k).any()
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    _check_arena(got, off, datas, skip=(k,))


@pytest.mark.gpu
def test_device_load_unaligned(gpu, streams):
    """The same batch from device-resident payload words at 4-byte-aligned, not 16-byte-aligned
    addresses; no gap pointer is given.  g != ceil(w / 4) is refused."""
    datas = [d for _, d, _ in streams]
    parsed = [gpu.parse(img) for _, _, img in streams]
    gaps = [_strip(gpu, img)[1] for _, _, img in streams]
    bufs, items = [], []
    try:
        for k, s in enumerate(parsed):
            words = s.raw[s.raw.size - 4 * s.w:].copy().view(np.uint32)
            pad = 1 + k % 3  # 4, 8 or 12 bytes past a 16-byte boundary
            buf = gpu.DeviceBuffer(4 * (words.size + pad) + 16)
            bufs.append(buf)
            if words.size:
                buf.upload(np.concatenate([np.zeros(pad, dtype=np.uint32), words]))
            pay_ptr = buf.addr + 4 * pad
            assert pay_ptr % 4 == 0 and pay_ptr % 16 != 0
            items.append((s, pay_ptr if s.w else 0, 0))
        with gpu.BatchDecoder(0) as b:
            b.load_raw_device(items)
            assert b.raw_kernel_shape() == "batchraw<fb=1>"
            _check_gaps(b, gaps)
            _decode_into(gpu, b, datas)
            k = next(i for i, s in enumerate(parsed) if s.g > 1)
            wrong = copy.copy(parsed[k])
            wrong.c = type(parsed[k].c).from_buffer_copy(parsed[k].c)
            wrong.c.g = parsed[k].g - 1
            with pytest.raises(gpu.GapHuffError) as e:
                b.load_raw_device(items[:k] + [(wrong, items[k][1], 0)] + items[k + 1:])
            assert e.value.code == GH_E_ARG and f"stream {k}:" in str(e.value)
    finally:
        for buf in bufs:
            buf.close()


@pytest.mark.gpu
def test_raw_load_refusals_name_the_stream(gpu, streams):
    """A raw stream that fails gh_raw_parse's checks (more symbols than its bits can hold; a
    code that is not canonical) fails the whole load with that check's code and its index in
    the message; the batch then holds nothing.  A short buffer for the gap words is refused."""
    by_name = {s[0]: s for s in streams}
    good = [_strip(gpu, by_name[n][2])[0] for n in ("gen_r0.5_g255", "n1", "gen_r0.1_g256")]
    symbols, n, units = good[2]
    with gpu.BatchDecoder(0) as b:
        for bad, code in (((symbols, 32 * units.size + 1, units), -2), ((symbols[::-1], n, units), -3)):
            with pytest.raises(gpu.GapHuffError) as e:
                b.load_raw([good[0], good[1], bad])
            assert e.value.code == code and "stream 2:" in str(e.value)
            with pytest.raises(gpu.GapHuffError) as e:
                b.decode()
            assert e.value.code == GH_E_STATE
            with pytest.raises(gpu.GapHuffError) as e:
                b.raw_gaps(0)
            assert e.value.code == GH_E_STATE
        b.load_raw(good)
        import ctypes
        nw = ctypes.c_uint64()
        out = np.zeros(64, dtype=np.uint32)
        L = gpu.lib()
        assert L.gh_batchraw_gaps(b._h, 0, out.ctypes.data, 3, ctypes.byref(nw)) == GH_E_SMALL and nw.value == 32
        assert L.gh_batchraw_gaps(b._h, 3, out.ctypes.data, 64, ctypes.byref(nw)) == GH_E_ARG and nw.value == 0
        assert L.gh_batchraw_gaps(b._h, 0, out.ctypes.data, 64, None) == GH_E_ARG
        assert not out.any()
        assert gpu.decode_batch_raw([]) == []


@pytest.mark.gpu
def test_encoder_items_without_gap_words(gpu, streams):
    """BatchEncoder.items() with the gap pointers nulled into load_raw_device: the gap words
    built on the device equal the encoder's own, downloaded; every output equals the input."""
    pick = [s for s in streams if s[0] in ("gen_r0.5_g1025", "ladder_1_16", "n1", "empty", "gen_r0.1_g256", "gen_300k")]
    datas = [d for _, d, _ in pick]
    with gpu.BatchEncoder(0) as e, gpu.BatchDecoder(0) as d:
        e.load(datas)
        e.plan()
        e.encode()
        assert e.wait().status == 0
        own = [_strip(gpu, e.download(i))[1] for i in range(len(datas))]
        d.load_raw_device([(s, pay, 0) for s, pay, _ in e.items()])
        _check_gaps(d, own)
        _decode_into(gpu, d, datas)


@pytest.mark.gpu
def test_reload_raw_gap_raw(gpu, streams):
    """Raw, then gap-array, then raw on one BatchDecoder; raw_report's launch count is the
    same for 1 stream and for the mixed batch, and GH_E_STATE after a gap-array load."""
    by_name = {s[0]: s for s in streams}
    one = by_name["gen_r0.9_g257"]
    small = [by_name[n] for n in SMALL]
    with gpu.BatchDecoder(0) as b:
        with pytest.raises(gpu.GapHuffError) as e:
            b.raw_report()
        assert e.value.code == GH_E_STATE
        raws, gaps = zip(*[_strip(gpu, img) for _, _, img in streams])
        b.load_raw(raws)
        many = b.raw_report().launches
        _check_gaps(b, gaps)
        b.load([img for _, _, img in small])
        with pytest.raises(gpu.GapHuffError) as e:
            b.raw_report()
        assert e.value.code == GH_E_STATE
        with pytest.raises(gpu.GapHuffError) as e:
            b.raw_kernel_shape()
        assert e.value.code == GH_E_STATE
        _decode_into(gpu, b, [d for _, d, _ in small])
        raw, gap = _strip(gpu, one[2])
        b.load_raw([raw])
        assert b.raw_report().launches == many == 3
        _check_gaps(b, [gap])
        _decode_into(gpu, b, [one[1]])
        raws, gaps = zip(*[_strip(gpu, img) for _, _, img in small])
        b.load_raw(raws)
        assert b.raw_kernel_shape() == "batchraw<fb=0>" and b.kernel_shape() == "batch<fb=0>"
        _check_gaps(b, gaps)
        _decode_into(gpu, b, [d for _, d, _ in small])
        b.load_raw([])
        assert b.raw_kernel_shape() == "" and b.raw_report().launches == 3 and b.raw_report().scratch_bytes == 0
        b.decode()
        assert b.wait().nstreams == 0


@pytest.mark.gpu
def test_index_and_gather_on_a_raw_batch(gpu, streams):
    """index() + gather() run unchanged on a raw batch: three ranges longer than any unit's
    bytes (a unit of 256 segments holds at most 16 384 codewords of 2 bits or more), so each
    crosses a unit edge and is cut into several pieces."""
    by_name = {s[0]: s for s in streams}
    pick = [by_name[n] for n in ("gen_300k", "gen_r0.5_g1025", "gen_r0.1_g1024")]
    datas = [d for _, d, _ in pick]
    assert datas[0].size >= 40_010 and datas[1].size >= 20_000
    assert all(min(l for _, l in gpu.parse(img).symbols) >= 2 for _, _, img in pick)
    ranges = [(0, 10, 40_010), (2, 3, datas[2].size), (1, datas[1].size - 20_000, datas[1].size), (0, 7, 7)]
    with gpu.BatchDecoder(0) as b:
        b.load_raw([_strip(gpu, img)[0] for _, _, img in pick])
        b.index()
        got = b.gather(ranges)
        assert b.gather_pieces().size >= 2 * 3
        assert gpu.decode_batch_raw([_strip(gpu, pick[1][2])[0]])[0].size == datas[1].size
    for (s, lo, hi), out in zip(ranges, got):
        assert np.array_equal(out, datas[s][lo:hi]), (s, lo, hi)


# ---- the CLI ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_raw_batch(gpu, streams, tmp_path):
    by_name = {s[0]: s for s in streams}
    pick = [by_name[n] for n in ("gen_r0.5_g257", "ladder_1_16", "gen_r0.9_n1")]
    lines = []
    for name, _, img in pick:
        _container(_strip(gpu, img)[0]).tofile(tmp_path / (name + ".raw"))
        lines.append(f"{tmp_path / (name + '.raw')}\t{tmp_path / (name + '.out')}\n")
    lst = tmp_path / "batch.txt"
    lst.write_text("".join(lines))
    r = subprocess.run([DECODER, "--batch", str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "Batch: 3 streams" in r.stdout
    for name, data, _ in pick:
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out"), dtype=np.uint8), data), name
    # --ranges on the raw batch
    rng_file = tmp_path / "ranges.txt"
    rng_file.write_text("1 100:50100\n0 0:10\n")
    r = subprocess.run([DECODER, "--batch", str(lst), "--ranges", str(rng_file), str(tmp_path / "ranges.out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert np.array_equal(np.fromfile(tmp_path / "ranges.out", dtype=np.uint8),
                          np.concatenate([pick[1][1][100:50100], pick[0][1][0:10]]))
    # a compressed.huff file on line 2 of a list of raw containers: refused, the line named
    np.asarray(pick[1][2]).tofile(tmp_path / "mixed.huff")
    lst.write_text(lines[0] + f"{tmp_path / 'mixed.huff'}\t{tmp_path / 'mixed.out'}\n" + lines[2])
    for name, _, _ in pick:
        (tmp_path / (name + ".out")).unlink()
    bad = subprocess.run([DECODER, "--batch", str(lst)], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "line 2" in bad.stderr and "mixed.huff" in bad.stderr, bad.stdout + bad.stderr
    assert not any((tmp_path / (name + ".out")).exists() for name, _, _ in pick)
