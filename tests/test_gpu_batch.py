"""Batched decode on the GPU: gh_batch_* / BatchDecoder / decode_batch and the decoder CLI's
--batch.

Every output is compared with the original input bytes.  The streams are made with
gh.encode; the prescribed-code helpers _ladder and _coded are copied from
tests/test_gpu_gather.py.  The set is the smallest that reaches each hazard: the empty
stream; n = 1; the one-symbol code (incomplete: every lookup of a 1 bit misses) at n = 128
(one segment of 128 one-bit codewords) and n = 129 (two segments); a 1..16-bit ladder at
n = 65536 (a 1-bit codeword, 16-bit codewords past the 10-bit table, the canonical fallback,
up to 143 symbols per segment); a grouped 4/8-bit code and a 2..7-bit ladder; generated data
at r = 0.1 / 0.5 / 0.9 cut so that G = 255, 256, 257, 1023, 1024, 1025 (work-unit edges); one
stream of 300 000 bytes (dozens of units: the in-stream prefix); three goldens."""
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


# ---- prescribed codes (copied from tests/test_gpu_gather.py) ---------------------------
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
    "ladder_1_16": (_ladder(1, 16), 1 << 16),
    "one_symbol_128": ({1: 1}, 128),
    "one_symbol_129": ({1: 1}, 129),
    "grouped_4_8": ({4: 2, 8: 224}, 1 << 16),
    "ladder_2_7": (_ladder(2, 7, 3), 1 << 16),
}
GOLDENS = ("gen_r0.9_n1", "gen_r0.5_n7", "uniform256_exact_segments")
CUTS = [(r, g) for r in (0.1, 0.5, 0.9) for g in (255, 256, 257, 1023, 1024, 1025)]


def _cut(gh, r, target, seed):
    """Generated data cut where its bits fill exactly `target` segments (the construction of
    test_gpu_gather's g_256k_plus_1, repeated until the cut's own code gives that G)."""
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
    # interleaved: a fixed shuffle in which no two neighbours share a code
    order = np.random.default_rng(3).permutation(len(out))
    out = [out[i] for i in order]
    tables = [tuple(gh.parse(img).symbols) for _, _, img in out]
    for k in range(1, len(out)):
        if tables[k] == tables[k - 1]:  # (the two one-symbol streams): move one to the front
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


def _decode_into(gh, b, datas, hip_stream=0):
    """Decode b's loaded batch into a 0xA5-filled caller buffer with a guard; check every
    stream, every pad byte, the guard, the status, the counts and the offsets."""
    ns = [d.size for d in datas]
    off = gh.batch_layout(ns)
    assert np.array_equal(b.offsets(), off)
    arena = int(off[-1])
    with gh.DeviceBuffer(arena + GUARD) as buf:
        buf.upload(np.full(arena + GUARD, 0xA5, dtype=np.uint8))
        b.decode(buf.addr, arena, hip_stream)
        rep = b.wait()
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    assert rep.nstreams == len(datas) and rep.bad_streams == 0 and rep.status == 0
    assert rep.out_bytes == sum(ns) and rep.kernel_ms >= 0 and 1 <= rep.launches <= 8
    _check_arena(got, off, datas)
    st, sy = b.status()
    assert not st.any()
    assert (sy >= np.asarray(ns, dtype=np.uint64)).all()
    return rep


def _check_arena(got, off, datas, skip=()):
    for i, d in enumerate(datas):
        lo, hi = int(off[i]), int(off[i + 1])
        if i not in skip:
            assert np.array_equal(got[lo: lo + d.size], d), f"stream {i} differs"
            assert (got[lo + d.size: hi] == 0xA5).all(), f"pad bytes after stream {i} were written"
    assert (got[int(off[-1]):] == 0xA5).all(), "guard bytes after the arena were written"


# ---- the batch --------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_batch(gpu, streams):
    datas = [d for _, d, _ in streams]
    with gpu.BatchDecoder(0) as b:
        b.load([img for _, _, img in streams])
        assert b.kernel_shape() == "batch<fb=1>"  # (the ladder's 16-bit codewords, the one-symbol code)
        rep = _decode_into(gpu, b, datas)
        assert rep.launches == 3
        # the batch's own arena, through download
        b.decode()
        b.wait()
        for d, got in zip(datas, b.download_all()):
            assert np.array_equal(got, d)
        addr, cap = b.output()
        assert addr and cap >= int(gpu.batch_layout([d.size for d in datas])[-1])


_ONE_WAVE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import gaphuff as gh
tiny = [gh.generate(40 + i, r, n) for i, (r, n) in enumerate([(0.1, 700), (0.5, 5000), (0.9, 9000), (0.5, 1), (0.0, 300)])]
tiny.append(np.full(2000, 7, dtype=np.uint8))  # the one-symbol code: fallback lookups
imgs = [gh.encode(d) for d in tiny]
order = np.random.default_rng(11).permutation(np.repeat(np.arange(5), 300))
order = np.concatenate([order, [5, 0, 5]])
with gh.BatchDecoder(0) as b:
    b.load([imgs[i] for i in order])
    b.decode()
    rep = b.wait()
    assert rep.bad_streams == 0 and rep.nstreams == order.size
    for k, got in zip(order, b.download_all()):
        assert np.array_equal(got, tiny[k]), k
    print("one-wave ok", b.kernel_shape())
"""


@pytest.mark.gpu
def test_one_wave_walks_many_streams(gpu):
    """GH_BATCH_GRID=1: one workgroup's four waves walk 1503 streams of six codes, so every
    wave reloads its tables again and again and strides over many units."""
    r = subprocess.run([sys.executable, "-c", _ONE_WAVE, PKG], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, GH_BATCH_GRID="1"))
    assert r.returncode == 0 and "one-wave ok batch<fb=1>" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_device_load(gpu, streams):
    """The same batch from device-resident words at 4-byte-aligned, not 16-byte-aligned
    addresses."""
    datas = [d for _, d, _ in streams]
    parsed = [gpu.parse(img) for _, _, img in streams]
    bufs, items = [], []
    try:
        for k, s in enumerate(parsed):
            gw = -(-s.g // 8)
            words = s.raw[s.raw.size - 4 * (gw + s.w):].copy().view(np.uint32)  # gap words, then payload
            assert words.size == gw + s.w
            pad = 1 + k % 3  # 4, 8 or 12 bytes past a 16-byte boundary
            buf = gpu.DeviceBuffer(4 * (words.size + pad) + 16)
            bufs.append(buf)
            if words.size:
                buf.upload(np.concatenate([np.zeros(pad, dtype=np.uint32), words]))
            gap_ptr = buf.addr + 4 * pad
            pay_ptr = gap_ptr + 4 * gw
            assert pay_ptr % 4 == 0 and (gap_ptr % 16 != 0)
            items.append((s, pay_ptr if s.w else 0, gap_ptr if s.g else 0))
        with gpu.BatchDecoder(0) as b:
            b.load_device(items)
            assert b.kernel_shape() == "batch<fb=1>"
            _decode_into(gpu, b, datas)
    finally:
        for buf in bufs:
            buf.close()


@pytest.mark.gpu
def test_caller_stream_and_reuse(gpu, streams):
    """A caller's destination on a caller's stream; two decodes without a reload; then a
    smaller, different batch (complete codes of at most 10 bits: batch<fb=0>) in the same
    object."""
    import torch
    datas = [d for _, d, _ in streams]
    small = [s for s in streams if s[0] in ("gen_r0.5_g1024", "gen_r0.1_g255", "ladder_2_7", "grouped_4_8",
                                            "uniform256_exact_segments", "gen_r0.5_n7", "empty")]
    assert len(small) == 7
    for _, _, img in small:  # complete codes of at most 10 bits: no lookup can miss
        lens = [l for _, l in gpu.parse(img).symbols]
        assert max(lens, default=0) <= 10 and sum(2.0 ** -l for l in lens) in (0, 1.0)
    st = torch.cuda.Stream()
    with gpu.BatchDecoder(0) as b:
        with pytest.raises(gpu.GapHuffError) as e:
            b.decode()
        assert e.value.code == GH_E_STATE
        b.load([img for _, _, img in streams])
        _decode_into(gpu, b, datas, hip_stream=st.cuda_stream)
        _decode_into(gpu, b, datas, hip_stream=st.cuda_stream)
        b.load([img for _, _, img in small])
        assert b.kernel_shape() == "batch<fb=0>"
        _decode_into(gpu, b, [d for _, d, _ in small], hip_stream=st.cuda_stream)
        # refusals: a short destination, a misaligned one
        arena = int(b.offsets()[-1])
        with gpu.DeviceBuffer(arena + 16) as buf:
            with pytest.raises(gpu.GapHuffError) as e:
                b.decode(buf.addr, arena - 1)
            assert e.value.code == GH_E_SMALL
            with pytest.raises(gpu.GapHuffError) as e:
                b.decode(buf.addr + 4, arena)
            assert e.value.code == GH_E_ARG
        b.load([])
        assert b.kernel_shape() == "" and b.offsets().tolist() == [0]
        b.decode()
        assert b.wait().nstreams == 0


def _raise_n(img, by):
    """The image with its header N raised (v1 header: u64 S, S x 2 bytes, u32 N)."""
    bad = np.array(img, dtype=np.uint8)
    s = int(bad[:8].view("<u8")[0])
    assert s <= 256
    at = 8 + 2 * s
    bad[at: at + 4] = np.asarray([int(bad[at: at + 4].view("<u4")[0]) + by], dtype="<u4").view(np.uint8)
    return bad


@pytest.mark.gpu
def test_one_bad_stream_among_good_ones(gpu, streams):
    """A stream whose header claims 1000 symbols more than it holds (more than the at most
    143 padding codewords of a last segment): GH_E_CORRUPT, that stream flagged, every other
    stream exact and its pad bytes untouched.  A handled error path: the walk is bounded by
    G, the stores are clipped at N."""
    names = [n for n, _, _ in streams]
    k = names.index("gen_r0.5_g257")
    datas = [d for _, d, _ in streams]
    imgs = [img for _, _, img in streams]
    imgs[k] = _raise_n(imgs[k], 1000)
    assert gpu.parse(imgs[k]).n == datas[k].size + 1000
    ns = [d.size for d in datas]
    ns[k] += 1000
    off = gpu.batch_layout(ns)
    arena = int(off[-1])
    with gpu.BatchDecoder(0) as b, gpu.DeviceBuffer(arena + GUARD) as buf:
        b.load(imgs)
        buf.upload(np.full(arena + GUARD, 0xA5, dtype=np.uint8))
        b.decode(buf.addr, arena)
        with pytest.raises(gpu.GapHuffError) as e:
            b.wait()
        assert e.value.code == GH_E_CORRUPT
        assert e.value.report.bad_streams == 1 and e.value.report.status == gpu.GH_ST_BADCODE
        st, sy = b.status()
        assert st[k] & gpu.GH_ST_BADCODE and not np.delete(st, k).any()
        assert datas[k].size <= sy[k] < ns[k]
        got = buf.download(np.zeros(arena + GUARD, dtype=np.uint8))
    _check_arena(got, off, datas, skip=(k,))
    # the bad stream's own bytes: what it holds is decoded, nothing past its counted symbols
    lo = int(off[k])
    assert np.array_equal(got[lo: lo + datas[k].size], datas[k])
    assert (got[lo + int(sy[k]): int(off[k + 1])] == 0xA5).all()


@pytest.mark.gpu
def test_load_refusals_name_the_stream(gpu, streams):
    """A stream that fails the host validation fails the whole load with that check's code
    and its index in the message; the batch then holds nothing."""
    import copy
    by_name = {s[0]: s for s in streams}
    good = [gpu.parse(by_name[n][2]) for n in ("gen_r0.5_g255", "n1", "gen_r0.1_g256")]
    with gpu.BatchDecoder(0) as b:
        for field, value, code in (("w", 4 * good[2].g + 1, -2), ("n", 1 << 40, -2)):
            bad = copy.copy(good[2])
            bad.c = type(good[2].c).from_buffer_copy(good[2].c)
            setattr(bad.c, field, value)
            with pytest.raises(gpu.GapHuffError) as e:
                b.load([good[0], good[1], bad])
            assert e.value.code == code and "stream 2:" in str(e.value)
            with pytest.raises(gpu.GapHuffError) as e:
                b.decode()
            assert e.value.code == GH_E_STATE
        b.load(good)
        with pytest.raises(gpu.GapHuffError) as e:
            b.wait()  # no decode since the load
        assert e.value.code == GH_E_STATE
        b.decode()
        b.wait()
        assert np.array_equal(b.download(2), by_name["gen_r0.1_g256"][1])


@pytest.mark.gpu
def test_every_compiled_shape_is_picked(gpu):
    """Each name of batch_kernel_shapes() is asserted through kernel_shape() by a case above:
    fb=1 by the mixed batch, the device load and the one-wave walk, fb=0 by the reuse case."""
    assert sorted(gpu.batch_kernel_shapes()) == ["batch<fb=0>", "batch<fb=1>"]


@pytest.mark.gpu
def test_decode_batch_one_shot(gpu, streams):
    pick = [s for s in streams if s[0] in ("empty", "n1", "gen_r0.1_g256", "one_symbol_129")]
    for (_, d, _), got in zip(pick, gpu.decode_batch([img for _, _, img in pick])):
        assert np.array_equal(got, d)
    assert gpu.decode_batch([]) == []


# ---- the CLI ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_batch(gpu, streams, tmp_path):
    by_name = {s[0]: s for s in streams}
    pick = [by_name[n] for n in ("gen_r0.5_g257", "ladder_1_16", "gen_r0.9_n1")]
    lines = []
    for name, _, img in pick:
        np.asarray(img).tofile(tmp_path / (name + ".huff"))
        lines.append(f"{tmp_path / (name + '.huff')}\t{tmp_path / (name + '.out')}\n")
    lst = tmp_path / "batch.txt"
    lst.write_text("".join(lines))
    r = subprocess.run([DECODER, "--batch", str(lst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "Batch: 3 streams" in r.stdout
    for name, data, _ in pick:
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out"), dtype=np.uint8), data), name
    # a corrupt stream on line 2: non-zero exit, its line named, the others still written
    _raise_n(pick[0][2], 1000).tofile(tmp_path / "bad.huff")
    lst.write_text(lines[1] + f"{tmp_path / 'bad.huff'}\t{tmp_path / 'bad.out'}\n" + lines[2])
    for name, _, _ in pick:
        (tmp_path / (name + ".out")).unlink()
    bad = subprocess.run([DECODER, "--batch", str(lst)], capture_output=True, text=True, timeout=120)
    assert bad.returncode not in (0, 2), bad.stdout + bad.stderr
    assert "line 2" in bad.stderr and "bad.huff" in bad.stderr
    assert not (tmp_path / "bad.out").exists()
    for name, data, _ in pick[1:]:
        assert np.array_equal(np.fromfile(tmp_path / (name + ".out"), dtype=np.uint8), data), name
