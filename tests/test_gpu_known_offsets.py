"""Known piece offsets of the tile kernel (csrc/gh_tile.hip, DESIGN.md "Known piece offsets").

The first decodes after a load run the chained kernel, which records every wave piece's
output offset; once the host has seen such a decode finish with status 0
(Decoder.offsets_state() == GH_OFFS_READY) later decodes of the same load run the
known-offsets instantiation, which reads the offsets, stages every piece at the 16-byte
phase of its output offset and copies it out with aligned LDS reads.

Every test decodes one context several times.  The device output (and the guard bytes the
allocation keeps after it) is filled with a pattern before each decode, so the bytes
compared are the ones that decode wrote, and the bytes past the capacity must still hold
the pattern.  Outputs are compared with the input, which the stream builders of
tests/test_gpu_shapes.py and tests/test_gpu_tile_tail.py have already compared with
oracle.decode.  No test provokes a failing status."""
import ctypes

import numpy as np
import pytest

import foreign_codes as fc
import test_gpu_shapes as shapes
import test_gpu_tile_tail as tail

NONE, RECORDED, READY = 0, 1, 2
FILL = 0xA5
GUARD = 64  # bytes the context allocates past max(out_cap, 16)
SETTINGS = {"default": {}, "grid3": {"GH_TILE_GRID": "3"}}


def _setenv(monkeypatch, env):
    shapes._setenv(monkeypatch, env)
    if "GH_TILE_OFFS" not in env:
        monkeypatch.delenv("GH_TILE_OFFS", raising=False)


def _fill(gpu, d, nbytes):
    ptr, cap = d.output()
    assert nbytes <= max(cap, 16) + GUARD
    pat = np.full(nbytes, FILL, np.uint8)
    assert gpu.lib().gh_dev_copy(ctypes.c_void_p(ptr), pat.ctypes.data_as(ctypes.c_void_p), nbytes) == 0


def _read(gpu, d, nbytes):
    ptr, _ = d.output()
    out = np.empty(nbytes, np.uint8)
    assert gpu.lib().gh_dev_copy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), nbytes) == 0
    return out


def _check_bytes(what, out, want, keep, slack=0):
    """out[:keep] are the wanted bytes; everything after them (after the `slack` bytes a
    stream's last segment may decode from its padding) still holds the pattern."""
    if not np.array_equal(out[:keep], want[:keep]):
        bad = np.flatnonzero(out[:keep] != want[:keep])
        raise AssertionError(f"{what}: {bad.size} wrong bytes of {keep}, first at {bad[0]}")
    over = np.flatnonzero(out[keep + slack:] != FILL)
    assert over.size == 0, f"{what}: {over.size} bytes written past the end, first at {keep + slack + over[0]}"


def _three_decodes(gpu, d, want, keep, what, ready=True, slack=0):
    """Three decodes of the loaded shard, a report after the first; `want[:keep]` is what
    each must write, the guard bytes stay.  Returns the states seen before each decode."""
    _, cap = d.output()
    span = max(cap, 16) + GUARD
    states = []
    for i in range(3):
        _fill(gpu, d, span)
        states.append(d.offsets_state())
        d.decode()
        if i == 0:
            if ready:
                assert d.offsets_state() == RECORDED
            rep = d.report()
            assert rep.status == 0
        out = _read_after(gpu, d, span)
        _check_bytes(f"{what}, decode {i + 1}", out, want, keep, slack)
    rep = d.report()
    assert rep.status == 0
    assert states == ([NONE, READY, READY] if ready else [NONE, NONE, NONE]), states
    assert d.offsets_state() == (READY if ready else NONE)
    return rep


def _read_after(gpu, d, span):
    d.download(1)  # waits for the last decode, whatever stream it ran on
    return _read(gpu, d, span)


# ---- all nine shapes ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in shapes.TILE_ROWS for st in SETTINGS])
def test_every_tile_shape(gpu, orc, monkeypatch, row, setting):
    code, name = shapes.TILE_ROWS[row]
    data, img, total = shapes._case(gpu, orc, code, shapes.N_TILE, "shuffled")
    _setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        assert d.kernel_shape() == name and d.offsets_state() == NONE
        rep = _three_decodes(gpu, d, data, s.n, f"{name} {setting}")
        assert d.kernel_shape() == name  # a shape names U / G / OW / MINL, not the mode
        assert rep.symbols == total and rep.out_bytes == s.n and gpu.MODE_NAMES[rep.mode] == "tile"
        if setting == "grid3":
            assert rep.grid == 3


# ---- extreme piece lengths ----------------------------------------------------------
# id: (code, U, expected kernel, length of nearly every codeword, one codeword in `every` of
# the other length, tiles).  A stream of one codeword length alone gives its wave pieces
# lengths of a short period (64 U x 128 bits hold 2048 12-bit codewords when U = 3, and
# three pieces of U = 2 hold 4096), so their offsets would reach one to five residues mod 16
# only; one codeword in a few thousand therefore has the other length, which moves the
# phase by a byte every piece or two.  The 4-bit and 3-bit streams exceed every staging region: all
# their pieces take the direct-store path.
EXTREME = {
    "longest_u2_12bit": ({3: 4, 8: 120, 12: 128}, 2, "tile<1024,2,2,11,3>", 12, 1000, 8, 24),
    "longest_u3_12bit": ({4: 2, 8: 222, 12: 32}, 3, "tile<1024,3,2,8,4>", 12, 1000, 8, 20),
    "longest_u2_10bit": ({3: 7, 8: 28, 10: 16}, 2, "tile<1024,2,3,11,3>", 10, 1000, 8, 24),
    "shortest_4bit_ow8": ({4: 2, 8: 224}, 3, "tile<1024,3,4,8,4>", 4, 3001, 8, 20),
    "shortest_3bit_ow11": ({3: 4, 8: 128}, 2, "tile<1024,2,4,11,3>", 3, 3001, 8, 20),
}
_extreme = {}


def _extreme_case(gh, orc, row):
    if row not in _extreme:
        code, u, _, ln, every, other, tiles = EXTREME[row]
        vals, lens = shapes._symbols(code)
        rng = np.random.default_rng(len(row))
        nseg = tiles * 1024 * u - 777  # (a partial last tile)
        n = nseg * 128 // ln
        pool = vals[lens == ln]
        data = pool[rng.integers(0, pool.size, n)]
        if every:
            opool = vals[lens == other]
            data[every - 1::every] = opool[rng.integers(0, opool.size, data[every - 1::every].size)]
        syms = [(int(v), int(l)) for v, l in zip(vals, lens)]
        assert fc.kraft(syms) == 65536
        img = fc.image(orc, syms, data)
        ref, _ = orc.decode(img)
        assert np.array_equal(ref, data), "the oracle does not return the input"
        # on the CPU: the offsets of the wave pieces (64 U segments each) reach every residue
        kept, _, _ = tail._kept(code, data)
        s = gh.parse(img)
        assert kept.size == s.g
        per_seg = data.size / s.g
        assert (10 <= per_seg <= 13) if ln >= 10 else (per_seg > 31)
        piece = np.add.reduceat(kept, np.arange(0, kept.size, 64 * u))
        goff = np.cumsum(piece) - piece
        assert set((goff & 15).tolist()) == set(range(16)), "the pieces do not start at every residue mod 16"
        data.setflags(write=False)
        _extreme[row] = (data, img)
    return _extreme[row]


@pytest.mark.parametrize("row", EXTREME)
def test_extreme_streams_reach_every_phase(gh, orc, row):
    """No GPU: the preconditions of the extreme streams."""
    _extreme_case(gh, orc, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in EXTREME for st in SETTINGS])
def test_extreme_piece_lengths(gpu, orc, monkeypatch, row, setting):
    data, img = _extreme_case(gpu, orc, row)
    _setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        assert d.kernel_shape() == EXTREME[row][2]
        _three_decodes(gpu, d, data, s.n, f"{row} {setting}")


# ---- shard ranges -------------------------------------------------------------------
def _ranges(u, g):
    t = 1024 * u
    rs = [(1, g), (7, t + 64 * u), (9, t + 16),   # b inside a gap dword
          (0, 3 * t + 1), (3, 2 * t + 4),          # a last tile of one segment
          (0, t), (5, 5 + t),                      # exactly one tile
          (11, 12)]                                # one segment
    rs += [(5, 5 + 2 * t + r) for r in range(8)]   # e - b = 0 .. 7 mod 8
    return rs


@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in tail.ROWS for st in SETTINGS])
def test_shard_ranges(gpu, orc, monkeypatch, row, setting):
    ref, img, kept = tail._case(gpu, orc, row)
    _, u, _, name, _ = tail.ROWS[row]
    _setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:  # one context: every load but the first is a reload
        for b, e in _ranges(u, s.g):
            off, n = int(kept[:b].sum()), int(kept[b:e].sum())
            d.load(s, b, e)
            assert d.kernel_shape() == name and d.offsets_state() == NONE
            # (the stream's last segment: its padding decodes to symbols too, within the capacity)
            rep = _three_decodes(gpu, d, ref[off:], n, f"{name} [{b}, {e}) {setting}", slack=43 if e == s.g else 0)
            assert gpu.MODE_NAMES[rep.mode] == "tile" and rep.tiles == -(-(e - b) // (1024 * u))
            assert (rep.symbols == n) if e < s.g else (n <= rep.symbols < n + 43)


@pytest.mark.gpu
def test_shards_the_tile_kernel_does_not_take_stay_none(gpu, orc, monkeypatch):
    """An empty shard and a shard decoded by another kernel never leave NONE and decode."""
    code, _ = shapes.TILE_ROWS["g3_ow7"]
    data, img, _ = shapes._case(gpu, orc, code, shapes.N_TILE, "shuffled")
    s = gpu.parse(img)
    _setenv(monkeypatch, {})
    with gpu.Decoder(0) as d:
        d.load(s, 100, 100)
        for _ in range(3):
            assert d.offsets_state() == NONE
            d.decode()
            rep = d.report()
            assert rep.status == 0 and rep.symbols == 0
    _setenv(monkeypatch, {"GH_MODE": "wsplit"})
    with gpu.Decoder(0) as d:
        d.load(s)
        rep = _three_decodes(gpu, d, data, s.n, "wsplit", ready=False)
        assert gpu.MODE_NAMES[rep.mode] == "split"


# ---- out_cap below the output -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in ("g3_ow7", "g4_ow11") for st in SETTINGS])
def test_output_capacity(gpu, orc, monkeypatch, row, setting):
    """Capacities inside a piece, at a piece boundary, and the smallest ones (1; 0 selects
    the default capacity, the whole output): the exact prefix on every decode, the guard
    bytes after the buffer untouched."""
    ref, img, kept = tail._case(gpu, orc, row)
    _, u, _, name, _ = tail.ROWS[row]
    _setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    piece = np.add.reduceat(kept, np.arange(0, kept.size, 64 * u))
    goff = np.cumsum(piece) - piece
    caps = [int(goff[21]) + 5, int(goff[21]), int(goff[37]), int(goff[16]) - 1, s.n - 3, 1, 0]
    with gpu.Decoder(0) as d:
        for cap in caps:
            d.load(s, 0, s.g, out_cap=cap)
            keep = cap or s.n
            rep = _three_decodes(gpu, d, ref, keep, f"{name} cap {cap} {setting}")
            assert rep.out_bytes == keep and rep.symbols >= s.n


# ---- every piece through the direct-store path --------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", shapes.TILE_ROWS)
def test_direct_store_path(gpu, orc, monkeypatch, row):
    code, name = shapes.TILE_ROWS[row]
    data, img, _ = shapes._case(gpu, orc, code, shapes.N_TILE, "shuffled")
    _setenv(monkeypatch, {"GH_TILE_GRID": "3", "GH_TILE_SCAP": "4"})
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s)
        _three_decodes(gpu, d, data, s.n, f"{name} scap4")
        d.load(s, 0, s.g, out_cap=s.n // 3 + 7)
        _three_decodes(gpu, d, data, s.n // 3 + 7, f"{name} scap4 cap")


# ---- reload -------------------------------------------------------------------------
def _device_words(gpu, s):
    """The stream's payload and gap words in device memory (for gh_ctx_load_device)."""
    base = s.raw.ctypes.data
    po, go = int(s.c.payload) - base, int(s.c.gap_words) - base
    pay = np.frombuffer(s.raw[po: po + 4 * s.w].tobytes(), "<u4")
    gaps = np.frombuffer(s.raw[go: go + 4 * ((s.g + 7) // 8)].tobytes(), "<u4")
    return gpu.DeviceBuffer(pay.nbytes).upload(pay), gpu.DeviceBuffer(gaps.nbytes).upload(gaps)


@pytest.mark.gpu
@pytest.mark.parametrize("device_load", [False, True])
def test_reload_drops_the_offsets(gpu, orc, monkeypatch, device_load):
    """Shard A decoded until READY, then a different shard B in the same context: NONE, and
    B decodes correctly three times (a stale table of A would fail its guard)."""
    code_a, _ = shapes.TILE_ROWS["g3_ow7"]
    code_b, name_b = shapes.TILE_ROWS["g4_ow7_67"]  # another code of the same kernel family
    da, ia, _ = shapes._case(gpu, orc, code_a, shapes.N_TILE, "shuffled")
    db, ib, _ = shapes._case(gpu, orc, code_b, shapes.N_TILE, "sorted")
    _setenv(monkeypatch, {})
    sa, sb = gpu.parse(ia), gpu.parse(ib)
    bufs = _device_words(gpu, sb) if device_load else ()
    try:
        with gpu.Decoder(0) as d:
            d.load(sa)
            d.decode()
            assert d.report().status == 0 and d.offsets_state() == READY
            d.decode()
            assert np.array_equal(d.download(sa.n), da) and d.offsets_state() == READY
            for b, e in ((0, sb.g), (3, sb.g - 5)):
                if device_load:
                    d.load_device(sb, bufs[0].addr + 16 * b, sb.w - 4 * b, bufs[1].addr, b, e)
                else:
                    d.load(sb, b, e)
                assert d.offsets_state() == NONE and d.kernel_shape() == name_b
                kept, _, _ = tail._kept(code_b, db)
                off, n = int(kept[:b].sum()), int(kept[b:e].sum())
                _three_decodes(gpu, d, db[off:], n, f"reload [{b}, {e})")
            d.load(sa, 0, sa.g)  # and back to A
            assert d.offsets_state() == NONE
            _three_decodes(gpu, d, da, sa.n, "reload A")
    finally:
        for x in bufs:
            x.close()


# ---- streams and timing -------------------------------------------------------------
@pytest.mark.gpu
def test_streams_and_timing_mixed(gpu, orc, monkeypatch):
    """Chained and known-offsets decodes on the context's stream and on a caller's stream,
    timed and untimed, in turn; the timed ones are all reported."""
    import torch
    code, name = shapes.TILE_ROWS["g3_ow7"]
    data, img, _ = shapes._case(gpu, orc, code, shapes.N_TILE, "shuffled")
    _setenv(monkeypatch, {})
    s = gpu.parse(img)
    cs = torch.cuda.Stream()
    plan = [(0, True), (cs.cuda_stream, False), (cs.cuda_stream, True), (0, False), (cs.cuda_stream, True), (0, True)]
    for first in range(len(plan)):  # every kind of decode is once the recording one
        order = plan[first:] + plan[:first]
        with gpu.Decoder(0) as d:
            d.load(s)
            span = s.n + GUARD
            timed = 0
            for i, (st, tm) in enumerate(order):
                _fill(gpu, d, span)
                assert d.offsets_state() == (NONE if i == 0 else READY)
                d.decode(st, timed=tm)
                timed += tm
                _check_bytes(f"order {first}, decode {i}", _read_after(gpu, d, span), data, s.n)
            rep = d.report(cs.cuda_stream)
            assert rep.status == 0 and rep.launches == timed and rep.kernel_ms > 0
            # back to back, no wait between them: two on each stream
            _fill(gpu, d, span)
            for st, tm in order[:4]:
                d.decode(st, timed=tm)
            _check_bytes(f"order {first}, back to back", _read_after(gpu, d, span), data, s.n)
            assert d.report().status == 0 and d.offsets_state() == READY


# ---- GH_TILE_OFFS=0 -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", ["g3_ow7", "g3_ow11"])
def test_offsets_switched_off(gpu, orc, monkeypatch, row):
    code, name = shapes.TILE_ROWS[row]
    data, img, _ = shapes._case(gpu, orc, code, shapes.N_TILE, "shuffled")
    s = gpu.parse(img)
    outs = []
    for off in ("0", None):
        _setenv(monkeypatch, {"GH_TILE_OFFS": "0"} if off else {})
        with gpu.Decoder(0) as d:
            d.load(s)
            assert d.kernel_shape() == name
            _three_decodes(gpu, d, data, s.n, f"{name} offs {off}", ready=off is None)
            outs.append(d.download(s.n))
    assert np.array_equal(outs[0], outs[1])
