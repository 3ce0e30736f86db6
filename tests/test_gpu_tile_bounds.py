"""The tile kernel's never-borrow prefix, on streams whose segments end as early as a
valid stream allows.

decode_tile_rolling (csrc/gh_tile.hip) skips the borrow test of the first NB = 112 / LMAX
codewords of every segment and starts its liveness test at the group that holds codeword
NB, where LMAX = 12, 10, 8 is the longest codeword a code decoded with G = 2, 3, 4
codewords per window shift can have.  A segment that kept fewer than NB + 1 codewords
would be decoded wrongly, so the streams here hold runs of LMAX-bit codewords: a segment
that starts at bit 8 and holds 12-bit (10-bit) codewords keeps ten (twelve), which is
NB + 1 exactly.  Every test first counts the codewords each segment keeps on the CPU, from
the code lengths alone, and asserts that minimum before anything is decoded, so a wrong NB
cannot pass unnoticed.  Each stream is a little over four tiles with a ragged tail.  The
same decodes cover the symbol placement's cut-short dwords: a wave leaves the decode after
the group in which its last segment ends, so its last output dword holds one to four
symbols depending on the data."""
import numpy as np
import pytest

import test_gpu_shapes as shapes

# id: (code {length: symbols}, U segments per lane, G, expected kernel); the longest
# codeword is LMAX(G) in every row
ROWS = {
    "g2_ow7": ({5: 4, 8: 220, 9: 4, 10: 4, 12: 16}, 3, 2, "tile<1024,3,2,7,5>"),
    "g2_ow8": ({4: 2, 8: 222, 12: 32}, 3, 2, "tile<1024,3,2,8,4>"),
    "g2_ow11": ({3: 4, 8: 120, 12: 128}, 2, 2, "tile<1024,2,2,11,3>"),
    "g3_ow7": ({5: 4, 8: 220, 10: 16}, 3, 3, "tile<1024,3,3,7,5>"),
    "g3_ow8": ({4: 2, 8: 220, 10: 16}, 3, 3, "tile<1024,3,3,8,4>"),
    "g3_ow11": ({3: 7, 8: 28, 10: 16}, 2, 3, "tile<1024,2,3,11,3>"),
    "g4_ow7": ({5: 4, 8: 224}, 3, 4, "tile<1024,3,4,7,5>"),
    "g4_ow8": ({4: 2, 8: 224}, 3, 4, "tile<1024,3,4,8,4>"),
    "g4_ow11": ({3: 4, 8: 128}, 2, 4, "tile<1024,2,4,11,3>"),
}
LMAX = {2: 12, 3: 10, 4: 8}
NB = {g: 112 // l for g, l in LMAX.items()}  # 9, 11, 14
RUN = 130    # codewords per run of the longest length: more than two periods of the start offsets
NRUNS = 5
TILES = 4.3  # stream length in tiles
SETTINGS = {"default": {}, "grid3": {"GH_TILE_GRID": "3"}}


def _stream(code, u, seed):
    """Bytes whose histogram forces `code` (dyadic counts, as in test_gpu_shapes), shuffled,
    with NRUNS runs of RUN longest-codeword symbols spread over the stream."""
    vals, lens = shapes._symbols(code)
    hi = int(lens.max())
    avg = float(sum(c * l * 2.0 ** -l for l, c in code.items()))  # bits per symbol
    m = int(TILES * u * 1024 * 128 / avg) >> hi
    cnt = m * (1 << (hi - lens))
    rng = np.random.default_rng(seed)
    long_ = rng.permutation(np.repeat(vals[lens == hi], cnt[lens == hi]))
    assert long_.size >= NRUNS * RUN
    rest = rng.permutation(np.concatenate([long_[NRUNS * RUN:], np.repeat(vals[lens != hi], cnt[lens != hi])]))
    parts = np.array_split(rest, NRUNS + 1)
    out = [parts[0]]
    for i in range(NRUNS):
        out += [long_[i * RUN:(i + 1) * RUN], parts[i + 1]]
    return np.concatenate(out)


def _kept(code, data):
    """Per 128-bit segment: the codewords that start in it (those the decoder keeps) and
    the bit at which its first one starts, from the code lengths alone."""
    vals, lens = shapes._symbols(code)
    len_of = np.zeros(256, np.int64)
    len_of[vals] = lens
    l = len_of[data]
    assert l.min() > 0
    begin = np.cumsum(l) - l
    seg = begin >> 7
    kept = np.bincount(seg)
    first = np.concatenate([[0], np.cumsum(kept)[:-1]])  # index of each segment's first codeword
    assert kept.min() > 0
    return kept, (begin[first] & 127)


_cache = {}


def _case(gh, row):
    """(data, image, kept counts, start bits) of a row, encoded once; the preconditions
    are asserted here, before any decode."""
    if row not in _cache:
        code, u, g, _ = ROWS[row]
        assert max(code) == LMAX[g] and 32 // max(code) == g
        data = _stream(code, u, seed=1000 * g + u + min(code))
        img = gh.encode(data)
        shapes._assert_code(gh, img, code)
        s = gh.parse(img)
        kept, start = _kept(code, data)
        # the CPU model is the file's: as many segments, the same start offsets
        assert kept.size == s.g
        assert np.array_equal(start[1:], shapes._gap_values(gh, img))
        tile = u * 1024
        assert 4 * tile < s.g < 5 * tile and s.g % (64 * u) != 0  # four tiles and a ragged tail
        # runs of the longest codeword, at least 64 long
        lens_hi = np.isin(data, shapes._symbols(code)[0][shapes._symbols(code)[1] == max(code)])
        edges = np.flatnonzero(np.diff(np.concatenate([[0], lens_hi.view(np.int8), [0]])))
        assert (edges[1::2] - edges[::2]).max() >= 64
        # the last segment is cut short by the stream's end, not by its codewords
        lo = int(kept[:-1].min())
        assert lo >= NB[g] + 1, f"a segment keeps {lo} codewords: the never-borrow prefix of {NB[g]} is too long"
        if g < 4:
            assert lo == NB[g] + 1, "the stream does not hold the tight case"
            tight = np.flatnonzero(kept[:-1] == lo)
            assert (start[tight] >= 8).all()
        data.setflags(write=False)
        _cache[row] = (data, img, kept, start)
    return _cache[row]


@pytest.mark.parametrize("row", ROWS)
def test_streams_end_segments_as_early_as_possible(gh, row):
    """No GPU: the preconditions of every row (the decodes below assert them again)."""
    _case(gh, row)


def _decode(gpu, s, b, e, name):
    with gpu.Decoder(0) as d:
        d.load(s, b, e)
        shape = d.kernel_shape()
        d.decode()
        rep = d.report()
        out = d.download(min(int(rep.out_bytes), s.n))
    assert shape == name
    assert rep.status == 0
    assert gpu.MODE_NAMES[rep.mode] == "tile"
    return rep, out


@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in ROWS for st in SETTINGS])
def test_tile_bounds(gpu, monkeypatch, row, setting):
    data, img, kept, _ = _case(gpu, row)
    shapes._setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    rep, out = _decode(gpu, s, 0, s.g, ROWS[row][3])
    if setting == "grid3":
        assert rep.grid == 3
    assert rep.tiles == 5
    assert kept.sum() == s.n <= rep.symbols < s.n + 43  # (the last segment's padding decodes to symbols too)
    assert out.size == s.n
    if not np.array_equal(out, data):
        bad = np.flatnonzero(out != data)
        raise AssertionError(f"{bad.size} wrong bytes of {s.n}, first at {bad[0]}")


@pytest.mark.gpu
@pytest.mark.parametrize("row", ["g3_ow7", "g2_ow8"])
def test_tile_bounds_shard_from_mid_stream(gpu, monkeypatch, row):
    """A shard whose first segment is a tight one: it starts at bit >= 8 (first_start) and
    keeps NB + 1 codewords."""
    data, img, kept, start = _case(gpu, row)
    g = ROWS[row][2]
    tight = np.flatnonzero((kept[:-1] == NB[g] + 1) & (start[:-1] >= 8))
    b = int(tight[tight > kept.size // 8][0])
    assert start[b] >= 8
    shapes._setenv(monkeypatch, {})
    s = gpu.parse(img)
    rep, out = _decode(gpu, s, b, s.g, ROWS[row][3])
    off = int(kept[:b].sum())
    assert s.n - off <= rep.symbols < s.n - off + 43
    assert out.size >= s.n - off
    assert np.array_equal(out[:s.n - off], data[off:])
