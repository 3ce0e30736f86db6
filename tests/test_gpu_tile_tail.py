"""The tile kernel's decode exit and its lane-major loads, on streams whose every segment
keeps a planned number of codewords.

decode_tile_rolling (csrc/gh_tile.hip) leaves the decode at the end of the window-shift
group in which the wave's last live segment ends; the dword that group ends in is completed
from the one to three symbols it has, and the staging rounds are bounded by the groups run.
The lane-major load takes the last chain's look-ahead word from the next lane's registers
(lane 63: one load of the word after the wave's segments) and a lane's U gap nibbles from
one 8-byte load.

So the streams here fix how many codewords every single segment keeps.  A stream is three
tiles and five segments.  Every segment of a tile keeps exactly c codewords (c differs by
tile), except one planted segment in most waves, which keeps c + 1, c + 2 or c + 3 and sits
in chain 0 of a lane, in chain U - 1 of a lane, or in lane 63: that segment alone decides
where the wave leaves, its last codeword falls at every residue of the position mod 4 and
mod G, and the other chains are dead for up to three codewords before it.  The kernel has
no exit inside a group and no per-chain tail today (DESIGN.md says why); these streams are
what such an exit has to decode.  The segments' compositions are drawn so that their start
offsets (the gap nibbles) vary from segment to segment and nearly every segment's last
codeword runs into the next segment, the look-ahead word of lane 63 at wave and tile
boundaries included.

A histogram with dyadic counts (tests/test_gpu_tile_bounds.py) cannot do that: a complete
code gives its shortest codeword at least 2^-minlen of all symbols, which then cannot be
kept out of all but a few segments.  The images are therefore assembled from the prescribed
complete table and the drawn data by the oracle's raw-stream restatement, as in
tests/foreign_codes.py.  The kept counts are computed on the CPU from the code lengths
alone and asserted before anything is decoded; every decode is compared byte for byte with
oracle.decode of the same file and names the kernel that ran."""
import numpy as np
import pytest

import foreign_codes as fc
import test_gpu_shapes as shapes

# id: (code {length: symbols}, U, G, expected kernel, c per tile)
ROWS = {
    "g3_ow7": ({5: 4, 8: 196, 9: 56}, 3, 3, "tile<1024,3,3,7,5>", (16, 15, 18)),
    "g2_ow8": ({4: 2, 7: 110, 12: 64}, 3, 2, "tile<1024,3,2,8,4>", (16, 13, 20)),
    "g4_ow11": ({3: 4, 7: 32, 8: 64}, 2, 4, "tile<1024,2,4,11,3>", (17, 19, 22)),
}
NB = {2: 9, 3: 11, 4: 14}  # codewords of a segment that cannot reach its end (112 // LMAX)
TAIL = 5                   # segments of the fourth tile
SETTINGS = {
    "default": {},
    "grid3": {"GH_TILE_GRID": "3"},                             # two decoding workgroups, two rounds
    "grid3_scap4": {"GH_TILE_GRID": "3", "GH_TILE_SCAP": "4"},  # every tile through the direct-store path
}


def _plant(u, wave):
    """(segment of the wave, extra codewords) planted in global wave `wave`: the twelve
    combinations of 0..3 extra codewords and chain 0 / chain U - 1 / lane 63 in turn."""
    extra, where = wave % 4, (wave // 4) % 3
    lane = (5 * wave + 3) % 63
    if where == 0:
        return lane * u, extra
    if where == 1:
        return lane * u + u - 1, extra
    return 63 * u + wave % u, extra


def _targets(u, cs):
    """Codewords kept by each of the 3 * 1024 U + TAIL segments."""
    tile = 1024 * u
    k = np.repeat(np.asarray(cs, np.int64), tile)
    for wave in range(3 * 16):
        seg, extra = _plant(u, wave)
        k[wave * 64 * u + seg] += extra
    tail = np.full(TAIL, cs[0], np.int64)
    tail[1] += 2
    return np.concatenate([k, tail])


def _compositions(lens, o, k, last):
    """Every (n_0, n_1, n_2) codewords of the three lengths, k in all, that a segment whose
    first codeword starts at bit o keeps in any order: the k-th starts before bit 128 and
    (unless the stream ends here) the next one does not."""
    out = []
    for a in range(k + 1):
        for b in range(k + 1 - a):
            n = (a, b, k - a - b)
            bits = sum(x * l for x, l in zip(n, lens))
            shortest = min(l for x, l in zip(n, lens) if x)  # the k-th codeword, at worst
            if o + bits - shortest < 128 and (last or o + bits >= 128):
                out.append(n)
    return out


def _stream(code, u, cs, seed):
    """(data, kept targets): the segments' lengths drawn from their feasible compositions,
    the symbols of each length drawn at random."""
    vals, slens = shapes._symbols(code)
    lens = sorted(code)
    assert len(lens) == 3
    rng = np.random.default_rng(seed)
    target = _targets(u, cs)
    memo, o, chunks = {}, 0, []
    for i, k in enumerate(target.tolist()):
        last = i == target.size - 1
        key = (o, k, last)
        if key not in memo:
            memo[key] = _compositions(lens, o, k, last)
            assert memo[key], f"no segment starting at bit {o} keeps {k} codewords of lengths {lens}"
        n = memo[key][rng.integers(len(memo[key]))]
        seg = rng.permutation(np.repeat(lens, n))
        chunks.append(seg)
        o = max(0, o + int(seg.sum()) - 128)
    l = np.concatenate(chunks)
    data = np.empty(l.size, np.uint8)
    for ln in lens:
        pool = vals[slens == ln]
        m = l == ln
        data[m] = pool[rng.integers(0, pool.size, int(m.sum()))]
    return data, target


def _kept(code, data):
    """Per 128-bit segment: the codewords that start in it, and the bit its first one starts
    at, from the code lengths alone."""
    vals, lens = shapes._symbols(code)
    len_of = np.zeros(256, np.int64)
    len_of[vals] = lens
    l = len_of[data]
    assert l.min() > 0
    begin = np.cumsum(l) - l
    kept = np.bincount(begin >> 7)
    first = np.concatenate([[0], np.cumsum(kept)[:-1]])
    return kept, begin[first] & 127, (begin + l - 1) >> 7 != begin >> 7


_cache = {}


def _case(gh, orc, row):
    """(data, image, kept counts) of a row, built once; the preconditions are asserted here."""
    if row not in _cache:
        code, u, g, _, cs = ROWS[row]
        assert min(4, 32 // max(code)) == g
        data, target = _stream(code, u, cs, seed=17 * g + u)
        vals, lens = shapes._symbols(code)
        syms = [(int(v), int(n)) for v, n in zip(vals, lens)]
        assert fc.kraft(syms) == 65536
        img = fc.image(orc, syms, data)
        s = gh.parse(img)
        tile = 1024 * u
        assert s.g == 3 * tile + TAIL and s.n == data.size
        kept, start, crosses = _kept(code, data)
        # the CPU model is the file's: as many segments, the same start offsets
        assert np.array_equal(start[1:], shapes._gap_values(gh, img))
        assert np.array_equal(kept, target), "a segment does not keep the codewords planned for it"
        assert kept.min() >= NB[g] + 1
        # every wave: all segments keep the tile's c but the planted one; every number of extra
        # codewords in every place, at every residue of the exit position mod 4 and mod G
        seen = set()
        for wave in range(48):
            seg, extra = _plant(u, wave)
            w = kept[wave * 64 * u:(wave + 1) * 64 * u]
            c = cs[wave // 16]
            assert w[seg] == c + extra and np.count_nonzero(w != c) == (1 if extra else 0)
            chain = "lane63" if seg >= 63 * u else seg % u
            seen.add((extra, chain))
        assert seen >= {(x, ch) for x in range(4) for ch in (0, u - 1, "lane63")}
        exits = {int(kept[w * 64 * u:(w + 1) * 64 * u].max()) - 1 for w in range(48)}
        assert {p & 3 for p in exits} == {0, 1, 2, 3} and {p % g for p in exits} == set(range(g))
        # start offsets vary (the gap nibbles of a lane's U segments differ) and codewords run
        # into the next segment at lane 63 of a wave and of a tile
        assert np.unique(start).size >= 4
        assert np.count_nonzero(np.diff(start) != 0) > kept.size // 2
        ends = np.arange(64 * u - 1, 3 * tile, 64 * u)
        last_cw = np.cumsum(kept) - 1
        assert crosses[last_cw[ends]].sum() >= 24
        assert crosses[last_cw[[tile - 1, 2 * tile - 1, 3 * tile - 1]]].any()
        ref, _ = orc.decode(img)
        assert np.array_equal(ref, data), "the oracle does not return the input"
        ref.setflags(write=False)
        _cache[row] = (ref, img, kept)
    return _cache[row]


def _shards(u, g):
    """(b, e): the whole stream; a last tile of one segment (chains 1 .. U - 1 of its wave
    wholly past the shard end); segment counts 0, 1, 7, 8 mod 8; first segments 1, 7, 8, 9
    (the gap nibbles then start inside a gap dword), ending at the stream's end (the
    look-ahead past it is padding) and inside it."""
    t = 1024 * u
    assert t % 8 == 0
    return [(0, g), (0, 3 * t + 1), (0, 3 * t), (0, 2 * t + 7), (0, 2 * t + 8), (0, 63),
            (1, g), (7, g), (8, g), (9, g),
            (1, 2 * t + 2), (7, t + 64 * u), (8, 3 * t + 3), (9, t + 16)]


@pytest.mark.parametrize("row", ROWS)
def test_streams_keep_the_planned_codewords(gh, orc, row):
    """No GPU: the preconditions of every row (the decodes below assert them again)."""
    _case(gh, orc, row)


@pytest.mark.gpu
@pytest.mark.parametrize("row,setting", [(r, st) for r in ROWS for st in SETTINGS])
def test_tile_tail(gpu, orc, monkeypatch, row, setting):
    ref, img, kept = _case(gpu, orc, row)
    _, u, _, name, _ = ROWS[row]
    shapes._setenv(monkeypatch, SETTINGS[setting])
    s = gpu.parse(img)
    bad = []
    for b, e in _shards(u, s.g):
        off, n = int(kept[:b].sum()), int(kept[b:e].sum())
        with gpu.Decoder(0) as d:
            d.load(s, b, e)
            shape = d.kernel_shape()
            d.decode()
            rep = d.report()
            out = d.download(min(int(rep.out_bytes), n))
        assert shape == name
        assert rep.status == 0
        assert gpu.MODE_NAMES[rep.mode] == "tile"
        if setting != "default":
            assert rep.grid == min(3, rep.tiles + 1)  # (a workgroup per tile and the leader, at most)
        assert rep.tiles == -(-(e - b) // (1024 * u))
        # (the stream's last segment: its padding decodes to symbols too)
        if not ((rep.symbols == n) if e < s.g else (n <= rep.symbols < n + 43)):
            bad.append(f"[{b}, {e}): {rep.symbols} symbols counted, {n} kept")
        if out.size != n or not np.array_equal(out, ref[off:off + n]):
            wrong = np.flatnonzero(out != ref[off:off + out.size])
            bad.append(f"[{b}, {e}): {out.size} of {n} bytes, {wrong.size} wrong, first at {wrong[:1]}")
    assert not bad, "; ".join(bad)
