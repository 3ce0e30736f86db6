"""Every compiled decode kernel shape, decoded once per ordering and setting.

The host picks one template instantiation per stream (tile_kernel_for, mtile_kernel_for,
ws_kernels in csrc/gh_decode.hip) from the code's shortest and longest codeword, the
table widths and the staging size.  gh_generate's codes reach only a few of them, so the
streams here carry a *prescribed* code: for a complete length list, symbol i occurs
m * 2^(maxlen - len_i) times; dyadic counts leave package-merge no choice, and every test
asserts the lengths it got.  Each decode is compared with the CPU oracle's bit-serial
decode of the same file and with the input, and asserts the name of the instantiation
that ran (gh_ctx_kernel_shape), so a row cannot silently drift to another kernel.

test_tables_cover_every_shape needs no GPU: the names expected by the tables below must
be exactly the names the pickers can return (gh_kernel_shapes)."""
import math

import numpy as np
import pytest

N_TILE = 1 << 20   # a multiple of 2^maxlen for every code; 17..32 tiles of the tile kernels
N_WS = 1 << 18     # wave split: about 200 K symbols

# ---- codes: {length: symbols}, complete ---------------------------------------------
# single-pass tile kernel (grouped codes: 4 <= len <= 12; minlen-3 codes)
TILE_ROWS = {
    # id: (code, expected kernel)
    "g4_ow8": ({4: 2, 8: 224}, "tile<1024,3,4,8,4>"),
    "g3_ow8": ({4: 2, 8: 222, 9: 4}, "tile<1024,3,3,8,4>"),
    "g2_ow8": ({4: 2, 8: 222, 12: 32}, "tile<1024,3,2,8,4>"),
    "g4_ow7_mixed": ({5: 4, 8: 224}, "tile<1024,3,4,7,5>"),
    "g4_ow7_67": ({6: 32, 7: 64}, "tile<1024,3,4,7,5>"),
    "g3_ow7": ({5: 4, 8: 196, 9: 56}, "tile<1024,3,3,7,5>"),
    "g2_ow7": ({5: 4, 8: 220, 9: 4, 10: 4, 12: 16}, "tile<1024,3,2,7,5>"),
    "g4_ow11": ({3: 4, 8: 128}, "tile<1024,2,4,11,3>"),
    "g3_ow11": ({3: 7, 8: 28, 10: 16}, "tile<1024,2,3,11,3>"),
    "g2_ow11": ({3: 4, 8: 120, 12: 128}, "tile<1024,2,2,11,3>"),
}
ORDERINGS = ("shuffled", "sorted", "striped")
TILE_SETTINGS = {
    "default": {},
    "grid3": {"GH_TILE_GRID": "3"},                             # many tiles and rounds per workgroup
    "grid3_scap4": {"GH_TILE_GRID": "3", "GH_TILE_SCAP": "4"},  # every tile through the direct-store path
}


def _ladder(lo, hi, first=1):
    """`first` codewords of lo bits, one of each length up to hi - 1, two (or as many as
    complete the code) of hi bits."""
    code = {lo: first}
    for l in range(lo + 1, hi):
        code[l] = 1
    left = 1.0 - sum(c * 2.0 ** -l for l, c in code.items())
    code[hi] = round(left * 2 ** hi)
    return code


def _fours(lo, hi):
    """Four codewords of every length lo .. hi - 1, eight of hi bits."""
    code = {l: 4 for l in range(lo, hi)}
    code[hi] = 8
    return code


# Two-pass tile kernel (GH_MODE=mtile): lookups per window shift GL from the table width
# (GH_WS_K: <= 7 -> 4, <= 10 -> 3, else 2; 11 at most with a 1-bit codeword), NS from the
# staged piece = max(128 * bytes per segment (GH_TILE_SCAP), 64 * ceil(128 / minlen)):
# <= 4 KB -> 4, <= 6 KB -> 6, <= 8 KB -> 8, more (a 1-bit codeword: 64 x 128) -> 5 x 2;
# fb: codewords longer than the table.
MTILE_ROWS = {
    # id: (code, environment, expected kernel)
    "gl4_ns4": (_fours(3, 7), {"GH_WS_K": "7", "GH_TILE_SCAP": "20"}, "mtile<1024,4,4,fb=0,np=1>"),
    "gl4_ns6": (_fours(3, 7), {"GH_WS_K": "7", "GH_TILE_SCAP": "40"}, "mtile<1024,4,6,fb=0,np=1>"),
    "gl4_ns8": (_ladder(2, 7, 3), {"GH_WS_K": "7"}, "mtile<1024,4,8,fb=0,np=1>"),
    "gl4_ns10": (_ladder(1, 6), {"GH_WS_K": "7"}, "mtile<1024,4,5,fb=0,np=2>"),
    "gl3_ns4": (_fours(3, 10), {"GH_WS_K": "10", "GH_TILE_SCAP": "20"}, "mtile<1024,3,4,fb=0,np=1>"),
    "gl3_ns6": (_fours(3, 10), {"GH_WS_K": "10", "GH_TILE_SCAP": "40"}, "mtile<1024,3,6,fb=0,np=1>"),
    "gl3_ns8": (_ladder(2, 10, 3), {"GH_WS_K": "10"}, "mtile<1024,3,8,fb=0,np=1>"),
    "gl3_ns10": (_ladder(1, 10), {"GH_WS_K": "10"}, "mtile<1024,3,5,fb=0,np=2>"),
    "gl2_ns4": (_fours(3, 12), {"GH_WS_K": "12", "GH_TILE_SCAP": "20"}, "mtile<1024,2,4,fb=0,np=1>"),
    "gl2_ns6": (_fours(3, 12), {"GH_WS_K": "12", "GH_TILE_SCAP": "40"}, "mtile<1024,2,6,fb=0,np=1>"),
    "gl2_ns8": (_ladder(2, 11, 3), {"GH_WS_K": "11"}, "mtile<1024,2,8,fb=0,np=1>"),
    "gl2_ns10": (_ladder(1, 11), {"GH_WS_K": "12"}, "mtile<1024,2,5,fb=0,np=2>"),
    "fb_ns4": (_fours(3, 16), {"GH_WS_K": "12", "GH_TILE_SCAP": "20"}, "mtile<1024,2,4,fb=1,np=1>"),
    "fb_ns6": (_fours(3, 16), {"GH_WS_K": "12", "GH_TILE_SCAP": "40"}, "mtile<1024,2,6,fb=1,np=1>"),
    # (12-bit tables leave 8 KB regions only beside a 12-bit count table)
    "fb_ns8": (_ladder(2, 16, 3), {"GH_WS_K": "12", "GH_MT_KC": "12"}, "mtile<1024,2,8,fb=1,np=1>"),
    "fb_ns10": (_ladder(1, 16), {"GH_WS_K": "12"}, "mtile<1024,2,5,fb=1,np=2>"),
}
MTILE_RUNS = (("shuffled", False), ("sorted", False), ("shuffled", True))  # (ordering, GH_TILE_GRID=3)

# Wave split (GH_MODE=wsplit): count kernel by GH_WS_KC, write kernel by GH_WS_K and
# GH_WS_NS (lookups per shift as above); fb: an incomplete code (here the one-symbol code;
# multi-symbol ones are in tests/test_gpu_foreign_codes.py) or codewords longer than the tables.
ONE_SYMBOL = {1: 1}


def _ws(gc, g, ns, fb=0):
    return f"ws_count<4,256,{gc},fb={fb}>+ws_write<2,512,{g},{ns},fb={fb}>"


WS_ROWS = {
    # id: (code, GH_WS_KC, GH_WS_K, GH_WS_NS, expected kernels)
    "c4_w4_ns2": (_ladder(2, 7, 3), 7, 7, 2, _ws(4, 4, 2)),
    "c4_w4_ns3": (_fours(3, 7), 7, 7, 3, _ws(4, 4, 3)),
    "c2_w4_ns4": (_ladder(1, 6), 13, 7, 4, _ws(2, 4, 4)),
    "c3_w4_ns6": (_ladder(2, 7, 3), 10, 7, 6, _ws(3, 4, 6)),
    "c4_w4_ns8": (_ladder(1, 6), 6, 6, 8, _ws(4, 4, 8)),
    "c3_w3_ns2": (_fours(3, 10), 10, 10, 2, _ws(3, 3, 2)),
    "c3_w3_ns3": (_ladder(2, 10, 3), 10, 10, 3, _ws(3, 3, 3)),
    "c2_w3_ns4": (_ladder(1, 10), 12, 10, 4, _ws(2, 3, 4)),
    "c3_w3_ns6": (_ladder(2, 8, 3), 8, 8, 6, _ws(3, 3, 6)),
    "c4_w3_ns8": (_ladder(1, 6), 7, 9, 8, _ws(4, 3, 8)),
    "c2_w2_ns2": (_fours(3, 12), 12, 12, 2, _ws(2, 2, 2)),
    "c2_w2_ns3": (_ladder(2, 11, 3), 11, 11, 3, _ws(2, 2, 3)),
    "c2_w2_ns4": ({3: 4, 8: 120, 12: 128}, 13, 12, 4, _ws(2, 2, 4)),
    "c3_w2_ns6": (_ladder(2, 10, 3), 10, 12, 6, _ws(3, 2, 6)),
    "c2_w2_ns8": (_ladder(1, 11), 14, 11, 8, _ws(2, 2, 8)),
    "fb_one_ns2": (ONE_SYMBOL, 2, 2, 2, _ws(2, 2, 2, 1)),
    "fb_16_ns3": (_ladder(2, 16, 3), 13, 12, 3, _ws(2, 2, 3, 1)),
    "fb_one_ns4": (ONE_SYMBOL, 13, 12, 4, _ws(2, 2, 4, 1)),
    "fb_16_ns6": (_fours(3, 16), 14, 12, 6, _ws(2, 2, 6, 1)),
    "fb_16_ns8": (_ladder(1, 16), 13, 10, 8, _ws(2, 2, 8, 1)),
}

ENV_KNOBS = ("GH_MODE", "GH_TILE_GRID", "GH_TILE_SCAP", "GH_TILE_SCAPF", "GH_WS_K", "GH_WS_KC", "GH_WS_NS",
             "GH_WS_GRID", "GH_WS_STAGE", "GH_WS_LGC", "GH_MT_KC", "GH_MT_CLGR", "GH_LUT_BITS", "GH_LGR",
             "GH_TILE_IDLE", "GH_ENC_GRID", "GH_ENC_INDEX_GRID")


# ---- streams ------------------------------------------------------------------------
def _symbols(code):
    """(byte value, length) per symbol, shortest first; the byte values are spread over
    0..255 so neighbouring codewords do not carry neighbouring bytes."""
    lens = [l for l in sorted(code) for _ in range(code[l])]
    assert len(lens) <= 256
    if len(lens) > 1:
        assert sum(2.0 ** -l for l in lens) == 1.0, "the length list is not a complete code"
    vals = (np.arange(len(lens)) * 37 + 11) % 256
    return vals.astype(np.uint8), np.asarray(lens)


def _pools(code, n, rng):
    vals, lens = _symbols(code)
    if len(lens) == 1:
        return vals, lens, np.array([n])
    maxlen = int(lens.max())
    m, rem = divmod(n, 1 << maxlen)
    assert m >= 1 and rem == 0
    return vals, lens, m * (1 << (maxlen - lens))


def _stream(code, n, ordering, seed):
    """n bytes whose histogram forces `code`, in one of the three orderings."""
    rng = np.random.default_rng(seed)
    vals, lens, cnt = _pools(code, n, rng)
    if ordering == "sorted":  # falling frequency: runs of segments full of the shortest codewords
        return np.repeat(vals, cnt)
    if ordering == "shuffled":
        return rng.permutation(np.repeat(vals, cnt))
    assert ordering == "striped"
    # j shortest-codeword symbols then k longest-codeword symbols, j = 1..ceil(128 / minlen) + 1,
    # k = 1..12, cycling until either pool is empty; the rest shuffled
    lo, hi = int(lens.min()), int(lens.max())
    assert lo < hi
    short = rng.permutation(np.repeat(vals[lens == lo], cnt[lens == lo]))
    long_ = rng.permutation(np.repeat(vals[lens == hi], cnt[lens == hi]))
    J = -(-128 // lo) + 1
    js, ks = np.repeat(np.arange(1, J + 1), 12), np.tile(np.arange(1, 13), J)
    reps = min(short.size // js.sum(), long_.size // ks.sum()) + 1
    js, ks = np.tile(js, reps), np.tile(ks, reps)
    npairs = int(np.count_nonzero((np.cumsum(js) <= short.size) & (np.cumsum(ks) <= long_.size)))
    assert npairs >= J * 12, "the stripes do not reach every (j, k)"
    js, ks = js[:npairs], ks[:npairs]
    runs = np.stack([js, ks], axis=1).ravel()
    is_long = np.repeat(np.tile([False, True], npairs), runs)
    ns, nl = int(js.sum()), int(ks.sum())
    head = np.empty(ns + nl, np.uint8)
    head[~is_long] = short[:ns]
    head[is_long] = long_[:nl]
    mid = (lens != lo) & (lens != hi)
    rest = np.concatenate([short[ns:], long_[nl:], np.repeat(vals[mid], cnt[mid])])
    return np.concatenate([head, rng.permutation(rest)])


_cache = {}


def _case(gh, orc, code, n, ordering):
    """(data, file image, oracle total): encoded and oracle-decoded once per stream; the
    file's code is the prescribed one and the oracle returns the input."""
    key = (tuple(sorted(code.items())), n, ordering)
    if key not in _cache:
        if len(_cache) >= 8:
            _cache.pop(next(iter(_cache)))
        data = _stream(code, n, ordering, seed=len(code) * 1000 + n % 997 + ORDERINGS.index(ordering))
        img = gh.encode(data)
        _assert_code(gh, img, code)
        ref, total = orc.decode(img)
        assert np.array_equal(ref, data), "the oracle does not return the input"
        data.setflags(write=False)
        _cache[key] = (data, img, total)
    return _cache[key]


def _assert_code(gh, img, code):
    vals, lens = _symbols(code)
    want = dict(zip(vals.tolist(), lens.tolist()))
    got = dict(gh.parse(img).symbols)
    assert got == want, "package-merge did not return the prescribed lengths"


def _gap_values(gh, img):
    """The 4-bit start offsets of segments 1 .. G - 1 (the file's gap nibbles)."""
    s = gh.parse(img)
    off = int(s.c.gap_words) - s.raw.ctypes.data
    words = np.frombuffer(s.raw[off: off + 4 * ((s.g + 7) // 8)].tobytes(), "<u4")
    nib = (words[:, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15
    return nib.ravel()[: s.g - 1]


def _setenv(monkeypatch, env):
    for k in ENV_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _decode_and_check(gpu, data, img, total, name, cap=0):
    s = gpu.parse(img)
    with gpu.Decoder(0) as d:
        d.load(s, 0, s.g, out_cap=cap)
        shape = d.kernel_shape()
        d.decode()
        rep = d.report()
        keep = cap or s.n
        out = d.download(keep)
    assert shape == name
    assert rep.status == 0
    assert rep.symbols == total  # the count pass, the last segment's padding included
    assert rep.out_bytes == keep
    if not np.array_equal(out, data[:keep]):
        bad = np.nonzero(out != data[:keep])[0]
        raise AssertionError(f"{shape}: {bad.size} wrong bytes of {keep}, first at {bad[0]}")
    return rep


# ---- no GPU -------------------------------------------------------------------------
def test_tables_cover_every_shape(gh):
    """The kernels named by the tables above are exactly those the pickers can return:
    a new instantiation needs a row here, a removed one loses its row."""
    want = {name for _, name in TILE_ROWS.values()}
    want |= {name for _, _, name in MTILE_ROWS.values()}
    for row in WS_ROWS.values():
        want |= set(row[4].split("+"))
    have = gh.kernel_shapes()
    assert len(have) == len(set(have))
    assert want == set(have)
    kinds = [sum(n.startswith(p) for n in have) for p in ("tile<", "mtile<", "ws_count<", "ws_write<")]
    assert kinds == [9, 16, 4, 20]


def test_shape_queries_check_their_buffers(gh):
    import ctypes
    small = ctypes.create_string_buffer(8)
    assert gh.lib().gh_kernel_shapes(small, len(small)) == -9  # GH_E_SMALL
    assert gh.lib().gh_kernel_shapes(None, 0) == -1            # GH_E_ARG
    assert gh.lib().gh_ctx_kernel_shape(None, small, len(small)) == -1


@pytest.mark.parametrize("row", TILE_ROWS)
def test_tile_streams_meet_their_preconditions(gh, row):
    """The shuffled stream of every tile row carries the prescribed code and starts
    segments at every offset the code allows: gap values 0 .. maxlen - 1 (codewords start
    at multiples of the lengths' common divisor only: 4/8- and 4/8/12-bit codes start
    every segment at a multiple of 4)."""
    code, _ = TILE_ROWS[row]
    data = _stream(code, N_TILE, "shuffled", seed=len(code) * 1000 + N_TILE % 997)
    img = gh.encode(data)
    _assert_code(gh, img, code)
    step = math.gcd(*code)
    want = set(range(0, max(code), step))
    assert set(np.unique(_gap_values(gh, img)).tolist()) == want


# ---- single-pass tile kernel --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row,ordering,setting",
                         [(r, o, s) for r in TILE_ROWS for o in ORDERINGS for s in TILE_SETTINGS])
def test_tile_shape(gpu, orc, monkeypatch, row, ordering, setting):
    code, name = TILE_ROWS[row]
    data, img, total = _case(gpu, orc, code, N_TILE, ordering)
    _setenv(monkeypatch, TILE_SETTINGS[setting])
    rep = _decode_and_check(gpu, data, img, total, name)
    assert gpu.MODE_NAMES[rep.mode] == "tile"
    if "GH_TILE_GRID" in TILE_SETTINGS[setting]:
        assert rep.grid == 3 and rep.tiles >= 3 * (rep.grid - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("row", TILE_ROWS)
def test_tile_shape_output_capacity(gpu, orc, monkeypatch, row):
    """An output capacity a few bytes below the total, and one inside a tile of the
    second round of a three-workgroup grid: the exact prefix, nothing past it."""
    code, name = TILE_ROWS[row]
    data, img, total = _case(gpu, orc, code, N_TILE, "shuffled")
    _setenv(monkeypatch, {})
    _decode_and_check(gpu, data, img, total, name, cap=N_TILE - 5)
    _setenv(monkeypatch, {"GH_TILE_GRID": "3"})
    _decode_and_check(gpu, data, img, total, name, cap=N_TILE // 8 + 12345)


# ---- two-pass tile kernel -----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row,ordering,grid3", [(r, o, g) for r in MTILE_ROWS for o, g in MTILE_RUNS])
def test_mtile_shape(gpu, orc, monkeypatch, row, ordering, grid3):
    code, env, name = MTILE_ROWS[row]
    data, img, total = _case(gpu, orc, code, N_TILE, ordering)
    _setenv(monkeypatch, {"GH_MODE": "mtile", **env, **({"GH_TILE_GRID": "3"} if grid3 else {})})
    rep = _decode_and_check(gpu, data, img, total, name)
    assert gpu.MODE_NAMES[rep.mode] == "mtile"
    if grid3:
        assert rep.grid == 3 and rep.tiles >= 3 * (rep.grid - 1)


# ---- wave split ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("row", WS_ROWS)
def test_wsplit_shape(gpu, orc, monkeypatch, row):
    code, kc, k, ns, name = WS_ROWS[row]
    data, img, total = _case(gpu, orc, code, N_WS, "shuffled")
    _setenv(monkeypatch, {"GH_MODE": "wsplit", "GH_WS_KC": kc, "GH_WS_K": k, "GH_WS_NS": ns})
    rep = _decode_and_check(gpu, data, img, total, name)
    assert gpu.MODE_NAMES[rep.mode] == "split"
