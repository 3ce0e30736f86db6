"""The range-gather planner (gh_gather_plan / Index.plan) on the CPU.

Index images are made here, not by the library: offsets computed from data as in
tests/test_gpu_index.py (codewords that start before each block's first payload bit), and
one hand-built image with blocks that hold no symbol.  Every plan is compared with a pure
numpy reference that cuts each range at the entries it spans; the properties the kernel
relies on are asserted one by one as well."""
import ctypes

import numpy as np
import pytest

GH_E_ARG, GH_E_SMALL = -1, -9


def _image(offsets, g, log2_stride):
    off = np.asarray(offsets, dtype="<u8")
    hdr = np.zeros(5, dtype="<u8")
    hdr[0] = 0x0000315844494847
    hdr[1] = log2_stride
    hdr[2] = off[-1]
    hdr[3] = g
    hdr[4] = off.size
    return np.concatenate([hdr, off]).view(np.uint8)


def _from_data(gh, seed, r, n, log2_stride):
    data = gh.generate(seed, r, n)
    img = gh.encode(data)
    s = gh.parse(img)
    length_of = np.zeros(256, dtype=np.int64)
    for sym, l in s.symbols:
        length_of[sym] = l
    bits = length_of[data]
    starts = np.cumsum(bits) - bits
    nblocks = -(-s.g // (1 << log2_stride))
    off = np.searchsorted(starts, 128 * (1 << log2_stride) * np.arange(nblocks, dtype=np.int64), "left")
    return _image(np.append(off, s.n), s.g, log2_stride)


@pytest.fixture(scope="module")
def indexes(gh):
    """Parsed indexes: two from data (strides 2^8 and 2^10), one hand-built with empty
    blocks and a one-symbol block, at an odd address."""
    out = [gh.parse_index(_from_data(gh, 3, 0.5, 400_000, 8)), gh.parse_index(_from_data(gh, 4, 0.9, 400_000, 10))]
    hand = _image([0, 0, 5, 5, 5, 6, 4000, 4000, 9000], 8 * 256 - 3, 8)
    odd = np.zeros(hand.size + 1, dtype=np.uint8)
    odd[1:] = hand
    out.append(gh.parse_index(odd[1:]))
    assert out[0].offsets.size > 50 and out[1].offsets.size > 8
    return out


def _reference(off, ranges):
    """Pieces (dst, block, a, b) of the ranges, cut at the entries; the byte total."""
    off = [int(v) for v in off]
    pieces, dst = [], 0
    for lo, hi in ranges:
        for k in range(len(off) - 1):
            a, b = max(lo, off[k]), min(hi, off[k + 1])
            if a < b:
                pieces.append((dst, k, a - off[k], b - off[k]))
                dst += b - a
    return pieces, dst


def _as_tuples(p):
    assert not p["pad"].any()
    return list(zip(p["dst"].tolist(), p["block"].tolist(), p["a"].tolist(), p["b"].tolist()))


def _check(ix, ranges):
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    pieces, total = ix.plan(ranges)
    off = ix.offsets.astype(np.int64)
    want, want_total = _reference(off, ranges)
    assert total == want_total == sum(hi - lo for lo, hi in ranges)
    assert _as_tuples(pieces) == want
    # the properties, each on its own
    blk = pieces["block"].astype(np.int64)
    a, b = pieces["a"].astype(np.int64), pieces["b"].astype(np.int64)
    assert (a < b).all() and (b <= off[blk + 1] - off[blk]).all()
    assert np.array_equal(pieces["dst"].astype(np.int64), np.cumsum(b - a) - (b - a))  # the running sum
    at = 0
    for lo, hi in ranges:  # the pieces of one range tile [lo, hi) exactly and in order
        cur = lo
        while cur < hi:
            assert off[blk[at]] + a[at] == cur
            cur = off[blk[at]] + b[at]
            at += 1
        assert cur == hi
    assert at == pieces.size
    return pieces, total


def _edge_ranges(ix):
    n = ix.n
    off = ix.offsets.astype(np.int64)
    out = [(0, 0), (n, n), (n // 2, n // 2), (0, n), (n - 1, n), (0, 1)]
    for e in off.tolist():
        for v in (e - 1, e, e + 1):  # lo and hi on an entry and one byte either side
            if 0 <= v <= n:
                out += [(v, min(v + 1, n)), (max(v - 1, 0), v), (v, min(v + 5000, n)), (max(v - 5000, 0), v)]
    k = len(off) // 2
    out.append((int(off[k]), int(off[k + 1])))  # exactly one block
    return out


def test_random_batches(gh, indexes):
    rng = np.random.default_rng(1)
    for ix in indexes:
        for _ in range(20):
            lo = rng.integers(0, ix.n + 1, size=40)
            ln = rng.integers(0, 5001, size=40)
            ln[rng.integers(0, 40, size=4)] = 0
            _check(ix, list(zip(lo, np.minimum(lo + ln, ix.n))))


def test_edges_on_and_beside_entries(gh, indexes):
    for ix in indexes:
        rs = _edge_ranges(ix)
        _check(ix, rs)
        for r in rs[:6]:
            pieces, total = _check(ix, [r])
            assert total == r[1] - r[0] and (pieces.size == 0) == (r[0] == r[1])


def test_repeated_overlapping_unsorted(gh, indexes):
    for ix in indexes:
        n = ix.n
        rs = [(n // 2, n // 2 + 3000), (n // 2, n // 2 + 3000), (n // 2 + 1000, n // 2 + 4000), (10, 2000),
              (0, n), (n // 2 - 7, n // 2 + 1), (0, n)]
        fwd, total = _check(ix, rs)
        rev, total_r = _check(ix, rs[::-1])
        assert total == total_r and fwd.size == rev.size
    pieces, total = indexes[0].plan([])
    assert pieces.size == 0 and total == 0


def test_sizing_call_then_exact_cap(gh, indexes):
    ix = indexes[0]
    rs = np.asarray([(5, ix.n - 5), (100, 100), (7, 9000)], dtype=np.uint64)
    want, want_total = _reference(ix.offsets, rs.tolist())
    L = gh.lib()
    npieces, total = ctypes.c_uint64(123), ctypes.c_uint64(123)
    rc = L.gh_gather_plan(ctypes.byref(ix.c), rs.ctypes.data, 3, None, 0, ctypes.byref(npieces), ctypes.byref(total))
    assert rc == GH_E_SMALL and npieces.value == len(want) and total.value == want_total
    buf = np.zeros(len(want) + 1, dtype=gh.PIECE_DTYPE)
    buf["pad"][-1] = 0xABCD  # a guard record past the exact cap
    for cap in (len(want) - 1, len(want)):
        npieces.value = total.value = 0
        rc = L.gh_gather_plan(ctypes.byref(ix.c), rs.ctypes.data, 3, buf.ctypes.data, cap, ctypes.byref(npieces),
                              ctypes.byref(total))
        assert rc == (GH_OK if cap == len(want) else GH_E_SMALL)
        assert npieces.value == len(want) and total.value == want_total
        assert buf["pad"][-1] == 0xABCD
    assert _as_tuples(buf[:-1]) == want
    # only empty ranges: no piece, GH_OK even with cap = 0
    e = np.asarray([(4, 4), (ix.n, ix.n)], dtype=np.uint64)
    assert L.gh_gather_plan(ctypes.byref(ix.c), e.ctypes.data, 2, None, 0, ctypes.byref(npieces), ctypes.byref(total)) == 0
    assert npieces.value == 0 and total.value == 0


GH_OK = 0


def test_bad_ranges(gh, indexes):
    for ix in indexes:
        for bad in ([(0, ix.n + 1)], [(5, 4)], [(0, 10), (ix.n, ix.n + 1)], [(ix.n + 1, ix.n + 1)]):
            with pytest.raises(gh.GapHuffError) as e:
                ix.plan(bad)
            assert e.value.code == GH_E_ARG


def test_struct_mirrors(gh):
    assert ctypes.sizeof(gh.gh_range) == 16 and ctypes.sizeof(gh.gh_gather_piece) == 24 == gh.PIECE_DTYPE.itemsize
    assert {"gh_gather_plan", "gh_ctx_gather"} <= set(gh.EXPORTED)
