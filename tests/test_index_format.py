"""Seek index: the sidecar image and the host-side locate (gh_index_bytes, gh_index_parse,
gh_index_locate).  CPU only: the images are built here from synthetic offset arrays, and
locate is compared with numpy.searchsorted over the same arrays."""
import ctypes
import struct

import numpy as np
import pytest

MAGIC = b"GHIDX1\0\0"
GH_E_ARG, GH_E_FORMAT = -1, -2


def _image(log2_stride, n, g, offsets, magic=MAGIC, nentries=None):
    nentries = len(offsets) if nentries is None else nentries
    head = magic + struct.pack("<IIQQQ", log2_stride, 0, n, g, nentries)
    return head + np.asarray(offsets, dtype="<u8").tobytes()


def _synthetic(log2_stride, g, seed):
    """Monotone offsets for G segments: per-block steps between 0 and 143 * stride
    (zero steps included: a run of equal entries), the last entry N."""
    rng = np.random.default_rng(seed)
    stride = 1 << log2_stride
    nblocks = -(-g // stride)
    steps = rng.integers(0, 143 * stride + 1, size=nblocks)
    if nblocks > 3:
        steps[1] = 0
        steps[2] = 143 * stride
    off = np.concatenate([[0], np.cumsum(steps)]).astype(np.uint64)
    return off, int(off[-1])


def _expect(off, log2_stride, g, lo, hi):
    if lo == hi:
        return (0, 0, 0)
    nblocks = len(off) - 1
    k = int(np.searchsorted(off[:nblocks], lo, "right")) - 1
    m = int(np.searchsorted(off, hi, "left"))
    return (k << log2_stride, min(m << log2_stride, g), lo - int(off[k]))


CASES = [(k, g) for k in (8, 9, 12) for g in ((1 << k) * 5 - 1, (1 << k) * 5, (1 << k) * 5 + 1)] + [(8, 1), (12, 100)]


@pytest.mark.parametrize("log2_stride,g", CASES)
def test_parse_round_trip_and_locate(gh, log2_stride, g):
    off, n = _synthetic(log2_stride, g, seed=log2_stride * 131 + g)
    img = _image(log2_stride, n, g, off)
    assert gh.lib().gh_index_bytes(g, log2_stride) == len(img)
    ix = gh.parse_index(img)
    assert (ix.log2_stride, ix.n, ix.g) == (log2_stride, n, g)
    assert np.array_equal(ix.offsets, off)
    # an image at an odd address parses and locates too (entries are read bytewise)
    odd = np.frombuffer(b"\0" + img, dtype=np.uint8)[1:]
    assert gh.parse_index(odd).locate(0, n) == ix.locate(0, n)
    rng = np.random.default_rng(g)
    ranges = [(0, 0), (0, n)]
    if n:
        ranges += [(0, 1), (n - 1, n)]
    for e in off.tolist():
        for v in (e - 1, e, e + 1):
            if 0 <= v <= n:
                ranges += [(v, n), (0, v), (v, v), (v, min(v + 1, n))]
    for _ in range(200):
        a, b = sorted(rng.integers(0, n + 1, size=2).tolist())
        ranges.append((a, b))
    for lo, hi in ranges:
        assert ix.locate(lo, hi) == _expect(off, log2_stride, g, lo, hi), (lo, hi)


def test_locate_covers_the_range(gh):
    """What the caller relies on: the located segments' symbols [offsets[k], offsets[m])
    contain [lo, hi), and skip is lo's distance from the first of them."""
    k, g = 8, 256 * 7 + 3
    off, n = _synthetic(k, g, seed=3)
    ix = gh.parse_index(_image(k, n, g, off))
    rng = np.random.default_rng(4)
    for _ in range(300):
        lo, hi = sorted(rng.integers(0, n + 1, size=2).tolist())
        if lo == hi:
            continue
        b, e, skip = ix.locate(lo, hi)
        assert b % 256 == 0 and b < e <= g
        first, last = int(off[b >> k]), int(off[-(-e // 256)])
        assert first <= lo and hi <= last and skip == lo - first


def test_empty_stream(gh):
    img = _image(8, 0, 0, [0])
    assert gh.lib().gh_index_bytes(0, 8) == len(img) == 48
    ix = gh.parse_index(img)
    assert ix.locate(0, 0) == (0, 0, 0)
    with pytest.raises(gh.GapHuffError):
        ix.locate(0, 1)


def _refused(gh, img):
    with pytest.raises(gh.GapHuffError) as e:
        gh.parse_index(img)
    assert e.value.code == GH_E_FORMAT
    return True


def test_parse_refuses_malformed_images(gh):
    k, g = 8, 256 * 4 + 1
    off, n = _synthetic(k, g, seed=9)
    good = _image(k, n, g, off)
    gh.parse_index(good)
    for cut in (0, 7, 39, 40, len(good) - 8, len(good) - 1):  # truncated
        assert _refused(gh, good[:cut])
    assert _refused(gh, _image(k, n, g, off, magic=b"GHIDX2\0\0"))
    for bad_k in (0, 7, 21, 64):  # bad stride (the entry count made to fit where it can)
        nb = -(-g // (1 << bad_k)) if bad_k < 64 else 1
        assert _refused(gh, _image(bad_k, n, g, np.linspace(0, n, nb + 1).astype(np.uint64)))
    assert _refused(gh, _image(k, n, g, off, nentries=len(off) - 1))       # wrong nentries
    assert _refused(gh, _image(k, n, g, np.append(off, n)))                 # one entry too many
    assert _refused(gh, _image(k, n, g + 256, off))                         # G of another stream
    dec = off.copy()
    dec[4] = dec[3] - np.uint64(1)  # (entry 3 is past a full block: not 0)
    assert _refused(gh, _image(k, n, g, dec))                               # a decreasing entry
    big = off.copy()
    big[1:] += np.uint64(143 * 256 + 1 - int(off[1]))
    assert _refused(gh, _image(k, int(big[-1]), g, big))                    # an over-large step
    assert _refused(gh, _image(k, n + 1, g, off))                           # last entry != N
    first = off.copy()
    first[0] = 1
    assert _refused(gh, _image(k, n, g, first))                             # first entry != 0
    rsv = bytearray(good)
    rsv[12] = 1
    assert _refused(gh, bytes(rsv))                                         # reserved field


def test_locate_refuses_bad_ranges(gh):
    off, n = _synthetic(9, 512 * 3, seed=1)
    ix = gh.parse_index(_image(9, n, 512 * 3, off))
    for lo, hi in ((2, 1), (n, n - 1), (0, n + 1), (n + 1, n + 1)):
        with pytest.raises(gh.GapHuffError) as e:
            ix.locate(lo, hi)
        assert e.value.code == GH_E_ARG
    assert ix.locate(n, n) == (0, 0, 0)


def test_null_arguments_and_bad_strides(gh):
    L = gh.lib()
    buf = ctypes.create_string_buffer(64)
    assert L.gh_ctx_build_index(None, 8, buf, len(buf), None, None) == GH_E_ARG
    assert L.gh_index_parse(None, 0, None) == GH_E_ARG
    assert L.gh_index_locate(None, 0, 0, None, None, None) == GH_E_ARG
    for k in (7, 21):
        assert L.gh_index_bytes(1000, k) == 0
    assert L.gh_index_bytes(1000, 8) == 40 + 8 * 5
    assert L.gh_index_bytes(1024, 8) == 40 + 8 * 5
    assert L.gh_index_bytes(1025, 8) == 40 + 8 * 6
    assert L.gh_index_bytes(1, 20) == 40 + 8 * 2
