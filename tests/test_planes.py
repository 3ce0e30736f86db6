"""Byte planes on the CPU: the gh_planes_* ABI, the host twins of the split and join kernels,
the layout, the container, and the reason the feature exists (a float's exponent byte codes
well, its mantissa bytes do not)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_ARG, GH_E_FORMAT, GH_E_NODEV, GH_E_SMALL = -1, -2, -5, -9
ELEMS = (1, 2, 4, 8)
NELEMS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)
PLANES_NAMES = {
    "gh_planes_layout", "gh_planes_split_host", "gh_planes_join_host", "gh_planes_load", "gh_planes_load_device",
    "gh_planes_load_times", "gh_planes_join_device", "gh_planes_wait", "gh_planes_image_bytes", "gh_planes_image_write", "gh_planes_parse",
}


def bf16_weights(seed=7, n=65536):
    """N(0, 0.02) float32 weights rounded to nearest-even bfloat16, as uint16."""
    u = np.random.default_rng(seed).normal(0, 0.02, n).astype(np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_names_declared_listed_and_exported(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src) if n.startswith("gh_planes_")}
    listed = {n for n in gh.EXPORTED if n.startswith("gh_planes_")}
    assert declared == listed == PLANES_NAMES
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert ctypes.sizeof(gh.gh_planes_item) == 24 and ctypes.sizeof(gh.gh_planes_slot) == 16
    assert gh.GH_PLANES_MAGIC.to_bytes(8, "little") == b"GHPLN1\0\0"


@pytest.mark.parametrize("e", ELEMS)
def test_host_twins_against_numpy(gh, e):
    for nelem in NELEMS:
        a = np.random.default_rng(100 * e + nelem).integers(0, 256, nelem * e, dtype=np.uint8)
        planes = gh.planes_split_host(a, e)
        assert len(planes) == e
        for p in range(e):
            assert np.array_equal(planes[p], a.reshape(-1, e)[:, p]), (e, nelem, p)
        assert np.array_equal(gh.planes_join_host(planes), a), (e, nelem)
    # typed arrays: the element size is the dtype's
    t = np.arange(1000, dtype={1: np.uint8, 2: np.uint16, 4: np.float32, 8: np.float64}[e])
    assert np.array_equal(gh.planes_join_host(gh.planes_split_host(t)), t.view(np.uint8))


def test_layout_numbering_and_offsets(gh):
    items = [(0, 100, 2, 0b10), (0, 0, 4, 0b1111), (0, 5, 4, 0b0101), (0, 17, 1, 0), (0, 1024, 8, 0b10000001), (0, 3, 1, 1)]
    slots, nstreams, stored_bytes = gh.planes_layout(items)
    S = gh.GH_PLANES_STORED
    assert S == 0xFFFFFFFF
    pad = lambda n: -(-n // 16) * 16
    want, s, at = [], 0, 0
    for _, nelem, e, mask in items:
        row = []
        for p in range(8):
            if p < e and (mask >> p) & 1:
                row.append((s, 0))
                s += 1
            elif p < e:
                row.append((S, at))
                at += pad(nelem)
            else:
                row.append((S, 0))
        want.append(row)
    assert slots == want and nstreams == s == 10 and stored_bytes == at
    assert at == 112 + 2 * 16 + 32 + 6 * 1024
    assert all(off % 16 == 0 for row in slots for _, off in row)
    assert gh.planes_layout([]) == ([], 0, 0)


def test_layout_refusals(gh):
    def refused(items):
        with pytest.raises(gh.GapHuffError) as e:
            gh.planes_layout(items)
        return e.value.code

    for bad_e in (0, 3, 5, 6, 7, 9, 16):
        assert refused([(0, 10, 2, 1), (0, 10, bad_e, 0)]) == GH_E_ARG
    for e in ELEMS:
        assert refused([(0, 10, e, 1 << e)]) == GH_E_ARG
        gh.planes_layout([(0, 10, e, (1 << e) - 1)])
    assert refused([(0, 2 ** 64 - 5, 1, 0)]) == GH_E_ARG                      # round_up(nelem, 16) overflows
    assert refused([(0, 2 ** 63, 2, 0)]) == GH_E_ARG                          # the sum overflows
    # null pointers
    L = gh.lib().gh_planes_layout
    it = (gh.gh_planes_item * 1)()
    it[0].nelem, it[0].elem_size, it[0].coded_mask = 4, 2, 1
    sl = (gh.gh_planes_slot * 8)()
    ns, sb = ctypes.c_uint32(), ctypes.c_uint64()
    assert L(it, 1, sl, ctypes.byref(ns), ctypes.byref(sb)) == 0 and ns.value == 1 and sb.value == 16
    assert L(None, 1, sl, ctypes.byref(ns), ctypes.byref(sb)) == GH_E_ARG
    assert L(it, 1, None, ctypes.byref(ns), ctypes.byref(sb)) == GH_E_ARG
    assert L(it, 1, sl, None, ctypes.byref(sb)) == GH_E_ARG
    assert L(it, 1, sl, ctypes.byref(ns), None) == GH_E_ARG
    # more than 2^24 coded planes: 2^21 + 1 tensors of 8 coded planes
    many = (1 << 21) + 1
    arr = (gh.gh_planes_item * many)()
    buf = np.frombuffer(arr, dtype=np.dtype([("data", "<u8"), ("nelem", "<u8"), ("e", "<u4"), ("mask", "<u4")]))
    buf["nelem"], buf["e"], buf["mask"] = 1, 8, 0xFF
    slots = (gh.gh_planes_slot * (8 * many))()
    assert L(arr, many, slots, ctypes.byref(ns), ctypes.byref(sb)) == GH_E_ARG
    assert L(arr, many - 1, slots, ctypes.byref(ns), ctypes.byref(sb)) == 0 and ns.value == 1 << 24


def _container(gh, a, e, mask):
    planes = gh.planes_split_host(a, e)
    parts = [gh.encode(pl) if (mask >> p) & 1 else pl for p, pl in enumerate(planes)]
    return gh.planes_image(planes[0].size, e, mask, parts), planes, parts


def test_container_round_trip(gh, orc):
    """planes_split_host, gh.encode per coded plane, the container, parse_planes, the oracle's
    decode per coded plane, planes_join_host: the input."""
    rng = np.random.default_rng(3)
    for e, nelem, mask in ((1, 700, 1), (2, 4101, 0b10), (4, 1025, 0b1001), (8, 300, 0b10101010), (4, 0, 0b1000),
                           (2, 17, 0), (8, 16, 0xFF)):
        a = (rng.integers(0, 256, nelem * e) >> rng.integers(0, 6, nelem * e)).astype(np.uint8)  # skewed bytes
        img, planes, parts = _container(gh, a, e, mask)
        im = gh.parse_planes(img)
        assert (im.nelem, im.elem_size, im.coded_mask) == (nelem, e, mask)
        # the layout: header, sizes, then every plane on an 8-byte boundary, in order
        assert img[:8].tobytes() == b"GHPLN1\0\0"
        assert img[8:24].view("<u4")[:2].tolist() == [e, mask] and int(img[16:24].view("<u8")[0]) == nelem
        sizes = img[24: 24 + 8 * e].view("<u8").tolist()
        assert sizes == [p.size for p in parts]
        at = 24 + 8 * e
        got = []
        for p in range(e):
            at = -(-at // 8) * 8
            assert np.array_equal(img[at: at + sizes[p]], parts[p])
            at += sizes[p]
            if (mask >> p) & 1:
                assert im.planes[p].n == nelem
                got.append(orc.decode(parts[p], out_cap=max(nelem, 1))[0][:nelem])
            else:
                assert np.array_equal(im.planes[p], planes[p])
                got.append(im.planes[p])
        assert at == img.size
        assert np.array_equal(gh.planes_join_host(got) if nelem else np.zeros(0, np.uint8), a)


def test_container_refusals(gh):
    a = np.random.default_rng(5).integers(0, 4, 2 * 500, dtype=np.uint8)
    img, planes, parts = _container(gh, a, 2, 0b10)

    def refused(image):
        with pytest.raises(gh.GapHuffError) as e:
            gh.parse_planes(image)
        return e.value.code

    gh.parse_planes(img)
    for cut in (0, 7, 8, 23, 39, 40, 41, 40 + 500, img.size - 1):  # truncated
        assert refused(img[:cut]) == GH_E_FORMAT, cut
    bad = img.copy()
    bad[0] ^= 1                                                  # the magic
    assert refused(bad) == GH_E_FORMAT
    for e_bad in (0, 3, 16):
        bad = img.copy()
        bad[8:12] = np.asarray([e_bad], "<u4").view(np.uint8)    # the element size
        assert refused(bad) == GH_E_FORMAT
    bad = img.copy()
    bad[12:16] = np.asarray([0b100], "<u4").view(np.uint8)       # a mask >= 1 << E
    assert refused(bad) == GH_E_FORMAT
    bad = img.copy()
    bad[24:32] = np.asarray([499], "<u8").view(np.uint8)         # a stored plane of the wrong size
    assert refused(bad) == GH_E_FORMAT
    bad = img.copy()
    bad[16:24] = np.asarray([501], "<u8").view(np.uint8)         # nelem: the stored plane and the coded n disagree
    assert refused(bad) == GH_E_FORMAT
    # a coded plane with n != nelem, everything else consistent
    other = gh.encode(np.zeros(499, dtype=np.uint8))
    assert refused(gh.planes_image(500, 2, 0b10, [planes[0], other])) == GH_E_FORMAT
    # a coded plane that is no stream
    assert refused(gh.planes_image(500, 2, 0b10, [planes[0], np.full(64, 0xEE, np.uint8)])) == GH_E_FORMAT
    # the writer's own refusals
    with pytest.raises(gh.GapHuffError) as e:
        gh.planes_image(500, 2, 0b10, [planes[0][:499], parts[1]])
    assert e.value.code == GH_E_ARG
    with pytest.raises(gh.GapHuffError) as e:
        gh.planes_image(500, 2, 0b100, parts)
    assert e.value.code == GH_E_ARG


def test_why_planes_bf16(gh):
    """The reason for the feature, pinned: bf16 N(0, 0.02) weights (seed 7, 65536 elements).  The
    container with the high plane coded and the low plane stored is smaller than the code of
    the interleaved bytes (measured: 0.675 against 0.807 of the raw bytes), and coding the
    low (mantissa) plane makes it larger than storing it (1.039)."""
    w = bf16_weights()
    raw = w.view(np.uint8)
    interleaved = gh.encode(raw).size / raw.size
    img, planes, parts = _container(gh, raw, 2, 0b10)
    container = img.size / raw.size
    low_coded = gh.encode(planes[0]).size / planes[0].size
    print(f"interleaved {interleaved:.3f} container {container:.3f} low plane coded {low_coded:.3f} "
          f"high plane coded {parts[1].size / planes[1].size:.3f}")
    assert container < interleaved
    assert low_coded > 1.0


def test_no_device_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    w = bf16_weights(n=1000)
    with pytest.raises(gh.GapHuffError) as e:
        gh.BatchEncoder(0).load_planes([w])
    assert e.value.code == GH_E_NODEV
    img, _, _ = _container(gh, w.view(np.uint8), 2, 0b10)
    with pytest.raises(gh.GapHuffError) as e:
        gh.decode_tensors([img])
    assert e.value.code == GH_E_NODEV
    with pytest.raises(gh.GapHuffError) as e:
        gh.encode_tensors([w])
    assert e.value.code == GH_E_NODEV
