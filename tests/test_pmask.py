"""Plane choice on the CPU: the gh_pmask_* ABI, the rule (a plane is coded iff its
compressed.huff image is smaller than its nelem raw bytes; a tie is stored), gh_pmask_host and
gh_pmask_from_counts.

The ground truth is the host encoder: len(gh.encode(plane)) and np.bincount."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gpu_planes import Tensor
from test_planes import bf16_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_ARG = -1
ELEMS = (1, 2, 4, 8)
NELEMS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)
PMASK_NAMES = {"gh_pmask_from_counts", "gh_pmask_host", "gh_pmask_device", "gh_pmask_counts"}
# nelem of a constant plane -> coded?  fb = 26 + 4 ceil(n / 32): 30 up to n = 32, then 34
TIES = ((29, False), (30, False), (31, True), (33, False), (34, False), (35, True))


def _planes(a, e):
    return [np.ascontiguousarray(a.reshape(-1, e)[:, p]) for p in range(e)]


def _want(gh, a, e):
    """(mask, sizes) of the bytes `a` as a tensor of e-byte elements, by gh.encode."""
    nelem = a.size // e
    sizes = [len(gh.encode(pl)) if nelem else 0 for pl in _planes(a, e)]
    return sum(1 << p for p in range(e) if nelem and sizes[p] < nelem), sizes + [0] * (8 - e)


def _as_dtype(raw, e):
    return raw.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[e])


def _int32_ids(n=65536, seed=11):
    return np.random.default_rng(seed).integers(0, 1000, n).astype(np.int32)


def _structural():
    """(tensor, its best mask) of the issue's table, 65 536 elements each."""
    rng = np.random.default_rng(5)
    return ((bf16_weights(), 0b10), (rng.normal(0, 0.02, 65536).astype(np.float32), 0b1000),
            (_int32_ids(), 0b1110), (rng.integers(0, 256, 65536, dtype=np.uint8), 0))


def test_names_declared_listed_and_exported(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = {n for n in re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src) if n.startswith("gh_pmask_")}
    listed = {n for n in gh.EXPORTED if n.startswith("gh_pmask_")}
    assert declared == listed == PMASK_NAMES
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert ctypes.sizeof(gh.gh_pmask_report) == 40
    assert gh.GH_PMASK_LAUNCHES == 4 and re.search(r"#define\s+GH_PMASK_LAUNCHES\s+4u", src)
    # the section stands after the element gather's
    assert src.index("gh_pgather(") < src.index("gh_pmask_from_counts(") < src.index("gh_planes_image_bytes(")


@pytest.mark.parametrize("e", ELEMS)
def test_rule_and_sizes(gh, e):
    for nelem in NELEMS:
        t = Tensor(gh, e, nelem, 0, 1000 * e + 7 * nelem)
        mask, sizes = _want(gh, t.data, e)
        for shift in (0, 1, 5):  # the tensor at byte offsets inside a larger buffer
            buf = np.full(t.data.size + 64, 0xFF, dtype=np.uint8)
            buf[shift: shift + t.data.size] = t.data
            arr, n = gh._planes_items([(buf.ctypes.data + shift, nelem, e, 0)])
            m, pb = np.full(1, 77, np.uint32), np.full(8, 77, np.uint64)
            assert gh.lib().gh_pmask_host(arr, n, gh._ptr(m), gh._ptr(pb)) == 0
            assert pb.tolist() == sizes, (e, nelem, shift)
            assert int(m[0]) == mask, (e, nelem, shift)
        masks, pb = gh.choose_planes_masks([_as_dtype(t.data, e)])
        assert masks.tolist() == [mask] and pb.tolist() == [sizes]


def test_tie_table(gh):
    for nelem, coded in TIES:
        const = np.full(nelem, 0x3C, dtype=np.uint8)
        fb = len(gh.encode(const))
        assert fb == 26 + 4 * -(-nelem // 32) and (fb < nelem) == coded
        masks, pb = gh.choose_planes_masks([const])
        assert int(masks[0]) == int(coded) and int(pb[0][0]) == fb, nelem
        # as one plane of a two-byte tensor whose other plane is random (and stays stored)
        for p in (0, 1):
            a = np.random.default_rng(nelem).integers(0, 256, 2 * nelem, dtype=np.uint8)
            a[p::2] = 0x3C
            masks, pb = gh.choose_planes_masks([a.view(np.uint16)])
            assert int(masks[0]) == (int(coded) << p), (nelem, p)
            assert int(pb[0][p]) == fb and int(pb[0][1 - p]) == len(gh.encode(a[1 - p::2])) > nelem


def test_structural_masks(gh):
    tensors = [a for a, _ in _structural()]
    masks, pb = gh.choose_planes_masks(tensors)
    assert masks.tolist() == [m for _, m in _structural()]
    for a, sizes in zip(tensors, pb):
        e = a.dtype.itemsize
        assert sizes.tolist() == _want(gh, a.view(np.uint8), e)[1]


def test_container_bound(gh, orc):
    """The chosen mask's container is no larger than the all-stored, the default and the all-coded
    one, and it parses and decodes."""
    rng = np.random.default_rng(9)
    tensors = [a for a, _ in _structural()] + [np.cumsum(rng.integers(0, 50, 4096)).astype(np.int64) + 1_700_000_000_000,
                                               _as_dtype(Tensor(gh, 4, 1025, 0, 3).data, 4), np.zeros(35, np.uint8),
                                               np.zeros(34, np.uint8)]
    masks, _ = gh.choose_planes_masks(tensors)
    for a, chosen in zip(tensors, masks.tolist()):
        e, raw = a.dtype.itemsize, a.view(np.uint8)
        planes = _planes(raw, e)
        images = [gh.encode(pl) for pl in planes]

        def container(mask):
            return gh.planes_image(a.size, e, mask, [images[p] if (mask >> p) & 1 else planes[p] for p in range(e)])

        img = container(chosen)
        for other in (0, gh.default_planes_mask(e), (1 << e) - 1):
            assert img.size <= container(other).size, (a.dtype, chosen, other)
        im = gh.parse_planes(img)
        assert (im.nelem, im.elem_size, im.coded_mask) == (a.size, e, chosen)
        got = [orc.decode(images[p], out_cap=a.size)[0][: a.size] if (chosen >> p) & 1 else im.planes[p] for p in range(e)]
        assert np.array_equal(gh.planes_join_host(got), raw)


def test_from_counts_equals_host(gh):
    ts = [Tensor(gh, e, nelem, 0, 31 * e + nelem) for e in ELEMS for nelem in (0, 17, 1025, 8192)]
    arrays = [_as_dtype(t.data, t.e) for t in ts]
    counts = np.asarray([np.bincount(pl, minlength=256) for t in ts for pl in t.planes], dtype=np.uint64).reshape(-1, 256)
    masks, pb = gh.planes_masks_from_counts(counts, [(t.nelem, t.e) for t in ts])
    want_m, want_pb = gh.choose_planes_masks(arrays)
    assert np.array_equal(masks, want_m) and np.array_equal(pb, want_pb)
    assert want_m.any() and not want_m[0]


@pytest.mark.parametrize("kind", ("skewed", "flat", "one"))
def test_from_counts_v2_header(gh, kind):
    """Counts no tensor in memory backs: sums >= 2^31 take the 64-bit header, as the plan does."""
    if kind == "skewed":
        counts = (np.arange(256, dtype=np.uint64) ** 3 * 2000 + 1).astype(np.uint64)
    elif kind == "flat":
        counts = np.full(256, 1 << 24, dtype=np.uint64)
    else:
        counts = np.zeros(256, dtype=np.uint64)
        counts[200] = (1 << 31) + 5
    n = int(counts.sum())
    assert n >= 1 << 31
    plan = gh.plan_from_counts(counts)
    assert plan.version == 2
    masks, pb = gh.planes_masks_from_counts(counts, [(n, 1)])
    assert int(pb[0][0]) == int(plan.file_bytes)
    assert int(masks[0]) == int(plan.file_bytes < n)
    # and one just below the limit keeps the 32-bit header
    small = np.zeros(256, dtype=np.uint64)
    small[7] = (1 << 31) - 1
    plan = gh.plan_from_counts(small)
    assert plan.version == 1
    assert int(gh.planes_masks_from_counts(small, [((1 << 31) - 1, 1)])[1][0][0]) == int(plan.file_bytes)


def test_refusals(gh):
    H, C = gh.lib().gh_pmask_host, gh.lib().gh_pmask_from_counts
    a = np.arange(64, dtype=np.uint8)
    it, n = gh._planes_items([(a.ctypes.data, 32, 2, 0)])
    m, pb = np.zeros(1, np.uint32), np.zeros(8, np.uint64)
    counts = np.asarray([np.bincount(a[p::2], minlength=256) for p in (0, 1)], dtype=np.uint64)
    assert H(it, 1, gh._ptr(m), gh._ptr(pb)) == 0 and C(gh._ptr(counts), it, 1, gh._ptr(m), gh._ptr(pb)) == 0
    assert H(it, 1, gh._ptr(m), None) == 0 and C(gh._ptr(counts), it, 1, gh._ptr(m), None) == 0  # sizes are optional
    # nulls
    assert H(None, 1, gh._ptr(m), gh._ptr(pb)) == GH_E_ARG and H(it, 1, None, gh._ptr(pb)) == GH_E_ARG
    assert C(None, it, 1, gh._ptr(m), gh._ptr(pb)) == GH_E_ARG and C(gh._ptr(counts), None, 1, gh._ptr(m), None) == GH_E_ARG
    assert C(gh._ptr(counts), it, 1, None, None) == GH_E_ARG
    null, _ = gh._planes_items([(0, 32, 2, 0)])
    assert H(null, 1, gh._ptr(m), None) == GH_E_ARG
    # a bad element size; the coded mask is ignored
    for bad_e in (0, 3, 5, 6, 7, 9, 16):
        bad, _ = gh._planes_items([(a.ctypes.data, 4, bad_e, 0)])
        assert H(bad, 1, gh._ptr(m), None) == GH_E_ARG and C(gh._ptr(counts), bad, 1, gh._ptr(m), None) == GH_E_ARG
    odd, _ = gh._planes_items([(a.ctypes.data, 32, 2, 0xFFFF)])
    assert H(odd, 1, gh._ptr(m), None) == 0
    # counts that do not sum to nelem
    for nelem in (31, 33):
        off, _ = gh._planes_items([(0, nelem, 2, 0)])
        assert C(gh._ptr(counts), off, 1, gh._ptr(m), None) == GH_E_ARG
    empty, _ = gh._planes_items([(0, 0, 2, 0)])
    assert C(gh._ptr(counts), empty, 1, gh._ptr(m), None) == GH_E_ARG
    # nelem = 0: mask 0, sizes 0
    m[:], pb[:] = 77, 77
    assert H(empty, 1, gh._ptr(m), gh._ptr(pb)) == 0 and m[0] == 0 and not pb.any()
    m[:], pb[:] = 77, 77
    zeros = np.zeros((2, 256), dtype=np.uint64)
    assert C(gh._ptr(zeros), empty, 1, gh._ptr(m), gh._ptr(pb)) == 0 and m[0] == 0 and not pb.any()
    # no tensors
    assert H(None, 0, None, None) == 0 and C(None, None, 0, None, None) == 0
    masks, sizes = gh.choose_planes_masks([])
    assert masks.size == 0 and sizes.shape == (0, 8)
    # more than 2^24 candidate planes: 2^21 + 1 tensors of 8
    many = (1 << 21) + 1
    arr = (gh.gh_planes_item * many)()
    buf = np.frombuffer(arr, dtype=np.dtype([("data", "<u8"), ("nelem", "<u8"), ("e", "<u4"), ("mask", "<u4")]))
    buf["nelem"], buf["e"] = 0, 8
    mm = np.zeros(many, np.uint32)
    assert H(arr, many, gh._ptr(mm), None) == GH_E_ARG
    assert H(arr, many - 1, gh._ptr(mm), None) == 0
