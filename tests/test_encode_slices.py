"""Sliced encode on the host (include/gaphuff.h, "sliced encode"): a stream built slice by
slice.  The invariant every test rests on: ORing all slices' outputs into an initialised
image gives exactly the bytes of gh_encode_write on the whole input.  Bytes are compared;
no tolerances.  No device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import slice_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(struct):
    return bytes(memoryview(struct))


# ---- 1. plans
@pytest.mark.parametrize("r", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [0, 1, 1000, 300000])
def test_plan_from_counts_equals_plan_make(gh, r, n):
    data = gh.generate(100 + n, r, n)
    counts = np.bincount(data, minlength=256).astype(np.uint64)
    assert _bytes(gh.plan_from_counts(counts)) == _bytes(gh.encode_plan(data))
    assert _bytes(gh.plan_from_counts(counts, force_version=2)) == _bytes(gh.encode_plan(data, force_version=2))


# ---- 2. merge identity, 3. edge bits and extents
@pytest.mark.parametrize("name,label", sc.CASES)
def test_merge_identity_and_edges(gh, name, label):
    data, plan, start, image = sc.case_input(gh, name)
    b = sc.case_bounds(name, label, data.size)
    parts = []
    for lo, hi in zip(b[:-1], b[1:]):
        base, bits = int(start[lo]), int(start[hi] - start[lo])
        s, words, gapw = gh.encode_slice(data[lo:hi], plan, base)
        sc.check_extents_and_edges(gh, s, words, gapw, base, bits)
        parts.append((s, words, gapw))
    order = np.random.default_rng(len(b)).permutation(len(parts))
    merged = gh.merge_slices(plan, [parts[i] for i in order])
    assert merged.size == image.size
    if not np.array_equal(merged, image):
        bad = np.nonzero(merged != image)[0]
        raise AssertionError(f"{bad.size} differing bytes, first at {bad[0]} of {image.size}")


def test_slice_buffers_do_not_depend_on_threads(gh):
    data = gh.generate(8, 0.5, 5_000_000)  # (the host encoder splits its input per MiB)
    plan = gh.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    lo, hi = 1_000_003, 4_500_001
    base = int(lens[data[:lo]].sum(dtype=np.uint64))
    one = gh.encode_slice(data[lo:hi], plan, base, threads=1)
    for t in (2, 3):
        s, w, g = gh.encode_slice(data[lo:hi], plan, base, threads=t)
        assert _bytes(s) == _bytes(one[0]) and np.array_equal(w, one[1]) and np.array_equal(g, one[2])


# ---- 4. shift invariance: base_bit >= 2^32
def shifted_case(gh):
    """A slice, a plan of a stream 2^24 times its size, and the two bases."""
    data = gh.generate(44, 0.5, 70_001)
    counts = np.bincount(data, minlength=256).astype(np.uint64) << np.uint64(24)
    plan = gh.plan_from_counts(counts)
    far = (1 << 33) + 77
    return data, plan, far, far % 1024


def test_shift_invariance_past_2_32(gh):
    data, plan, far, near = shifted_case(gh)
    assert (far - near) % 1024 == 0 and plan.bits > far + 16 * data.size
    s1, w1, g1 = gh.encode_slice(data, plan, far)
    s0, w0, g0 = gh.encode_slice(data, plan, near)
    assert np.array_equal(w1, w0) and np.array_equal(g1, g0) and w0.any() and g0.any()
    assert s1.bits == s0.bits and s1.nwords == s0.nwords and s1.ngapw == s0.ngapw
    assert s1.base_bit - s0.base_bit == far - near
    assert s1.word0 - s0.word0 == (far - near) // 32 and s1.gapw0 - s0.gapw0 == (far - near) // 1024
    sc.check_extents_and_edges(gh, s1, w1, g1, far, int(s0.bits))


# ---- 5. errors
def test_errors(gh):
    L = gh.lib()
    data = gh.generate(3, 0.9, 10_000)
    data = data[data != 7]  # byte 7 has no code
    plan = gh.encode_plan(data)
    assert plan.len[7] == 0
    with pytest.raises(gh.GapHuffError) as e:
        gh.encode_slice(np.array([data[0], 7, data[1]], dtype=np.uint8), plan, 0)
    assert e.value.code == -3  # GH_E_TABLE
    with pytest.raises(gh.GapHuffError) as e:
        gh.encode_slice(data, plan, 1)  # one bit past the plan's total
    assert e.value.code == -1  # GH_E_ARG
    # short caps: GH_E_SMALL, the extents filled all the same
    part = data[100:5000]
    s, words, gapw = gh.encode_slice(part, plan, 12345)
    assert s.nwords > 1 and s.ngapw > 1
    for wc, gc in ((0, 0), (s.nwords - 1, s.ngapw), (s.nwords, s.ngapw - 1)):
        t = gh.gh_slice()
        w = np.full(int(s.nwords), 0xA5A5A5A5, dtype=np.uint32)
        g = np.full(int(s.ngapw), 0xA5A5A5A5, dtype=np.uint32)
        rc = L.gh_encode_slice(part.ctypes.data, part.size, ctypes.byref(plan), 12345, 1, w.ctypes.data, wc,
                               g.ctypes.data, gc, ctypes.byref(t))
        assert rc == -9  # GH_E_SMALL
        assert _bytes(t) == _bytes(s)
        assert (w == 0xA5A5A5A5).all() and (g == 0xA5A5A5A5).all()  # nothing written
    # a short image
    img = np.zeros(plan.file_bytes, dtype=np.uint8)
    assert L.gh_encode_image_init(ctypes.byref(plan), img.ctypes.data, img.size - 1) == -9
    assert L.gh_encode_image_init(ctypes.byref(plan), img.ctypes.data, img.size) == 0
    assert L.gh_slice_merge(img.ctypes.data, img.size - 1, ctypes.byref(plan), ctypes.byref(s), words.ctypes.data,
                            gapw.ctypes.data) == -9
    # extents outside the stream
    bad = gh.slice_extent(plan.bits, 64)
    assert L.gh_slice_merge(img.ctypes.data, img.size, ctypes.byref(plan), ctypes.byref(bad), words.ctypes.data,
                            gapw.ctypes.data) == -1


def test_encode_bound(gh):
    assert gh.lib().gh_encode_bound(0) >= gh.encode_plan(b"").file_bytes
    rng = np.random.default_rng(2)
    for n in (1, 7, 8, 9, 255, 4096, 100_001):
        for data in (rng.integers(0, 256, n).astype(np.uint8), gh.generate(n, 0.5, n)):
            assert gh.encode_plan(data, force_version=2).file_bytes <= gh.lib().gh_encode_bound(n)
    # the bound is what 16-bit codes over 256 symbols under a v2 header take
    n = 1000
    assert gh.lib().gh_encode_bound(n) == 16 + 2 * 256 + 24 + 4 * ((n * 16 + 1023) // 1024) + 4 * (n * 16 // 32)


# ---- 6. struct layout
def test_gh_slice_layout(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    body = re.search(r"typedef struct gh_slice \{(.*?)\} gh_slice;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            assert decl.startswith("uint64_t "), decl
            fields += [f.strip() for f in decl[len("uint64_t "):].split(",")]
    assert fields == [f for f, _ in gh.gh_slice._fields_]
    assert all(t is ctypes.c_uint64 for _, t in gh.gh_slice._fields_)
    assert ctypes.sizeof(gh.gh_slice) == 8 * len(fields) == 48
