"""Batched gather without a GPU: the plan (gh_batchdec_plan through gh.batch_gather_plan)
against a plain numpy restatement, the piece bound, the refusals and the ABI.

The restatement walks every range's units one by one: stream s's entries are
unit_off[unit0[s] + j] - unit_off[unit0[s]], a range's first unit is the last one whose
entry is <= lo, and every unit from there whose entry is < hi gives one piece
{dst, global unit, pa - o0, pb - o0} with pa = max(lo, o0), pb = min(hi, o1)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_ARG, GH_E_NODEV, GH_E_SMALL = -1, -5, -9
NEW_NAMES = ("gh_batchdec_index", "gh_batchdec_gather_device", "gh_batchdec_gather_wait", "gh_batchdec_gather",
             "gh_batchdec_gather_pieces", "gh_batchdec_plan", "gh_batchdec_kernel_shape", "gh_batchdec_kernel_shapes")


def _batch(rng):
    """unit0, unit_off, n of a random batch: 1..40 streams of 0..12 units, non-last units of
    2048..36608 codewords (at least 8 per segment, at most 143), last ones of 1..36608."""
    ns = int(rng.integers(1, 41))
    units = rng.integers(0, 13, ns)
    unit0 = np.concatenate([[0], np.cumsum(units)]).astype(np.uint32)
    tot = []
    for u in units:
        if u:
            tot += rng.integers(2048, 36609, u - 1).tolist() + [int(rng.integers(1, 36609))]
    unit_off = np.concatenate([[0], np.cumsum(np.asarray(tot, dtype=np.uint64))]).astype(np.uint64)
    n = np.zeros(ns, dtype=np.uint64)
    for s in range(ns):
        total = int(unit_off[unit0[s + 1]] - unit_off[unit0[s]])
        # n <= the counted total: the last segment's padding decodes to codewords past N
        n[s] = total if rng.integers(0, 2) else max(total - int(rng.integers(0, 144)), min(total, 1))
    return unit0, unit_off, n


def _ranges(rng, unit0, unit_off, n):
    out = []
    for _ in range(int(rng.integers(0, 65))):
        s = int(rng.integers(0, n.size))
        N = int(n[s])
        ents = (unit_off[unit0[s]: unit0[s + 1] + 1] - unit_off[unit0[s]]).astype(np.int64)
        ents = ents[ents <= N]
        kind = int(rng.integers(0, 6))
        if kind == 0:
            lo = hi = int(rng.integers(0, N + 1))
        elif kind == 1:
            lo, hi = 0, N
        elif kind == 2 and ents.size:  # from a unit's first symbol to another unit's first symbol
            lo, hi = sorted(int(x) for x in rng.choice(ents, 2))
        elif kind == 3 and ents.size:  # around a unit offset
            e = int(rng.choice(ents))
            lo = max(e - int(rng.integers(0, 3)), 0)
            hi = min(e + int(rng.integers(0, 3)), N)
        elif kind == 4 and out:
            s, lo, hi = out[int(rng.integers(0, len(out)))]  # a repeat
        else:
            lo, hi = sorted(int(x) for x in rng.integers(0, N + 1, 2))
        out.append((s, lo, hi))
    return out


def _restate(unit0, unit_off, n, status, ranges):
    pieces, dst, bad = [], 0, 0
    for s, lo, hi in ranges:
        assert s < n.size and lo <= hi <= int(n[s])
        if status is not None and status[s]:
            bad += 1
            dst += hi - lo
            continue
        if lo == hi:
            continue
        u0, u1 = int(unit0[s]), int(unit0[s + 1])
        base = int(unit_off[u0])
        ent = [int(unit_off[u]) - base for u in range(u0, u1 + 1)]
        k = max(j for j in range(u1 - u0) if ent[j] <= lo)
        while k < u1 - u0 and ent[k] < hi:
            pa, pb = max(lo, ent[k]), min(hi, ent[k + 1])
            pieces.append((dst + pa - lo, u0 + k, pa - ent[k], pb - ent[k], 0))
            k += 1
        dst += hi - lo
    return pieces, dst, bad


def test_plan_matches_restatement(gh):
    rng = np.random.default_rng(375)
    seen = 0
    for it in range(2000):
        unit0, unit_off, n = _batch(rng)
        ranges = _ranges(rng, unit0, unit_off, n)
        want, total, _ = _restate(unit0, unit_off, n, None, ranges)
        # a condition on the inputs: the restatement alone meets the bound
        assert len(want) <= gh.gather_piece_bound(len(ranges), total, 8), it
        got, out_bytes, bad = gh.batch_gather_plan(unit0, unit_off, n, None, ranges)
        assert bad == 0 and out_bytes == total == sum(h - l for _, l, h in ranges), it
        assert got.size == len(want), it
        for name, col in zip(("dst", "block", "a", "b", "pad"), zip(*want) if want else [()] * 5):
            assert got[name].tolist() == list(col), (it, name)
        seen += len(want)
    assert seen > 20000


def test_refusals_and_sizing(gh):
    unit0 = np.asarray([0, 2, 2, 3], dtype=np.uint32)
    unit_off = np.asarray([0, 3000, 5000, 5100], dtype=np.uint64)
    n = np.asarray([4990, 0, 100], dtype=np.uint64)
    L = gh.lib()
    for bad in ((3, 0, 0), (0, 5, 4), (0, 0, 4991), (1, 0, 1), (2, 0, 101), ((1 << 40) + 1, 0, 0)):
        with pytest.raises(gh.GapHuffError) as e:
            gh.batch_gather_plan(unit0, unit_off, n, None, [(0, 0, 10), bad, (2, 0, 1)])
        assert e.value.code == GH_E_ARG, bad
    # sizing: cap = 0 fills the counts and returns GH_E_SMALL
    r = np.asarray([(0, 2990, 3010), (2, 0, 100), (1, 0, 0)], dtype=np.uint64)
    np_, total, nbad = ctypes.c_uint64(99), ctypes.c_uint64(99), ctypes.c_uint32(99)
    rc = L.gh_batchdec_plan(unit0.ctypes.data, unit_off.ctypes.data, n.ctypes.data, None, 3, r.ctypes.data, 3, None, 0,
                            ctypes.byref(np_), ctypes.byref(total), ctypes.byref(nbad))
    assert rc == GH_E_SMALL and (np_.value, total.value, nbad.value) == (3, 120, 0)
    got, total, nbad = gh.batch_gather_plan(unit0, unit_off, n, None, r)
    assert [tuple(p) for p in got.tolist()] == [(0, 0, 2990, 3000, 0), (10, 1, 0, 10, 0), (20, 2, 0, 100, 0)]
    # null pointers
    total_c, nbad_c = ctypes.c_uint64(), ctypes.c_uint32()
    assert L.gh_batchdec_plan(None, unit_off.ctypes.data, n.ctypes.data, None, 3, r.ctypes.data, 3, None, 0,
                              ctypes.byref(np_), ctypes.byref(total_c), ctypes.byref(nbad_c)) == GH_E_ARG
    assert L.gh_batchdec_plan(unit0.ctypes.data, unit_off.ctypes.data, n.ctypes.data, None, 3, r.ctypes.data, 3, None, 0,
                              None, ctypes.byref(total_c), ctypes.byref(nbad_c)) == GH_E_ARG


def test_flagged_stream_gets_no_pieces(gh):
    rng = np.random.default_rng(7)
    for it in range(200):
        unit0, unit_off, n = _batch(rng)
        status = (rng.integers(0, 4, n.size) == 0).astype(np.uint32)
        ranges = _ranges(rng, unit0, unit_off, n)
        want, total, bad = _restate(unit0, unit_off, n, status, ranges)
        got, out_bytes, nbad = gh.batch_gather_plan(unit0, unit_off, n, status, ranges)
        assert nbad == bad == sum(1 for s, _, _ in ranges if status[s]), it
        assert out_bytes == total == sum(h - l for _, l, h in ranges), it  # a flagged range keeps its slot
        assert [tuple(p) for p in got.tolist()] == want, it
        assert not any(status[np.searchsorted(unit0, b, "right") - 1] for b in got["block"].tolist()), it


def test_abi_names_and_sizes(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src))
    assert {x for x in declared if x.startswith("gh_batchdec_")} == set(NEW_NAMES)
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in NEW_NAMES:
        assert name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert ctypes.sizeof(gh.gh_brange) == 24 and ctypes.sizeof(gh.gh_bgather_report) == 32
    for t in ("gh_brange", "gh_bgather_report"):
        assert re.search(r"\}\s*%s\s*;" % t, src), t


def test_kernel_names(gh):
    names = gh.batchdec_kernel_shapes()
    assert sorted(names) == ["bgather<fb=0>", "bgather<fb=1>"]
    others = set(gh.kernel_shapes()) | set(gh.enc_kernel_shapes()) | set(gh.batch_kernel_shapes()) | set(gh.ebatch_kernel_shapes())
    assert not set(names) & others


def test_no_gpu_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(gh.GapHuffError) as e:
        gh.BatchDecoder(0)
    assert e.value.code == GH_E_NODEV
    with pytest.raises(gh.GapHuffError):
        gh.decode_batch_ranges([gh.encode(gh.generate(1, 0.5, 1000))], [(0, 0, 10)])
