"""Element gather without a GPU: the gh_pgather_ names in the header / EXPORTED / the library,
the struct sizes, and gh_pgather_plan against a plain-Python recomputation on a fixed mixed
tensor list (E in {1, 2, 4, 8}; masks none, top, all, 0b0101; nelem in {0, 1, 17, 1024, 2049}):
the byte ranges' order, the staging and destination offsets, the staging offsets against the
dst0 gh_batchdec_plan gives the same byte ranges, the refusals, flagged streams and the sizing
call."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PGATHER_NAMES = {"gh_pgather_plan", "gh_pgather_device", "gh_pgather_wait", "gh_pgather"}
GH_OK, GH_E_ARG, GH_E_SMALL = 0, -1, -9

# (nelem, elem_size, coded_mask): every E with masks none / top / all / 0b0101 where they exist
SHAPES = [
    (2049, 2, 0b10), (17, 4, 0b0101), (1024, 8, 0xFF), (1, 1, 0b1), (0, 2, 0b10), (1024, 4, 0),
    (2049, 8, 0b10000000), (17, 1, 0), (1, 8, 0b0101), (2049, 4, 0b1111), (1024, 2, 0b11), (17, 8, 0),
]
ITEMS = [(0, n, e, m) for n, e, m in SHAPES]


def _ranges():
    out = []
    for t, (n, e, m) in enumerate(SHAPES):
        out += [(t, 0, n), (t, n, n), (t, 0, 0), (t, n // 2, n), (t, min(1, n), n)]
        if n >= 1024:
            out += [(t, 16, 1024), (t, 1023, 1024), (t, 15, 17)]
    rng = np.random.default_rng(5)
    out = [out[i] for i in rng.permutation(len(out))]
    return out + out[:7]  # (repeats)


def _streams():
    """Coded planes in tensor order, then plane order: the tensor's list of stream numbers."""
    s, per = 0, []
    for n, e, m in SHAPES:
        per.append([])
        for p in range(e):
            if (m >> p) & 1:
                per[-1].append(s)
                s += 1
    return per, s


def _naive(ranges, status=None):
    per, ns = _streams()
    br, so, do, stage, dst, bad = [], [], [], 0, 0, 0
    for t, lo, hi in ranges:
        n, e, m = SHAPES[t]
        so.append(stage)
        do.append(dst)
        br += [(s, lo, hi) for s in per[t]]
        stage += (hi - lo) * len(per[t])
        dst += (hi - lo) * e
        if status is not None and any(status[s] for s in per[t]):
            bad += 1
    return br, so, do, dst, bad


def test_names_declared_listed_and_exported(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    declared = set(re.findall(r"\b(gh_pgather_?\w*)\s*\(", src))
    listed = {n for n in gh.EXPORTED if n.startswith("gh_pgather")}
    assert declared == listed == PGATHER_NAMES
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert ctypes.sizeof(gh.gh_erange) == 24 and ctypes.sizeof(gh.gh_pgather_report) == 40
    for t in ("gh_erange", "gh_pgather_report"):
        assert re.search(r"\}\s*%s\s*;" % t, src), t
    assert "these carry gh_pgather_" in src
    m = re.search(r"#define GH_PGATHER_LAUNCHES (\d+)u", src)
    assert m and int(m.group(1)) == gh.GH_PGATHER_LAUNCHES
    assert gh.GH_PGATHER_MAX_RANGES * 8 == gh.GH_GATHER_MAX_RANGES
    for attr in ("gather_elements_device", "elements_wait", "gather_elements"):
        assert callable(getattr(gh.BatchDecoder, attr))
    assert callable(gh.decode_tensor_ranges) and callable(gh.planes_gather_plan)


def test_plan_against_python(gh):
    ranges = _ranges()
    br, so, do, ob, bad = gh.planes_gather_plan(ITEMS, ranges)
    wbr, wso, wdo, wob, _ = _naive(ranges)
    assert br.tolist() == [list(x) for x in wbr]  # range-major, then plane order
    assert so.tolist() == wso and do.tolist() == wdo and ob == wob and bad == 0
    # a tensor without coded planes gives no byte ranges
    t0 = next(t for t, s in enumerate(SHAPES) if s[2] == 0 and s[0] == 1024)
    b0, s0, d0, o0, _ = gh.planes_gather_plan(ITEMS, [(t0, 3, 1000), (t0, 0, 1024)])
    assert b0.shape == (0, 3) and s0.tolist() == [0, 0] and d0.tolist() == [0, 997 * 4] and o0 == (997 + 1024) * 4
    assert gh.planes_gather_plan(ITEMS, [])[3] == 0


def test_stage_offsets_are_the_inner_gathers_dst0(gh):
    """stage_off[i] is the dst0 the batched gather assigns to range i's first byte range (the
    prefix of the byte ranges' lengths), coded plane c follows c * (hi - lo) bytes later, and
    the pieces gh_batchdec_plan cuts over a made-up index start at those offsets."""
    ranges = _ranges()
    br, so, _, _, _ = gh.planes_gather_plan(ITEMS, ranges)
    per, ns = _streams()
    n = np.zeros(ns, dtype=np.uint64)
    for (ne, e, m), ss in zip(SHAPES, per):
        n[ss] = ne
    # a made-up index: every stream ceil(n / 700) units of near-equal symbol counts, at least one symbol each
    units = [max(1, -(-int(x) // 700)) if x else 0 for x in n]
    unit0 = np.concatenate([[0], np.cumsum(units)]).astype(np.uint32)
    counts = []
    for x, u in zip(n.tolist(), units):
        counts += [x // u + (1 if j < x % u else 0) for j in range(u)]
    unit_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    pieces, out_bytes, bad = gh.batch_gather_plan(unit0, unit_off, n, None, br)
    assert bad == 0 and out_bytes == int((br[:, 2] - br[:, 1]).sum())
    dst0 = np.concatenate([[0], np.cumsum(br[:, 2] - br[:, 1])])[:-1]
    slot = 0
    for i, (t, lo, hi) in enumerate(ranges):
        c = len(per[t])
        if c:
            assert int(dst0[slot]) == int(so[i]), (i, t, lo, hi)
            for k in range(c):
                assert int(dst0[slot + k]) == int(so[i]) + k * (hi - lo)
        slot += c
    assert slot == br.shape[0]
    # and the pieces the plan cut carry those offsets: every non-empty byte range's first piece
    starts = sorted({int(p["dst"]) for p in pieces})
    want = sorted({int(d) for d, (s, lo, hi) in zip(dst0, br.tolist()) if hi > lo})
    assert set(want) <= set(starts)


def _rc_plan(gh, items, ranges, cap=64):
    arr, n = gh._planes_items(items)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
    br = np.zeros((cap, 3), dtype=np.uint64)
    so, do = np.zeros(len(r), np.uint64), np.zeros(len(r), np.uint64)
    nb, ob, bad = ctypes.c_uint64(99), ctypes.c_uint64(99), ctypes.c_uint32(99)
    rc = gh.lib().gh_pgather_plan(arr, n, None, r.ctypes.data, len(r), br.ctypes.data if cap else None, cap,
                                  ctypes.byref(nb), so.ctypes.data, do.ctypes.data, ctypes.byref(ob), ctypes.byref(bad))
    return rc, nb.value, ob.value, bad.value


def test_refusals_zero_the_counts(gh):
    nt = len(SHAPES)
    for bad in [(nt, 0, 0), (0, 5, 4), (0, 0, SHAPES[0][0] + 1)]:
        rc, nb, ob, nbad = _rc_plan(gh, ITEMS, [(0, 0, 10), bad, (1, 0, 1)])
        assert rc == GH_E_ARG and (nb, ob, nbad) == (0, 0, 0), bad
    assert _rc_plan(gh, ITEMS, [(0, 0, SHAPES[0][0])])[0] == GH_OK  # hi == nelem is the last valid one
    assert _rc_plan(gh, [(0, 10, 3, 1)], [(0, 0, 1)])[0] == GH_E_ARG  # what gh_planes_layout refuses
    assert _rc_plan(gh, [(0, 1 << 39, 2, 2)], [(0, 0, 1)])[0] == GH_E_ARG  # a tensor of 2^40 bytes


def test_flagged_stream_counts_per_element_range(gh):
    per, ns = _streams()
    t = next(t for t, s in enumerate(SHAPES) if s[2] == 0b1111)  # four coded planes, one flagged
    status = np.zeros(ns, dtype=np.uint32)
    status[per[t][2]] = 1
    ranges = [(t, 0, 100), (0, 0, 5), (t, 7, 7), (t, 2000, 2049), (2, 0, 1024)]
    br, so, do, ob, bad = gh.planes_gather_plan(ITEMS, ranges, status)
    wbr, wso, wdo, wob, wbad = _naive(ranges, status)
    assert bad == wbad == 3  # per element range, not per plane; an empty range counts as the batched gather's does
    assert br.tolist() == [list(x) for x in wbr] and so.tolist() == wso and do.tolist() == wdo and ob == wob


def test_sizing_call(gh):
    ranges = _ranges()
    want = len(_naive(ranges)[0])
    rc, nb, ob, bad = _rc_plan(gh, ITEMS, ranges, cap=0)
    assert rc == GH_E_SMALL and nb == want and ob == _naive(ranges)[3]
    assert _rc_plan(gh, ITEMS, ranges, cap=want)[0] == GH_OK
    assert _rc_plan(gh, ITEMS, ranges, cap=want - 1)[0] == GH_E_SMALL
