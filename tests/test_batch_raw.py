"""Batched gap-less decode without a GPU: the host twin of the raw load's kernels
(gh_batchraw_gaps_host: segment transition functions composed per 256-segment unit, then
chained) against the oracle's gap words and the encoder's own, the new entry points in the
header / EXPORTED / the library, the kernel names, argument refusals and the loud failure
without a device.

The streams are those of tests/test_gpu_batch.py (helpers copied from it): the empty stream,
n = 1, the one-symbol code at 128 / 129, a 1..16-bit ladder at 65 536 (16-bit codewords, gap
15), a grouped 4/8-bit code, a 2..7-bit ladder, generated data at r = 0.1 / 0.5 / 0.9 cut to
G = 255 .. 1025 (unit edges), the uniform golden whose every T_j is the identity, and the
sizes of test_sync's last-codeword crossing.  The r = 0.1 and r = 0.5 streams have T_j whose
image holds more than one value: a reversed composition order fails there."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GH_E_ARG, GH_E_TABLE, GH_E_NODEV, GH_E_SMALL = -1, -3, -5, -9
RAW_NAMES = ("gh_batchraw_load", "gh_batchraw_load_device", "gh_batchraw_gaps", "gh_batchraw_report_get",
             "gh_batchraw_gaps_host", "gh_batchraw_kernel_shape", "gh_batchraw_kernel_shapes")


# ---- prescribed codes (copied from tests/test_gpu_batch.py) -----------------------------
def _ladder(lo, hi, first=1):
    code = {lo: first}
    for l in range(lo + 1, hi):
        code[l] = 1
    left = 1.0 - sum(c * 2.0 ** -l for l, c in code.items())
    code[hi] = round(left * 2 ** hi)
    return code


def _coded(code, n, seed):
    lens = np.asarray([l for l in sorted(code) for _ in range(code[l])])
    vals = ((np.arange(len(lens)) * 37 + 11) % 256).astype(np.uint8)
    if len(lens) == 1:
        return np.repeat(vals, n), dict(zip(vals.tolist(), lens.tolist()))
    assert sum(2.0 ** -l for l in lens) == 1.0
    m, rem = divmod(n, 1 << int(lens.max()))
    assert m >= 1 and rem == 0
    data = np.random.default_rng(seed).permutation(np.repeat(vals, m * (1 << (int(lens.max()) - lens))))
    return data, dict(zip(vals.tolist(), lens.tolist()))


CODES = {
    "ladder_1_16": (_ladder(1, 16), 1 << 16),
    "one_symbol_128": ({1: 1}, 128),
    "one_symbol_129": ({1: 1}, 129),
    "grouped_4_8": ({4: 2, 8: 224}, 1 << 16),
    "ladder_2_7": (_ladder(2, 7, 3), 1 << 16),
}
CUTS = [(r, g) for r in (0.1, 0.5, 0.9) for g in (255, 256, 257, 1023, 1024, 1025)]


def _cut(gh, r, target, seed):
    data = gh.generate(seed, r, 60_000)
    n = data.size
    for _ in range(12):
        img = gh.encode(data[:n])
        s = gh.parse(img)
        if s.g == target:
            return data[:n].copy(), img
        length_of = np.full(256, 16, dtype=np.int64)
        for sym, l in s.symbols:
            length_of[sym] = l
        n = int(np.searchsorted(np.cumsum(length_of[data]), 128 * target, "right"))
    raise AssertionError(f"no cut of r = {r} gives G = {target}")


def _words(s):
    """(gap words, payload words) of a parsed image, copied."""
    nw = (s.g + 7) // 8
    gw = s.raw[s.raw.size - 4 * (nw + s.w): s.raw.size - 4 * s.w].copy().view(np.uint32)
    pw = s.raw[s.raw.size - 4 * s.w:].copy().view(np.uint32)
    return gw, pw


_cache = {}


def _streams(gh):
    if "all" in _cache:
        return _cache["all"]
    out = {"empty": np.zeros(0, dtype=np.uint8), "n1": np.asarray([200], dtype=np.uint8)}
    for name, (code, n) in CODES.items():
        data, want = _coded(code, n, seed=len(name))
        assert dict(gh.parse(gh.encode(data)).symbols) == want
        out[name] = data
    for i, (r, g) in enumerate(CUTS):
        out[f"gen_r{r}_g{g}"] = _cut(gh, r, g, seed=500 + i)[0]
    out["uniform256_exact_segments"] = np.fromfile(os.path.join(GOLDEN, "uniform256_exact_segments.bin"), dtype=np.uint8)
    for n in (200, 270, 290):
        out[f"crossing_{n}"] = gh.generate(11, 0.1, n)
    _cache["all"] = out
    return out


NAMES = (["empty", "n1"] + list(CODES) + [f"gen_r{r}_g{g}" for r, g in CUTS] + ["uniform256_exact_segments"]
         + [f"crossing_{n}" for n in (200, 270, 290)])


@pytest.mark.parametrize("name", NAMES)
def test_host_gaps_equal_oracle_and_encoder(gh, orc, name):
    data = _streams(gh)[name]
    s = gh.parse(gh.encode(data))
    gw, pw = _words(s)
    got = gh.raw_gaps_host(pw, s.symbols)
    assert got.dtype == np.uint32 and np.array_equal(got, gw), name
    assert np.array_equal(got, orc.raw_gaps(data, s.symbols)), name


def _host_T(pw, symbols):
    """T_j of every segment by a plain numpy-free restatement: 16 sequential walks."""
    codes, code = {}, 0
    for i, (sym, l) in enumerate(symbols):
        if i:
            code = (code + 1) << (l - symbols[i - 1][1])
        codes[(l, code)] = sym
    maxlen = max(l for _, l in symbols)
    bits = np.unpackbits(np.asarray(pw, dtype=np.uint32).astype(">u4").view(np.uint8))
    bits = np.concatenate([bits, np.zeros(64, dtype=np.uint8)])
    out = []
    for j in range(-(-len(pw) // 4)):
        t = []
        for x in range(16):
            pos = 128 * j + x
            while pos < 128 * (j + 1):
                c = 0
                for l in range(1, maxlen + 1):
                    c = (c << 1) | int(bits[pos + l - 1])
                    if (l, c) in codes:
                        break
                pos += l
            t.append(pos - 128 * (j + 1))
        out.append(t)
    return out


def test_images_of_transition_functions(gh):
    """What the order of composition rests on: every T_j of the uniform golden is the same
    phase-keeping function (8-bit codewords only: T(x) = x mod 8, the identity on the states a
    stream of 8-bit codewords can reach), while r = 0.1 and r = 0.5 streams hold T_j with more
    than one value (a walk from a wrong state can stay wrong across a segment), so composing
    in the wrong order changes their gap words."""
    st = _streams(gh)
    s = gh.parse(gh.encode(st["uniform256_exact_segments"]))
    assert {l for _, l in s.symbols} == {8}
    assert all(t == [x % 8 for x in range(16)] for t in _host_T(_words(s)[1], s.symbols))
    for name in ("gen_r0.1_g255", "gen_r0.5_g255"):
        s = gh.parse(gh.encode(st[name]))
        ts = _host_T(_words(s)[1][:4 * 64], s.symbols)
        assert max(len(set(t)) for t in ts) > 1, name


def test_arbitrary_words_equal_a_sequential_walk(gh):
    """Words that are no valid stream, under an incomplete code (patterns outside it advance
    maxlen bits) and a complete one: the host twin equals the walk from bit 0."""
    rng = np.random.default_rng(5)
    for symbols in ([(7, 1)], [(1, 2), (2, 3), (3, 3), (4, 5)], [(0, 1), (1, 2), (2, 3), (3, 3)]):
        for w in (0, 1, 3, 4, 5, 1021, 1024, 1027):
            pw = rng.integers(0, 1 << 32, w, dtype=np.uint64).astype(np.uint32)
            codes, code = {}, 0
            for i, (sym, l) in enumerate(symbols):
                if i:
                    code = (code + 1) << (l - symbols[i - 1][1])
                codes[(l, code)] = sym
            maxlen = max(l for _, l in symbols)
            g = -(-w // 4)
            bits = np.concatenate([np.unpackbits(pw.astype(">u4").view(np.uint8)), np.zeros(256, dtype=np.uint8)])
            nib = np.zeros(8 * (-(-g // 8)), dtype=np.uint32)
            pos = 0
            for j in range(1, g):
                while pos < 128 * j:
                    c, step = 0, maxlen
                    for l in range(1, maxlen + 1):
                        c = (c << 1) | int(bits[pos + l - 1])
                        if (l, c) in codes:
                            step = l
                            break
                    pos += step
                nib[j - 1] = pos - 128 * j
            want = np.bitwise_or.reduce(nib.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32)), axis=1) if g else nib
            assert np.array_equal(gh.raw_gaps_host(pw, symbols), want.astype(np.uint32)), (symbols, w)


def test_raw_names_declared_and_exported(gh):
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in RAW_NAMES:
        assert name in declared and name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert {n for n in declared if n.startswith("gh_batchraw_")} == set(RAW_NAMES)
    assert {n for n in gh.EXPORTED if n.startswith("gh_batchraw_")} == set(RAW_NAMES)
    assert re.search(r"\bgh_batchraw_report;", src)
    assert ctypes.sizeof(gh.gh_batchraw_report) == 16
    for attr in ("load_raw", "load_raw_device", "raw_gaps", "raw_report"):
        assert callable(getattr(gh.BatchDecoder, attr))
    assert callable(gh.decode_batch_raw)


def test_raw_kernel_shapes(gh):
    names = gh.batchraw_kernel_shapes()
    assert sorted(names) == ["batchraw<fb=0>", "batchraw<fb=1>"]
    for other in (gh.kernel_shapes(), gh.enc_kernel_shapes(), gh.batch_kernel_shapes(), gh.batchdec_kernel_shapes(),
                  gh.ebatch_kernel_shapes()):
        assert not set(names) & set(other)


def test_refusals(gh):
    L = gh.lib()
    sy = (gh.gh_sym * 2)()
    sy[0].symbol, sy[0].length, sy[1].symbol, sy[1].length = 1, 1, 2, 1
    words = np.zeros(40, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint32)
    P = ctypes.c_void_p
    ok = (ctypes.byref(sy), 2, P(words.ctypes.data), 40, P(out.ctypes.data), 2)
    assert L.gh_batchraw_gaps_host(*ok) == 0
    assert L.gh_batchraw_gaps_host(None, 2, *ok[2:]) == GH_E_ARG
    assert L.gh_batchraw_gaps_host(ok[0], 2, None, 40, ok[4], 2) == GH_E_ARG
    assert L.gh_batchraw_gaps_host(*ok[:4], None, 2) == GH_E_ARG
    assert L.gh_batchraw_gaps_host(*ok[:5], 1) == GH_E_SMALL  # G = 10: two gap words
    assert L.gh_batchraw_gaps_host(None, 0, ok[2], 40, ok[4], 2) == GH_E_TABLE  # segments, no code
    assert L.gh_batchraw_gaps_host(None, 0, None, 0, None, 0) == 0
    sy[1].length = 0
    assert L.gh_batchraw_gaps_host(*ok) == GH_E_TABLE
    # the entry points that take a batch refuse a null one before they touch a device
    n = ctypes.c_uint64(99)
    assert L.gh_batchraw_load(None, None, 0) == GH_E_ARG
    assert L.gh_batchraw_load_device(None, None, 0, None) == GH_E_ARG
    assert L.gh_batchraw_gaps(None, 0, None, 0, ctypes.byref(n)) == GH_E_ARG and n.value == 0
    assert L.gh_batchraw_report_get(None, None) == GH_E_ARG
    assert L.gh_batchraw_kernel_shape(None, None, 0) == GH_E_ARG
    assert L.gh_batchraw_kernel_shapes(None, 0) == GH_E_ARG
    buf = ctypes.create_string_buffer(8)
    assert L.gh_batchraw_kernel_shapes(buf, 8) == GH_E_SMALL


def test_no_gpu_raw_batch_fails_loudly(gh):
    if gh.device_count() > 0:
        pytest.skip("a GPU is visible")
    data = gh.generate(1, 0.5, 1000)
    s = gh.parse(gh.encode(data))
    with pytest.raises(gh.GapHuffError) as e:
        gh.decode_batch_raw([(s.symbols, s.n, _words(s)[1])])
    assert e.value.code == GH_E_NODEV
