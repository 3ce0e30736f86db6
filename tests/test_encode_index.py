"""The seek index from the host encoder: gh_encode_index (CPU, no device).

The expected offsets come from the data, as in test_gpu_index: with bits[i] the code
length of data[i] (from the encoded image's symbol list) and starts = exclusive
cumsum(bits), offsets[k] = number of codewords that start before payload bit
128 * stride * k (searchsorted "left"), then N.

Streams: every golden input; gh_generate at r = 0.0 .. 1.0; the prescribed codes of
test_gpu_index (a 1..16-bit ladder, the one-symbol code, a grouped 4/8-bit code, a
2..7-bit ladder); one stream with G = 256 k + 1; N = 0, 1 and 7.  Strides 2^8, 2^9, 2^12
and 2^20 (one block for all of them)."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENCODER = os.path.join(ROOT, "bin", "encoder")
N_GEN = 300_000
N_CODE = 1 << 18
STRIDES = (8, 9, 12, 20)
GH_E_ARG, GH_E_SMALL = -1, -9


# ---- prescribed codes (the dyadic construction of test_gpu_index) ----------------------
def _ladder(lo, hi, first=1):
    code = {lo: first}
    for l in range(lo + 1, hi):
        code[l] = 1
    left = 1.0 - sum(c * 2.0 ** -l for l, c in code.items())
    code[hi] = round(left * 2 ** hi)
    return code


def _coded(code, n, seed):
    """n bytes whose histogram forces `code` ({length: symbols}): symbol i occurs
    m * 2^(maxlen - len_i) times, shuffled."""
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
    "ladder_1_16": _ladder(1, 16),
    "one_symbol": {1: 1},
    "grouped_4_8": {4: 2, 8: 224},
    "ladder_2_7": _ladder(2, 7, 3),
}
GEN = {"gen_r0.0": 0.0, "gen_r0.1": 0.1, "gen_r0.5": 0.5, "gen_r0.9": 0.9, "gen_r1.0": 1.0}
GOLDENS = tuple(sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.bin"))))
TINY = {"n0": 0, "n1": 1, "n7": 7}
STREAMS = (*GEN, *CODES, *GOLDENS, "g_256k_plus_1", *TINY)

_cache = {}


def _lengths(gh, img):
    length_of = np.zeros(256, dtype=np.int64)
    for sym, l in gh.parse(img).symbols:
        length_of[sym] = l
    return length_of


def _make(gh, name):
    if name in GEN:
        return gh.generate(375 + int(GEN[name] * 10), GEN[name], N_GEN)
    if name in CODES:
        data, want = _coded(CODES[name], N_CODE, seed=len(name))
        assert dict(gh.parse(gh.encode(data)).symbols) == want, "package-merge did not return the prescribed lengths"
        return data
    if name in GOLDENS:
        return np.fromfile(os.path.join(GOLDEN, name + ".bin"), dtype=np.uint8)
    if name in TINY:
        return gh.generate(5, 0.5, TINY[name])
    # G = 256 k + 1: cut a generated stream where its bits fill 256 k + 1 segments
    data = gh.generate(77, 0.5, 100_000)
    bits = _lengths(gh, gh.encode(data))[data]
    g = -(-int(bits.sum()) // 128)
    target = (g - 1) // 256 * 256 + 1
    n = int(np.searchsorted(np.cumsum(bits), 128 * target, "right"))
    data = data[:n].copy()
    assert gh.parse(gh.encode(data)).g == target and target % 256 == 1 and target > 256
    return data


def _expected(gh, data, img, log2_stride):
    s = gh.parse(img)
    bits = _lengths(gh, img)[data]
    assert data.size == s.n and bits.min(initial=1) >= 1
    starts = np.cumsum(bits) - bits
    nblocks = -(-s.g // (1 << log2_stride))
    off = np.searchsorted(starts, 128 * (1 << log2_stride) * np.arange(nblocks, dtype=np.int64), "left")
    return np.append(off, s.n).astype(np.uint64)


@pytest.fixture
def case(gh, request):
    """(name, data, encoded image), made once."""
    name = request.param
    if name not in _cache:
        data = _make(gh, name)
        data.setflags(write=False)
        _cache[name] = (name, data, gh.encode(data))
    return _cache[name]


def test_golden_inputs_are_covered():
    assert len(GOLDENS) >= 10 and "uniform256_exact_segments" in GOLDENS


@pytest.mark.parametrize("case", STREAMS, indirect=True)
def test_encode_index_is_exact(gh, case):
    name, data, img = case
    s = gh.parse(img)
    for k in STRIDES:
        image = gh.encode_index(data, k)
        assert image.size == gh.lib().gh_index_bytes(s.g, k)
        ix = gh.parse_index(image)
        assert (ix.log2_stride, ix.n, ix.g) == (k, s.n, s.g)
        want = _expected(gh, data, img, k)
        assert ix.offsets.size == -(-s.g // (1 << k)) + 1
        assert np.array_equal(ix.offsets, want), (name, k, np.nonzero(ix.offsets != want)[0][:4])
    if s.n == 0:
        assert gh.parse_index(gh.encode_index(data, 8)).offsets.tolist() == [0]


@pytest.mark.parametrize("case", ["gen_r0.5", "ladder_1_16", "one_symbol", "n7"], indirect=True)
def test_threads_and_version_do_not_change_the_image(gh, case):
    name, data, img = case
    for k in (8, 12):
        base = gh.encode_index(data, k, threads=1)
        for t in (2, 7):
            assert np.array_equal(gh.encode_index(data, k, threads=t), base), (name, k, t)
        assert np.array_equal(gh.encode_index(data, k, force_version=2), base)


def test_threads_split_a_large_input(gh):
    """3 MiB + 5: the host encoder gives a thread at least 1 MiB, so `threads` = 2, 3 and 7
    really split this input (bit ranges that begin inside an index block)."""
    data = gh.generate(91, 0.5, 3 * (1 << 20) + 5)
    img = gh.encode(data)
    for k in (8, 10):
        want = _expected(gh, data, img, k)
        for t in (1, 2, 3, 7):
            got = gh.parse_index(gh.encode_index(data, k, threads=t)).offsets
            assert np.array_equal(got, want), (k, t)


@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_refusals(gh, case):
    name, data, img = case
    L = gh.lib()
    plan = gh.encode_plan(data)
    need = int(L.gh_index_bytes(plan.g, 8))
    buf = np.zeros(need, dtype=np.uint8)
    import ctypes
    p, b = ctypes.byref(plan), buf.ctypes.data
    for k in (7, 21):
        assert L.gh_encode_index(data.ctypes.data, p, k, 1, b, buf.size) == GH_E_ARG
        with pytest.raises(gh.GapHuffError) as e:
            gh.encode_index(data, k)
        assert e.value.code == GH_E_ARG
    assert L.gh_encode_index(data.ctypes.data, p, 8, 1, b, need - 1) == GH_E_SMALL
    assert L.gh_encode_index(None, p, 8, 1, b, need) == GH_E_ARG
    assert L.gh_encode_index(data.ctypes.data, None, 8, 1, b, need) == GH_E_ARG
    assert L.gh_encode_index(data.ctypes.data, p, 8, 1, None, need) == GH_E_ARG
    # an input that does not match the plan: the rarest symbol (the longest codeword)
    # replaced by the most frequent one, so the bit total differs
    other = data.copy()
    other[other == plan.syms[plan.nsyms - 1].symbol] = plan.syms[0].symbol
    assert plan.len[plan.syms[plan.nsyms - 1].symbol] > plan.len[plan.syms[0].symbol]
    assert L.gh_encode_index(other.ctypes.data, p, 8, 1, b, need) == GH_E_ARG
    assert L.gh_encode_index(data.ctypes.data, p, 8, 1, b, need) == 0
    assert np.array_equal(buf, gh.encode_index(data, 8))


# ---- the CLI ------------------------------------------------------------------------------
def _run(*args):
    return subprocess.run([ENCODER, *map(str, args)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("case", ["gen_r0.5", "n0"], indirect=True)
def test_cli_write_index(gh, case, tmp_path):
    name, data, img = case
    src, plain, out, idx = (tmp_path / f for f in ("in.bin", "plain.huff", "out.huff", "out.ghidx"))
    data.tofile(src)
    r0 = _run(src, plain)
    assert r0.returncode == 0, r0.stderr
    r = _run(src, out, "--write-index", idx, "--index-stride", 9)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), np.fromfile(plain, dtype=np.uint8))
    assert np.array_equal(np.fromfile(out, dtype=np.uint8), img)
    want = gh.encode_index(data, 9)
    assert np.array_equal(np.fromfile(idx, dtype=np.uint8), want)
    # the existing lines stay (timings differ), one line is added
    heads = [l.split(":")[0] for l in r0.stdout.splitlines()]
    assert [l.split(":")[0] for l in r.stdout.splitlines()] == heads + ["Index"]
    assert f"Index: {(want.size - 40) // 8} entries, stride 2^9, {want.size} bytes" in r.stdout
    # the default stride is 2^8; --raw writes the same index
    for extra in ((), ("--raw",)):
        r = _run(src, out, "--write-index", idx, *extra)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(idx, dtype=np.uint8), gh.encode_index(data, 8))


@pytest.mark.parametrize("case", ["gen_r0.5"], indirect=True)
def test_cli_bad_stride(gh, case, tmp_path):
    name, data, img = case
    data.tofile(tmp_path / "in.bin")
    for k in (7, 21):
        r = _run(tmp_path / "in.bin", tmp_path / "out.huff", "--write-index", tmp_path / "x.ghidx", "--index-stride", k)
        assert r.returncode != 0
        assert "stride" in r.stderr
