"""The level-by-level package-merge (gh_package_merge_flat, csrc/gh_pm_flat.hpp) against the
lazily evaluated one (gh_package_merge): the same lengths for every input.  No device.

The flat form is what the batched encoder's code kernel runs per stream; its claim is that
"package first on ties" with every list cut to 2n - 2 items reproduces the reference's
tie-breaking.  The cases: every multiset of 2 to 6 counts from 1..7 (all small tie patterns),
all-equal counts at n = 1, 2, 3, 255, 256, Fibonacci counts over 17, 20 and 40 symbols and
powers of two over 17 and 64 symbols (the 16-bit limit binds), 256 counts of 1 under one count
of 2^40, and 3 000 seeded random histograms of five kinds.  Counts stay below 2^42: a package
weighs at most 2^15 times the largest count, so no u64 weight wraps in either form."""
import ctypes
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GH_E_ARG = -1
NAMES = ("gh_package_merge_flat", "gh_batchenc_plan_device", "gh_batchenc_plan_times")


def _same(gh, counts):
    c = sorted(int(x) for x in counts)
    want = gh.package_merge(c)
    got = gh.package_merge_flat(c)
    assert got == want, (c, got, want)
    return got


def test_names_declared_and_exported(gh):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaphuff.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gh_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(gh.LIB_PATH)
    for name in NAMES:
        assert name in declared and name in gh.EXPORTED and hasattr(lib, name), name
        assert getattr(gh.lib(), name).argtypes is not None, name
    assert ctypes.sizeof(gh.gh_ebatch_report) == 40


def test_small_multisets(gh):
    cases = 0
    for n in range(2, 7):
        for c in itertools.combinations_with_replacement(range(1, 8), n):
            _same(gh, c)
            cases += 1
    assert cases == 28 + 84 + 210 + 462 + 924


def test_equal_counts(gh):
    for n in (1, 2, 3, 255, 256):
        for v in (1, 4, 1 << 33):
            got = _same(gh, [v] * n)
            assert len(got) == n
    assert gh.package_merge_flat([7]) == [1]
    assert gh.package_merge_flat([]) == []
    assert _same(gh, [4] * 256) == [8] * 256


def test_length_limit_binds(gh):
    for n in (17, 20, 40):
        fib = [1, 1]
        while len(fib) < n:
            fib.append(fib[-1] + fib[-2])
        got = _same(gh, fib)
        assert max(got) == 16  # (an unlimited Huffman code would reach n - 1 bits)
    for n in (17, 64):
        got = _same(gh, [1 << (i % 41) for i in range(n)])
        assert max(got) == 16
    assert max(_same(gh, [1 << i for i in range(17)])) == 16
    _same(gh, [1] * 256)
    got = _same(gh, [1] * 255 + [1 << 40])
    assert got[-1] == 1


def _random_counts(rng, kind, n):
    if kind == 0:
        return rng.integers(1, 1 << 20, n)
    if kind == 1:  # tiny counts: many ties
        return rng.integers(1, 4, n)
    if kind == 2:  # geometric: the 16-bit limit binds
        return np.maximum(1, (float(rng.uniform(1.2, 2.0)) ** np.minimum(np.arange(n), 40) * rng.uniform(0.5, 1.5, n))).astype(np.uint64)
    if kind == 3:  # powers of two
        return np.uint64(1) << rng.integers(0, 40, n).astype(np.uint64)
    return np.maximum(1, rng.exponential(float(rng.uniform(1, 5000)), n)).astype(np.uint64)


def test_random_histograms(gh):
    rng = np.random.default_rng(20261020)
    for i in range(3000):
        n = int(rng.integers(2, 257)) if i % 10 else 256
        got = _same(gh, _random_counts(rng, i % 5, n))
        assert sum(2.0 ** -l for l in got) == 1.0  # a complete code


def test_refusals(gh):
    L = gh.lib()
    out = np.zeros(512, dtype=np.uint8)
    c = np.ones(512, dtype=np.uint64)
    for fn in (L.gh_package_merge, L.gh_package_merge_flat):
        assert fn(c.ctypes.data, 2, None) == GH_E_ARG
        assert fn(None, 2, out.ctypes.data) == GH_E_ARG
        assert fn(c.ctypes.data, 257, out.ctypes.data) == GH_E_ARG
        assert fn(None, 0, out.ctypes.data) == 0
        assert fn(c.ctypes.data, 256, out.ctypes.data) == 0
