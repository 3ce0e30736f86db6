"""Inputs, cuts and checks shared by tests/test_encode_slices.py (host) and
tests/test_gpu_encode_slices.py (device): the sliced-encode matrix.

A case is an input and a list of cut points 0 = b[0] <= b[1] <= ... <= b[K] = n; slice i is
data[b[i]:b[i + 1]] at base_bit = the code bits of data[:b[i]] under the whole input's plan.
"""
import functools

import numpy as np

INPUTS = ("gen", "two", "flat", "long")


@functools.lru_cache(maxsize=None)
def _input(gh, name):
    if name == "gen":  # generated, r = 0.5
        data = gh.generate(31, 0.5, 200_000)
    elif name == "two":  # two symbols: 1-bit codes
        data = np.random.default_rng(5).integers(0, 2, 50_001).astype(np.uint8) + 48
    elif name == "flat":  # every byte value equally often: 8-bit codes
        data = np.random.default_rng(6).permutation(np.tile(np.arange(256, dtype=np.uint8), 64))
    elif name == "long":  # tests/test_gpu_encode.py::test_long_codes_and_all_gap_values: 16-bit codes
        data = np.minimum(np.random.default_rng(11).geometric(0.45, 2_000_000) - 1, 255).astype(np.uint8)
    else:
        raise KeyError(name)
    data.setflags(write=False)
    plan = gh.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    start = np.concatenate([[0], np.cumsum(lens[data], dtype=np.uint64)]).astype(np.uint64)  # first bit of byte i
    image = gh.encode(data)
    image.setflags(write=False)
    return data, plan, start, image


def case_input(gh, name):
    """(data, plan, start, image): the input, its plan, every byte's first bit (n + 1
    entries) and the host encoder's image.  Built once; read-only."""
    return _input(gh, name)


def cut_sets(name, n):
    """[(label, bounds)] for input `name` of n bytes."""
    sets = [(f"K{k}", [n * i // k for i in range(k + 1)]) for k in (1, 2, 3, 7, 64)]
    # repeated cut points (empty slices) and 1-byte slices, at both ends and inside
    sets.append(("empty_and_1byte", [0, 0, 1, 1, 2, n // 3, n // 3, n // 3 + 1, n - 1, n, n]))
    if name == "two":  # 3 bits a slice: 40 slices and their seams inside one gap word, ~10 a payload word
        sets.append(("every3", list(range(0, 121, 3)) + [n]))
    if name == "flat":  # 8-bit codes: seams exactly on word (4 B), segment (16 B) and gap-word (128 B) boundaries
        sets.append(("aligned", [0, 4, 8, 16, 32, 128, 256, 260, 384, 1024, 1040, n]))
    return sets


CASES = [(name, label) for name in INPUTS for label in
         ["K1", "K2", "K3", "K7", "K64", "empty_and_1byte"] + {"two": ["every3"], "flat": ["aligned"]}.get(name, [])]


def case_bounds(name, label, n):
    return dict(cut_sets(name, n))[label]


def check_extents_and_edges(gh, s, words, gapw, base_bit, bits):
    """The slice's extents equal gh_slice_extent's, the buffers have those sizes, and in the
    edge words every bit outside [base_bit, base_bit + bits) is zero."""
    want = gh.slice_extent(base_bit, bits)
    for f in ("base_bit", "bits", "word0", "nwords", "gapw0", "ngapw"):
        assert getattr(s, f) == getattr(want, f), f
    end = base_bit + bits
    assert s.word0 == base_bit >> 5 and s.gapw0 == base_bit >> 10
    assert s.nwords == ((end + 31) // 32 - s.word0 if bits else 0)
    assert s.ngapw == (((end - 1) >> 10) + 1 - s.gapw0 if bits else 0)
    assert words.size == s.nwords and gapw.size == s.ngapw
    if not bits:
        return
    # payload: codewords MSB-first, so stream bit p is bit 31 - p % 32 of word p // 32
    lead = base_bit & 31
    assert int(words[0]) >> (32 - lead) == 0 if lead else True
    tail = end & 31
    assert int(words[-1]) & ((1 << (32 - tail)) - 1) == 0 if tail else True
    # gap words: segment j's nibble is nibble j % 8 (LSB first) of word j // 8
    j0, j1 = base_bit >> 7, (end - 1) >> 7
    assert int(gapw[0]) & ((1 << (4 * (j0 & 7))) - 1) == 0
    assert int(gapw[-1]) >> (4 * ((j1 & 7) + 1)) == 0
