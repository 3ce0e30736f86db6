"""Gap-array images under code tables the encoder never writes: shared by
tests/test_foreign_codes.py (host) and tests/test_gpu_foreign_codes.py (device).

gh_stream_parse accepts any canonical table of 1..16-bit codewords with Kraft sum <= 1, but
gh.encode only ever writes the package-merge code of the data's own histogram: complete (bar
the one-symbol code), with symbol frequencies near 2^-length.  The images here are assembled
from a *given* table and *given* data with the oracle's raw-stream restatement
(oracle.raw_encode / raw_gaps; tests/test_sync.py pins a gap-array file's payload and gap
words to them), so a table may be incomplete, may hold symbols the data never uses, and the
data may sit almost entirely on the table's longest or shortest codeword.

A case is (code, profile) or an edge case of EDGE; case() builds it once and keeps it
read-only.  The oracle stays the only reference: nothing here decodes.
"""
import collections

import numpy as np

PROFILES = ("uniform", "long", "short")  # over the table; 95 % the last symbol; 95 % the first

# name: ({length: codewords}, or None for the generated lists; n).  n is odd-sized so that G is
# no multiple of 256, and large enough for several tiles of the tile kernels where those run.
_CODES = {
    "k3": ({2: 3}, (1 << 17) + 3),                          # smallest multi-symbol hole ('11')
    "flat8_200": ({8: 200}, 70_001),                        # incomplete, within every table
    "holes16": ({2: 2, 5: 3, 9: 1, 16: 2}, 70_001),         # empty lengths, 16-bit codewords, a hole
    "one_and_16": ({1: 1, 16: 1}, 70_001),                  # a 1-bit codeword, half the code space unused
    "lengthened_0": (None, 70_001),                         # package-merge lengths, the last three lengthened
    "lengthened_1": (None, 70_001),
    "lengthened_2": (None, 70_001),
    "cfg4like": ({5: 4, 8: 196, 9: 56}, 200_003),           # a grouped tile code on data it was not made for
    "minlen3": ({3: 4, 8: 120, 12: 128}, 200_003),          # the tile kernel's minlen-3 shape likewise
    # 1..15, 16, 16: the two-pass fallback; 8 or 128 symbols per segment by profile
    "ladder_1_16": ({**{l: 1 for l in range(1, 16)}, 16: 2}, (1 << 18) - 5),
    "unused_syms": ({8: 256}, 70_001),                      # the data holds two of the table's 256 symbols
}
CODES = tuple(_CODES)
INCOMPLETE = ("k3", "flat8_200", "holes16", "one_and_16", "lengthened_0", "lengthened_1", "lengthened_2")
COMPLETE = tuple(c for c in CODES if c not in INCOMPLETE)
CASES = [(c, p) for c in CODES for p in PROFILES]
# G = 255, 256, 257 (the edges of a 256-segment work unit and index block) under incomplete
# codes of fixed-length codewords, where n fixes G: id -> (code, profile, n)
EDGE = {
    "k3_g255": ("k3", "uniform", 64 * 255 - 3),
    "k3_g256": ("k3", "uniform", 64 * 256),
    "k3_g257": ("k3", "uniform", 64 * 256 + 1),
    "flat8_200_g257": ("flat8_200", "uniform", 16 * 256 + 1),
}

Case = collections.namedtuple("Case", "symbols data image")
_cache = {}


def kraft(symbols):
    """Kraft sum of a (symbol, length) list on a 2^16 scale (65536: complete)."""
    return sum(1 << (16 - l) for _, l in symbols)


def _lengthened(orc, seed):
    """_random_code of tests/test_sync.py with its lengthening forced: package-merge lengths
    of random counts, the last three one bit longer (16 at most), redrawn until that left the
    code incomplete."""
    rng = np.random.default_rng(seed)
    while True:
        ns = int(rng.integers(2, 257))
        counts = np.sort(rng.geometric(rng.uniform(0.01, 0.5), ns).astype(np.uint64) *
                         rng.integers(1, 1000, ns).astype(np.uint64))
        lens = sorted(orc.package_merge(counts))
        for i in range(len(lens) - 1, max(-1, len(lens) - 4), -1):
            lens[i] = min(16, lens[i] + 1)
        lens = sorted(lens)
        if sum(1 << (16 - l) for l in lens) < 65536:
            return lens


def symbols(orc, code):
    """The canonical (symbol, length) list of `code`: lengths ascending, the byte values a
    seeded permutation of 0..255 (so neighbouring codewords do not carry neighbouring bytes)."""
    key = ("symbols", code)
    if key not in _cache:
        spec = _CODES[code][0]
        if spec is None:
            lens = _lengthened(orc, 7000 + int(code[-1]))
        else:
            lens = [l for l in sorted(spec) for _ in range(spec[l])]
        vals = np.random.default_rng(CODES.index(code)).permutation(256)[: len(lens)]
        _cache[key] = [(int(v), int(l)) for v, l in zip(vals, lens)]
    return list(_cache[key])


def profile_data(code, syms, profile, n):
    """n bytes over the table of `syms`: uniform, or 95 % the table's last (longest) / first
    (shortest) symbol and the rest uniform.  unused_syms draws from the table's first and last
    symbol only."""
    vals = np.asarray([s for s, _ in syms], dtype=np.uint8)
    if code == "unused_syms":
        vals = vals[[0, -1]]
    rng = np.random.default_rng([CODES.index(code), PROFILES.index(profile), n])
    data = vals[rng.integers(0, vals.size, n)]
    if profile != "uniform":
        data[rng.random(n) < 0.95] = vals[-1 if profile == "long" else 0]
    return data


def image(orc, syms, data):
    """The gap-array file (v1 header: u64 S, S x (symbol, length), u32 N, W, G; ceil(G / 8)
    gap words; W payload words) of `data` under the canonical list `syms`."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    units = orc.raw_encode(data, syms)
    gaps = orc.raw_gaps(data, syms)
    w = int(units.size)
    g = -(-w // 4)
    assert gaps.size == -(-g // 8) and data.size < 1 << 32
    return np.concatenate([
        np.asarray([len(syms)], dtype="<u8").view(np.uint8),
        np.asarray(syms, dtype=np.uint8).reshape(-1),
        np.asarray([data.size, w, g], dtype="<u4").view(np.uint8),
        gaps.astype("<u4").view(np.uint8),
        units.astype("<u4").view(np.uint8),
    ])


def split(img):
    """(symbols, n, gap words, payload words) of a v1 image, parsed here."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    s = int(img[:8].view("<u8")[0])
    syms = [(int(a), int(b)) for a, b in img[8: 8 + 2 * s].reshape(-1, 2)]
    n, w, g = (int(x) for x in img[8 + 2 * s: 20 + 2 * s].view("<u4"))
    at = 20 + 2 * s
    gw = -(-g // 8)
    assert img.size == at + 4 * (gw + w)
    return syms, n, img[at: at + 4 * gw].copy().view("<u4"), img[at + 4 * gw:].copy().view("<u4")


def case(orc, code, profile="uniform", n=None):
    """Case(symbols, data, image) of one (code, profile), or of an EDGE id; built once."""
    if code in EDGE:
        code, profile, n = EDGE[code]
    n = _CODES[code][1] if n is None else n
    key = (code, profile, n)
    if key not in _cache:
        syms = symbols(orc, code)
        data = profile_data(code, syms, profile, n)
        img = image(orc, syms, data)
        data.setflags(write=False)
        img.setflags(write=False)
        _cache[key] = Case(syms, data, img)
    return _cache[key]


def damage(img, syms, data):
    """(the image with one kept codeword overwritten by ones, that codeword's index): the
    first codeword from the middle of the stream on whose all-ones pattern, whatever follows
    it, no lookup can match: no codeword is a prefix of the pattern and the pattern is a prefix
    of none.  Such a codeword exists only under an incomplete code (a complete one ends in
    the all-ones codeword).  The header, the gap words and every other payload bit stay."""
    from oracle import canonical_codes
    length_of = np.zeros(256, dtype=np.int64)
    ok = np.zeros(256, dtype=bool)
    codes = canonical_codes(syms)
    for s, l in syms:
        length_of[s] = l
        ok[s] = all(c != (1 << k) - 1 if k <= l else c >> (k - l) != (1 << l) - 1 for (_, k), c in zip(syms, codes))
    data = np.asarray(data)
    bits = length_of[data]
    assert bits.all()
    mid = data.size // 2
    i = mid + int(np.flatnonzero(ok[data[mid:]])[0])
    lo = int(bits[:i].sum())
    parsed, n, gaps, pay = split(img)
    assert parsed == list(syms) and n == data.size
    for p in range(lo, lo + int(bits[i])):
        pay[p >> 5] |= np.uint32(1 << (31 - (p & 31)))
    out = np.array(img, dtype=np.uint8)
    out[out.size - 4 * pay.size:] = pay.view(np.uint8)
    return out, i
