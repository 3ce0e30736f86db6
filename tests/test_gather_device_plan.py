"""gh_gather_piece_bound, the size of a device-planned gather's piece buffer, on the CPU.

The bound, 2 * nranges + dst_len / (8 * stride), must hold for every batch over the index
of a real stream when dst_len is exactly the batch's bytes (gh_gather_plan / Index.plan
counts the pieces), and it must be tight: a hand-built index whose every block holds
exactly 8 * stride symbols, with ranges that start one byte before a block boundary, meets
it.  Indexes are computed from the data as in tests/test_gather_plan.py."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDENS = ("gen_r0.9_n1", "gen_r0.5_n7", "uniform256_exact_segments")
STRIDES = (8, 10, 12)
N_GEN = 300_000
N_CODE = 1 << 18


def _image(offsets, g, log2_stride):
    off = np.asarray(offsets, dtype="<u8")
    hdr = np.asarray([0x0000315844494847, log2_stride, off[-1], g, off.size], dtype="<u8")
    return np.concatenate([hdr, off]).view(np.uint8)


def _ladder_1_16_data():
    """Bytes whose histogram forces a 1..16-bit ladder code (tests/test_gpu_gather.py)."""
    code = {1: 1, **{l: 1 for l in range(2, 16)}}
    code[16] = round((1.0 - sum(c * 2.0 ** -l for l, c in code.items())) * 2 ** 16)
    lens = np.asarray([l for l in sorted(code) for _ in range(code[l])])
    vals = ((np.arange(len(lens)) * 37 + 11) % 256).astype(np.uint8)
    m = N_CODE >> 16
    return np.random.default_rng(11).permutation(np.repeat(vals, m * (1 << (16 - lens)))), dict(
        zip(vals.tolist(), lens.tolist()))


def _offsets(gh, data, img, log2_stride):
    s = gh.parse(img)
    length_of = np.zeros(256, dtype=np.int64)
    for sym, l in s.symbols:
        length_of[sym] = l
    bits = length_of[data]
    starts = np.cumsum(bits) - bits
    nblocks = -(-s.g // (1 << log2_stride))
    off = np.searchsorted(starts, 128 * (1 << log2_stride) * np.arange(nblocks, dtype=np.int64), "left")
    return np.append(off, s.n), s.g


@pytest.fixture(scope="module")
def streams(gh):
    """(name, data, image) of every stream."""
    out = [(f"gen_r{r}", d, gh.encode(d)) for r in (0.1, 0.5, 0.9) for d in [gh.generate(375 + int(r * 10), r, N_GEN)]]
    data, want = _ladder_1_16_data()
    img = gh.encode(data)
    assert dict(gh.parse(img).symbols) == want, "package-merge did not return the prescribed lengths"
    out.append(("ladder_1_16", data, img))
    for name in GOLDENS:
        out.append((name, np.fromfile(os.path.join(GOLDEN, name + ".bin"), dtype=np.uint8),
                    np.fromfile(os.path.join(GOLDEN, name + ".huff"), dtype=np.uint8)))
    return out


def _batches(rng, off, n):
    """Random batches; ranges a byte either side of entries; the whole stream; empty ones."""
    ent = [int(v) for v in off]
    for _ in range(6):
        nr = int(rng.integers(1, 60))
        lo = rng.integers(0, n + 1, size=nr)
        ln = rng.integers(0, int(rng.choice([3, 5000, n + 1])), size=nr)
        yield [(int(a), int(min(a + b, n))) for a, b in zip(lo, ln)]
    edge = [(0, n), (0, 0), (n, n)]
    for e in ent:
        for v in (e - 1, e, e + 1):
            if 0 <= v <= n:
                edge += [(v, min(v + 1, n)), (max(v - 1, 0), min(v + 1, n))]
    # one byte before an entry to one byte past a later one
    for i in range(len(ent) - 1):
        j = min(i + 1 + int(rng.integers(0, 4)), len(ent) - 1)
        if ent[i] >= 1:
            edge.append((ent[i] - 1, min(ent[j] + 1, n)))
    yield edge
    for r in edge[:40]:
        yield [r]


def test_bound_holds_for_real_streams(gh, streams):
    rng = np.random.default_rng(5)
    checked = 0
    for name, data, img in streams:
        for k in STRIDES:
            off, g = _offsets(gh, data, img, k)
            ix = gh.parse_index(_image(off, g, k))
            for ranges in _batches(rng, off, ix.n):
                pieces, total = ix.plan(ranges)
                assert total == sum(hi - lo for lo, hi in ranges)
                bound = gh.gather_piece_bound(len(ranges), total, k)  # dst_len: exactly the batch's bytes
                assert bound == 2 * len(ranges) + total // (8 << k)
                assert pieces.size <= bound, (name, k, len(ranges), total, pieces.size, bound)
                checked += 1
    assert checked > 500


@pytest.mark.parametrize("k", STRIDES)
def test_bound_is_tight(gh, k):
    """Every block holds exactly 8 * stride symbols; each range runs from one byte before a
    block boundary over j whole blocks to one byte past another: j + 2 pieces, j * 8 *
    stride + 2 bytes."""
    stride, nblocks = 1 << k, 40
    per = 8 * stride
    off = per * np.arange(nblocks + 1, dtype=np.int64)
    ix = gh.parse_index(_image(off, nblocks * stride, k))
    rng = np.random.default_rng(k)
    for nr in (1, 7, 100):
        a = rng.integers(1, nblocks - 6, size=nr)
        j = rng.integers(0, 6, size=nr)
        ranges = [(int(off[x]) - 1, int(off[x + y]) + 1) for x, y in zip(a, j)]
        pieces, total = ix.plan(ranges)
        assert pieces.size == int((j + 2).sum()) and total == int(j.sum()) * per + 2 * nr
        bound = gh.gather_piece_bound(nr, total, k)
        assert 0 <= bound - pieces.size <= 2, (nr, pieces.size, bound)
    # a whole-stream read of it: nblocks pieces, bound nblocks + 2
    pieces, total = ix.plan([(0, ix.n)])
    assert pieces.size == nblocks and gh.gather_piece_bound(1, total, k) == nblocks + 2


def test_bound_monotone_and_stride_range(gh):
    rng = np.random.default_rng(9)
    for k in range(8, 21):
        nr = np.sort(rng.integers(0, 1 << 24, size=20))
        dl = np.sort(rng.integers(0, 1 << 40, size=20))
        b = [gh.gather_piece_bound(int(a), int(d), k) for a, d in zip(nr, dl)]
        assert all(x <= y for x, y in zip(b, b[1:]))
        assert gh.gather_piece_bound(5, 1 << 30, k) <= gh.gather_piece_bound(6, 1 << 30, k)
        assert gh.gather_piece_bound(5, 1 << 30, k) <= gh.gather_piece_bound(5, (1 << 30) + (8 << k), k)
        assert gh.gather_piece_bound(0, 0, k) == 0
        if k < 20:  # a larger stride never needs more pieces
            assert gh.gather_piece_bound(5, 1 << 30, k + 1) <= gh.gather_piece_bound(5, 1 << 30, k)
    for k in (0, 7, 21, 64, 0xFFFFFFFF):
        assert gh.gather_piece_bound(1000, 1 << 30, k) == 0
    assert gh.gather_piece_bound(0xFFFFFFFF, (1 << 64) - 1, 8) == 2 * 0xFFFFFFFF + (((1 << 64) - 1) >> 11)


def test_struct_and_exports(gh):
    assert ctypes.sizeof(gh.gh_gather_report) == 24
    assert {"gh_ctx_set_index", "gh_gather_piece_bound", "gh_ctx_gather_device", "gh_ctx_gather_wait",
            "gh_ctx_gather_pieces"} <= set(gh.EXPORTED)
    assert gh.GH_GATHER_MAX_RANGES >= 1 << 20
