"""The seek index of a sliced stream on the host: gh_index_slice_extent,
gh_encode_index_slice, gh_index_image_init, gh_index_slice_merge (CPU, no device).

The ownership rule (include/gaphuff.h, "the index of a sliced stream"), restated in numpy:
with S = 128 << log2_stride and start[i] the first bit of byte i under the stream's plan, the
slice of bytes [lo, hi) holds bits [start[lo], start[hi]) and owns the entries k with
start[lo] <= S * k < start[hi]; entry k = lo + the number of i in [lo, hi) with start[i] <
S * k (searchsorted "left" over start[lo:hi]).  Over the slices of a stream the k0 values
chain, the nk values sum to nblocks, and the entries merged in any order are
gh_encode_index's image byte for byte.
"""
import ctypes
import functools

import numpy as np
import pytest

import slice_cases as sc
from test_encode_index import _expected

GH_E_ARG, GH_E_FORMAT, GH_E_TABLE, GH_E_SMALL = -1, -2, -3, -9


def S_of(k):
    return 128 << k


def owned(start, lo, hi, sym_base, k):
    """(k0, entries) of the slice whose bytes' first bits are start[lo:hi] and whose end bit is
    start[hi]: the numpy statement of the ownership rule.  `start`: np.uint64, first bits."""
    S = S_of(k)
    b0, b1 = int(start[lo]), int(start[hi])
    k0, k1 = -(-b0 // S), -(-b1 // S)
    bounds = np.asarray([S * j for j in range(k0, k1)], dtype=np.uint64)
    cnt = np.searchsorted(start[lo:hi], bounds, "left").astype(np.uint64)
    return k0, cnt + np.uint64(sym_base)


@functools.lru_cache(maxsize=None)
def whole_index(gh, name, k):
    img = gh.encode_index(sc.case_input(gh, name)[0], k)
    img.setflags(write=False)
    return img


def slices_of(gh, data, plan, start, bounds, k, threads=0):
    """[(entries, k0)] of every slice, checked against the numpy statement, the chain and
    the sum."""
    parts, nxt = [], 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        base, bits = int(start[lo]), int(start[hi] - start[lo])
        ent, k0 = gh.encode_index_slice(data[lo:hi], plan, base, lo, k, threads)
        assert (k0, ent.size) == gh.index_slice_extent(base, bits, k)
        wk0, want = owned(start, lo, hi, lo, k)
        assert k0 == wk0 == nxt, (lo, hi, k0, wk0, nxt)  # the k0 values chain
        assert np.array_equal(ent, want), (lo, hi, ent[:4], want[:4])
        nxt = k0 + ent.size
        parts.append((ent, k0))
    assert nxt == -(-plan.g // (1 << k))  # the nk values sum to nblocks
    return parts


def merged_shuffled(gh, plan, k, parts, seed):
    order = np.random.default_rng(seed).permutation(len(parts))
    return gh.merge_index_slices(plan, k, [parts[i] for i in order])


# ---- 1. the full matrix
@pytest.mark.parametrize("k", [8, 9])
@pytest.mark.parametrize("name,label", sc.CASES)
def test_slices_merge_to_the_whole_index(gh, name, label, k):
    data, plan, start, image = sc.case_input(gh, name)
    b = sc.case_bounds(name, label, data.size)
    parts = slices_of(gh, data, plan, start, b, k)
    img = merged_shuffled(gh, plan, k, parts, len(b) + k)
    assert np.array_equal(img, whole_index(gh, name, k))
    assert gh.parse_index(img).offsets.size == -(-plan.g // (1 << k)) + 1


# ---- 2. seams on boundaries
def test_seams_on_boundaries(gh):
    data, plan, start, image = sc.case_input(gh, "flat")
    assert set(bytes(plan.len)) == {8}  # 8-bit codes: at stride 2^8 a boundary every 4096 bytes
    n = data.size
    b = [0, 4096, 4096, 4097, 8191, 8192, 12304, n]
    parts = slices_of(gh, data, plan, start, b, 8)
    got = [(k0, ent.tolist()) for ent, k0 in parts]
    assert got[0] == (0, [0])          # [0, 4096): ends on boundary 1, which it does not own
    assert got[1] == (1, [])           # the empty slice on the boundary owns nothing
    assert got[2] == (1, [4096])       # the 1-byte slice owns it, with count 0
    assert got[3] == (2, [])
    assert got[4] == (2, [])           # [8191, 8192) ends on boundary 2
    assert got[5] == (2, [8192, 12288])
    assert got[6] == (4, [])           # n = 16384: G = 1024, nblocks = 4
    assert np.array_equal(merged_shuffled(gh, plan, 8, parts, 1), whole_index(gh, "flat", 8))


# ---- 3. boundaries inside codewords
def straddled(gh, k=8, count=6):
    """The first `count` (entry index, off[entry]) of "long" whose boundary lies inside a
    codeword: start[off] > S * entry."""
    data, plan, start, image = sc.case_input(gh, "long")
    off = gh.parse_index(whole_index(gh, "long", k)).offsets[:-1].astype(np.int64)
    ks = [j for j in range(1, off.size) if int(start[off[j]]) > S_of(k) * j][:count]
    assert len(ks) == count
    return ks, [int(off[j]) for j in ks]


@pytest.mark.parametrize("shift", [0, 1])
def test_boundaries_inside_codewords(gh, shift):
    """shift 0: cut at off[k], the straddling codeword is a slice's last and the entry is that
    slice's sym_base + n.  shift 1: cut at off[k] - 1, it is the next slice's first: count 1."""
    data, plan, start, image = sc.case_input(gh, "long")
    ks, offs = straddled(gh)
    b = [0] + [o - shift for o in offs] + [data.size]
    assert b == sorted(b) and len(set(b)) == len(b)
    parts = slices_of(gh, data, plan, start, b, 8)
    for i, (j, o) in enumerate(zip(ks, offs)):
        ent, k0 = parts[i + shift]  # shift 0: the slice that ends at off[k]; 1: the one that starts at off[k] - 1
        if shift == 0:
            assert k0 + ent.size - 1 == j and int(ent[-1]) == b[i + 1] == o  # sym_base + n
        else:
            assert k0 == j and int(ent[0]) == b[i + 1] + 1 == o              # sym_base + 1
    assert np.array_equal(merged_shuffled(gh, plan, 8, parts, 2 + shift), whole_index(gh, "long", 8))


# ---- 4. 64-bit origins without large data
def big_origin_case(gh):
    """(data, plan, base_bit, sym_base, local start): a 20 000-byte slice far into a stream
    of more than 2^33 bits (the plan of the slice's histogram, scaled)."""
    data = gh.generate(77, 0.5, 20_000)
    plan = gh.plan_from_counts(np.bincount(data, minlength=256).astype(np.uint64) << np.uint64(20))
    assert plan.bits > 1 << 33
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    base, sym = (1 << 32) + 12345, (1 << 33) + 7
    start = np.concatenate([[0], np.cumsum(lens[data], dtype=np.uint64)]).astype(np.uint64) + np.uint64(base)
    return data, plan, base, sym, start


def test_origins_past_2_32(gh):
    data, plan, base, sym, start = big_origin_case(gh)
    for k in (8, 9):
        ent, k0 = gh.encode_index_slice(data, plan, base, sym, k)
        wk0, want = owned(start, 0, data.size, sym, k)
        assert k0 == wk0 and ent.size == want.size and (k, ent.size) != (8, 0)
        assert np.array_equal(ent, want)
        assert int(ent.min(initial=sym)) >= sym


def test_entries_do_not_depend_on_threads(gh):
    """3 MiB: the host walk gives a thread at least 1 MiB, so 2, 3 and 7 threads really split
    the slice (bit ranges that begin inside an index block)."""
    data = gh.generate(91, 0.5, 3 * (1 << 20) + 5)
    plan = gh.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    lo = 5
    base = int(lens[data[:lo]].sum())
    want = gh.encode_index_slice(data[lo:], plan, base, lo, 8, threads=1)
    whole = gh.parse_index(gh.encode_index(data, 8)).offsets
    assert np.array_equal(want[0], whole[want[1]:-1])
    for t in (2, 3, 7):
        got = gh.encode_index_slice(data[lo:], plan, base, lo, 8, threads=t)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), t


# ---- 5. refusals
def test_refusals(gh):
    data, plan, start, image = sc.case_input(gh, "gen")
    L = gh.lib()
    p = ctypes.byref(plan)
    lo, hi = 50_000, 150_000
    base, bits = int(start[lo]), int(start[hi] - start[lo])
    sl = np.ascontiguousarray(data[lo:hi])
    k0, nk = ctypes.c_uint64(), ctypes.c_uint64()
    args = lambda k=8, b=base: (sl.ctypes.data, sl.size, p, b, lo, k, 1)  # noqa: E731
    # cap = 0 sizes the buffer
    assert L.gh_encode_index_slice(*args(), None, 0, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_SMALL
    assert (k0.value, nk.value) == gh.index_slice_extent(base, bits, 8) and nk.value > 2
    ent = np.zeros(nk.value, dtype=np.uint64)
    assert L.gh_encode_index_slice(*args(), ent.ctypes.data, nk.value - 1, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_SMALL
    assert not ent.any()
    for k in (7, 21):
        assert L.gh_encode_index_slice(*args(k), ent.ctypes.data, ent.size, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_ARG
        assert L.gh_index_slice_extent(base, bits, k, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_ARG
        assert L.gh_index_image_init(p, k, ent.ctypes.data, 1 << 20) == GH_E_ARG
    assert L.gh_index_slice_extent((1 << 64) - 5, 10, 8, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_ARG
    # the slice ends past the plan's bits
    past = plan.bits - bits + 1
    assert L.gh_encode_index_slice(*args(8, past), ent.ctypes.data, ent.size, ctypes.byref(k0), ctypes.byref(nk)) == GH_E_ARG
    # nulls
    assert L.gh_encode_index_slice(None, sl.size, p, base, lo, 8, 1, ent.ctypes.data, ent.size, ctypes.byref(k0),
                                   ctypes.byref(nk)) == GH_E_ARG
    assert L.gh_encode_index_slice(sl.ctypes.data, sl.size, None, base, lo, 8, 1, ent.ctypes.data, ent.size,
                                   ctypes.byref(k0), ctypes.byref(nk)) == GH_E_ARG
    assert L.gh_encode_index_slice(*args(), ent.ctypes.data, ent.size, None, ctypes.byref(nk)) == GH_E_ARG
    # a byte without a code
    other = gh.encode_plan(data[data != data[lo]])
    assert other.len[int(data[lo])] == 0
    with pytest.raises(gh.GapHuffError) as e:
        gh.encode_index_slice(sl, other, 0, 0, 8)
    assert e.value.code == GH_E_TABLE
    # the real call
    assert L.gh_encode_index_slice(*args(), ent.ctypes.data, ent.size, ctypes.byref(k0), ctypes.byref(nk)) == 0
    assert np.array_equal(ent, owned(start, lo, hi, lo, 8)[1])


def test_merge_refusals_and_the_missing_slice(gh):
    data, plan, start, image = sc.case_input(gh, "gen")
    L = gh.lib()
    b = sc.case_bounds("gen", "K7", data.size)
    parts = slices_of(gh, data, plan, start, b, 8)
    need = int(L.gh_index_bytes(plan.g, 8))
    nblocks = (need - 40) // 8 - 1
    img = np.zeros(need, dtype=np.uint8)
    p = ctypes.byref(plan)
    assert L.gh_index_image_init(p, 8, img.ctypes.data, need - 1) == GH_E_SMALL
    assert L.gh_index_image_init(p, 8, img.ctypes.data, need) == 0
    fresh = img.copy()
    hdr = gh.encode_index(data, 8)
    assert np.array_equal(img[:40], hdr[:40]) and np.array_equal(img[-8:], hdr[-8:]) and not img[40:-8].any()
    ent, k0 = parts[-1]
    assert ent.size >= 2
    # past the image's entries: the terminal entry is nobody's
    assert L.gh_index_slice_merge(img.ctypes.data, need, k0 + 1, ent.size, ent.ctypes.data) == GH_E_ARG
    assert L.gh_index_slice_merge(img.ctypes.data, need, nblocks, 1, ent.ctypes.data) == GH_E_ARG
    assert L.gh_index_slice_merge(img.ctypes.data, need, (1 << 64) - 1, 2, ent.ctypes.data) == GH_E_ARG
    # a too-short image, a header that is none
    assert L.gh_index_slice_merge(img.ctypes.data, need - 1, k0, ent.size, ent.ctypes.data) == GH_E_SMALL
    assert L.gh_index_slice_merge(img.ctypes.data, 39, k0, ent.size, ent.ctypes.data) == GH_E_SMALL
    junk = np.zeros(need, dtype=np.uint8)
    assert L.gh_index_slice_merge(junk.ctypes.data, need, k0, ent.size, ent.ctypes.data) == GH_E_FORMAT
    assert L.gh_index_slice_merge(None, need, k0, ent.size, ent.ctypes.data) == GH_E_ARG
    assert L.gh_index_slice_merge(img.ctypes.data, need, k0, ent.size, None) == GH_E_ARG
    assert np.array_equal(img, fresh)  # no refusal wrote
    assert L.gh_index_slice_merge(img.ctypes.data, need, nblocks, 0, None) == 0  # nothing to store
    # one slice left out: its zeros follow non-zero entries, and the image does not parse
    assert parts[3][0].size >= 1 and parts[3][1] > 0
    with pytest.raises(gh.GapHuffError) as e:
        gh.parse_index(gh.merge_index_slices(plan, 8, parts[:3] + parts[4:]))
    assert e.value.code == GH_E_FORMAT
    assert np.array_equal(gh.merge_index_slices(plan, 8, parts[::-1]), hdr)


def test_stream_from_plan(gh):
    """The header-only stream that Decoder.load_device takes: the plan's sizes and code."""
    data, plan, start, image = sc.case_input(gh, "gen")
    s, want = gh.Stream.from_plan(plan), gh.parse(image)
    assert (s.n, s.w, s.g, s.version, s.symbols) == (want.n, want.w, want.g, want.version, want.symbols)
    assert not s.c.gap_words and not s.c.payload
    assert gh.lib().gh_stream_validate(ctypes.byref(s.c)) == 0


# ---- 6. gh_encode_index is unchanged
@pytest.mark.parametrize("name", sc.INPUTS)
def test_whole_index_unchanged(gh, name):
    data, plan, start, image = sc.case_input(gh, name)
    for k in (8, 9, 12):
        got = gh.parse_index(gh.encode_index(data, k)).offsets
        assert np.array_equal(got, _expected(gh, data, image, k)), (name, k)
