"""Every compiled shape of the GPU encoder's write kernel, encoded once per ordering and
grid setting.

The host picks one of 14 instantiations gh_enc_write_kernel<NSW, SLICE> per encode
(enc_write_kernel_for in csrc/gh_encode.hip) from the input's code bits per byte:
need = ceil(1.05 * (8192 * ceil(bits / 32) / n + 2) / 512), about 0.525 * bits per byte, so
NSW 1, 2, 3, 4, 5, 6, 9 take inputs of up to about 1.9, 3.8, 5.7, 7.6, 9.5, 11.4 and 16 bits
per byte.  As in tests/test_gpu_shapes.py the streams carry a *prescribed* code (symbol i
occurs m * 2^(maxlen - len_i) times, so package-merge has no choice), every test asserts the
lengths the plan returned, and every encode asserts the name of the instantiation that ran
(gh_ectx_kernel_shape).  Every image is compared byte for byte with the CPU oracle's
restatement of the reference encoder and with the host encoder; every slice word for word
with the host's slice encoder.

The CPU tests pin the tables: the names the rows expect are exactly gh_enc_kernel_shapes(),
and gh_enc_kernel_shape_for(n, bits, slice), the picker itself, returns each row's and each
slice's expected name for the n and bits of its stream."""
import ctypes

import numpy as np
import pytest

import slice_cases as sc
from test_gpu_shapes import ENV_KNOBS, _assert_code, _fours, _ladder, _setenv, _stream, _symbols

GH_E_ARG, GH_E_STATE, GH_E_SMALL = -1, -8, -9
NSWS = (1, 2, 3, 4, 5, 6, 9)


def _name(nsw, slice_):
    return f"enc_write<{nsw},slice={int(slice_)}>"


def _n_for(code):
    """About 2^20 bytes = 128 chunks of 8 KiB: many iterations per workgroup on a grid of
    three.  m odd where the code allows it, so the last chunk is partial."""
    maxlen = max(code)
    return (1 << 20) + (1 << maxlen) if maxlen <= 12 else 1 << 20


LADDER8_1516 = {**{l: 1 for l in range(1, 9)}, 15: 64, 16: 128}  # 16 KiB of 15/16-bit codewords in 4 MiB
N_1516 = 1 << 22

# ---- whole streams (SLICE = false) --------------------------------------------------
# id: (code, n, orderings, NSW).  One code per NSW 1..5, each average well inside its band.
# NSW 6 and 9 are out of a long whole stream's reach: a Huffman code never averages above
# 8 bits per byte, so they are picked only where one payload word is spread over n <= 3
# bytes (n = 3: 6; n = 1, 2: 9).  The rows n3, n2 and n1 are the only whole-stream inputs
# that reach them; the slice rows below encode full chunks with their SLICE = true twins.
ALL4 = ("shuffled", "sorted", "sorted_rev", "striped")
FLAT = ("shuffled", "sorted", "sorted_rev")  # one codeword length: nothing to stripe
WHOLE_ROWS = {
    "one_symbol": ({1: 1}, (1 << 20) + 1, ("sorted",), 1),                # 1 bit per byte
    "two_symbols": ({1: 2}, _n_for({1: 2}), FLAT, 1),                     # 1
    # (its two 8-bit symbols are too few for the striped generator's 129 x 12 stripes: the
    # next row is the striped NSW 2 stream)
    "ladder_1_8": (_ladder(1, 8), _n_for(_ladder(1, 8)), FLAT, 2),        # ~1.98
    "ladder_2_7": (_ladder(2, 7, 3), _n_for(_ladder(2, 7, 3)), ("striped",), 2),  # ~2.48
    "fours_3_7": (_fours(3, 7), _n_for(_fours(3, 7)), ALL4, 3),           # ~3.94
    "six_seven": ({6: 32, 7: 64}, _n_for({6: 32, 7: 64}), ALL4, 4),       # 6.5
    "flat_8": ({8: 256}, _n_for({8: 256}), FLAT, 5),                      # 8
    # a low-NSW kernel over runs of chunks at the longest codewords, in both directions:
    # those chunks go through the tail loop past NSW * 512 words and fill the LDS image
    # towards the bound it is sized for at launch.  At 2^20 bytes dyadic counts leave
    # fours_3_16 four chunks of 8..16-bit codewords, the last of them at 10..16 bits (128
    # bytes at 16); the second stream, 2^22 bytes, holds two whole chunks at 15 and 16 bits
    "fours_3_16": (_fours(3, 16), 1 << 20, ("sorted", "sorted_rev"), 3),       # ~4.0
    "ladder_1_8_15_16": (LADDER8_1516, N_1516, ("sorted", "sorted_rev"), 2),   # ~2.03
    "n3": (None, 3, ("as_is",), 6),
    "n2": (None, 2, ("as_is",), 9),
    "n1": (None, 1, ("as_is",), 9),
}
SETTINGS = {"default": {}, "grid3": {"GH_ENC_GRID": "3"}}

# ---- slices (SLICE = true) ----------------------------------------------------------
# Sorted streams cut at the boundaries between length classes: a slice is a pure run of one
# class, encoded under the whole input's plan at its true base_bit, so it can average up to
# 16 bits per byte: a shard of rare values under the plan of the sum.
# id: (code, n, dense, per-class NSW in sorted order (the dense classes as one slice),
#      NSW of the rest as one slice, NSW of the dense slice).
# `dense`: the lengths of the class(es) the cuts are made around.
_HEAD5 = {l: 1 for l in range(1, 6)}
SLICE_ROWS = {
    "s4": ({6: 32, 7: 64}, 1025 << 7, (7,), [4, 4], 4, 4),                      # 3.15, 3.68 need
    "s5": ({**_HEAD5, 8: 8}, 1 << 20, (8,), [1, 2, 2, 3, 3, 5], 1, 5),          # 32 KiB at 8 bits
    "s6": ({**_HEAD5, 10: 32}, 1 << 20, (10,), [1, 2, 2, 3, 3, 6], 1, 6),       # 32 KiB at 10 bits
    "s9": ({**_HEAD5, 12: 128}, 1 << 20, (12,), [1, 2, 2, 3, 3, 9], 1, 9),      # 32 KiB at 12 bits
    "s9_1516": (LADDER8_1516, N_1516, (15, 16), [1, 2, 2, 3, 3, 4, 4, 5, 9], 2, 9),  # 16 KiB at ~15.5
}
SLICE_ORDERINGS = ("sorted", "sorted_rev")
VARIANTS = ("class", "minus1", "plus1", "mid")


# ---- streams ------------------------------------------------------------------------
_cache = {}


def _data(code, n, ordering):
    if code is None:  # the tiny rows: n different bytes
        return np.arange(1, n + 1, dtype=np.uint8)
    seed = len(code) * 1000 + n % 997
    if ordering == "sorted_rev":  # longest codewords first, shortest last
        return np.ascontiguousarray(_stream(code, n, "sorted", seed)[::-1])
    return _stream(code, n, ordering, seed)


def _case(gh, orc, code, n, ordering):
    """(data, plan, start, image): the stream, its host plan (with the prescribed lengths),
    every byte's first bit (n + 1 entries) and the oracle's image, which the host encoder
    reproduces.  Built once per stream; read-only."""
    key = (None if code is None else tuple(sorted(code.items())), n, ordering)
    if key not in _cache:
        if len(_cache) >= 6:
            _cache.pop(next(iter(_cache)))
        data = _data(code, n, ordering)
        image = orc.encode(data)
        assert np.array_equal(gh.encode(data), image), "host encoder and oracle differ"
        if code is not None:
            _assert_code(gh, image, code)
        plan = gh.encode_plan(data)
        lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
        start = np.concatenate([[0], np.cumsum(lens[data], dtype=np.uint64)]).astype(np.uint64)
        assert int(start[-1]) == plan.bits
        for a in (data, image, start):
            a.setflags(write=False)
        _cache[key] = (data, plan, start, image)
    return _cache[key]


def _class_bounds(code, n):
    """Byte offsets of the length classes of the sorted stream: [0, ..., n], shortest first."""
    _, lens = _symbols(code)
    maxlen = int(lens.max())
    cnt = (n >> maxlen) * (1 << (maxlen - lens))
    per_len = [int(cnt[lens == l].sum()) for l in sorted(code)]
    return [0] + np.cumsum(per_len).tolist()


def _slices(row, ordering, variant):
    """[(lo, hi, NSW)] of a slice row's partition.  Around the dense class [d0, d1):
    class: every class boundary; minus1 / plus1: the boundary between the dense class and
    the rest moved by one byte, so the dense slice starts or ends with one byte of the
    neighbouring class (or lacks one of its own); mid: the boundary, and an odd offset
    inside the dense class."""
    code, n, dense, per_class, rest, dns = SLICE_ROWS[row]
    cb = _class_bounds(code, n)
    nd = len(dense)  # the dense classes are the longest: the last nd of the sorted stream
    bounds = cb[:len(cb) - nd] + [n]
    d = bounds[-2]
    assert len(bounds) - 1 == len(per_class)
    if variant == "class":
        sl = list(zip(bounds[:-1], bounds[1:], per_class))
    elif variant == "minus1":
        sl = [(0, d - 1, rest), (d - 1, n, dns)]
    elif variant == "plus1":
        sl = [(0, d + 1, rest), (d + 1, n, dns)]
    else:
        mid = d + (n - d) // 2 + 3
        sl = [(0, d, rest), (d, mid, dns), (mid, n, dns)]
    if ordering == "sorted_rev":  # the stream reversed: the dense class first
        sl = [(n - hi, n - lo, nsw) for lo, hi, nsw in reversed(sl)]
    return sl


def _same(got, want, what):
    assert got.size == want.size, f"{what}: {got.size} for {want.size} elements"
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: "
                             f"{int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}")


WHOLE_CASES = [(r, o) for r, row in WHOLE_ROWS.items() for o in row[2]]
SLICE_CASES = [(r, o, v) for r in SLICE_ROWS for o in SLICE_ORDERINGS for v in VARIANTS]


# ---- no GPU -------------------------------------------------------------------------
def test_rows_cover_every_shape(gh):
    """The kernels named by the rows are exactly those the picker can return: a new
    instantiation needs a row here, a removed one loses its row."""
    want = {_name(row[3], False) for row in WHOLE_ROWS.values()}
    for r, o, v in SLICE_CASES:
        want |= {_name(nsw, True) for _, _, nsw in _slices(r, o, v)}
    have = gh.enc_kernel_shapes()
    assert len(have) == len(set(have)) == 14
    assert want == set(have)
    assert set(have) == {_name(nsw, s) for nsw in NSWS for s in (False, True)}
    assert not set(have) & set(gh.kernel_shapes())  # the decoder's list stays decode-only


@pytest.mark.parametrize("row,ordering", WHOLE_CASES)
def test_picker_agrees_with_whole_rows(gh, orc, row, ordering):
    """The host plan returns the prescribed lengths (_case) and the picker, asked for the
    stream's n and bits, returns the row's kernel."""
    code, n, _, nsw = WHOLE_ROWS[row]
    data, plan, start, image = _case(gh, orc, code, n, ordering)
    assert data.size == n == plan.n
    assert gh.enc_kernel_shape_for(n, plan.bits, False) == _name(nsw, False)
    if code is not None and max(code) <= 12:
        assert n % 8192  # a partial last chunk


@pytest.mark.parametrize("row,ordering", [(r, o) for r in SLICE_ROWS for o in SLICE_ORDERINGS])
def test_picker_agrees_with_slice_rows(gh, orc, row, ordering):
    code, n = SLICE_ROWS[row][:2]
    data, plan, start, image = _case(gh, orc, code, n, ordering)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    for variant in VARIANTS:
        sl = _slices(row, ordering, variant)
        assert sl[0][0] == 0 and sl[-1][1] == n and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        for lo, hi, nsw in sl:
            bits = int(start[hi] - start[lo])
            assert gh.enc_kernel_shape_for(hi - lo, bits, True) == _name(nsw, True), (variant, lo, hi)
    # the class cuts are pure runs of one length (the dense classes: of theirs)
    dense = SLICE_ROWS[row][2]
    for lo, hi, nsw in _slices(row, ordering, "class"):
        got = set(np.unique(lens[data[lo:hi]]).tolist())
        assert got == set(dense) or (len(got) == 1 and not got & set(dense))


def test_dense_slices_hold_several_chunks():
    """Every slice shape meets several full 8 KiB chunks in some slice, and the dense
    slices of NSW 6 and 9 more chunks than the three workgroups of the grid3 setting."""
    most = {}
    for r, o, v in SLICE_CASES:
        for lo, hi, nsw in _slices(r, o, v):
            most[nsw] = max(most.get(nsw, 0), (hi - lo) // 8192)
    assert set(most) == set(NSWS)
    assert all(c >= 4 for c in most.values()), most


def test_picker_at_the_smallest_inputs(gh):
    """One payload word over n <= 3 bytes: the only whole streams that pick NSW 6 and 9."""
    assert gh.enc_kernel_shape_for(1, 1, False) == _name(9, False)
    assert gh.enc_kernel_shape_for(2, 2, False) == _name(9, False)
    assert gh.enc_kernel_shape_for(3, 5, False) == _name(6, False)
    assert gh.enc_kernel_shape_for(3, 3, False) == _name(6, False)
    # a long whole stream at the fixed 8-bit code's 8 bits per byte, the most a plan gives
    assert gh.enc_kernel_shape_for(1 << 30, 8 << 30, False) == _name(5, False)
    assert gh.enc_kernel_shape_for(0, 0, False) == ""  # nothing to launch


def test_encoder_shape_queries_check_their_arguments(gh):
    L = gh.lib()
    small, buf = ctypes.create_string_buffer(8), ctypes.create_string_buffer(1 << 10)
    assert L.gh_enc_kernel_shapes(small, len(small)) == GH_E_SMALL
    assert L.gh_enc_kernel_shapes(None, 0) == GH_E_ARG
    assert L.gh_enc_kernel_shapes(buf, len(buf)) == 0 and buf.value.decode().count("\n") == 14
    assert L.gh_enc_kernel_shape_for(1 << 20, 1 << 20, 0, small, len(small)) == GH_E_SMALL
    assert L.gh_enc_kernel_shape_for(1 << 20, 1 << 20, 0, None, 0) == GH_E_ARG
    assert L.gh_enc_kernel_shape_for(1 << 20, 1 << 20, 2, buf, len(buf)) == GH_E_ARG
    assert L.gh_enc_kernel_shape_for(1 << 20, (16 << 20) + 1, 1, buf, len(buf)) == GH_E_ARG  # > 16 bits a byte
    assert L.gh_enc_kernel_shape_for(1 << 20, 16 << 20, 1, buf, len(buf)) == 0
    assert buf.value.decode() == _name(9, True)
    name = _name(1, False).encode()
    exact = ctypes.create_string_buffer(len(name) + 1)
    assert L.gh_enc_kernel_shape_for(1 << 20, 1 << 20, 0, exact, len(name)) == GH_E_SMALL
    assert L.gh_enc_kernel_shape_for(1 << 20, 1 << 20, 0, exact, len(name) + 1) == 0 and exact.value == name
    assert L.gh_ectx_kernel_shape(None, buf, len(buf)) == GH_E_ARG


def test_env_knobs_cleared():
    assert "GH_ENC_GRID" in ENV_KNOBS and "GH_ENC_INDEX_GRID" in ENV_KNOBS


# ---- GPU ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def enc(gpu):
    with gpu.Encoder(0) as e:
        yield e


def _encode_whole(gpu, e, data, image, name):
    e.load(data)
    plan = e.make_plan()
    e.encode()
    shape = e.kernel_shape()
    img = e.download()
    assert shape == name
    assert img.size == plan.file_bytes
    _same(img, image, f"{shape}: image")
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("row,ordering,setting", [(r, o, s) for r, o in WHOLE_CASES for s in SETTINGS])
def test_whole_stream_shape(gpu, orc, enc, monkeypatch, row, ordering, setting):
    code, n, _, nsw = WHOLE_ROWS[row]
    data, plan, start, image = _case(gpu, orc, code, n, ordering)
    _setenv(monkeypatch, SETTINGS[setting])
    _encode_whole(gpu, enc, data, image, _name(nsw, False))


@pytest.mark.gpu
@pytest.mark.parametrize("row", WHOLE_ROWS)
def test_whole_stream_decode_and_index(gpu, orc, enc, monkeypatch, row):
    """Once per row, on three workgroups: the encoder's image decodes to the input, and the
    seek index built from what the encode left on the device equals the host's."""
    code, n, orderings, nsw = WHOLE_ROWS[row]
    data, plan, start, image = _case(gpu, orc, code, n, orderings[0])
    _setenv(monkeypatch, {"GH_ENC_GRID": "3"})
    img = _encode_whole(gpu, enc, data, image, _name(nsw, False))
    idx, _ = enc.index(8)
    _same(idx, gpu.encode_index(data, 8), "index")
    _same(gpu.decode(img), data, "decoded bytes")


def _encode_slices(gpu, e, data, plan, start, slices, dense_nsw):
    """Every slice on the device against the host's slice encoder; the parts."""
    parts = []
    for lo, hi, nsw in slices:
        base, bits = int(start[lo]), int(start[hi] - start[lo])
        e.load(data[lo:hi])
        s, _ = e.encode_slice(plan, base)
        shape = e.kernel_shape()
        words, gapw = e.download_slice()
        assert shape == _name(nsw, True), (lo, hi)
        sc.check_extents_and_edges(gpu, s, words, gapw, base, bits)
        hs, hw, hg = gpu.encode_slice(data[lo:hi], plan, base)
        _same(words, hw, f"{shape} [{lo}, {hi}) words")
        _same(gapw, hg, f"{shape} [{lo}, {hi}) gap words")
        if nsw == dense_nsw:  # the index kernel reuses the write kernel's chunk offsets
            ent, k0, _ = e.index_slice(lo, 8)
            hent, hk0 = gpu.encode_index_slice(data[lo:hi], plan, base, lo, 8)
            assert k0 == hk0
            _same(ent, hent, f"{shape} [{lo}, {hi}) index entries")
        parts.append((s, words, gapw))
    return parts


@pytest.mark.gpu
@pytest.mark.parametrize("row,ordering,variant,setting", [c + (s,) for c in SLICE_CASES for s in SETTINGS])
def test_slice_shape(gpu, orc, enc, monkeypatch, row, ordering, variant, setting):
    code, n = SLICE_ROWS[row][:2]
    data, plan, start, image = _case(gpu, orc, code, n, ordering)
    _setenv(monkeypatch, SETTINGS[setting])
    parts = _encode_slices(gpu, enc, data, plan, start, _slices(row, ordering, variant), SLICE_ROWS[row][5])
    _same(gpu.merge_slices(plan, parts[::-1]), image, "merged image")


@pytest.mark.gpu
def test_context_reuse_across_shapes(gpu, orc, monkeypatch):
    """One context through rows that alternate the highest and the lowest NSW, whole streams
    and slices, the default grid and three workgroups: the image, gap and junk buffers grow
    and shrink, and nothing of an earlier encode (gap words ORed in, image words) may show."""
    steps = [("slice", "s9_1516", "sorted"), ("whole", "two_symbols", "sorted"), ("slice", "s9", "sorted_rev"),
             ("whole", "n1", "as_is"), ("whole", "flat_8", "shuffled"), ("slice", "s6", "sorted"),
             ("whole", "one_symbol", "sorted"), ("whole", "n3", "as_is"), ("whole", "ladder_1_8_15_16", "sorted_rev"),
             ("slice", "s5", "sorted_rev"), ("whole", "six_seven", "striped")]
    with gpu.Encoder(0) as e:
        with pytest.raises(gpu.GapHuffError) as err:
            e.kernel_shape()
        assert err.value.code == GH_E_STATE
        for i, (kind, row, ordering) in enumerate(steps):
            _setenv(monkeypatch, SETTINGS["grid3" if i % 2 else "default"])
            if kind == "whole":
                code, n, _, nsw = WHOLE_ROWS[row]
                data, plan, start, image = _case(gpu, orc, code, n, ordering)
                _encode_whole(gpu, e, data, image, _name(nsw, False))
            else:
                code, n = SLICE_ROWS[row][:2]
                data, plan, start, image = _case(gpu, orc, code, n, ordering)
                parts = _encode_slices(gpu, e, data, plan, start, _slices(row, ordering, "mid"), SLICE_ROWS[row][5])
                _same(gpu.merge_slices(plan, parts), image, "merged image")
        e.load(np.zeros(0, dtype=np.uint8))
        with pytest.raises(gpu.GapHuffError) as err:
            e.kernel_shape()  # a load forgets the last encode
        assert err.value.code == GH_E_STATE
        e.make_plan()
        e.encode()
        assert e.kernel_shape() == ""  # an empty input launches no kernel
