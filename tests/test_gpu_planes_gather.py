"""Element gather on the GPU (gh_pgather_*): element ranges (tensor, lo, hi) of a resident batch
of coded byte planes, interleaved as in the tensors, after an index pass alone.

Fixture: eight tensors, nelem in {1, 17, 1023, 1024, 1025, 2049, 4096, 70 000}, E in {1, 2, 4, 8},
masks top, all, none and 0b0101, encoded once with gh.encode_tensors.  The reference everywhere is
the original numpy array sliced.
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODER = os.path.join(ROOT, "bin", "decoder")
GH_E_ARG, GH_E_CORRUPT, GH_E_STATE, GH_E_SMALL = -1, -7, -8, -9
FILL, GUARD = 0xA5, 64
EDGES = (0, 1, 15, 16, 17, 1023, 1024, 1025)
# (nelem, elem_size, coded_mask)
SHAPES = [(1, 1, 0b1), (17, 2, 0b10), (1023, 4, 0b0101), (1024, 8, 0xFF), (1025, 2, 0b11), (2049, 4, 0),
          (4096, 8, 0x80), (70000, 2, 0b10)]
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


class Packed:
    pass


@pytest.fixture(scope="module")
def packed(gpu):
    rng = np.random.default_rng(41)
    arrays = []
    for n, e, m in SHAPES:
        x = rng.normal(0, 0.02, n)
        a = {1: (np.abs(x) * 400).astype(np.uint8), 2: x.astype(np.float16).view(np.uint16),
             4: x.astype(np.float32).view(np.uint32), 8: x.view(np.uint64)}[e]
        arrays.append(np.ascontiguousarray(a))
    pk = Packed()
    pk.arrays = arrays
    pk.images = gpu.encode_tensors(arrays, [m for _, _, m in SHAPES])
    pk.parsed = [gpu.parse_planes(im) for im in pk.images]
    pk.shapes, pk.streams, pk.stored = gpu._planes_streams(pk.parsed)
    assert [(s[1], s[2], s[3]) for s in pk.shapes] == SHAPES
    # one coded plane spans more than one 256-segment unit of the batch
    big = pk.parsed[-1].planes[1]
    assert big.n == 70000 and -(-big.g // 256) > 1
    return pk


def _want(pk, ranges):
    return np.frombuffer(b"".join(pk.arrays[t][lo:hi].tobytes() for t, lo, hi in ranges), dtype=np.uint8)


def _gather(gpu, pk, dec, ranges, shift=0, dst_len=None, stream=0, timed=True, shapes=None, stored_len=None):
    """One device-level gather into a sentinel-filled buffer; returns (report or error, the
    buffer's bytes, the destination's offset in it, the ranges' bytes)."""
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 3))
    total = sum((hi - lo) * SHAPES[t][1] for t, lo, hi in ranges if 0 <= t < len(SHAPES) and hi >= lo)
    dst_len = total if dst_len is None else dst_len
    size = GUARD + shift + total + GUARD
    with gpu.DeviceBuffer(size) as buf, gpu.DeviceBuffer(max(r.nbytes, 16)) as dr, \
            gpu.DeviceBuffer(max(pk.stored.size, 16)) as st:
        buf.upload(np.full(size, FILL, dtype=np.uint8))
        dr.upload(r)
        if pk.stored.size:
            st.upload(pk.stored)
        assert buf.addr % 64 == 0
        try:
            dec.gather_elements_device(shapes or pk.shapes, st.addr, pk.stored.size if stored_len is None else stored_len,
                                       dr.addr, r.shape[0], buf.addr + GUARD + shift, dst_len, stream, timed)
            rep = dec.elements_wait()
        except gpu.GapHuffError as e:
            rep = e
        got = buf.download(np.zeros(size, dtype=np.uint8))
    return rep, got, GUARD + shift, total


def _check_exact(pk, ranges, got, at, total):
    assert (got[:at] == FILL).all() and (got[at + total:] == FILL).all()
    want = _want(pk, ranges)
    assert want.size == total
    if not np.array_equal(got[at: at + total], want):
        pos = 0
        for t, lo, hi in ranges:
            nb = (hi - lo) * SHAPES[t][1]
            assert np.array_equal(got[at + pos: at + pos + nb], want[pos: pos + nb]), (t, lo, hi)
            pos += nb


def _mixed_ranges(seed=3):
    out = []
    for t, (n, e, m) in enumerate(SHAPES):
        pts = sorted({min(x, n) for x in EDGES + (n,)})
        out += [(t, lo, hi) for lo in pts for hi in pts if lo <= hi]  # empty, whole, overlapping
    rng = np.random.default_rng(seed)
    out = [out[i] for i in rng.permutation(len(out))]
    return out + out[:9]  # repeated


@pytest.fixture()
def dec(gpu, packed):
    with gpu.BatchDecoder(0) as b:
        b.load(packed.streams)
        b.index()
        yield b


@pytest.mark.gpu
def test_mixed_ranges_after_index_only(gpu, packed, dec):
    ranges = _mixed_ranges()
    assert any(lo % 16 == 0 and (hi - lo) >= 16 for _, lo, hi in ranges) and any(lo % 16 for _, lo, _ in ranges)
    rep, got, at, total = _gather(gpu, packed, dec, ranges)
    assert not isinstance(rep, Exception), rep
    assert rep.status == 0 and rep.bad_ranges == 0 and rep.out_bytes == total and rep.npieces > 0
    assert rep.launches == gpu.GH_PGATHER_LAUNCHES
    src = open(os.path.join(ROOT, "include", "gaphuff.h")).read()
    assert "#define GH_PGATHER_LAUNCHES %du" % rep.launches in src
    _check_exact(packed, ranges, got, at, total)
    # the host-ranges convenience: one array per range at the tensor's element size
    sub = ranges[:60]
    for (t, lo, hi), a in zip(sub, dec.gather_elements(packed.shapes, packed.stored, sub)):
        assert a.dtype == UINT[SHAPES[t][1]] and np.array_equal(a, packed.arrays[t][lo:hi].view(a.dtype)), (t, lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 4, 8])
def test_destination_shift(gpu, packed, dec, shift):
    # aligned rows first (the vector path at shift 0), then ranges that break every alignment
    ranges = [(7, 1024, 2048), (3, 0, 1024), (6, 16, 4096), (2, 0, 1023), (4, 1, 1025), (7, 69999, 70000), (5, 15, 2049),
              (0, 0, 1), (1, 0, 17), (7, 4096, 4096 + 1040)]
    rep, got, at, total = _gather(gpu, packed, dec, ranges, shift=shift)
    assert not isinstance(rep, Exception), rep
    assert rep.out_bytes == total
    _check_exact(packed, ranges, got, at, total)


@pytest.mark.gpu
def test_vector_rows(gpu, packed, dec):
    """Rows of 64 elements by row id into a 64-byte aligned destination: every lane of every
    range takes the 16-byte path (one coded plane, eight coded planes, a stored-only tensor)."""
    rng = np.random.default_rng(9)
    ranges = []
    for t in (7, 6, 3, 5):
        rows = SHAPES[t][0] // 64
        ranges += [(t, 64 * int(i), 64 * int(i) + 64) for i in rng.integers(0, rows, 200)]
    rep, got, at, total = _gather(gpu, packed, dec, ranges)
    assert not isinstance(rep, Exception), rep
    assert at % 64 == 0 and total == sum(64 * SHAPES[t][1] for t, _, _ in ranges)
    _check_exact(packed, ranges, got, at, total)


@pytest.mark.gpu
def test_constant_launches_reuse_and_caller_stream(gpu, packed, dec):
    import torch
    st = torch.cuda.Stream()
    rng = np.random.default_rng(10)
    many = []
    for _ in range(3000):
        t = int(rng.integers(0, len(SHAPES)))
        lo = int(rng.integers(0, SHAPES[t][0] + 1))
        many.append((t, lo, min(SHAPES[t][0], lo + int(rng.integers(0, 40)))))
    reps = []
    for ranges, timed in ((many, True), (many[:1], True), (many[:700], False), (many, True)):
        rep, got, at, total = _gather(gpu, packed, dec, ranges, stream=st.cuda_stream, timed=timed)
        assert not isinstance(rep, Exception), rep
        _check_exact(packed, ranges, got, at, total)
        assert (rep.kernel_ms > 0) == timed
        if timed:
            assert rep.expand_ms > 0 and rep.join_ms > 0 and rep.expand_ms + rep.join_ms <= rep.kernel_ms * (1 + 1e-5)  # (disjoint spans of one; float sums)
        reps.append(rep)
    assert {r.launches for r in reps} == {gpu.GH_PGATHER_LAUNCHES}  # 1 range or 3000
    dec.gather_elements_device(packed.shapes, 0, 0, 0, 0, 0, 0)  # nothing is launched: the last report stays
    assert dec.elements_wait().out_bytes == reps[-1].out_bytes
    assert dec.gather_elements(packed.shapes, packed.stored, []) == []


@pytest.mark.gpu
def test_one_workgroup_walks_many_ranges(gpu, packed, dec, monkeypatch):
    monkeypatch.setenv("GH_PLANES_GRID", "1")
    rng = np.random.default_rng(11)
    ranges = []
    for _ in range(4000):
        t = int(rng.integers(1, len(SHAPES)))
        lo = int(rng.integers(0, SHAPES[t][0]))
        ranges.append((t, lo, min(SHAPES[t][0], lo + int(rng.integers(1, 21)))))
    rep, got, at, total = _gather(gpu, packed, dec, ranges)
    assert not isinstance(rep, Exception), rep
    _check_exact(packed, ranges, got, at, total)


@pytest.mark.gpu
def test_refusals(gpu, packed):
    good = [(7, 0, 100), (3, 5, 900), (5, 0, 2049)]
    with gpu.BatchDecoder(0) as b:
        b.load(packed.streams)
        rep, got, _, _ = _gather(gpu, packed, b, good)
        assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_STATE and (got == FILL).all()  # before index()
        b.index()
        for bad in [(len(SHAPES), 0, 0), (3, 7, 6), (7, 0, 70001)]:
            rep, got, _, _ = _gather(gpu, packed, b, good + [bad] + good)
            assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_ARG, bad
            assert rep.report.status & gpu.GH_ST_RANGE and (got == FILL).all(), bad
        total = sum((hi - lo) * SHAPES[t][1] for t, lo, hi in good)
        rep, got, _, _ = _gather(gpu, packed, b, good, dst_len=total - 1)
        assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_SMALL
        assert rep.report.status & gpu.GH_ST_DSTSMALL and rep.report.out_bytes == total and (got == FILL).all()
        # a layout that differs from the loaded batch's: another mask (a stream more), another nelem
        for k, item in ((5, (0, 2049, 4, 1)), (7, (0, 69999, 2, 2))):
            shapes = list(packed.shapes)
            shapes[k] = item
            rep, got, _, _ = _gather(gpu, packed, b, good, shapes=shapes, stored_len=1 << 20)
            assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_ARG and (got == FILL).all(), item
        rep, _, _, _ = _gather(gpu, packed, b, good, stored_len=packed.stored.size - 1)
        assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_SMALL
        with gpu.DeviceBuffer(64) as d:
            for args in [(d.addr, 64, 0, 1, d.addr, 64), (d.addr, 64, d.addr, 1, 0, 64),
                         (d.addr + 4, 1 << 20, d.addr, 1, d.addr, 64),
                         (d.addr, 1 << 20, d.addr, gpu.GH_PGATHER_MAX_RANGES + 1, d.addr, 64)]:
                with pytest.raises(gpu.GapHuffError) as e:
                    b.gather_elements_device(packed.shapes, args[0], max(args[1], packed.stored.size), *args[2:])
                assert e.value.code == GH_E_ARG, args
        # and the batch still gathers
        rep, got, at, total = _gather(gpu, packed, b, good)
        assert not isinstance(rep, Exception)
        _check_exact(packed, good, got, at, total)


def _raise_n(img, by):
    """The image with its header N raised (v1 header: u64 S, S x 2 bytes, u32 N); the recipe of
    tests/test_gpu_planes.py."""
    bad = np.array(img, dtype=np.uint8)
    s = int(bad[:8].view("<u8")[0])
    assert s <= 256
    at = 8 + 2 * s
    bad[at: at + 4] = np.asarray([int(bad[at: at + 4].view("<u4")[0]) + by], dtype="<u4").view(np.uint8)
    return bad


@pytest.mark.gpu
def test_one_corrupt_tensor_among_good_ones(gpu, packed):
    """Tensor 4 (two coded planes) claims 100 elements more than its streams hold: both streams
    are flagged, its ranges keep their sentinel bytes and count once each, not once per plane."""
    k = 4
    slots, _, _ = gpu.planes_layout(packed.shapes)
    mine = [slots[k][p][0] for p in range(2)]
    streams = list(packed.streams)
    for s in mine:
        streams[s] = gpu.parse(_raise_n(streams[s].raw, 100))
    shapes = list(packed.shapes)
    shapes[k] = (0, SHAPES[k][0] + 100, 2, 0b11)
    ranges = [(7, 0, 64), (k, 0, 1025), (3, 1, 1000), (k, 7, 7), (k, 16, 48), (5, 0, 2049), (0, 0, 1)]
    nbad = sum(1 for t, _, _ in ranges if t == k)
    with gpu.BatchDecoder(0) as b:
        b.load(streams)
        b.index()
        rep, got, at, total = _gather(gpu, packed, b, ranges, shapes=shapes)
        assert isinstance(rep, gpu.GapHuffError) and rep.code == GH_E_CORRUPT
        assert rep.report.bad_ranges == nbad and rep.report.status & gpu.GH_ST_BADCODE and rep.report.out_bytes == total
        st, _ = b.status()
        assert sorted(np.flatnonzero(st).tolist()) == sorted(mine)
    assert (got[:at] == FILL).all() and (got[at + total:] == FILL).all()
    pos = at
    for t, lo, hi in ranges:
        nb = (hi - lo) * SHAPES[t][1]
        if t == k:
            assert (got[pos: pos + nb] == FILL).all(), (t, lo, hi)
        else:
            assert got[pos: pos + nb].tobytes() == packed.arrays[t][lo:hi].tobytes(), (t, lo, hi)
        pos += nb


@pytest.mark.gpu
def test_after_a_full_decode(gpu, packed):
    ranges = _mixed_ranges(seed=4)[:120]
    with gpu.BatchDecoder(0) as b:
        b.load(packed.streams)
        b.decode()
        b.wait()
        rep, got, at, total = _gather(gpu, packed, b, ranges)
        assert not isinstance(rep, Exception), rep
        _check_exact(packed, ranges, got, at, total)


@pytest.mark.gpu
def test_one_shot_and_cli(gpu, packed, tmp_path):
    ranges = [(7, 1000, 3000), (2, 0, 1023), (3, 17, 17), (6, 4000, 4096), (5, 1, 2), (7, 0, 70000), (0, 0, 1)]
    for (t, lo, hi), a in zip(ranges, gpu.decode_tensor_ranges(packed.images, ranges)):
        assert a.dtype == UINT[SHAPES[t][1]] and np.array_equal(a, packed.arrays[t][lo:hi]), (t, lo, hi)
    with pytest.raises(gpu.GapHuffError) as e:
        gpu.decode_tensor_ranges(packed.images, [(0, 0, 2)])
    assert e.value.code == GH_E_ARG
    # the CLI
    for i, im in enumerate(packed.images):
        im.tofile(tmp_path / f"t{i}.ghp")
    (tmp_path / "list.txt").write_text("".join(f"{tmp_path}/t{i}.ghp\n" for i in range(len(SHAPES))))
    (tmp_path / "el.txt").write_text("".join(f"{t} {lo}:{hi}\n" for t, lo, hi in ranges))
    out = tmp_path / "el.out"
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "list.txt"), "--elements", str(tmp_path / "el.txt"), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Element gather: 8 tensors, 7 ranges" in r.stdout, r.stdout + r.stderr
    assert out.read_bytes() == _want(packed, ranges).tobytes()
    # refusals: a range outside its tensor; --ranges on containers stays refused; --elements on compressed streams
    (tmp_path / "bad.txt").write_text("0 0:1\n1 0:18\n")
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "list.txt"), "--elements", str(tmp_path / "bad.txt"),
                        str(tmp_path / "bad.out")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "range 2" in r.stderr and not (tmp_path / "bad.out").exists(), r.stdout + r.stderr
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "list.txt"), "--ranges", str(tmp_path / "el.txt"),
                        str(tmp_path / "r.out")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "gather a plane's stream instead" in r.stderr, r.stdout + r.stderr
    gpu.encode(np.arange(500, dtype=np.uint8)).tofile(tmp_path / "s.huff")
    (tmp_path / "plain.txt").write_text(f"{tmp_path}/s.huff\n")
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "plain.txt"), "--elements", str(tmp_path / "el.txt"),
                        str(tmp_path / "p.out")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--elements takes byte-plane containers only" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "p.out").exists()
