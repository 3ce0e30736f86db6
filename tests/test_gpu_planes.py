"""Byte planes on the GPU: gh_planes_load_device's split kernel, gh_planes_join_device's join
kernel, the one-call forms and the CLIs.

The reference for every coded plane is gh.encode of the host plane (numpy
a.reshape(-1, E)[:, p]); for every tensor, its own bytes.  Sizes: every element size crossed
with nelem = 0, 1, 15, 16, 17 (the lane edges: a lane owns 16 elements), 1023, 1024, 1025 (the
unit edges: a unit is 1024 elements), 4101 (several units and a ragged tail) and 65536 (64
units: more than one workgroup); masks: all planes, the top plane, none, alternating."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cse375-finalproj-huffman-decoding_amd")
ENCODER = os.path.join(ROOT, "bin", "encoder")
DECODER = os.path.join(ROOT, "bin", "decoder")
GH_E_ARG, GH_E_CORRUPT, GH_E_STATE, GH_E_SMALL = -1, -7, -8, -9
GUARD = 4096
ELEMS = (1, 2, 4, 8)
NELEMS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 4101, 65536)
SRC_FILL, SENTINEL = 0xFF, 0xA5


def _masks(e):
    return ((1 << e) - 1, 1 << (e - 1), 0, sum(1 << p for p in range(e - 1, -1, -2)))


def _pad16(n):
    return -(-n // 16) * 16


class Tensor:
    def __init__(self, gh, e, nelem, mask, seed):
        rng = np.random.default_rng(seed)
        self.e, self.nelem, self.mask = e, nelem, mask
        self.data = (rng.integers(0, 256, nelem * e) >> rng.integers(0, 7, nelem * e)).astype(np.uint8)  # skewed bytes
        self.planes = [np.ascontiguousarray(self.data.reshape(-1, e)[:, p]) for p in range(e)]
        self.coded = [p for p in range(e) if (mask >> p) & 1]
        self._gh = gh
        self._images = None

    @property
    def images(self):
        """gh.encode of every coded plane, in plane order (made once)."""
        if self._images is None:
            self._images = [self._gh.encode(self.planes[p]) for p in self.coded]
        return self._images


@pytest.fixture(scope="module")
def tensors(gh):
    out = []
    for e in ELEMS:
        for nelem in NELEMS:
            for k, mask in enumerate(_masks(e)):
                out.append(Tensor(gh, e, nelem, mask, 1000 * e + 7 * nelem + k))
    return out


def _place(ts, shift):
    """Offsets of the tensors in one buffer: each `shift` bytes past a 16-byte boundary, at least
    16 fill bytes behind it, none at the buffer's end."""
    offs, cur = [], 0
    for t in ts:
        o = _pad16(cur) + shift
        offs.append(o)
        cur = o + t.data.size + 16
    return offs, _pad16(cur) + 64


def _items(ts, base, offs, nelems=None):
    return [(base + o, t.nelem if nelems is None else nelems[i], t.e, t.mask) for i, (t, o) in enumerate(zip(ts, offs))]


def _stored_want(gpu, ts, nelems=None):
    """(slots, nstreams, the stored arena as the split must leave it)."""
    slots, ns, sb = gpu.planes_layout(_items(ts, 0, [0] * len(ts), nelems))
    want = np.zeros(sb, dtype=np.uint8)
    for t, sl in zip(ts, slots):
        for p in range(t.e):
            if sl[p][0] == gpu.GH_PLANES_STORED:
                want[sl[p][1]: sl[p][1] + t.nelem] = t.planes[p]
    return slots, ns, want


def _encode(gpu, enc, ts, shift=0, device_plan=False):
    """load_planes_device from one fill-padded source buffer, plan, encode, wait; checks the
    images and the stored arena."""
    offs, total = _place(ts, shift)
    host = np.full(total, SRC_FILL, dtype=np.uint8)
    for t, o in zip(ts, offs):
        host[o: o + t.data.size] = t.data
    _, ns, want = _stored_want(gpu, ts)
    with gpu.DeviceBuffer(total) as src, gpu.DeviceBuffer(want.size + GUARD) as st:
        src.upload(host)
        st.upload(np.full(want.size + GUARD, SENTINEL, dtype=np.uint8))
        assert st.addr % 16 == 0 and src.addr % 16 == 0
        enc.load_planes_device(_items(ts, src.addr, offs), st.addr, want.size)
        got = st.download(np.zeros(want.size + GUARD, dtype=np.uint8))
    assert len(enc.ns) == ns
    assert np.array_equal(got[: want.size], want), "stored arena (planes and zero pads)"
    assert (got[want.size:] == SENTINEL).all(), "guard after stored_len"
    if device_plan:
        enc.plan_device()
    else:
        enc.plan()
    enc.encode()
    rep = enc.wait()
    assert rep.nstreams == ns
    refs = [img for t in ts for img in t.images]
    for i, (img, ref) in enumerate(zip(enc.download_all(), refs)):
        assert np.array_equal(img, ref), f"stream {i}: image differs from gh.encode(host plane)"
    return want


def _join(gpu, dec, ts, stored, shift=0, nelems=None, skip=(), wait=True):
    """join_planes_device into one sentinel-filled buffer; checks every tensor and every byte
    around it.  Returns the report (or the raised error's)."""
    sizes = [(t.nelem if nelems is None else nelems[i]) * t.e for i, t in enumerate(ts)]
    offs, cur = [], 0
    for s in sizes:
        offs.append(_pad16(cur) + shift)
        cur = offs[-1] + s + 16
    total = _pad16(cur) + 64
    with gpu.DeviceBuffer(total) as dst, gpu.DeviceBuffer(max(stored.size, 16)) as st:
        dst.upload(np.full(total, SENTINEL, dtype=np.uint8))
        if stored.size:
            st.upload(stored)
        dec.join_planes_device(_items(ts, dst.addr, offs, nelems), st.addr, stored.size)
        if not wait:
            return None
        err = None
        try:
            rep = dec.planes_wait()
        except gpu.GapHuffError as e:
            err, rep = e, e.report
        got = dst.download(np.zeros(total, dtype=np.uint8))
    mask = np.ones(total, dtype=bool)
    for i, (t, o) in enumerate(zip(ts, offs)):
        if i in skip:
            assert (got[o: o + sizes[i]] == SENTINEL).all(), f"tensor {i} was flagged and yet written"
        else:
            assert np.array_equal(got[o: o + t.data.size], t.data), f"tensor {i} (E={t.e} nelem={t.nelem} mask={t.mask:#x})"
            mask[o: o + t.data.size] = False
    assert (got[mask] == SENTINEL).all(), "a byte before or after a tensor was written"
    if err is not None:
        raise err
    return rep


# ---- (a) the mixed batch -------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_batch_split(gpu, tensors):
    assert any(not t.coded for t in tensors) and len(tensors) == 160
    with gpu.BatchEncoder(0) as enc:
        _encode(gpu, enc, tensors)
    # a batch without a single stream: every plane stored
    none = [t for t in tensors if not t.coded]
    with gpu.BatchEncoder(0) as enc:
        _encode(gpu, enc, none)
        assert enc.ns == [] and enc.download_all() == []


# ---- (b) alignment and plan kind, (c) the round trip on the device -------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shift", (0, 1, 2, 3, 4, 8))
def test_round_trip_on_device(gpu, tensors, shift):
    """Sources and destinations `shift` bytes past a 16-byte boundary (0: the vector path);
    shift 4 with the codes built on the device."""
    with gpu.BatchEncoder(0) as enc, gpu.BatchDecoder(0) as dec:
        stored = _encode(gpu, enc, tensors, shift, device_plan=shift == 4)
        dec.load_device(enc.items())
        dec.decode()
        rep = _join(gpu, dec, tensors, stored, shift)
        assert rep.bad_tensors == 0 and rep.ntensors == len(tensors)
        assert rep.out_bytes == sum(t.data.size for t in tensors)
        # twice without a reload: the same bytes again
        dec.decode()
        _join(gpu, dec, tensors, stored, shift)


@pytest.mark.gpu
def test_launches_do_not_depend_on_the_tensor_count(gpu, tensors):
    one = [t for t in tensors if t.e == 4 and t.nelem == 4101 and t.mask == 0b1000]
    assert len(one) == 1
    counts = []
    for ts in (one, tensors):
        with gpu.BatchEncoder(0) as enc, gpu.BatchDecoder(0) as dec:
            stored = _encode(gpu, enc, ts)
            dec.load_device(enc.items())
            dec.decode()
            counts.append(_join(gpu, dec, ts, stored).launches)
    assert counts[0] == counts[1] > 0


# ---- (d) many tiny tensors through one workgroup ------------------------------------------
_ONE_WAVE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import gaphuff as gh
rng = np.random.default_rng(23)
ts = []
for i in range(1503):
    e = (1, 2, 4, 8)[int(rng.integers(0, 4))]
    nelem = 1 + i % 40
    mask = int(rng.integers(0, 1 << e))
    ts.append((e, nelem, mask, rng.integers(0, 6, nelem * e).astype(np.uint8)))
offs, cur = [], 0
for e, nelem, mask, d in ts:
    offs.append(-(-cur // 16) * 16 + (len(offs) % 3))
    cur = offs[-1] + d.size + 16
total = cur + 64
host = np.full(total, 0xFF, dtype=np.uint8)
for (e, nelem, mask, d), o in zip(ts, offs):
    host[o: o + d.size] = d
shapes = [(0, nelem, e, mask) for e, nelem, mask, _ in ts]
_, ns, sb = gh.planes_layout(shapes)
refs = [gh.encode(np.ascontiguousarray(d.reshape(-1, e)[:, p])) for e, nelem, mask, d in ts for p in range(e) if (mask >> p) & 1]
with gh.BatchEncoder(0) as enc, gh.BatchDecoder(0) as dec, gh.DeviceBuffer(total) as src, \
        gh.DeviceBuffer(total) as dst, gh.DeviceBuffer(max(sb, 16)) as st:
    src.upload(host)
    enc.load_planes_device([(src.addr + o, s[1], s[2], s[3]) for o, s in zip(offs, shapes)], st.addr, sb)
    enc.plan()
    enc.encode()
    enc.wait()
    imgs = enc.download_all()
    assert len(imgs) == ns == len(refs)
    for a, b in zip(imgs, refs):
        assert np.array_equal(a, b)
    dec.load_device(enc.items())
    dec.decode()
    dst.upload(np.full(total, 0xA5, dtype=np.uint8))
    dec.join_planes_device([(dst.addr + o, s[1], s[2], s[3]) for o, s in zip(offs, shapes)], st.addr, sb)
    rep = dec.planes_wait()
    assert rep.bad_tensors == 0 and rep.ntensors == 1503
    got = dst.download(np.zeros(total, dtype=np.uint8))
    keep = np.zeros(total, dtype=bool)
    for (e, nelem, mask, d), o in zip(ts, offs):
        assert np.array_equal(got[o: o + d.size], d)
        keep[o: o + d.size] = True
    assert (got[~keep] == 0xA5).all()
    print("planes one-wave ok", ns)
"""


@pytest.mark.gpu
def test_one_workgroup_walks_many_tensors(gpu):
    """GH_PLANES_GRID=1: one workgroup's four waves walk 1503 tensors of 1..40 elements and
    mixed element sizes, in both directions."""
    r = subprocess.run([sys.executable, "-c", _ONE_WAVE, PKG], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, GH_PLANES_GRID="1"))
    assert r.returncode == 0 and "planes one-wave ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


# ---- (e) one bad plane among good ones ------------------------------------------------------
def _raise_n(img, by):
    """The image with its header N raised (v1 header: u64 S, S x 2 bytes, u32 N); the recipe of
    tests/test_gpu_batch.py."""
    bad = np.array(img, dtype=np.uint8)
    s = int(bad[:8].view("<u8")[0])
    assert s <= 256
    at = 8 + 2 * s
    bad[at: at + 4] = np.asarray([int(bad[at: at + 4].view("<u4")[0]) + by], dtype="<u4").view(np.uint8)
    return bad


@pytest.mark.gpu
def test_one_bad_plane_among_good_ones(gpu, tensors):
    k = next(i for i, t in enumerate(tensors) if t.e == 2 and t.nelem == 4101 and t.mask == 0b10)
    imgs = [[img for img in t.images] for t in tensors]
    imgs[k][0] = _raise_n(imgs[k][0], 1000)
    nelems = [t.nelem for t in tensors]
    nelems[k] += 1000
    slots, ns, sb = gpu.planes_layout(_items(tensors, 0, [0] * len(tensors), nelems))
    stored = np.zeros(sb, dtype=np.uint8)
    for t, sl in zip(tensors, slots):
        for p in range(t.e):
            if sl[p][0] == gpu.GH_PLANES_STORED:
                stored[sl[p][1]: sl[p][1] + t.nelem] = t.planes[p]
    with gpu.BatchDecoder(0) as dec:
        dec.load([img for row in imgs for img in row])
        dec.decode()
        with pytest.raises(gpu.GapHuffError) as e:
            _join(gpu, dec, tensors, stored, nelems=nelems, skip=(k,))
        assert e.value.code == GH_E_CORRUPT
        assert e.value.report.bad_tensors == 1 and e.value.report.ntensors == len(tensors)
        st, _ = dec.status()
        assert np.count_nonzero(st) == 1 and st[slots[k][1][0]] & gpu.GH_ST_BADCODE


# ---- (f) refusals ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu, tensors):
    ts = [t for t in tensors if t.nelem in (17, 1025) and t.e in (2, 4)]
    slots, ns, want = _stored_want(gpu, ts)
    assert ns and want.size
    offs, total = _place(ts, 0)
    imgs = [img for t in ts for img in t.images]

    def code(fn, *a, **kw):
        with pytest.raises(gpu.GapHuffError) as e:
            fn(*a, **kw)
        return e.value.code

    with gpu.DeviceBuffer(total) as buf, gpu.DeviceBuffer(want.size + 32) as st:
        buf.upload(np.zeros(total, dtype=np.uint8))
        st.upload(np.zeros(want.size + 32, dtype=np.uint8))
        items = _items(ts, buf.addr, offs)
        with gpu.BatchEncoder(0) as enc:
            assert code(enc.load_planes_device, items, st.addr, want.size - 1) == GH_E_SMALL
            assert code(enc.load_planes_device, items, st.addr + 4, want.size) == GH_E_ARG
            assert code(enc.load_planes_device, [(buf.addr, 10, 3, 1)], st.addr, want.size) == GH_E_ARG
            assert code(enc.plan) == GH_E_STATE  # (a refused load leaves no batch)
        with gpu.BatchDecoder(0) as dec:
            assert code(dec.planes_wait) == GH_E_STATE
            dec.load(imgs)
            assert code(dec.join_planes_device, items, st.addr, want.size) == GH_E_STATE      # before a decode
            arena = int(dec.offsets()[-1])
            with gpu.DeviceBuffer(arena + 16) as out:
                dec.decode(out.addr, arena)
                dec.wait()
                assert code(dec.join_planes_device, items, st.addr, want.size) == GH_E_STATE  # a caller's arena
            dec.decode()
            assert code(dec.planes_wait) == GH_E_STATE                                        # no join yet
            assert code(dec.join_planes_device, items[:-1], st.addr, want.size) == GH_E_ARG   # fewer streams
            wrong = list(items)
            wrong[0] = (wrong[0][0], wrong[0][1] + 1, wrong[0][2], wrong[0][3])
            assert code(dec.join_planes_device, wrong, st.addr, want.size + 16) == GH_E_ARG   # another nelem
            assert code(dec.join_planes_device, items, st.addr, want.size - 1) == GH_E_SMALL
            assert code(dec.join_planes_device, items, st.addr + 8, want.size) == GH_E_ARG
            dec.join_planes_device(items, st.addr, want.size)
            assert dec.planes_wait().bad_tensors == 0
            dec.load(imgs)
            assert code(dec.planes_wait) == GH_E_STATE                                        # a load drops the join


# ---- (g) the one-call forms and the CLIs ---------------------------------------------------
@pytest.mark.gpu
def test_one_call_forms(gpu):
    rng = np.random.default_rng(9)
    arrays = [rng.normal(0, 0.02, 5000).astype(np.float32), rng.normal(0, 1, 1025).astype(np.float64),
              rng.normal(0, 0.02, 70001).astype(np.float16), rng.integers(0, 9, 333).astype(np.uint8),
              np.zeros(0, dtype=np.float32)]
    for device_plan in (False, True):
        images = gpu.encode_tensors(arrays, device_plan=device_plan)
        for a, img in zip(arrays, images):
            im = gpu.parse_planes(img)
            assert (im.nelem, im.elem_size, im.coded_mask) == (a.size, a.itemsize, 1 << (a.itemsize - 1))
        for a, got in zip(arrays, gpu.decode_tensors(images)):
            assert np.array_equal(got, a.view(np.uint8))
    masks = [0b0110, 0, 0b11, 1, 0b1111]
    for a, got in zip(arrays, gpu.decode_tensors(gpu.encode_tensors(arrays, masks))):
        assert np.array_equal(got, a.view(np.uint8))
    # the float32 tensor: the top plane coded beats the interleaved bytes
    assert images[0].size < gpu.encode(arrays[0].view(np.uint8)).size


@pytest.mark.gpu
def test_cli_round_trip_and_refusals(gpu, tmp_path):
    rng = np.random.default_rng(13)
    arrays = [rng.normal(0, 0.02, n).astype(np.float32).view(np.uint32) for n in (4101, 1, 0, 65536)]
    halves = [(a >> 16).astype(np.uint16) for a in arrays]  # bf16 by truncation
    lines_e, lines_d = [], []
    for i, h in enumerate(halves):
        h.tofile(tmp_path / f"t{i}.bin")
        lines_e.append(f"{tmp_path}/t{i}.bin\t{tmp_path}/t{i}.ghp")
        lines_d.append(f"{tmp_path}/t{i}.ghp\t{tmp_path}/t{i}.out")
    (tmp_path / "enc.txt").write_text("\n".join(lines_e) + "\n")
    (tmp_path / "dec.txt").write_text("\n".join(lines_d) + "\n")
    for extra in ([], ["--device-plan"]):
        r = subprocess.run([ENCODER, "--batch", str(tmp_path / "enc.txt"), "--planes", "2"] + extra, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0 and "Planes: 4 tensors" in r.stdout, r.stdout + r.stderr
        for i, h in enumerate(halves):
            img = np.fromfile(tmp_path / f"t{i}.ghp", dtype=np.uint8)
            planes = gpu.planes_split_host(h)
            assert np.array_equal(img, gpu.planes_image(h.size, 2, 0b10, [planes[0], gpu.encode(planes[1])]))
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "dec.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Planes batch: 4 tensors" in r.stdout, r.stdout + r.stderr
    for i, h in enumerate(halves):
        assert np.array_equal(np.fromfile(tmp_path / f"t{i}.out", dtype=np.uint16), h)
    # an explicit mask: both planes coded
    r = subprocess.run([ENCODER, "--batch", str(tmp_path / "enc.txt"), "--planes", "2:3"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and gpu.parse_planes(np.fromfile(tmp_path / "t0.ghp", dtype=np.uint8)).coded_mask == 3
    # a size that is no multiple of E: refused, the line named
    np.arange(5, dtype=np.uint8).tofile(tmp_path / "odd.bin")
    (tmp_path / "odd.txt").write_text(lines_e[0] + "\n\n" + f"{tmp_path}/odd.bin\t{tmp_path}/odd.ghp\n")
    r = subprocess.run([ENCODER, "--batch", str(tmp_path / "odd.txt"), "--planes", "2"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "line 3" in r.stderr and "odd.bin" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "odd.ghp").exists()
    r = subprocess.run([ENCODER, "--batch", str(tmp_path / "enc.txt"), "--planes", "3"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2
    # a list that mixes containers and compressed.huff files: refused, the line named
    gpu.encode(halves[0].view(np.uint8)).tofile(tmp_path / "plain.huff")
    for first, second, line in ((lines_d[0], f"{tmp_path}/plain.huff\t{tmp_path}/p.out", 2),
                                (f"{tmp_path}/plain.huff\t{tmp_path}/p.out", lines_d[0], 2)):
        (tmp_path / "mix.txt").write_text(first + "\n" + second + "\n")
        r = subprocess.run([DECODER, "--batch", str(tmp_path / "mix.txt")], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and f"line {line}" in r.stderr and "byte-plane" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "p.out").exists()
