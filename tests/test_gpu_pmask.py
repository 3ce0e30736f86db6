"""Plane choice on the GPU: gh_pmask_device's histogram and decide kernels around the batched
encode's code kernel, encode_tensors(..., "auto") and bin/encoder --planes E:auto.

The ground truth is the host encoder and numpy: np.bincount of every plane (numpy
a.reshape(-1, E)[:, p]) and len(gh.encode(plane)).  Sizes: every element size crossed with
nelem = 0, 1, 15, 16, 17 (the lane edges: a lane owns 16 elements), 1023, 1024, 1025 (the unit
edges: a unit is 1024 elements), 4101 (several units and a ragged tail) and 65536 (64 units: more
than one workgroup), all as one tensor list from one fill-padded source buffer."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_planes import DECODER, ELEMS, ENCODER, NELEMS, SRC_FILL, Tensor, _items, _place
from test_planes import bf16_weights

GH_E_ARG, GH_E_STATE = -1, -8
TIES = ((29, 0), (30, 0), (31, 1), (33, 0), (34, 0), (35, 1))


@pytest.fixture(scope="module")
def tensors(gh):
    return [Tensor(gh, e, nelem, 0, 500 * e + 3 * nelem) for e in ELEMS for nelem in NELEMS]


@pytest.fixture(scope="module")
def cpu_rule(gh, tensors):
    """(masks, plane_bytes) of `tensors` by gh.encode, computed once."""
    masks, sizes = [], []
    for t in tensors:
        fb = [len(gh.encode(pl)) if t.nelem else 0 for pl in t.planes]
        masks.append(sum(1 << p for p in range(t.e) if t.nelem and fb[p] < t.nelem))
        sizes.append(fb + [0] * (8 - t.e))
    return np.asarray(masks, dtype=np.uint32), np.asarray(sizes, dtype=np.uint64)


def _upload(gpu, ts, shift):
    offs, total = _place(ts, shift)
    host = np.full(total, SRC_FILL, dtype=np.uint8)
    for t, o in zip(ts, offs):
        host[o: o + t.data.size] = t.data
    src = gpu.DeviceBuffer(total)
    src.upload(host)
    assert src.addr % 16 == 0
    return src, _items(ts, src.addr, offs)


def _check_counts(enc, ts):
    q = 0
    for t in ts:
        for p in range(t.e):
            want = np.bincount(t.planes[p], minlength=256)
            got = enc.pmask_counts(q)
            assert np.array_equal(got, want), (t.e, t.nelem, p, int(got[SRC_FILL]), int(want[SRC_FILL]))
            q += 1
    with pytest.raises(Exception) as e:
        enc.pmask_counts(q)
    assert e.value.code == GH_E_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ("0", "1"))
@pytest.mark.parametrize("shift", (0, 1, 5))
def test_counts_and_decisions(gpu, tensors, cpu_rule, shift, merge, monkeypatch):
    monkeypatch.setenv("GH_PMASK_MERGE", merge)
    with gpu.BatchEncoder(0) as enc:
        src, items = _upload(gpu, tensors, shift)
        with src:
            masks, pb = enc.choose_masks_device(items)
        _check_counts(enc, tensors)
    assert np.array_equal(pb, cpu_rule[1]), "plane_bytes against len(gh.encode(plane))"
    assert np.array_equal(masks, cpu_rule[0])
    hm, hpb = gpu.choose_planes_masks([t.data.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.e]) for t in tensors])
    assert np.array_equal(masks, hm) and np.array_equal(pb, hpb)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ("0", "1"))
@pytest.mark.parametrize("grid", ("1", "3"))
def test_few_workgroups_walk_all_tensors(gpu, tensors, cpu_rule, grid, merge, monkeypatch):
    """GH_PLANES_GRID: a wave's run crosses tensors of every element size, so its counters are
    flushed when it leaves a tensor."""
    monkeypatch.setenv("GH_PLANES_GRID", grid)
    monkeypatch.setenv("GH_EBATCH_GRID", grid)
    monkeypatch.setenv("GH_PMASK_MERGE", merge)
    order = tensors[::-1]
    with gpu.BatchEncoder(0) as enc:
        src, items = _upload(gpu, order, 1)
        with src:
            masks, pb = enc.choose_masks_device(items)
        _check_counts(enc, order)
    assert np.array_equal(masks, cpu_rule[0][::-1]) and np.array_equal(pb, cpu_rule[1][::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ("0", "1"))
def test_hot_bins(gpu, merge, monkeypatch):
    monkeypatch.setenv("GH_PMASK_MERGE", merge)
    zeros = np.zeros(65536, dtype=np.int32)
    with gpu.BatchEncoder(0) as enc, gpu.DeviceBuffer(zeros.nbytes) as src:
        src.upload(zeros.view(np.uint8))
        masks, pb = enc.choose_masks_device([(src.addr, zeros.size, 4)])
        for q in range(4):
            assert enc.pmask_counts(q).tolist() == [65536] + [0] * 255
    assert masks.tolist() == [0b1111]
    assert pb[0].tolist() == [len(gpu.encode(np.zeros(65536, np.uint8)))] * 4 + [0] * 4


@pytest.mark.gpu
def test_tie_table(gpu):
    ts = [np.full(n, 0x3C, dtype=np.uint8) for n, _ in TIES]
    host = np.concatenate(ts)
    offs = np.concatenate([[0], np.cumsum([t.size for t in ts])])
    with gpu.BatchEncoder(0) as enc, gpu.DeviceBuffer(host.size) as src:
        src.upload(host)
        masks, pb = enc.choose_masks_device([(src.addr + int(o), t.size, 1) for o, t in zip(offs, ts)])
        rep = enc.pmask_report()
    assert masks.tolist() == [c for _, c in TIES]
    assert pb[:, 0].tolist() == [26 + 4 * -(-n // 32) for n, _ in TIES] == [len(gpu.encode(t)) for t in ts]
    assert rep.coded_planes == 2 and rep.raw_bytes == host.size and rep.chosen_bytes == 29 + 30 + 30 + 33 + 34 + 34


@pytest.mark.gpu
def test_state_is_left_alone(gpu, tensors):
    """A choose call between a plan and an encode, on other tensors: the images are those of a
    run without it.  And a choose call is legal before any load."""
    loaded = [Tensor(gpu, t.e, t.nelem, (1 << t.e) - 1, 77 + i) for i, t in enumerate(tensors) if t.nelem in (17, 1025, 4101)]
    others = [t for t in tensors if t.nelem in (1024, 65536)]
    images = []
    for choose in (False, True):
        with gpu.BatchEncoder(0) as enc:
            src, items = _upload(gpu, loaded, 5)
            osrc, oitems = _upload(gpu, others, 1)
            with src, osrc:
                if choose:
                    first, _ = enc.choose_masks_device(oitems)  # before any load
                enc.load_planes_device(items, 0, 0)
                enc.plan_device()
                if choose:
                    masks, _ = enc.choose_masks_device(oitems)
                    assert np.array_equal(masks, first)
                    assert np.array_equal(enc.pmask_counts(0), np.bincount(others[0].planes[0], minlength=256))
                enc.encode()
                rep = enc.wait()
                assert rep.nstreams == sum(t.e for t in loaded)
                images.append(enc.download_all())
    assert len(images[0]) == len(images[1])
    for a, b in zip(*images):
        assert np.array_equal(a, b)
    refs = [img for t in loaded for img in t.images]
    for a, ref in zip(images[1], refs):
        assert np.array_equal(a, ref)


@pytest.mark.gpu
def test_report_and_refusals(gpu, tensors, cpu_rule):
    with gpu.BatchEncoder(0) as enc:
        with pytest.raises(gpu.GapHuffError) as e:
            enc.pmask_counts(0)
        assert e.value.code == GH_E_STATE
        src, items = _upload(gpu, tensors, 0)
        with src:
            masks, pb = enc.choose_masks_device(items)
            rep = enc.pmask_report()
            assert rep.launches == gpu.GH_PMASK_LAUNCHES == 4 and rep.ntensors == len(tensors)
            assert rep.coded_planes == sum(bin(int(m)).count("1") for m in cpu_rule[0])
            assert rep.raw_bytes == sum(t.data.size for t in tensors)
            want = sum(int(fb) if int(fb) < t.nelem else t.nelem for t, row in zip(tensors, cpu_rule[1]) for fb in row[: t.e])
            assert rep.chosen_bytes == want
            assert rep.hist_ms > 0 and rep.code_ms > 0 and rep.decide_ms > 0
            # refusals: nulls, a bad element size, a null tensor; the last result stays readable
            L = gpu.lib().gh_pmask_device
            arr, n = gpu._planes_items(items)
            m = np.zeros(n, np.uint32)
            assert L(enc._h, None, n, gpu._ptr(m), None, None, None) == GH_E_ARG
            assert L(enc._h, arr, n, None, None, None, None) == GH_E_ARG
            assert L(None, arr, n, gpu._ptr(m), None, None, None) == GH_E_ARG
            for bad in ((items[5][0], 4, 3, 0), (0, 4, 2, 0)):
                with pytest.raises(gpu.GapHuffError) as e:
                    enc.choose_masks_device(items[:3] + [bad])
                assert e.value.code == GH_E_ARG
            # no tensors: nothing launched, nothing to read
            masks0, pb0 = enc.choose_masks_device([])
            assert masks0.size == 0 and pb0.shape == (0, 8) and enc.pmask_report().launches == 0
            with pytest.raises(gpu.GapHuffError) as e:
                enc.pmask_counts(0)
            assert e.value.code == GH_E_ARG
            # sizes are optional
            assert L(enc._h, arr, n, gpu._ptr(m), None, None, None) == 0 and np.array_equal(m, cpu_rule[0])


@pytest.mark.gpu
@pytest.mark.parametrize("device_plan", (False, True))
def test_encode_tensors_auto(gpu, device_plan):
    rng = np.random.default_rng(21)
    arrays = [bf16_weights(), rng.integers(0, 1000, 65536).astype(np.int32), rng.integers(0, 256, 65536, dtype=np.uint8),
              np.zeros(0, dtype=np.float32), np.cumsum(rng.integers(0, 50, 17)).astype(np.int64) + 1_700_000_000_000]
    want, _ = gpu.choose_planes_masks(arrays)
    assert want.tolist()[:4] == [0b10, 0b1110, 0, 0]
    images = gpu.encode_tensors(arrays, "auto", device_plan=device_plan)
    assert [gpu.parse_planes(img).coded_mask for img in images] == want.tolist()
    for a, img in zip(arrays, images):
        planes = gpu.planes_split_host(a)
        m = gpu.parse_planes(img).coded_mask
        assert np.array_equal(img, gpu.planes_image(a.size, a.dtype.itemsize, m,
                                                    [gpu.encode(pl) if (m >> p) & 1 else pl for p, pl in enumerate(planes)]))
    for a, out in zip(arrays, gpu.decode_tensors(images)):
        assert np.array_equal(out, a.view(np.uint8).reshape(-1))
    # the default stays the top plane
    assert [gpu.parse_planes(img).coded_mask for img in gpu.encode_tensors(arrays[:3])] == [0b10, 0b1000, 1]
    with pytest.raises(gpu.GapHuffError):
        gpu.encode_tensors(arrays[:1], "best")


@pytest.mark.gpu
def test_cli_auto(gpu, tmp_path):
    rng = np.random.default_rng(4)
    files = [rng.integers(0, 1000, 20000).astype(np.int32), rng.normal(0, 0.02, 20000).astype(np.float32)]
    want, _ = gpu.choose_planes_masks(files)
    assert want.tolist() == [0b1110, 0b1000]
    lines_e, lines_d = [], []
    for i, a in enumerate(files):
        a.tofile(tmp_path / f"t{i}.bin")
        lines_e.append(f"{tmp_path}/t{i}.bin\t{tmp_path}/t{i}.ghp")
        lines_d.append(f"{tmp_path}/t{i}.ghp\t{tmp_path}/t{i}.out")
    (tmp_path / "enc.txt").write_text("\n".join(lines_e) + "\n")
    (tmp_path / "dec.txt").write_text("\n".join(lines_d) + "\n")
    r = subprocess.run([ENCODER, "--batch", str(tmp_path / "enc.txt"), "--planes", "4:auto"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "mask auto: 4 coded planes" in r.stdout, r.stdout + r.stderr
    for i, m in enumerate(want.tolist()):
        assert gpu.parse_planes(np.fromfile(tmp_path / f"t{i}.ghp", dtype=np.uint8)).coded_mask == m
    r = subprocess.run([DECODER, "--batch", str(tmp_path / "dec.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for i, a in enumerate(files):
        assert np.array_equal(np.fromfile(tmp_path / f"t{i}.out", dtype=a.dtype), a)
    r = subprocess.run([ENCODER, "--batch", str(tmp_path / "enc.txt"), "--planes", "4:autox"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2
    assert os.path.exists(tmp_path / "t0.ghp")
