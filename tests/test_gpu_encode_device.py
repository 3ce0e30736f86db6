"""Slices from and to device memory: gh_ectx_load_device, gh_ectx_merge_device
(gh_enc_merge_kernel) and, with gh_ectx_index_slice and gh_ctx_load_device, the round trip
in which no byte of input, payload or gap array crosses to the host.  The oracle is the host
encoder's image (gh_encode_write) and the data itself.
"""
import numpy as np
import pytest

import slice_cases as sc

pytestmark = pytest.mark.gpu

GH_E_ARG, GH_E_STATE = -1, -8
SENTINEL = 0xA5C3F00D
PAD = 64  # sentinel words past each array's end


def _same(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ, first at {bad[0]}: "
                             f"{int(got[bad[0]]):#x} for {int(want[bad[0]]):#x}")


def image_words(plan, image):
    """(gap words, payload words) of a compressed.huff image, as np.uint32."""
    gw, w = -(-plan.g // 8), plan.w
    body = np.frombuffer(image.tobytes()[image.size - 4 * (gw + w):], dtype=np.uint32)
    return body[:gw], body[gw:]


class Arrays:
    """Zeroed device arrays of the stream's W payload and ceil(G / 8) gap words, each followed
    by PAD sentinel words."""

    def __init__(self, gh, plan):
        self.w, self.gw = plan.w, -(-plan.g // 8)
        self.pay = gh.DeviceBuffer(4 * (self.w + PAD))
        self.gap = gh.DeviceBuffer(4 * (self.gw + PAD))
        for buf, n in ((self.pay, self.w), (self.gap, self.gw)):
            init = np.zeros(n + PAD, dtype=np.uint32)
            init[n:] = SENTINEL
            buf.upload(init)

    def merge(self, e, **kw):
        e.merge_device(self.pay.addr, self.w, self.gap.addr, self.gw, **kw)

    def check(self, plan, image, what):
        pay = self.pay.download(np.zeros(self.w + PAD, dtype=np.uint32))
        gap = self.gap.download(np.zeros(self.gw + PAD, dtype=np.uint32))
        wg, ww = image_words(plan, image)
        _same(gap[: self.gw], wg, f"{what}: gap words")
        _same(pay[: self.w], ww, f"{what}: payload words")
        assert (pay[self.w:] == SENTINEL).all() and (gap[self.gw:] == SENTINEL).all(), f"{what}: sentinels"

    def close(self):
        self.pay.close()
        self.gap.close()


# ---- 1. load_device
@pytest.mark.parametrize("n", [0, 1, 8193, 1_000_003])
def test_load_device_from_a_device_buffer(gpu, n):
    data = gpu.generate(7, 0.5, n)
    with gpu.DeviceBuffer(n + 16) as buf, gpu.Encoder(0) as e:
        for off in (0, 1):  # an aligned and an odd source address
            buf.upload(np.concatenate([np.zeros(off, dtype=np.uint8), data, np.zeros(16 - off, dtype=np.uint8)]))
            e.load_device(buf.addr + off, n)
            e.make_plan()
            e.encode()
            _same(e.download(), gpu.encode(data), f"n = {n}, source offset {off}")
    with gpu.Encoder(0) as e:
        with pytest.raises(gpu.GapHuffError) as err:
            e.load_device(0, 5)
        assert err.value.code == GH_E_ARG


@pytest.mark.parametrize("n", [0, 1, 8193, 1_000_003])
def test_load_device_from_a_torch_tensor(gpu, n):
    """The tensor is filled by torch ops enqueued just before the load, on a stream of torch's
    own: the load's copy must wait for them."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    dev = torch.device("cuda:0")
    want = ((np.arange(n, dtype=np.int64) * 7 + 3) % 61).astype(np.uint8)
    with gpu.Encoder(0) as e, torch.cuda.stream(torch.cuda.Stream(device=dev)):
        t = ((torch.arange(n, device=dev, dtype=torch.int64) * 7 + 3) % 61).to(torch.uint8)
        e.load_device(t.data_ptr() if n else 0, n, torch.cuda.current_stream().cuda_stream)
        e.make_plan()
        e.encode()
        _same(e.download(), gpu.encode(want), f"n = {n}")
        # the load resets the state as gh_ectx_load does
        e.load_device(t.data_ptr() if n else 0, n, torch.cuda.current_stream().cuda_stream)
        with pytest.raises(gpu.GapHuffError) as err:
            e.encode()
        assert err.value.code == GH_E_STATE


# ---- 2. merge_device
def device_merge(gpu, name, label, order):
    data, plan, start, image = sc.case_input(gpu, name)
    b = sc.case_bounds(name, label, data.size)
    cuts = list(zip(b[:-1], b[1:]))
    arr = Arrays(gpu, plan)
    try:
        with gpu.Encoder(0) as e:
            for lo, hi in (cuts if order > 0 else cuts[::-1]):
                e.load(data[lo:hi])
                e.encode_slice(plan, int(start[lo]))
                arr.merge(e)
        arr.check(plan, image, f"{name} {label} order {order}")
    finally:
        arr.close()


@pytest.mark.parametrize("order", [1, -1])
@pytest.mark.parametrize("name,label", [("gen", "K7"), ("two", "every3"), ("flat", "aligned")])
def test_merge_device(gpu, name, label, order):
    device_merge(gpu, name, label, order)


def test_merge_device_whole_encode(gpu):
    """A whole encode is the slice at bit 0."""
    data, plan, start, image = sc.case_input(gpu, "gen")
    arr = Arrays(gpu, plan)
    try:
        with gpu.Encoder(0) as e:
            e.load(data)
            e.make_plan()
            e.encode()
            arr.merge(e)
        arr.check(plan, image, "whole encode")
    finally:
        arr.close()


def test_merge_device_two_contexts_two_streams(gpu):
    """Two contexts of one device merge halves that share their seam words, each on a stream
    of its own (torch's), the later slice first."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    data, plan, start, image = sc.case_input(gpu, "gen")
    arr = Arrays(gpu, plan)
    mid = data.size // 2 + 1
    try:
        with gpu.Encoder(0) as e0, gpu.Encoder(0) as e1:
            s0, s1 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
            e0.load(data[:mid])
            e0.encode_slice(plan, 0)
            e1.load(data[mid:])
            e1.encode_slice(plan, int(start[mid]))
            arr.merge(e1, hip_stream=s1.cuda_stream)
            arr.merge(e0, hip_stream=s0.cuda_stream)
        arr.check(plan, image, "two contexts, two streams")
    finally:
        arr.close()


def test_merge_device_refusals(gpu):
    data, plan, start, image = sc.case_input(gpu, "gen")
    arr = Arrays(gpu, plan)
    try:
        with gpu.Encoder(0) as e:
            e.load(data[1000:])
            with pytest.raises(gpu.GapHuffError) as err:
                arr.merge(e)  # before any encode
            assert err.value.code == GH_E_STATE
            e.encode_slice(plan, int(start[1000]))
            bad = (
                (arr.pay.addr + 4, arr.w, arr.gap.addr, arr.gw),   # misaligned destinations
                (arr.pay.addr, arr.w, arr.gap.addr + 8, arr.gw),
                (arr.pay.addr, arr.w - 1, arr.gap.addr, arr.gw),   # extents past the caps
                (arr.pay.addr, arr.w, arr.gap.addr, arr.gw - 1),
                (0, arr.w, arr.gap.addr, arr.gw),                  # nulls
                (arr.pay.addr, arr.w, 0, arr.gw),
            )
            for args in bad:
                with pytest.raises(gpu.GapHuffError) as err:
                    e.merge_device(*args)
                assert err.value.code == GH_E_ARG, args
            e.load(data[:1000])  # a load drops the encode
            with pytest.raises(gpu.GapHuffError) as err:
                arr.merge(e)
            assert err.value.code == GH_E_STATE
        # nothing was written by a refused call
        pay = arr.pay.download(np.zeros(arr.w + PAD, dtype=np.uint32))
        gap = arr.gap.download(np.zeros(arr.gw + PAD, dtype=np.uint32))
        assert not pay[: arr.w].any() and not gap[: arr.gw].any()
    finally:
        arr.close()


# ---- 3. the round trip with no host copy of the stream
def test_round_trip_on_the_device(gpu):
    data, plan_want, start, image = sc.case_input(gpu, "gen")
    n, K, k = data.size, 5, 8
    cuts = [n * i // K for i in range(K + 1)]
    rng = np.random.default_rng(12)
    with gpu.DeviceBuffer(n) as src:
        src.upload(data)  # the resident input; from here on only counts, bit totals and entries cross
        encs = [gpu.Encoder(0) for _ in range(K)]
        try:
            counts = []
            for e, lo, hi in zip(encs, cuts[:-1], cuts[1:]):
                e.load_device(src.addr + lo, hi - lo)
                counts.append(e.counts())
            plan = gpu.plan_from_counts(np.sum(counts, axis=0, dtype=np.uint64))
            assert bytes(plan) == bytes(plan_want)
            lens = np.frombuffer(bytes(plan.len), dtype=np.uint8).astype(np.uint64)
            arr = Arrays(gpu, plan)
            parts, base = [], 0
            for e, c, lo in zip(encs, counts, cuts[:-1]):
                s, _ = e.encode_slice(plan, base)
                ent, k0, _ = e.index_slice(lo, k)
                parts.append((ent, k0))
                arr.merge(e)
                base += int((c * lens).sum())
            assert base == plan.bits
        finally:
            for e in encs:
                e.close()
    try:
        index = gpu.merge_index_slices(plan, k, parts[::-1])
        _same(index, gpu.encode_index(data, k), "merged index")
        with gpu.Decoder(0) as d:
            d.load_device(gpu.Stream.from_plan(plan), arr.pay.addr, arr.w, arr.gap.addr)
            d.decode(timed=False)
            rep = d.report()
            assert rep.status == 0 and rep.symbols >= n
            _same(d.download(n), data, "decode of the merged arrays")
            d.set_index(index)
            lo = rng.integers(0, n - 2000, 300)
            r = np.stack([lo, lo + rng.integers(0, 2000, 300)], 1).astype(np.uint64)
            total = int((r[:, 1] - r[:, 0]).sum())
            with gpu.DeviceBuffer(r.nbytes) as dr, gpu.DeviceBuffer(total + 16) as dst:
                dr.upload(r)
                d.gather_device(dr.addr, 300, dst.addr, total)
                grep = d.gather_wait()
                assert grep.out_bytes == total and grep.status == 0
                got = dst.download(np.zeros(total + 16, dtype=np.uint8))[:total]
            want = np.concatenate([data[int(a):int(b)] for a, b in r])
            _same(got, want, "gather of 300 ranges")
    finally:
        arr.close()
