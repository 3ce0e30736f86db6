"""Batched encode with the codes built on the GPU: gh_batchenc_plan_device /
BatchEncoder.plan_device / encode_batch(device_plan=True) and the encoder CLI's --device-plan.

The reference is the host: every image is compared byte for byte with gh.encode(data), every
plan_of(i) with gh_ebatch_plan's on the same loaded batch, field by field and as bytes
(count[] included).  The inputs are the smallest that reach each step of gh_ebatch_code_kernel:
  empty, 1 byte, one symbol x 1 000: the paths without a package-merge (ns = 0, 1);
  two symbols: the smallest merge (need = 2);
  256 symbols x 1 and 256 symbols x 4 shuffled: full lists of 510 items at every level, all
    counts tied (the sort's tie-break by symbol value is the header's order);
  255 symbols: an odd list (the dropped last item);
  Fibonacci counts over 20 symbols (17 710 bytes) and powers of two over 17 symbols (131 071
    bytes): the 16-bit limit binds, lengths reach 16;
  gh.generate at r = 0, 0.5, 0.999 x 20 000 bytes, and every .bin under tests/golden.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENCODER = os.path.join(ROOT, "bin", "encoder")
GH_E_STATE = -8
FIELDS = ("n", "bits", "w", "g", "file_bytes", "nsyms", "version")

_cache = {}


def _inputs(gh):
    """[(name, data)] of the mixed batch, made once."""
    if "mixed" in _cache:
        return _cache["mixed"]
    rng = np.random.default_rng(528)
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    out = [
        ("empty", np.zeros(0, dtype=np.uint8)),
        ("one_byte", np.asarray([200], dtype=np.uint8)),
        ("one_symbol_1000", np.full(1000, 7, dtype=np.uint8)),
        ("two_symbols", np.asarray([3] * 5 + [250] * 2, dtype=np.uint8)),
        ("all256_x1", rng.permutation(256).astype(np.uint8)),
        ("all256_x4_shuffled", rng.permutation(np.repeat(np.arange(256), 4)).astype(np.uint8)),
        ("255_symbols", rng.permutation(np.repeat(np.arange(1, 256), 1 + np.arange(255) % 3)).astype(np.uint8)),
        ("fibonacci_20", rng.permutation(np.repeat((np.arange(20) * 11 + 5) % 256, fib)).astype(np.uint8)),
        ("powers_of_two_17", rng.permutation(np.repeat((np.arange(17) * 13 + 1) % 256, 1 << np.arange(17))).astype(np.uint8)),
    ]
    assert out[7][1].size == 17_710 and out[8][1].size == 131_071
    for i, r in enumerate((0.0, 0.5, 0.999)):
        out.append((f"gen_r{r}_20000", gh.generate(900 + i, r, 20_000)))
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.bin"))):
        out.append((os.path.basename(path), np.fromfile(path, dtype=np.uint8)))
    out = [(name, np.ascontiguousarray(d, dtype=np.uint8)) for name, d in out]
    for _, d in out:
        d.setflags(write=False)
    _cache["mixed"] = out
    return out


def _tiny(gh):
    """1 503 streams of 1 to 40 bytes from a seeded generator."""
    if "tiny" not in _cache:
        rng = np.random.default_rng(1503)
        ns = rng.integers(1, 41, 1503)
        _cache["tiny"] = [gh.generate(3000 + i, (0.1, 0.5, 0.9)[i % 3], int(n)) for i, n in enumerate(ns)]
    return _cache["tiny"]


def _want(gh, key, datas):
    """The host encoder's images of a batch, made once."""
    if key not in _cache:
        _cache[key] = [gh.encode(d) for d in datas]
    return _cache[key]


def _images(b, want):
    sizes = b.sizes()
    assert sizes.size == len(want)
    for i, ref in enumerate(want):
        got = b.download(i)
        assert got.size == int(sizes[i]) == ref.size, f"stream {i}: length {got.size}, host {ref.size}"
        assert np.array_equal(got, ref), f"stream {i} differs at byte {int(np.argmax(got != ref))}"


def _plans_equal(dev, host, i):
    for f in FIELDS:
        assert getattr(dev, f) == getattr(host, f), f"stream {i}: {f}"
    k = int(host.nsyms)
    assert [(s.symbol, s.length) for s in dev.syms[:k]] == [(s.symbol, s.length) for s in host.syms[:k]], f"stream {i}: syms"
    for f in ("code", "len", "count"):
        assert list(getattr(dev, f)) == list(getattr(host, f)), f"stream {i}: {f}[]"
    assert bytes(dev) == bytes(host), f"stream {i}: the structs differ outside their named fields"


def _check_batch(gh, datas, want):
    """plan_device + encode against the host images; every plan_of against gh_ebatch_plan's."""
    with gh.BatchEncoder(0) as b:
        b.load(datas)
        b.plan()
        host = [b.plan_of(i) for i in range(len(datas))]
        b.plan_device()
        b.encode()
        rep = b.wait()
        assert rep.status == 0 and rep.nstreams == len(datas)
        assert rep.out_bytes == sum(w.size for w in want)
        _images(b, want)
        for i in range(len(datas)):
            _plans_equal(b.plan_of(i), host[i], i)


@pytest.fixture
def mixed(gpu, monkeypatch):
    monkeypatch.delenv("GH_EBATCH_GRID", raising=False)
    datas = [d for _, d in _inputs(gpu)]
    return datas, _want(gpu, "mixed_img", datas)


@pytest.mark.gpu
def test_mixed_batch(gpu, mixed):
    datas, want = mixed
    lens = [max(l for _, l in gpu.parse(img).symbols) for (name, _), img in zip(_inputs(gpu), want)
            if name in ("fibonacci_20", "powers_of_two_17")]
    assert lens == [16, 16]
    _check_batch(gpu, datas, want)


def child_main():
    """GH_EBATCH_GRID=1 (set by the parent): one workgroup walks the mixed batch, then 1 503 tiny
    streams of different ns, through the code kernel's barriers."""
    assert os.environ.get("GH_EBATCH_GRID") == "1"
    try:
        import torch  # noqa: F401  (first, as tests/conftest.py)
    except ImportError:
        pass
    import gaphuff as gh
    datas = [d for _, d in _inputs(gh)]
    _check_batch(gh, datas, [gh.encode(d) for d in datas])
    tiny = _tiny(gh)
    _check_batch(gh, tiny, [gh.encode(d) for d in tiny])
    print(f"child ok: {len(datas)} + {len(tiny)} streams")


@pytest.mark.gpu
def test_many_streams_one_workgroup(gpu):
    code = ("import sys; sys.path[:0] = %r; import test_gpu_ebatch_plan_device as t; t.child_main()"
            % [os.path.join(ROOT, "cse375-finalproj-huffman-decoding_amd"), os.path.join(ROOT, "tests")])
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GH_EBATCH_GRID="1"))
    assert r.returncode == 0 and "child ok: " in r.stdout and "+ 1503 streams" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_round_trip_on_the_device(gpu, mixed):
    datas, _ = mixed
    with gpu.BatchEncoder(0) as e, gpu.BatchDecoder(0) as d:
        e.load(datas)
        e.plan_device()
        e.encode()
        e.wait()
        d.load_device(e.items())
        d.decode()
        rep = d.wait()
        assert rep.bad_streams == 0 and rep.nstreams == len(datas)
        for i, (got, x) in enumerate(zip(d.download_all(), datas)):
            assert np.array_equal(got, x), f"stream {i} did not round-trip"


@pytest.mark.gpu
def test_state_and_refusals(gpu, mixed):
    datas, want = mixed
    with gpu.BatchEncoder(0) as b:
        for f in (b.plan_device, b.plan_times):
            with pytest.raises(gpu.GapHuffError) as e:
                f()
            assert e.value.code == GH_E_STATE
        b.load(datas)
        with pytest.raises(gpu.GapHuffError) as e:
            b.plan_times()
        assert e.value.code == GH_E_STATE
        launches = []
        for plan, on_device in ((b.plan_device, True), (b.plan, False), (b.plan_device, True)):
            plan()
            t = b.plan_times()
            assert t["hist_ms"] > 0 and t["host_ms"] > 0
            assert (t["code_ms"] > 0) if on_device else (t["code_ms"] == 0)
            b.encode()
            rep = b.wait()
            assert rep.status == 0 and rep.hist_ms == pytest.approx(t["hist_ms"]) and rep.plan_host_ms == pytest.approx(t["host_ms"])
            launches.append(rep.launches)
            _images(b, want)
        assert launches[0] == launches[1] == launches[2] and 1 <= launches[0] <= 8
        b.load(datas[:3])  # a load invalidates the plan
        with pytest.raises(gpu.GapHuffError) as e:
            b.encode()
        assert e.value.code == GH_E_STATE
        b.plan_device(force_version=2)
        b.encode()
        b.wait()
        for i, d in enumerate(datas[:3]):
            assert b.plan_of(i).version == 2
            assert np.array_equal(b.download(i), gpu.encode(d, force_version=2)), i
        b.load([])
        b.plan_device()
        assert b.sizes().size == 0 and b.plan_times()["code_ms"] == 0


@pytest.mark.gpu
def test_encode_batch_device_plan(gpu, mixed):
    datas, want = mixed
    for got, ref in zip(gpu.encode_batch(datas[:8], device_plan=True), want[:8]):
        assert np.array_equal(got, ref)
    assert gpu.encode_batch([], device_plan=True) == []


@pytest.mark.gpu
def test_cli_device_plan(gpu, mixed, tmp_path):
    datas, want = mixed
    names = [n for n, _ in _inputs(gpu)]
    pick = [names.index(n) for n in ("empty", "one_byte", "all256_x4_shuffled", "fibonacci_20", "gen_r0.5_20000")]
    outs = {}
    for tag, extra in (("host", []), ("device", ["--device-plan"])):
        lines = []
        for k in pick:
            src = tmp_path / f"{k}.bin"
            datas[k].tofile(src)
            lines.append(f"{src}\t{tmp_path / f'{k}.{tag}.huff'}\n")
        lst = tmp_path / f"{tag}.txt"
        lst.write_text("".join(lines))
        r = subprocess.run([ENCODER, "--batch", str(lst), "--gpu", "0", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
        assert "Batch: 5 streams" in r.stdout and ("code kernel" in r.stdout) == bool(extra)
        outs[tag] = [np.fromfile(tmp_path / f"{k}.{tag}.huff", dtype=np.uint8) for k in pick]
    for k, a, c in zip(pick, outs["host"], outs["device"]):
        assert np.array_equal(a, c) and np.array_equal(c, want[k]), names[k]
    bad = subprocess.run([ENCODER, "--batch", str(tmp_path / "host.txt"), "--device-plans"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 2 and "--device-plan" in bad.stderr
