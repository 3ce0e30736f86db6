# Random access (DESIGN.md "Random access"): what the seek index costs to build and what a
# byte-range decode saves, on one GPU.  Per workload (1 GB at r = 0.1 and r = 0.9:
# BASELINE's cfg4 and cfg3), in one process:
#   * gh_ctx_build_index's kernel_ms at stride 2^8, next to the same context's full-decode
#     kernel_ms and a gh_bw_copy pass over the payload bytes;
#   * wall time of a byte-range decode (locate, load of the located segments, decode,
#     download) for a 1 MiB and a 64 MiB range, from a device-resident stream
#     (gh_ctx_load_device) and from host memory (decode_range);
#   * wall time of the whole-stream load, decode and download.
# Usage: python scripts/bench_index.py [cfg4 cfg3] [--out profiles/index.jsonl]
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

WORKLOADS = {"cfg2": (10**8, 0.5), "cfg3": (10**9, 0.9), "cfg4": (10**9, 0.1)}
REPS = 5


def med(xs):
    return round(float(np.median(xs)), 4)


def wall_ms(f, reps=REPS):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return med(out)


def range_from_device(s, ix, d_pay, d_gap, lo, hi):
    """decode_range with the stream's words already in device memory."""
    b, e, skip = ix.locate(lo, hi)
    with gh.Decoder(0) as d:
        gh._check(gh.lib().gh_ctx_load_device(d._h, ctypes.byref(s.c), b, e, ctypes.c_void_p(d_pay.addr + 16 * b),
                                              s.w - 4 * b, d_gap.ptr, skip + hi - lo))
        d.decode(timed=False)
        assert d.report().status == 0
        return d.download(hi - lo, offset=skip)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    lines = []
    for wl in args or ["cfg4", "cfg3"]:
        n, r = WORKLOADS[wl]
        data = gh.generate(375, r, n)
        img = gh.encode(data, threads=16)
        s = gh.parse(img)
        res = {"workload": wl, "n": n, "r": r, "g": s.g, "payload_bytes": 4 * s.w, "log2_stride": 8}
        with gh.Decoder(0) as d:
            d.load(s)
            d.decode()  # warm-up
            d.report()
            d.reset_timing()
            for _ in range(REPS):
                d.decode()
            rep = d.report()
            builds = [d.build_index(8) for _ in range(REPS + 1)][1:]
            image = builds[0][0]
            res.update({"mode": gh.MODE_NAMES[rep.mode], "decode_kernel_ms": round(rep.kernel_ms, 4),
                        "index_kernel_ms": med([b[2] for b in builds]), "index_bytes": int(image.size),
                        "symbols_match": builds[0][1] == rep.symbols})
        ix = gh.parse_index(image)
        gap_bytes = 4 * ((s.g + 7) // 8)
        off_gap = int(s.c.gap_words) - s.raw.ctypes.data
        off_pay = int(s.c.payload) - s.raw.ctypes.data
        nb = (4 * s.w + 15) // 16 * 16
        with gh.DeviceBuffer(nb + 64) as d_pay, gh.DeviceBuffer(gap_bytes + 64) as d_gap, \
                gh.DeviceBuffer(nb + 64) as d_tmp:
            d_pay.upload(s.raw[off_pay: off_pay + 4 * s.w])
            d_gap.upload(s.raw[off_gap: off_gap + gap_bytes])
            res["payload_copy_ms"] = round(gh.bw_copy(d_tmp.addr, d_pay.addr, nb, reps=REPS), 4)
            ok = True
            for label, size in (("1MiB", 1 << 20), ("64MiB", 64 << 20)):
                lo = n // 2 + 12345
                hi = lo + size
                ok &= bool(np.array_equal(range_from_device(s, ix, d_pay, d_gap, lo, hi), data[lo:hi]))
                ok &= bool(np.array_equal(gh.decode_range(s, ix, lo, hi), data[lo:hi]))
                res[f"range_{label}_device_ms"] = wall_ms(lambda: range_from_device(s, ix, d_pay, d_gap, lo, hi))
                res[f"range_{label}_host_ms"] = wall_ms(lambda: gh.decode_range(s, ix, lo, hi))

        def whole():
            with gh.Decoder(0) as d:
                d.load(s)
                d.decode(timed=False)
                d.report()
                return d.download(n)

        ok &= bool(np.array_equal(whole(), data))
        res["whole_stream_ms"] = wall_ms(whole, reps=3)
        res["bitexact"] = ok
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        if out_path:  # (rewritten after every workload: a later failure keeps the earlier lines)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")
        del data, img, s


if __name__ == "__main__":
    main()
