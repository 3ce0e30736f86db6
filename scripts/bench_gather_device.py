# Device-planned gather (DESIGN.md "Device-planned gather") against the host-planned one, on
# the batch of scripts/bench_gather.py: 4 096 random 4 KiB ranges of a 1 GB gh_generate
# stream (r = 0.1) with an index of stride 2^8, on one GPU, in one process.  Medians of 5
# calls after one warm-up call each:
#   (a) Decoder.gather into a device destination: the existing path (host plan, piece
#       upload, kernel into the context's buffer, copy to the destination, stream
#       synchronise), wall time of the call and its kernel_ms;
#   (b) Decoder.gather_device followed by gather_wait, the ranges already in device memory:
#       wall time, and the wall time of the gather_device call alone (the enqueue);
#   (c) 16 gather_device calls followed by one gather_wait: wall time per call;
#   (d) the reports' kernel_ms, split into the plan kernels and the gather kernel
#       (gh_ctx_gather_times).
# The bytes of (a) and (b) are checked against gh.generate slices (the generator is
# counter-based: any slice is reproducible on its own).  The device's clocks and performance
# level are recorded before and after (read-only rocm-smi queries), next to the numbers.
# Usage: python scripts/bench_gather_device.py [--n BYTES] [--ranges R] [--out profiles/gather_device.jsonl]
import json
import os
import shutil
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

SEED, R, LOG2_STRIDE, RANGE_BYTES, REPS, QUEUED = 375, 0.1, 8, 4096, 5, 16


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(xs):
    return round(float(np.median(xs)), 4)


def device_state():
    """Clocks and performance level as rocm-smi shows them (queries only)."""
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    try:
        r = subprocess.run([exe, "-d", "0", "--showclocks", "--showperflevel", "--json"], capture_output=True,
                           text=True, timeout=60)
        return json.loads(r.stdout) if r.returncode == 0 else {"error": r.stderr[-200:]}
    except Exception as e:  # the numbers stand without it; say so in the record
        return {"error": repr(e)}


def main():
    n = opt("--n", 10**9)
    nranges = opt("--ranges", 4096)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {"bench": "gather_device", "n": n, "r": R, "log2_stride": LOG2_STRIDE, "ranges": nranges,
           "range_bytes": RANGE_BYTES, "reps": REPS, "device_state_before": device_state()}
    data = gh.generate(SEED, R, n, threads=16)
    img = gh.encode(data, threads=16)
    del data
    s = gh.parse(img)
    rng = np.random.default_rng(SEED)
    lo = rng.integers(0, n - RANGE_BYTES + 1, size=nranges).astype(np.uint64)
    ranges = np.ascontiguousarray(np.stack([lo, lo + np.uint64(RANGE_BYTES)], axis=1))
    total = nranges * RANGE_BYTES
    want = np.concatenate([gh.generate(SEED, R, RANGE_BYTES, offset=int(v)) for v in lo])

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t0) * 1e3, r

    with gh.Decoder(0) as d, gh.DeviceBuffer(ranges.nbytes) as rbuf, gh.DeviceBuffer(total) as dst:
        d.load(s)
        image, _, _ = d.build_index(LOG2_STRIDE)
        ix = gh.parse_index(image)
        pieces, _ = ix.plan(ranges)
        res.update({"g": s.g, "pieces": int(pieces.size), "gather_bytes": total,
                    "piece_bound": gh.gather_piece_bound(nranges, total, LOG2_STRIDE)})
        zeros = np.zeros(total, dtype=np.uint8)
        # (a) the existing path into device memory; the first call builds the tables
        d.gather(ix, ranges, dst_ptr=dst.addr, dst_len=total)
        ok_a = bool(np.array_equal(dst.download(np.empty(total, dtype=np.uint8)), want))
        wall, kms = [], []
        for _ in range(REPS):
            w, (_, ms) = timed(lambda: d.gather(ix, ranges, dst_ptr=dst.addr, dst_len=total))
            wall.append(w)
            kms.append(ms)
        res.update({"a_gather_wall_ms": med(wall), "a_gather_wall_ms_all": [round(w, 4) for w in wall],
                    "a_gather_kernel_ms": med(kms)})
        # (b) ranges resident, planned on the device
        rbuf.upload(ranges)
        dst.upload(zeros)
        d.set_index(ix)

        def one():
            d.gather_device(rbuf.addr, nranges, dst.addr, total)
            return d.gather_wait()

        rep = one()
        ok_b = bool(np.array_equal(dst.download(np.empty(total, dtype=np.uint8)), want))
        res.update({"b_npieces": int(rep.npieces), "b_out_bytes": int(rep.out_bytes), "b_status": int(rep.status)})
        wall, enq, kms, plan_ms, gather_ms = [], [], [], [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            d.gather_device(rbuf.addr, nranges, dst.addr, total)
            t1 = time.perf_counter()
            rep = d.gather_wait()
            wall.append((time.perf_counter() - t0) * 1e3)
            enq.append((t1 - t0) * 1e3)
            kms.append(rep.kernel_ms)
            p, g = d.gather_times()
            plan_ms.append(p)
            gather_ms.append(g)
        res.update({"b_device_wall_ms": med(wall), "b_device_wall_ms_all": [round(w, 4) for w in wall],
                    "b_enqueue_ms": med(enq), "d_kernel_ms": med(kms), "d_plan_kernels_ms": med(plan_ms),
                    "d_gather_kernel_ms": med(gather_ms)})

        # (c) 16 calls in a row, one wait
        def many():
            for _ in range(QUEUED):
                d.gather_device(rbuf.addr, nranges, dst.addr, total)
            return d.gather_wait()

        many()
        wall = [timed(many)[0] / QUEUED for _ in range(REPS)]
        ok_c = bool(np.array_equal(dst.download(np.empty(total, dtype=np.uint8)), want))
        res.update({"c_queued_calls": QUEUED, "c_wall_ms_per_call": med(wall),
                    "c_wall_ms_per_call_all": [round(w, 4) for w in wall]})
    res.update({"bitexact": ok_a and ok_b and ok_c, "b_below_a": res["b_device_wall_ms"] < res["a_gather_wall_ms"],
                "device_state_after": device_state()})
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
