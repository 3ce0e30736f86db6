# GPU encoder measurement: per workload, the device encode
# (bits + scan + write kernels and the gap-array memset, input resident in HBM) timed
# with HIP events, the plan step (GPU histogram + host package-merge) by wall clock,
# and the host encoder (gh_encode_write, all cores) for comparison.  Checks the image
# against the host encoder byte for byte.
# Usage: python scripts/bench_encode.py [cfg2 cfg3 cfg4]   (prints one JSON line each)
#        python scripts/bench_encode.py [cfg4 ...] --slices 2,4,8 [--devices 0,1,...]
# --slices: the sliced encode (gh_encode_sharded) instead: one line for the whole encode
# (slices = 1, gh_ectx_encode) and one per slice count, on device 0 alone and, when
# --devices names more than one, round robin over them; kernel_ms is the slowest
# device's sum of its slices' encode times, wall_ms the whole call from host memory
# (loads, histograms, plan, encodes, downloads, merge).
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

WORKLOADS = {"cfg2": (10**8, 0.5), "cfg3": (10**9, 0.9), "cfg4": (10**9, 0.1)}
PEAK = 8000.0  # GB/s, MI355X HBM3E

argv = sys.argv[1:]
slices, devices = [], [0]
for flag in ("--slices", "--devices"):
    if flag in argv:
        i = argv.index(flag)
        vals = [int(x) for x in argv[i + 1].split(",")]
        del argv[i:i + 2]
        if flag == "--slices":
            slices = vals
        else:
            devices = vals

for w in argv or ["cfg2", "cfg3", "cfg4"]:
    n, r = WORKLOADS[w]
    data = gh.generate(375, r, n)
    with gh.Encoder(0) as e:
        e.load(data)
        t0 = time.perf_counter()
        plan = e.make_plan()
        plan_ms = (time.perf_counter() - t0) * 1e3
        for _ in range(3):
            e.encode()
        ms = sorted(e.encode() for _ in range(10))[5]
        img = e.download()
    t0 = time.perf_counter()
    host = gh.encode(data)
    host_ms = (time.perf_counter() - t0) * 1e3
    if slices:
        print(json.dumps({"workload": w, "n": n, "redundancy": r, "slices": 1, "devices": [0],
                          "kernel_ms": round(ms, 4), "identical_to_host": bool(np.array_equal(img, host))}), flush=True)
        del img
        for devs in ([0], devices) if len(devices) > 1 else ([0],):
            for k in slices:
                runs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    simg, kms = gh.encode_sharded(data, k, devices=devs, return_ms=True)
                    runs.append((kms, (time.perf_counter() - t0) * 1e3))
                kms, wall = sorted(runs)[1]
                print(json.dumps({"workload": w, "n": n, "redundancy": r, "slices": k, "devices": devs,
                                  "kernel_ms": round(kms, 4), "wall_ms": round(wall, 1),
                                  "identical_to_host": bool(np.array_equal(simg, host))}), flush=True)
                del simg
        continue
    gw = (plan.g + 7) // 8
    alg = n + 4 * plan.w + 4 * gw  # input read once, payload + gaps written once
    print(json.dumps({
        "workload": w, "n": n, "redundancy": r, "encode_ms": round(ms, 4),
        "input_GBps": round(n / ms / 1e6, 1), "alg_bytes": alg,
        "roofline_frac": round(alg / ms / 1e6 / PEAK, 3),
        "plan_ms_wall": round(plan_ms, 2), "host_encode_ms_wall": round(host_ms, 1),
        "host_threads": os.cpu_count(), "identical_to_host": bool(np.array_equal(img, host)),
    }), flush=True)
