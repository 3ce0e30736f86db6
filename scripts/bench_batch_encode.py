# Batched encode (DESIGN.md "Batched encode"): M independent 64 KiB inputs (gh_generate at
# r = 0.5, one seed per input, so each gets its own code), on one GPU:
#   (a) M = 256, one BatchEncoder, the inputs resident: wall time of plan() (with its split
#       into hist_ms, the histogram kernel by HIP events, and plan_host_ms, the host plans),
#       wall time from encode() to wait() returning, and kernel_ms (HIP events around the
#       encode's memsets and kernels), after warm-up calls;
#   (b) M = 256, the only way before the batch: 256 preloaded Encoder contexts, make_plan() +
#       encode() each, back to back; the same process, the same inputs, (a) and (b)
#       alternating rep by rep;
#   (c) M = 4096, the batch only (4096 contexts are not something to create on a shared
#       machine);
#   (d) for information, a ceiling: one input of the same total size as (a) (16 MiB of the
#       same generator) through one Encoder: plan + encode wall, and the encode's kernel_ms.
# Every batch image is checked against the host encoder once, outside the timed region.
# Usage: python scripts/bench_batch_encode.py [--m 256] [--big 4096] [--bytes 65536] [--out profiles/batch_encode.jsonl]
#
# --plan (DESIGN.md "Codes built on the device"): instead of the above, for M = 256 and
# M = 4096 the two ways to plan one loaded batch, alternating rep by rep in one process:
# plan() (histogram, read-back, host package-merges, upload) and plan_device() (histogram,
# code kernel, record read-back, descriptor upload), each followed by encode() + wait().
# Per way: wall time of the plan call, its parts from plan_times() (histogram and code kernel
# by HIP events, host work by wall clock), and plan + encode wall; medians, minima and maxima
# of 20 reps after 3 warm-up reps of each.  One JSON line per size.
# Usage: python scripts/bench_batch_encode.py --plan [--m 256] [--big 4096] [--bytes 65536] [--out profiles/batch_encode_plan.jsonl]
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

SEED, R, REPS, WARMUP = 375, 0.5, 20, 3


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(xs):
    return round(float(np.median(xs)), 4)


def time_batch(b, reps):
    """plan wall, hist_ms, plan_host_ms, encode-to-wait wall, kernel_ms per rep."""
    out = {k: [] for k in ("plan", "hist", "host", "enc", "kern")}
    for _ in range(reps):
        t0 = time.perf_counter()
        b.plan()
        t1 = time.perf_counter()
        b.encode()
        rep = b.wait()
        t2 = time.perf_counter()
        out["plan"].append((t1 - t0) * 1e3)
        out["enc"].append((t2 - t1) * 1e3)
        out["hist"].append(rep.hist_ms)
        out["host"].append(rep.plan_host_ms)
        out["kern"].append(rep.kernel_ms)
    return out


def time_loop(encs, reps):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for e in encs:
            e.make_plan()
            e.encode()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def batch_fields(prefix, t, m, nbytes):
    total = np.asarray(t["plan"]) + np.asarray(t["enc"])
    return {prefix + "_plan_wall_ms": med(t["plan"]), prefix + "_hist_ms": med(t["hist"]),
            prefix + "_plan_host_ms": med(t["host"]), prefix + "_encode_wall_ms": med(t["enc"]),
            prefix + "_encode_kernel_ms": med(t["kern"]), prefix + "_plan_encode_wall_ms": med(total),
            prefix + "_plan_encode_wall_ms_min": round(float(total.min()), 4),
            prefix + "_plan_encode_wall_ms_max": round(float(total.max()), 4),
            prefix + "_GBps_wall": round(m * nbytes / (float(np.median(total)) * 1e6), 3)}


def time_plan(b, device):
    """One rep of plan() or plan_device() + encode: plan wall, its parts, encode-to-wait wall."""
    t0 = time.perf_counter()
    if device:
        b.plan_device()
    else:
        b.plan()
    t1 = time.perf_counter()
    b.encode()
    b.wait()
    t2 = time.perf_counter()
    t = b.plan_times()
    return {"plan": (t1 - t0) * 1e3, "hist": t["hist_ms"], "code": t["code_ms"], "host": t["host_ms"],
            "total": (t2 - t0) * 1e3}


def plan_main():
    nbytes = opt("--bytes", 65536)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for m in (opt("--m", 256), opt("--big", 4096)):
        if not m:
            continue
        datas = [gh.generate(SEED + i, R, nbytes) for i in range(m)]
        res = {"bench": "batch_encode_plan", "r": R, "stream_bytes": nbytes, "m": m, "reps": REPS, "warmup": WARMUP}
        ok = True
        with gh.BatchEncoder(0) as b:
            b.load(datas)
            for device in (False, True):
                for _ in range(WARMUP):
                    time_plan(b, device)
                ok &= all(np.array_equal(b.download(i), gh.encode(datas[i])) for i in range(0, m, 1 if m <= 256 else 37))
            t = {False: [], True: []}
            for _ in range(REPS):  # alternating, one rep each
                for device in (False, True):
                    t[device].append(time_plan(b, device))
            ok &= all(np.array_equal(b.download(i), gh.encode(datas[i])) for i in range(0, m, 1 if m <= 256 else 37))
        for device, prefix in ((False, "host"), (True, "device")):
            for k in ("plan", "hist", "code", "host", "total"):
                xs = [x[k] for x in t[device]]
                name = {"plan": "plan_wall_ms", "hist": "hist_ms", "code": "code_ms", "host": "plan_host_ms",
                        "total": "plan_encode_wall_ms"}[k]
                res[f"{prefix}_{name}"] = med(xs)
                if k in ("plan", "total"):
                    res[f"{prefix}_{name}_min"] = round(min(xs), 4)
                    res[f"{prefix}_{name}_max"] = round(max(xs), 4)
        res["device_plan_below_host_plan"] = bool(res["device_plan_wall_ms"] < res["host_plan_wall_ms"])
        res["host_over_device_plan"] = round(res["host_plan_wall_ms"] / res["device_plan_wall_ms"], 2)
        res["bitexact"] = bool(ok)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    if "--plan" in sys.argv:
        return plan_main()
    m, big, nbytes = opt("--m", 256), opt("--big", 4096), opt("--bytes", 65536)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {"bench": "batch_encode", "r": R, "stream_bytes": nbytes, "m": m, "m_big": big, "reps": REPS}
    datas = [gh.generate(SEED + i, R, nbytes) for i in range(m)]
    ok = True
    with gh.BatchEncoder(0) as b:
        t0 = time.perf_counter()
        b.load(datas)
        res["a_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        time_batch(b, WARMUP)
        res["a_shape"] = b.kernel_shape()
        res["a_launches"] = int(b.wait().launches)
        ok &= all(np.array_equal(b.download(i), gh.encode(d)) for i, d in enumerate(datas))
        encs = []
        try:
            t0 = time.perf_counter()
            for d in datas:
                e = gh.Encoder(0)
                encs.append(e)
                e.load(d)
            res["b_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            time_loop(encs, WARMUP)
            ok &= all(np.array_equal(e.download(), gh.encode(d)) for e, d in zip(encs[:8], datas[:8]))
            res["b_shape"] = encs[0].kernel_shape()
            a = {k: [] for k in ("plan", "hist", "host", "enc", "kern")}
            bw = []
            for _ in range(REPS):  # alternating, one rep each
                for k, v in time_batch(b, 1).items():
                    a[k] += v
                bw += time_loop(encs, 1)
        finally:
            for e in encs:
                e.close()
    res.update(batch_fields("a", a, m, nbytes))
    at = float(np.median(np.asarray(a["plan"]) + np.asarray(a["enc"])))
    res.update({"b_loop_wall_ms": med(bw), "b_loop_wall_ms_min": round(min(bw), 4),
                "b_loop_wall_ms_max": round(max(bw), 4),
                "b_GBps_wall": round(m * nbytes / (float(np.median(bw)) * 1e6), 3),
                "batch_wall_below_loop_wall": bool(at < np.median(bw)),
                "loop_over_batch": round(float(np.median(bw)) / at, 2)})
    # (d) the ceiling: one input of the same total size
    whole = gh.generate(SEED, R, m * nbytes)
    with gh.Encoder(0) as e:
        e.load(whole)
        for _ in range(WARMUP):
            e.make_plan()
            e.encode()
        wall, kms = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            e.make_plan()
            kms.append(e.encode())
            wall.append((time.perf_counter() - t0) * 1e3)
        ok &= bool(np.array_equal(e.download(), gh.encode(whole)))
        res.update({"d_whole_plan_encode_wall_ms": med(wall), "d_whole_encode_kernel_ms": med(kms),
                    "d_whole_shape": e.kernel_shape()})
    del whole
    # (c) the large batch
    if big:
        datas = [gh.generate(SEED + i, R, nbytes) for i in range(big)]
        with gh.BatchEncoder(0) as b:
            t0 = time.perf_counter()
            b.load(datas)
            res["c_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            time_batch(b, WARMUP)
            c = time_batch(b, REPS)
            ok &= all(np.array_equal(b.download(i), gh.encode(datas[i])) for i in range(0, big, 37))
        res.update(batch_fields("c", c, big, nbytes))
    res["bitexact"] = bool(ok)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
