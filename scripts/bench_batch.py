# Batched decode (DESIGN.md "Batched decode"): M independent 64 KiB streams (gh_generate at
# r = 0.5, one seed per stream, each with its own code table), on one GPU:
#   (a) M = 256, one BatchDecoder: wall time from decode() to wait() returning, and kernel_ms
#       (HIP events around the batch's kernels), the streams resident, after warm-up calls;
#   (b) M = 256, the only way before the batch: 256 preloaded Decoder contexts, their decodes
#       enqueued back to back (untimed: no events), wall time until the last report() returns;
#       the same process, the same streams, (a) and (b) alternating rep by rep;
#   (c) M = 4096, the batch only (4096 contexts with a stream each are not something to
#       create on a shared machine);
#   (d) for information, a ceiling: one ordinary whole-stream decode of one stream of the same
#       total size as (a) (256 x 64 KiB = 16 MiB of the same generator), kernel_ms and wall.
# Every batch output is checked against the generator's bytes.  The load times (host
# validation, arena upload, the table kernel) are recorded next to the decode times.
# Usage: python scripts/bench_batch.py [--m 256] [--big 4096] [--bytes 65536] [--out profiles/batch_decode.jsonl]
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


def make(m, nbytes):
    datas = [gh.generate(SEED + i, R, nbytes) for i in range(m)]
    return datas, [gh.parse(gh.encode(d)) for d in datas]


def time_batch(b, reps):
    wall, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        b.decode()
        rep = b.wait()
        wall.append((time.perf_counter() - t0) * 1e3)
        kms.append(rep.kernel_ms)
    return wall, kms


def time_loop(decs, reps):
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for d in decs:
            d.decode(timed=False)
        for d in decs:
            d.report()
        wall.append((time.perf_counter() - t0) * 1e3)
    return wall


def main():
    m, big, nbytes = opt("--m", 256), opt("--big", 4096), opt("--bytes", 65536)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {"bench": "batch_decode", "r": R, "stream_bytes": nbytes, "m": m, "m_big": big, "reps": REPS}
    datas, streams = make(m, nbytes)
    ok = True
    with gh.BatchDecoder(0) as b:
        t0 = time.perf_counter()
        b.load(streams)
        res["a_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["a_shape"] = b.kernel_shape()
        time_batch(b, WARMUP)
        ok &= all(np.array_equal(g, d) for g, d in zip(b.download_all(), datas))
        decs = []
        try:
            t0 = time.perf_counter()
            for s in streams:
                d = gh.Decoder(0)
                decs.append(d)
                d.load(s)
            res["b_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            time_loop(decs, WARMUP)
            ok &= all(np.array_equal(d.download(nbytes), x) for d, x in zip(decs[:8], datas[:8]))
            res["b_shape"] = decs[0].kernel_shape()
            aw, ak, bw = [], [], []
            for _ in range(REPS):  # alternating, one rep each
                w, k = time_batch(b, 1)
                aw += w
                ak += k
                bw += time_loop(decs, 1)
        finally:
            for d in decs:
                d.close()
    res.update({"a_batch_wall_ms": med(aw), "a_batch_kernel_ms": med(ak), "a_batch_wall_ms_min": round(min(aw), 4),
                "a_batch_wall_ms_max": round(max(aw), 4), "b_loop_wall_ms": med(bw),
                "b_loop_wall_ms_min": round(min(bw), 4), "b_loop_wall_ms_max": round(max(bw), 4),
                "a_GBps_wall": round(m * nbytes / (float(np.median(aw)) * 1e6), 3),
                "b_GBps_wall": round(m * nbytes / (float(np.median(bw)) * 1e6), 3),
                "batch_wall_below_loop_wall": bool(np.median(aw) < np.median(bw)),
                "loop_over_batch": round(float(np.median(bw) / np.median(aw)), 2)})
    # (d) the ceiling: one stream of the same total size
    whole = gh.generate(SEED, R, m * nbytes)
    with gh.Decoder(0) as d:
        d.load(gh.parse(gh.encode(whole)))
        for _ in range(WARMUP):
            d.decode()
        d.report()
        d.reset_timing()
        for _ in range(REPS):
            d.decode()
        rep = d.report()
        wall = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            d.decode(timed=False)
            d.report()
            wall.append((time.perf_counter() - t0) * 1e3)
        ok &= bool(np.array_equal(d.download(whole.size), whole))
        res.update({"d_whole_kernel_ms": round(rep.kernel_ms, 4), "d_whole_wall_ms": med(wall),
                    "d_whole_shape": d.kernel_shape()})
    del whole
    # (c) the large batch
    if big:
        datas, streams = make(big, nbytes)
        with gh.BatchDecoder(0) as b:
            t0 = time.perf_counter()
            b.load(streams)
            res["c_load_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            time_batch(b, WARMUP)
            cw, ck = time_batch(b, REPS)
            ok &= all(np.array_equal(b.download(i), datas[i]) for i in range(0, big, 37))
        res.update({"c_batch_wall_ms": med(cw), "c_batch_kernel_ms": med(ck),
                    "c_GBps_wall": round(big * nbytes / (float(np.median(cw)) * 1e6), 3)})
    res["bitexact"] = bool(ok)
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
