# Batched gather (DESIGN.md "Batched gather"): byte ranges of M resident 64 KiB streams (the
# inputs of scripts/bench_batch.py: gh_generate at r = 0.5, one seed and one code per stream),
# on one GPU, M = 256 and M = 4096.  One loaded batch per size, indexed once.  Ranges of 256
# bytes at seeded random offsets, held in device memory:
#   one      one range per stream;
#   sorted   16 ranges per stream, sorted by stream;
#   shuffled the same 16 per stream in a shuffled order (the difference to `sorted` prices the
#            table reloads: a wave reloads its LDS tables when the stream changes).
# Timed: kernel_ms of gather_wait (HIP events around the memset, the three plan kernels and
# the gather kernel), of index() alone and of the full decode() of the same batch (the only
# way to those bytes without the gather), all in one process, alternating repetition by
# repetition: 20 timed repetitions after 3 warm-up repetitions, medians with minimum and
# maximum.  Every gathered byte is checked against the generator's bytes outside the timed
# region.  Acceptance: the `one` gather's median lies below the fastest decode repetition.
# Usage: python scripts/bench_batch_gather.py [--m 256] [--big 4096] [--bytes 65536] [--out profiles/batch_gather.jsonl]
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

SEED, R, REPS, WARMUP, LEN, PER = 375, 0.5, 20, 3, 256, 16


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def stats(xs, key):
    return {key + "_ms": round(float(np.median(xs)), 4), key + "_ms_min": round(float(min(xs)), 4),
            key + "_ms_max": round(float(max(xs)), 4)}


def run(m, nbytes):
    datas = [gh.generate(SEED + i, R, nbytes) for i in range(m)]
    streams = [gh.parse(gh.encode(d)) for d in datas]
    rng = np.random.default_rng(SEED + m)
    lo = rng.integers(0, nbytes - LEN + 1, (m, PER))
    sid = np.repeat(np.arange(m), PER).reshape(m, PER)
    many = np.stack([sid, lo, lo + LEN], axis=2).reshape(-1, 3).astype(np.int64)
    sets = {"one": np.ascontiguousarray(many[::PER]), "sorted": many, "shuffled": many[rng.permutation(many.shape[0])]}
    res = {"bench": "batch_gather", "r": R, "stream_bytes": nbytes, "m": m, "range_bytes": LEN, "reps": REPS}
    ms = {k: [] for k in list(sets) + ["index", "decode"]}
    ok = True
    with gh.BatchDecoder(0) as b:
        b.load(streams)
        res["shape"] = b.gather_kernel_shape()
        b.index()
        b.wait()
        bufs = {k: (gh.DeviceBuffer(r.nbytes).upload(r), gh.DeviceBuffer(r.shape[0] * LEN)) for k, r in sets.items()}
        try:
            for rep in range(WARMUP + REPS):
                b.decode()
                t = {"decode": b.wait().kernel_ms}
                b.index()
                t["index"] = b.wait().kernel_ms
                for k, (dr, dst) in bufs.items():
                    b.gather_device(dr.addr, sets[k].shape[0], dst.addr, dst.nbytes)
                    g = b.gather_wait()
                    t[k] = g.kernel_ms
                    res[k + "_pieces"], res["launches"] = int(g.npieces), int(g.launches)
                if rep >= WARMUP:
                    for k, v in t.items():
                        ms[k].append(v)
            for k, (dr, dst) in bufs.items():  # every gathered byte, outside the timed region
                got = dst.download(np.zeros(dst.nbytes, dtype=np.uint8)).reshape(-1, LEN)
                ok &= all(np.array_equal(row, datas[s][a:e]) for row, (s, a, e) in zip(got, sets[k].tolist()))
        finally:
            for dr, dst in bufs.values():
                dr.close()
                dst.close()
    for k, v in ms.items():
        res.update(stats(v, k))
    res["one_below_fastest_decode"] = bool(res["one_ms"] < res["decode_ms_min"])
    res["decode_over_one"] = round(res["decode_ms"] / res["one_ms"], 2)
    res["shuffled_minus_sorted_ms"] = round(res["shuffled_ms"] - res["sorted_ms"], 4)
    res["bitexact"] = bool(ok)
    return res


def main():
    nbytes = opt("--bytes", 65536)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for m in (opt("--m", 256), opt("--big", 4096)):
        if m:
            lines.append(json.dumps(run(m, nbytes)))
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
