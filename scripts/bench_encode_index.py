# The seek index from the GPU encoder (DESIGN.md "Random access", "The index from the
# encoders"): what gh_ectx_index costs next to the route a writer had before it, on one
# GPU, in one process.  Per workload (1 GB of gh_generate at r = 0.1 and r = 0.9:
# BASELINE's cfg4 and cfg3) and per stride (2^8, 2^10 segments), medians of 5 after one
# warm-up each:
#   * gh_ectx_encode's kernel_ms (the stream the index describes);
#   * gh_ectx_index: kernel_ms (HIP events around the index kernel) and the whole call's
#     wall time (kernel, the copy of the entries, the header);
#   * the earlier route from the same resident encoder: Encoder.download, parse,
#     Decoder.load, build_index -- its wall time, and build_index's kernel_ms alone.
# The two images must be equal byte for byte.
# Usage: python scripts/bench_encode_index.py [cfg4 cfg3] [--out profiles/encode_index.jsonl]
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

WORKLOADS = {"cfg2": (10**8, 0.5), "cfg3": (10**9, 0.9), "cfg4": (10**9, 0.1)}
STRIDES = (8, 10)
REPS = 5


def med(xs):
    return round(float(np.median(xs)), 4)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path in args:
        args.remove(out_path)
    if gh.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    lines = []
    for wl in args or ["cfg4", "cfg3"]:
        n, r = WORKLOADS[wl]
        data = gh.generate(375, r, n)
        with gh.Encoder(0) as e:
            e.load(data)
            plan = e.make_plan()
            e.encode()  # warm-up
            enc_ms = med([e.encode() for _ in range(REPS)])
            for k in STRIDES:
                res = {"workload": wl, "n": n, "r": r, "g": int(plan.g), "bits_per_byte": round(plan.bits / n, 4),
                       "log2_stride": k, "reps": REPS, "encode_kernel_ms": enc_ms}
                e.index(k)  # warm-up
                runs = [timed(lambda: e.index(k)) for _ in range(REPS)]
                image = runs[0][1][0]
                res.update({"index_bytes": int(image.size), "index_kernel_ms": med([x[1][1] for x in runs]),
                            "index_wall_ms": med([x[0] for x in runs])})

                def old_route():
                    img = e.download()
                    with gh.Decoder(0) as d:
                        d.load(gh.parse(img))
                        return d.build_index(k)

                old_route()  # warm-up
                old = [timed(old_route) for _ in range(REPS)]
                res.update({"old_route_wall_ms": med([x[0] for x in old]),
                            "build_index_kernel_ms": med([x[1][2] for x in old]),
                            "images_equal": bool(np.array_equal(image, old[0][1][0]))})
                line = json.dumps(res)
                print(line, flush=True)
                lines.append(line)
                if out_path:  # (rewritten after every line: a later failure keeps the earlier ones)
                    with open(out_path, "w") as f:
                        f.write("\n".join(lines) + "\n")
        del data


if __name__ == "__main__":
    main()
