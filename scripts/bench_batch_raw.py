# Batched gap-less decode (DESIGN.md "Batched gap-less decode"): the streams of
# scripts/bench_batch.py (M independent 64 KiB streams of gh_generate, one seed and one code
# each) with their gap words stripped, on one GPU, per configuration (M, r):
#   (a) load() of the gap-array images: wall time;
#   (b) load_raw() of the same streams without their gap words: wall time, and
#       raw_report().gap_ms (HIP events around the three gap kernels);
#   (c) the only route before this path: one Decoder, load_raw() stream after stream (host halo
#       estimate, allocations, a read-back per stream): wall time of the whole loop;
#   (d) decode() -> wait() after (a) and after (b): the same kernels on the same gap words;
#   (e) gap_ms beside the time of index() (the count and scan kernels) on the same batch.
# (a), (b) and (d) alternate rep by rep in one process, medians of REPS after WARMUP; (c) is
# timed on fewer reps where one rep takes seconds (recorded as c_reps).  Every output is checked
# against the generator's bytes and every stream's device-built gap words against its image's.
# Configurations: r = 0.5 at M = 256 and M = 4096, r = 0.1 and r = 0.9 at M = 256.
# Usage: python scripts/bench_batch_raw.py [--m 256] [--big 4096] [--bytes 65536] [--out profiles/batch_raw.jsonl]
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

SEED, REPS, WARMUP = 375, 20, 3


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(xs):
    return round(float(np.median(xs)), 4)


def strip(s):
    nw = (s.g + 7) // 8
    gaps = s.raw[s.raw.size - 4 * (nw + s.w): s.raw.size - 4 * s.w].copy().view(np.uint32)
    return (list(s.symbols), int(s.n), s.raw[s.raw.size - 4 * s.w:].copy().view(np.uint32)), gaps


def wall_ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def decode_ms(b):
    t0 = time.perf_counter()
    b.decode()
    rep = b.wait()
    return (time.perf_counter() - t0) * 1e3, rep.kernel_ms


def config(m, r, nbytes, c_reps):
    datas = [gh.generate(SEED + i, r, nbytes) for i in range(m)]
    streams = [gh.parse(gh.encode(d)) for d in datas]
    raws, gaps = zip(*[strip(s) for s in streams])
    # (b) takes the code tables as uint8 [nsyms, 2] arrays, marshalled once as (a)'s images are parsed once
    fast = [(np.asarray(sy, dtype=np.uint8).reshape(-1, 2), n, u) for sy, n, u in raws]
    res = {"bench": "batch_raw", "r": r, "m": m, "stream_bytes": nbytes, "reps": REPS, "c_reps": c_reps}
    ok = True
    a_load, b_load, gap, a_dec, a_k, b_dec, b_k, idx = [], [], [], [], [], [], [], []
    with gh.BatchDecoder(0) as ba, gh.BatchDecoder(0) as br:
        for rep in range(WARMUP + REPS):
            ta = wall_ms(lambda: ba.load(streams))
            tb = wall_ms(lambda: br.load_raw(fast))
            g = br.raw_report()
            da, ka = decode_ms(ba)
            db, kb = decode_ms(br)
            br.index()
            ki = br.wait().kernel_ms
            if rep >= WARMUP:
                a_load.append(ta), b_load.append(tb), gap.append(g.gap_ms), idx.append(ki)
                a_dec.append(da), a_k.append(ka), b_dec.append(db), b_k.append(kb)
        res.update({"shape": br.raw_kernel_shape(), "launches": g.launches, "scratch_bytes": g.scratch_bytes})
        br.decode()
        br.wait()
        step = max(1, m // 128)
        ok &= all(np.array_equal(br.download(i), datas[i]) for i in range(0, m, step))
        ok &= all(np.array_equal(ba.download(i), datas[i]) for i in range(0, m, step))
        ok &= all(np.array_equal(br.raw_gaps(i), gaps[i]) for i in range(m))
    c = []
    with gh.Decoder(0) as d:
        for rep in range(1 + c_reps):  # (one warm-up pass)
            t = wall_ms(lambda: [d.load_raw(sy, n, u) for sy, n, u in raws])
            if rep:
                c.append(t)
        d.decode(timed=False)
        d.report()
        ok &= bool(np.array_equal(d.download(nbytes), datas[-1]))
    res.update({"a_load_ms": med(a_load), "b_load_raw_ms": med(b_load), "b_gap_ms": med(gap),
                "b_gap_ms_min": round(min(gap), 4), "b_gap_ms_max": round(max(gap), 4),
                "c_loop_load_raw_ms": med(c), "c_over_b": round(float(np.median(c) / np.median(b_load)), 2),
                "d_decode_wall_ms_after_a": med(a_dec), "d_decode_wall_ms_after_b": med(b_dec),
                "d_kernel_ms_after_a": med(a_k), "d_kernel_ms_after_b": med(b_k),
                "e_index_ms": med(idx), "e_gap_over_index": round(float(np.median(gap) / np.median(idx)), 2),
                "bitexact": bool(ok)})
    return res


def main():
    m, big, nbytes = opt("--m", 256), opt("--big", 4096), opt("--bytes", 65536)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for mm, r, c_reps in ((m, 0.5, REPS), (m, 0.1, REPS), (m, 0.9, REPS), (big, 0.5, 2)):
        if mm:
            lines.append(json.dumps(config(mm, r, nbytes, c_reps)))
            print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
