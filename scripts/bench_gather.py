# Batched range gather (DESIGN.md "Range gather"): 4 096 random 4 KiB ranges of a 1 GB
# gh_generate stream (r = 0.1) with an index of stride 2^8, on one GPU, three ways:
#   (a) one Decoder.gather call on the resident stream: kernel_ms and the wall time of the
#       call (plan, piece upload, kernel, download of the 16 MiB), after one warm-up call;
#   (b) 64 of the same ranges one at a time through gh.decode_range from an in-memory
#       Stream (the only path before the gather): wall time per range;
#   (c) a full decode of the stream ("just decode everything"): kernel_ms of a decode on
#       the resident stream, and the wall time of decode + report + download of the N bytes.
# The gathered bytes are checked against gh.generate slices (the generator is counter-based:
# any slice is reproducible on its own).  The device's clocks and performance level are
# recorded before and after (read-only rocm-smi queries), next to the numbers.
# Usage: python scripts/bench_gather.py [--n BYTES] [--ranges R] [--out profiles/gather.jsonl]
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

SEED, R, LOG2_STRIDE, RANGE_BYTES, REPS = 375, 0.1, 8, 4096, 5


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
    res = {"bench": "gather", "n": n, "r": R, "log2_stride": LOG2_STRIDE, "ranges": nranges,
           "range_bytes": RANGE_BYTES, "device_state_before": device_state()}
    data = gh.generate(SEED, R, n, threads=16)
    img = gh.encode(data, threads=16)
    del data
    s = gh.parse(img)
    rng = np.random.default_rng(SEED)
    lo = rng.integers(0, n - RANGE_BYTES + 1, size=nranges).astype(np.uint64)
    ranges = np.stack([lo, lo + np.uint64(RANGE_BYTES)], axis=1)
    with gh.Decoder(0) as d:
        d.load(s)
        image, _, index_ms = d.build_index(LOG2_STRIDE)
        ix = gh.parse_index(image)
        pieces, total = ix.plan(ranges)
        res.update({"g": s.g, "mode": None, "index_kernel_ms": round(index_ms, 4), "pieces": int(pieces.size),
                    "gather_bytes": total})
        # (a) one gather call; the first call builds the tables and is the warm-up
        out, _ = d.gather(ix, ranges)
        ok = all(np.array_equal(out[i * RANGE_BYTES:(i + 1) * RANGE_BYTES],
                                gh.generate(SEED, R, RANGE_BYTES, offset=int(lo[i]))) for i in range(nranges))
        kms, wall = [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            out, ms = d.gather(ix, ranges)
            wall.append((time.perf_counter() - t0) * 1e3)
            kms.append(ms)
        res.update({"a_gather_kernel_ms": med(kms), "a_gather_wall_ms": med(wall),
                    "a_gather_wall_ms_all": [round(w, 3) for w in wall],
                    "a_per_range_us": round(1e3 * float(np.median(wall)) / nranges, 3)})
        # (c) the full decode on the same resident stream
        d.decode()
        d.report()
        d.reset_timing()
        for _ in range(REPS):
            d.decode()
        rep = d.report()
        res.update({"mode": gh.MODE_NAMES[rep.mode], "c_decode_kernel_ms": round(rep.kernel_ms, 4)})
        whole = []
        for _ in range(3):
            t0 = time.perf_counter()
            d.decode(timed=False)
            d.report()
            full = d.download(n)
            whole.append((time.perf_counter() - t0) * 1e3)
        ok &= all(np.array_equal(full[int(l):int(l) + RANGE_BYTES], out[i * RANGE_BYTES:(i + 1) * RANGE_BYTES])
                  for i, l in enumerate(lo[:256]))
        del full
        res["c_decode_download_wall_ms"] = med(whole)
    # (b) the per-range path of the parent commit, 64 of the same ranges
    per = []
    for i in range(min(64, nranges)):
        t0 = time.perf_counter()
        got = gh.decode_range(s, ix, int(lo[i]), int(lo[i]) + RANGE_BYTES)
        per.append((time.perf_counter() - t0) * 1e3)
        ok &= bool(np.array_equal(got, out[i * RANGE_BYTES:(i + 1) * RANGE_BYTES]))
    res.update({"b_decode_range_ms_per_range": med(per), "b_decode_range_ms_min": round(min(per), 4),
                "b_decode_range_ms_max": round(max(per), 4), "bitexact": bool(ok),
                "gather_wall_below_full_decode_kernel": res["a_gather_wall_ms"] < res["c_decode_kernel_ms"],
                "gather_wall_below_full_decode_wall": res["a_gather_wall_ms"] < res["c_decode_download_wall_ms"],
                "device_state_after": device_state()})
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
