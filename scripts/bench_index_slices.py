# The seek index of a sliced stream and slices in device memory (DESIGN.md "Sliced
# encode", "The index of a sliced stream"), on one GPU, in one process.  1 GB of gh_generate
# at r = 0.1 (BASELINE's cfg4), K = 8 slices on device 0, stride 2^8; every series is
# REPS runs after one warm-up, all values recorded:
#   * sharded_index: wall time of gh_encode_sharded_index against the route before it,
#     gh_encode_sharded then gh_encode_index on the host (THREADS threads); the two
#     index images must be equal byte for byte;
#   * per_slice: each slice's gh_ectx_index_slice kernel_ms beside its encode kernel_ms;
#   * merge: gh_enc_merge_kernel's time for the whole stream's words (a whole encode merged
#     as the slice at bit 0; HIP events on the stream the merge runs on) beside gh_bw_copy
#     over the same bytes;
#   * load: gh_ectx_load_device against gh_ectx_load, wall.
# Several devices: only when more than one is visible; "not measured" otherwise.
# Usage: python scripts/bench_index_slices.py [--n BYTES] [--series a,b] [--out profiles/index_slices.jsonl]
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
try:  # (torch first: one HIP runtime in the process, tests/conftest.py)
    import torch  # noqa: E402
except ImportError:
    torch = None
import gaphuff as gh  # noqa: E402

K, STRIDE, REPS = 8, 8, 3
# host threads: what the machine allows this process (OMP_NUM_THREADS where a scheduler sets it)
THREADS = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return round((time.perf_counter() - t0) * 1e3, 3), r


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    n, out_path, only = int(arg("--n", 10**9)), arg("--out", None), arg("--series", None)
    want = lambda series: only is None or series in only.split(",")  # noqa: E731
    if gh.device_count() < 1:
        raise SystemExit("no HIP device: nothing to measure")
    lines = []

    def emit(**res):
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        if out_path:  # (rewritten after every line: a later failure keeps the earlier ones)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    data = gh.generate(375, 0.1, n)
    common = {"n": n, "r": 0.1, "slices": K, "log2_stride": STRIDE, "host_threads": THREADS}

    # ---- one call against the earlier route
    def new_route():
        return gh.encode_sharded(data, K, index_log2_stride=STRIDE)

    def old_route():
        return gh.encode_sharded(data, K), gh.encode_index(data, STRIDE, threads=THREADS)

    if want("sharded_index"):
        new_route()
        old_route()
    for run in range(1, REPS + 1 if want("sharded_index") else 0):  # alternating
        t_new, (img_n, idx_n) = timed(new_route)
        t_enc, img_o = timed(lambda: gh.encode_sharded(data, K))
        t_idx, idx_o = timed(lambda: gh.encode_index(data, STRIDE, threads=THREADS))
        emit(series="sharded_index", run=run, sharded_index_wall_ms=t_new, sharded_wall_ms=t_enc,
             host_index_wall_ms=t_idx, old_route_wall_ms=round(t_enc + t_idx, 3),
             images_equal=bool(np.array_equal(img_n, img_o)), indexes_equal=bool(np.array_equal(idx_n, idx_o)), **common)

    # ---- per slice: the index kernel beside the encode kernels
    plan = gh.encode_plan(data)
    lens = np.frombuffer(bytes(plan.len), dtype=np.uint8)
    cuts = [n * i // K for i in range(K + 1)]
    base = 0
    with gh.Encoder(0) as e:
        for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:]) if want("per_slice") else ()):
            e.load(data[lo:hi])
            e.encode_slice(plan, base)
            enc = [round(e.encode_slice(plan, base)[1], 4) for _ in range(REPS)]
            e.index_slice(lo, STRIDE)
            runs = [e.index_slice(lo, STRIDE) for _ in range(REPS)]
            emit(series="per_slice", slice=i, bytes=hi - lo, entries=int(runs[0][0].size),
                 encode_kernel_ms=enc, index_kernel_ms=[round(r[2], 4) for r in runs], **common)
            base += int(lens[data[lo:hi]].sum(dtype=np.uint64))

        # ---- the merge kernel beside the copy yardstick, a whole encode as the slice at bit 0
        e.load(data)
        e.make_plan()
        e.encode()
        w, gw = int(plan.w), -(-int(plan.g) // 8)
        nbytes = 4 * (w + gw)
        with gh.DeviceBuffer(4 * w + 64) as pay, gh.DeviceBuffer(4 * gw + 64) as gap, \
                gh.DeviceBuffer(nbytes + 64) as a, gh.DeviceBuffer(nbytes + 64) as b:
            copy_bytes = nbytes // 16 * 16
            for run in range(1, REPS + 2 if want("merge") else 0):
                if torch is not None and torch.cuda.is_available():
                    st = torch.cuda.Stream(device="cuda:0")
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    wall, _ = timed(lambda: e.merge_device(pay.addr, w, gap.addr, gw, hip_stream=st.cuda_stream))
                    e1.record(st)
                    e1.synchronize()
                    ms, how = round(e0.elapsed_time(e1), 4), "events"
                else:
                    ms, _ = timed(lambda: e.merge_device(pay.addr, w, gap.addr, gw))
                    wall, how = ms, "wall"
                copy_ms = round(gh.bw_copy(b.addr, a.addr, copy_bytes, reps=5), 4)
                if run > 1:  # (the first is the warm-up)
                    emit(series="merge", run=run - 1, stream_bytes=nbytes, merge_ms=ms, merge_timing=how,
                         merge_call_wall_ms=wall, bw_copy_ms=copy_ms, merge_over_copy=round(ms / copy_ms, 3), **common)

    # ---- load_device against load
    with gh.Encoder(0) as e, gh.DeviceBuffer(n) as src:
        src.upload(data)
        e.load(data)
        e.load_device(src.addr, n)
        for run in range(1, REPS + 1 if want("load") else 0):
            t_h, _ = timed(lambda: e.load(data))
            t_d, _ = timed(lambda: e.load_device(src.addr, n))
            emit(series="load", run=run, load_wall_ms=t_h, load_device_wall_ms=t_d, **common)

    # ---- several devices
    nd = gh.device_count()
    if not want("sharded_index_multi"):
        pass
    elif nd < 2:
        emit(series="sharded_index_multi", devices=nd, result="not measured: one device visible", **common)
    else:
        devs = list(range(min(nd, 8)))
        gh.encode_sharded(data, K, devices=devs, index_log2_stride=STRIDE)
        for run in range(1, REPS + 1):
            t_new, (img, idx) = timed(lambda: gh.encode_sharded(data, K, devices=devs, index_log2_stride=STRIDE))
            emit(series="sharded_index_multi", run=run, devices=len(devs), sharded_index_wall_ms=t_new, **common)


if __name__ == "__main__":
    main()
