# Plane choice (DESIGN.md "Plane choice"): bf16 and fp32 tensors of N(0, 0.02) weights and int32
# ids in [0, 1000) (two all-zero planes: the hot-bin worst case) on one GPU, in one process, at
# two sizes: 256 tensors of 64 KiB and 8 tensors of 128 MiB.  Per configuration:
#   (a) kernel rate: gh_pmask_hist_kernel (gh_pmask_report.hist_ms), with and without the
#       lane's merge of equal bytes (GH_PMASK_MERGE=1 / 0), beside gh_bw_copy of the same bytes.
#       The histogram only reads: its rate is nelem * E bytes per hist_ms.  The copy reads and
#       writes them: its rate is 2 * nelem * E bytes per copy_ms.  The fraction reported is the
#       ratio of the two rates, beside the split kernel's fraction of the same shape from
#       profiles/planes.jsonl (which counts its own read + written bytes the same way);
#   (b) the whole choose_masks_device call (default variant) beside the route a caller had
#       before it: load_planes_device with every plane coded, plan_device(), sizes();
#   (c) (once) the containers of encode_tensors(..., "auto") beside the default mask's for the
#       five tensors of the size table, 65 536 elements each.
# Variants alternate rep by rep; medians of REPS after WARMUP.  The new path is accepted when
# its median is not above the other route's fastest rep.  Every output is checked against the
# CPU rule (gh.choose_planes_masks).
# Usage: python scripts/bench_pmask.py [--small 256] [--big 8] [--out profiles/pmask.jsonl]
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "cse375-finalproj-huffman-decoding_amd"))
import numpy as np  # noqa: E402
import gaphuff as gh  # noqa: E402

REPS, WARMUP = 20, 3


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(xs):
    return round(float(np.median(xs)), 4)


def wall_ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def pad16(n):
    return -(-n // 16) * 16


def split_fractions():
    """(dtype, tensors, tensor_bytes) -> the split kernel's fraction of the copy's rate."""
    out = {}
    try:
        for line in open(os.path.join(ROOT, "profiles", "planes.jsonl")):
            r = json.loads(line)
            if r.get("bench") == "planes":
                out[(r["dtype"], r["tensors"], r["tensor_bytes"])] = r["k_split_over_copy_rate"]
    except OSError:
        pass
    return out


def make(kind, nelem, m):
    g = torch.Generator(device="cuda").manual_seed(375)
    if kind == "int32_ids":
        return [torch.randint(0, 1000, (nelem,), device="cuda", generator=g, dtype=torch.int32) for _ in range(m)]
    dtype = {"bfloat16": torch.bfloat16, "float32": torch.float32}[kind]
    return [(torch.randn(nelem, device="cuda", generator=g) * 0.02).to(dtype) for _ in range(m)]


def config(kind, m, tensor_bytes, split):
    e = 2 if kind == "bfloat16" else 4
    nelem = tensor_bytes // e
    ts = make(kind, nelem, m)
    total = m * tensor_bytes
    items = [(t.data_ptr(), nelem, e, (1 << e) - 1) for t in ts]
    cp_src = torch.empty(pad16(total), dtype=torch.uint8, device="cuda")
    cp_dst = torch.empty(pad16(total), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    # the CPU rule, once
    want_m, want_pb = gh.choose_planes_masks([t.view(torch.uint8).cpu().numpy().view({2: np.uint16, 4: np.uint32}[e]) for t in ts])
    res = {"bench": "pmask", "dtype": kind, "tensors": m, "tensor_bytes": tensor_bytes, "reps": REPS,
           "masks": sorted({int(x) for x in want_m})}
    ok = True
    hist = {"0": [], "1": []}
    call = {"0": [], "1": [], "default": []}
    code_k, decide_k, copy_k, old = [], [], [], []

    def choose(enc, merge):
        if merge == "default":
            os.environ.pop("GH_PMASK_MERGE", None)
        else:
            os.environ["GH_PMASK_MERGE"] = merge
        return enc.choose_masks_device(items, hip_stream=stream)

    def old_route(enc):
        enc.load_planes_device(items, 0, 0, hip_stream=stream)
        enc.plan_device()
        return enc.sizes()

    with gh.BatchEncoder(0) as enc, gh.BatchEncoder(0) as enc_old:
        torch.cuda.synchronize()
        for rep in range(WARMUP + REPS):
            t_new = {}
            for merge in ("0", "1", "default"):
                t_new[merge], (masks, pb) = wall_ms(lambda: choose(enc, merge))
                r = enc.pmask_report()
                ok &= bool(np.array_equal(masks, want_m) and np.array_equal(pb, want_pb))
                if rep >= WARMUP and merge != "default":
                    hist[merge].append(r.hist_ms)
                if rep >= WARMUP and merge == "default":
                    code_k.append(r.code_ms), decide_k.append(r.decide_ms)
            kc = gh.bw_copy(cp_dst.data_ptr(), cp_src.data_ptr(), pad16(total), reps=1)
            to, sizes = wall_ms(lambda: old_route(enc_old))
            ok &= bool(np.array_equal(sizes.reshape(m, e), want_pb[:, :e]))
            if rep >= WARMUP:
                for k in call:
                    call[k].append(t_new[k])
                copy_k.append(kc), old.append(to)
        os.environ.pop("GH_PMASK_MERGE", None)
        res["launches"] = enc.pmask_report().launches
    copy_rate = 2 * total / 1e6 / np.median(copy_k)  # GB/s: read + written
    for k in ("0", "1"):
        rate = total / 1e6 / np.median(hist[k])    # GB/s: read only
        res[f"k_hist_merge{k}_ms"] = med(hist[k])
        res[f"k_hist_merge{k}_GBps"] = round(rate, 1)
        res[f"k_hist_merge{k}_over_copy_rate"] = round(float(rate / copy_rate), 3)
        res[f"call_merge{k}_ms"] = med(call[k])
    res.update({
        "bytes": total, "k_copy_ms": med(copy_k), "k_copy_GBps": round(copy_rate, 1),
        "k_split_over_copy_rate": split.get(("float32" if kind == "int32_ids" else kind, m, tensor_bytes)),
        "k_code_ms": med(code_k), "k_decide_ms": med(decide_k),
        "call_new_ms": med(call["default"]), "call_old_route_ms": med(old), "call_old_route_min_ms": round(min(old), 4),
        "call_accepted": bool(np.median(call["default"]) <= min(old)), "checked": bool(ok)})
    return res


def sizes_line():
    """The size table from the GPU path: container bytes with the default mask and with "auto"."""
    rng = np.random.default_rng(7)
    w = rng.normal(0, 0.02, 65536).astype(np.float32)
    bf16 = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)  # nearest-even
    tensors = (("bf16", bf16), ("fp32", w), ("int32_ids", rng.integers(0, 1000, 65536).astype(np.int32)),
               ("int64_ms", np.cumsum(rng.integers(0, 50, 65536)).astype(np.int64) + 1_700_000_000_000),
               ("uint8_uniform", rng.integers(0, 256, 65536, dtype=np.uint8)))
    arrays = [a for _, a in tensors]
    want_m, want_pb = gh.choose_planes_masks(arrays)
    auto, default = gh.encode_tensors(arrays, "auto"), gh.encode_tensors(arrays)
    res = {"bench": "pmask_sizes", "seed": 7, "nelem": 65536}
    for (name, a), ia, idf, m, pb in zip(tensors, auto, default, want_m, want_pb):
        pa = gh.parse_planes(ia)
        assert pa.coded_mask == int(m) and np.array_equal(gh.decode_tensors([ia])[0], a.view(np.uint8))
        res[name] = {"plane_bytes": [int(x) for x in pb[: a.itemsize]], "default_mask": gh.default_planes_mask(a.itemsize),
                     "auto_mask": int(m), "container_default": int(idf.size), "container_auto": int(ia.size)}
    return res


def main():
    small, big = opt("--small", 256), opt("--big", 8)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    split = split_fractions()
    lines = [json.dumps(sizes_line())]
    print(lines[-1], flush=True)
    for kind in ("bfloat16", "float32", "int32_ids"):
        for m, nbytes in ((small, 64 << 10), (big, 128 << 20)):
            if m:
                lines.append(json.dumps(config(kind, m, nbytes, split)))
                print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
