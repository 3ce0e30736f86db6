# Byte planes (DESIGN.md "Byte planes"): bf16 and fp32 tensors of N(0, 0.02) weights on one
# GPU, in one process, at two sizes: 256 tensors of 64 KiB and 8 tensors of 128 MiB.  Per
# configuration:
#   (1) kernel rate: the split kernel (gh_planes_load_times) and the join kernel
#       (gh_planes_report.kernel_ms) beside gh_bw_copy of the same bytes (nelem * E read,
#       nelem * E written), and their fraction of the copy's rate;
#   (2) load: load_planes_device's wall time beside what a caller has to do without it: the
#       torch de-interleave t.view(uint8).view(-1, E).t().contiguous() of every tensor, then
#       BatchEncoder.load_device of the coded planes; and decode() + join + planes_wait beside
#       decode() into a torch arena + wait + the torch re-interleave of every tensor;
#   (3) (once) the compressed sizes of the seeded recipe (seed 7, 65536 elements, nearest-even)
#       for bf16, fp32 and fp16 from the GPU path (encode_tensors): the container with the top
#       plane coded, and every plane's coded size.
# Variants alternate rep by rep; medians of REPS after WARMUP.  The new path is accepted when
# its median is not above the other route's fastest rep.  Every output is checked.
# Usage: python scripts/bench_planes.py [--small 256] [--big 8] [--out profiles/planes.jsonl]
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "cse375-finalproj-huffman-decoding_amd"))
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


def config(dtype, m, tensor_bytes):
    e = torch.empty(0, dtype=dtype).element_size()
    nelem = tensor_bytes // e
    mask = 1 << (e - 1)
    g = torch.Generator(device="cuda").manual_seed(375)
    ts = [(torch.randn(nelem, device="cuda", generator=g) * 0.02).to(dtype) for _ in range(m)]
    total = m * tensor_bytes
    items = [(t.data_ptr(), nelem, e, mask) for t in ts]
    _, ns, stored_bytes = gh.planes_layout(items)
    stored = torch.empty(stored_bytes, dtype=torch.uint8, device="cuda")
    cp_src = torch.empty(pad16(total), dtype=torch.uint8, device="cuda")
    cp_dst = torch.empty(pad16(total), dtype=torch.uint8, device="cuda")
    outs = [torch.empty_like(t) for t in ts]
    out_items = [(o.data_ptr(), nelem, e, mask) for o in outs]
    arena_off = gh.batch_layout([nelem] * m)
    arena = torch.empty(int(arena_off[-1]), dtype=torch.uint8, device="cuda")
    res = {"bench": "planes", "dtype": str(dtype).replace("torch.", ""), "tensors": m, "tensor_bytes": tensor_bytes,
           "coded_mask": mask, "reps": REPS}
    ok = True
    split_k, copy_k, join_k, new_load, old_load, new_dec, old_dec = [], [], [], [], [], [], []

    def deinterleave():
        return [t.view(torch.uint8).view(-1, e).t().contiguous() for t in ts]

    def old_route_load(enc):
        mats = deinterleave()
        enc.load_device([(mt[e - 1].data_ptr(), nelem) for mt in mats], hip_stream=torch.cuda.current_stream().cuda_stream)
        return mats

    def new_route_decode(dec):
        dec.decode(timed=False)
        dec.join_planes_device(out_items, stored.data_ptr(), stored_bytes)
        return dec.planes_wait()

    def old_route_decode(dec, mats):
        dec.decode(arena.data_ptr(), arena.numel(), timed=False)
        dec.wait()
        back = []
        for i, mt in enumerate(mats):
            top = arena[int(arena_off[i]): int(arena_off[i]) + nelem]
            back.append(torch.stack([mt[p] for p in range(e - 1)] + [top]).t().contiguous())
        torch.cuda.synchronize()
        return back

    with gh.BatchEncoder(0) as enc, gh.BatchEncoder(0) as enc_old, gh.BatchDecoder(0) as dec, gh.BatchDecoder(0) as dec_old:
        torch.cuda.synchronize()
        # one full pass of both routes: the batches the decode side times, and the checks
        enc.load_planes_device(items, stored.data_ptr(), stored_bytes)
        enc.plan()
        enc.encode()
        rep_e = enc.wait()
        mats = old_route_load(enc_old)
        enc_old.plan()
        enc_old.encode()
        enc_old.wait()
        sizes_new, sizes_old = enc.sizes(), enc_old.sizes()
        ok &= bool(np.array_equal(sizes_new, sizes_old))
        step = max(1, m // 16)
        ok &= all(np.array_equal(enc.download(i), enc_old.download(i)) for i in range(0, m, step)) if tensor_bytes <= 1 << 20 \
            else bool(np.array_equal(enc.download(0)[:1 << 20], enc_old.download(0)[:1 << 20]))
        dec.load_device(enc.items())
        dec_old.load_device(enc_old.items())
        for rep in range(WARMUP + REPS):
            tl, _ = wall_ms(lambda: enc.load_planes_device(items, stored.data_ptr(), stored_bytes))
            ks = enc.planes_load_ms()
            kc = gh.bw_copy(cp_dst.data_ptr(), cp_src.data_ptr(), pad16(total), reps=1)
            to, _ = wall_ms(lambda: old_route_load(enc_old))
            td, rj = wall_ms(lambda: new_route_decode(dec))
            tod, back = wall_ms(lambda: old_route_decode(dec_old, mats))
            if rep >= WARMUP:
                split_k.append(ks), copy_k.append(kc), join_k.append(rj.kernel_ms)
                new_load.append(tl), old_load.append(to), new_dec.append(td), old_dec.append(tod)
        # (the loads above replaced the encoders' batches: the decoders' words are their own copies)
        torch.cuda.synchronize()
        ok &= all(bool(torch.equal(o, t)) for o, t in zip(outs, ts))
        ok &= all(bool(torch.equal(b.reshape(-1).view(dtype), t)) for b, t in zip(back, ts))
        res["join_launches"] = rj.launches
    gb = 2 * total / 1e6  # bytes moved per ms -> GB/s: read + written
    res.update({
        "bytes": total, "coded_bytes": int(sizes_new.sum()), "stored_bytes": stored_bytes,
        "ratio": round((int(sizes_new.sum()) + m * nelem * (e - 1)) / total, 4),
        "encode_kernel_ms": round(rep_e.kernel_ms, 4),
        "k_split_ms": med(split_k), "k_join_ms": med(join_k), "k_copy_ms": med(copy_k),
        "k_split_GBps": round(gb / np.median(split_k), 1), "k_join_GBps": round(gb / np.median(join_k), 1),
        "k_copy_GBps": round(gb / np.median(copy_k), 1),
        "k_split_over_copy_rate": round(float(np.median(copy_k) / np.median(split_k)), 3),
        "k_join_over_copy_rate": round(float(np.median(copy_k) / np.median(join_k)), 3),
        "load_new_ms": med(new_load), "load_torch_route_ms": med(old_load), "load_torch_route_min_ms": round(min(old_load), 4),
        "load_accepted": bool(np.median(new_load) <= min(old_load)),
        "decode_join_new_ms": med(new_dec), "decode_torch_route_ms": med(old_dec),
        "decode_torch_route_min_ms": round(min(old_dec), 4),
        "decode_accepted": bool(np.median(new_dec) <= min(old_dec)),
        "bitexact": bool(ok)})
    return res


def sizes_line():
    """The compressed sizes of the seeded recipe from the GPU path, as fractions of the raw bytes."""
    w = np.random.default_rng(7).normal(0, 0.02, 65536).astype(np.float32)
    bf16 = torch.from_numpy(w).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)  # nearest-even
    res = {"bench": "planes_sizes", "seed": 7, "nelem": 65536}
    for name, a in (("bf16", bf16), ("fp32", w), ("fp16", w.astype(np.float16))):
        e = a.itemsize
        raw = a.view(np.uint8)
        top = gh.encode_tensors([a])[0]
        every = gh.parse_planes(gh.encode_tensors([a], [(1 << e) - 1])[0])
        assert np.array_equal(gh.decode_tensors([top])[0], raw)
        res[name] = {"interleaved": round(gh.encode_gpu(raw).size / raw.size, 4),
                     "planes_coded": [round(every.planes[p].raw.size / a.size, 4) for p in range(e)],
                     "top_plane_coded_rest_stored": round(top.size / raw.size, 4)}
    return res


def main():
    small, big = opt("--small", 256), opt("--big", 8)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = [json.dumps(sizes_line())]
    print(lines[-1], flush=True)
    for dtype in (torch.bfloat16, torch.float32):
        for m, nbytes in ((small, 64 << 10), (big, 128 << 20)):
            if m:
                lines.append(json.dumps(config(dtype, m, nbytes)))
                print(lines[-1], flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
