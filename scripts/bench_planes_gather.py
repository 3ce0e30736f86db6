# Element gather (DESIGN.md "Element gather"): rows of 1024 elements of bf16 tables of N(0, 0.02)
# weights with the top plane coded, gathered by random row ids from a resident, indexed batch, on
# one GPU, in one process.  Two tables: 256 tensors of 64 KiB and 8 tensors of 128 MiB; batches of
# 64, 4 096 and 65 536 row ids.  Per cell, three routes to the same rows:
#   new  the ranges from the ids by torch ops on the device, gather_elements_device, elements_wait;
#   (a)  what a caller had before without a full decode: (stream, lo, hi) byte ranges built on the
#        host and uploaded, gather_device of the coded plane, torch index_select of the stored
#        arena's rows, the torch re-interleave;
#   (b)  the full decode() + join_planes_device + planes_wait, then torch index_select of the rows.
# Variants alternate rep by rep; medians of REPS after WARMUP.  A cell is accepted when the new
# median is not above the other route's fastest rep.  Every output is checked.  Also: the split of
# the new route's kernel time (plan kernels, inner batched gather, range join) and the range join's
# rate beside gh_bw_copy of the same bytes.
# Usage: python scripts/bench_planes_gather.py [--small 256] [--big 8] [--out profiles/planes_gather.jsonl]
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
ROW = 1024  # elements per row
BATCHES = (64, 4096, 65536)


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def med(xs):
    return round(float(np.median(xs)), 4)


def wall_ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def config(m, tensor_bytes):
    dtype, e = torch.bfloat16, 2
    nelem = tensor_bytes // e
    rows_per = nelem // ROW
    mask = 1 << (e - 1)
    g = torch.Generator(device="cuda").manual_seed(375)
    table = torch.empty(m * nelem, dtype=dtype, device="cuda")
    for i in range(m):
        table[i * nelem: (i + 1) * nelem] = (torch.randn(nelem, device="cuda", generator=g) * 0.02).to(dtype)
    whole = torch.empty_like(table)  # route (b)'s joined tensors
    items = [(table.data_ptr() + i * tensor_bytes, nelem, e, mask) for i in range(m)]
    out_items = [(whole.data_ptr() + i * tensor_bytes, nelem, e, mask) for i in range(m)]
    slots, ns, stored_bytes = gh.planes_layout(items)
    stored = torch.empty(stored_bytes, dtype=torch.uint8, device="cuda")
    # (nelem is a multiple of 16: the stored planes lie back to back, the arena is a [rows, ROW] matrix)
    assert ns == m and stored_bytes == m * nelem and [sl[0][1] for sl in slots] == [i * nelem for i in range(m)]
    rows_view = table.view(torch.int16).view(-1, ROW)
    lines = []
    with gh.BatchEncoder(0) as enc, gh.BatchDecoder(0) as dec, gh.BatchDecoder(0) as dec_b:
        enc.load_planes_device(items, stored.data_ptr(), stored_bytes)
        enc.plan()
        enc.encode()
        enc.wait()
        coded = int(enc.sizes().sum())
        dec.load_device(enc.items())
        dec_b.load_device(enc.items())
        dec.index()
        dec.wait()
        torch.cuda.synchronize()
        for n in BATCHES:
            ids = torch.randint(0, m * rows_per, (n,), device="cuda", generator=g)
            ids_h = ids.cpu().numpy()
            nbytes = n * ROW * e
            dst = torch.empty(n * ROW, dtype=dtype, device="cuda")
            top = torch.empty(n * ROW, dtype=torch.uint8, device="cuda")
            cp_src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            cp_dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            want = rows_view.index_select(0, ids)

            def new_route():
                t = ids // rows_per
                lo = (ids - t * rows_per) * ROW
                ranges = torch.stack((t, lo, lo + ROW), 1)
                torch.cuda.current_stream().synchronize()  # (the gather runs on the batch's stream: the ranges are ready)
                dec.gather_elements_device(items, stored.data_ptr(), stored_bytes, ranges.data_ptr(), n, dst.data_ptr(),
                                           nbytes)
                return dec.elements_wait()

            def route_a():
                t = ids_h // rows_per
                lo = (ids_h - t * rows_per) * ROW
                br = torch.from_numpy(np.stack((t, lo, lo + ROW), 1)).cuda()
                torch.cuda.current_stream().synchronize()
                dec.gather_device(br.data_ptr(), n, top.data_ptr(), n * ROW)
                dec.gather_wait()
                low = stored.view(-1, ROW).index_select(0, ids)
                out = torch.stack((low, top.view(n, ROW)), 2).contiguous()
                torch.cuda.synchronize()
                return out

            def route_b():
                dec_b.decode(timed=False)
                dec_b.join_planes_device(out_items, stored.data_ptr(), stored_bytes)
                dec_b.planes_wait()
                out = whole.view(-1, ROW).index_select(0, ids)
                torch.cuda.synchronize()
                return out

            t_new, t_a, t_b, k_all, k_exp, k_join, k_copy = [], [], [], [], [], [], []
            ok = True
            for rep in range(WARMUP + REPS):
                tn, r = wall_ms(new_route)
                ta, oa = wall_ms(route_a)
                tb, ob = wall_ms(route_b)
                kc = gh.bw_copy(cp_dst.data_ptr(), cp_src.data_ptr(), nbytes, reps=1)
                if rep >= WARMUP:
                    t_new.append(tn), t_a.append(ta), t_b.append(tb)
                    k_all.append(r.kernel_ms), k_exp.append(r.expand_ms), k_join.append(r.join_ms), k_copy.append(kc)
                if rep in (0, WARMUP + REPS - 1):
                    ok &= bool(torch.equal(dst.view(torch.int16).view(n, ROW), want))
                    ok &= bool(torch.equal(oa.view(n, ROW * e).view(torch.int16), want))
                    ok &= bool(torch.equal(ob.view(torch.int16), want))
            gb = 2 * nbytes / 1e6  # read + written per ms -> GB/s
            res = {"bench": "planes_gather", "dtype": "bfloat16", "tensors": m, "tensor_bytes": tensor_bytes, "row_elems": ROW,
                   "rows": n, "bytes": nbytes, "table_fraction": round(n / (m * rows_per), 5), "coded_bytes": coded,
                   "reps": REPS, "launches": r.launches, "npieces": int(r.npieces),
                   "new_ms": med(t_new), "route_a_ms": med(t_a), "route_a_min_ms": round(min(t_a), 4),
                   "route_b_ms": med(t_b), "route_b_min_ms": round(min(t_b), 4),
                   "accepted_vs_a": bool(np.median(t_new) <= min(t_a)), "accepted_vs_b": bool(np.median(t_new) <= min(t_b)),
                   "k_all_ms": med(k_all), "k_plan_ms": med(k_exp), "k_join_ms": med(k_join),
                   "k_inner_gather_ms": med(np.asarray(k_all) - np.asarray(k_exp) - np.asarray(k_join)),
                   "k_copy_ms": med(k_copy), "k_join_GBps": round(gb / np.median(k_join), 1),
                   "k_copy_GBps": round(gb / np.median(k_copy), 1),
                   "k_join_over_copy_rate": round(float(np.median(k_copy) / np.median(k_join)), 3), "bitexact": bool(ok)}
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
    return lines


def main():
    small, big = opt("--small", 256), opt("--big", 8)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    lines = []
    for m, nbytes in ((small, 64 << 10), (big, 128 << 20)):
        if m:
            lines += config(m, nbytes)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
