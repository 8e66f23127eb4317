#!/usr/bin/env python3
"""A/B of the HELL SpMM for a caller who holds the reference's multivector layout (vector j at base + j*pitch).

One process, one set of allocations, the matrices of bench.py's SpMM leg (synth.hell_uniform_on_device, fp64, 5 M rows x 32,
hackSize --hack, default 32), the vectors in the pitch layout with pitch = rows.  Three routes:

  a  spgpuDhellspmmMv                                                   (include/spgpu/ext/spmm_mv.h)
  b  mvInterleave(X) [+ mvInterleave(Y)] -> spgpuDhellspmm -> mvDeinterleave(Z)     what such a caller had before
  c  spgpuDhellspmm alone on data that is already interleaved           the ceiling a holder of pitch vectors does not reach

Before any timing a and b must agree bit for bit.  Then the routes are timed in alternating blocks (a b c a b c ...), each block
a number of back-to-back calls between two device events; per route the median over the blocks is the figure and
(max - min) / median over its blocks the spread that a difference between routes has to clear.  GB/s and the fraction of the
8 TB/s roofline use the ALGORITHMIC bytes of the product (the matrix once, X once, Z once, Y once if beta != 0) for every
route: the transposes of route b are time it spends, not bytes the product owes.

    python tools/bench_spmm_mv.py                       # all cases -> profiles/spmm_mv_ab.json
    python tools/bench_spmm_mv.py --cases banded16 --routes a --blocks 2 --out /dev/null      # under a profiler
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOFLINE_BYTES_PER_S = 8.0e12
CASES = {  # name -> (pattern, right-hand sides, beta)
    "banded16": ("banded", 16, 0.0), "banded8": ("banded", 8, 0.0), "banded16_beta": ("banded", 16, -0.5),
    "window16": ("window", 16, 0.0), "window8": ("window", 8, 0.0), "random16": ("random", 16, 0.0),
}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def algorithmic_bytes(rows, cols, nnz, hack, count, beta):
    return nnz * (8 + 4) + rows * 4 + (rows // hack) * 4 + count * (cols + rows * (2 if beta != 0 else 1)) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000 // 32 * 32)
    ap.add_argument("--nnz-per-row", type=int, default=32)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--routes", default="a,b,c")
    ap.add_argument("--hack", type=int, default=32, help="hackSize of the matrices (a multiple of 32 reaches the strip kernels)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=60.0, help="device time a block aims at (5 to 100 calls)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_mv_ab.json"))
    args = ap.parse_args()

    import torch
    from spgpu_amd import capi, synth
    assert torch.cuda.is_available(), "bench_spmm_mv.py measures on the GPU; there is none"
    h = capi.create_handle(0)
    n, L, hack = args.rows, args.nnz_per_row, args.hack
    routes = args.routes.split(",")
    kmax = max(CASES[c][1] for c in args.cases.split(","))
    Xp, Yp = synth.device_vector(n * kmax, "D", 3), synth.device_vector(n * kmax, "D", 4)   # pitch layout, pitch = n
    Zp, Zb = torch.empty_like(Yp), torch.empty_like(Yp)
    Xi, Yi, Zi = torch.empty_like(Xp), torch.empty_like(Yp), torch.empty_like(Yp)          # interleaved, ld = count
    result = dict(device=torch.cuda.get_device_name(0), rows=n, nnz_per_row=L, hack_size=hack, type="fp64", pitch=n,
                  roofline_bytes_per_s=ROOFLINE_BYTES_PER_S, blocks=args.blocks, cases={})
    built = {}
    for name in args.cases.split(","):
        pattern, k, beta = CASES[name]
        if pattern not in built:
            built.clear()
            built[pattern] = synth.hell_uniform_on_device(n, L, pattern, "D", hack, seed=1)
        m = built[pattern]
        mat = (_p(m["cM"]), _p(m["rP"]), hack, _p(m["hack_offsets"]), _p(m["rS"]), None, L, n)
        y_p, y_i = (Yp, Yi) if beta != 0 else (None, None)

        def route_a():
            capi.hellspmm_mv["D"](h, _p(Zp), _p(y_p), 1.0, *mat, _p(Xp), beta, 0, k, n, n)

        def route_b():
            capi.mv_interleave["D"](h, _p(Xi), k, _p(Xp), n, n, k)
            if beta != 0:
                capi.mv_interleave["D"](h, _p(Yi), k, _p(Yp), n, n, k)
            capi.hellspmm["D"](h, _p(Zi), _p(y_i), 1.0, *mat, _p(Xi), beta, 0, k, k, k)
            capi.mv_deinterleave["D"](h, _p(Zb), n, _p(Zi), k, n, k)

        def route_c():   # Xi / Yi hold the interleaved copies the check below made through route b
            capi.hellspmm["D"](h, _p(Zi), _p(y_i), 1.0, *mat, _p(Xi), beta, 0, k, k, k)

        run = {"a": route_a, "b": route_b, "c": route_c}
        # ---- the same bits, before any timing ----
        Zp.fill_(float("nan"))
        Zb.fill_(float("nan"))
        route_a()
        route_b()
        torch.cuda.synchronize()
        same = torch.equal(Zp[:n * k].view(torch.int64), Zb[:n * k].view(torch.int64)) and not torch.isnan(Zp[:n * k]).any().item()
        assert same, f"{name}: routes a and b differ"

        def block(fn, calls):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / calls

        calls = {}
        for r in routes:   # warm-up, and the number of calls that fills a block
            block(run[r], 2)
            calls[r] = max(5, min(100, int(args.block_ms / max(block(run[r], 3), 1e-3))))
        times = {r: [] for r in routes}
        for _ in range(args.blocks):
            for r in routes:
                times[r].append(block(run[r], calls[r]))
        nbytes = algorithmic_bytes(n, m["cols"], m["nnz"], hack, k, beta)
        case = dict(pattern=pattern, rhs=k, beta=beta, algorithmic_bytes=nbytes, bits_a_equal_b=True, routes={})
        for r in routes:
            med = statistics.median(times[r])
            case["routes"][r] = dict(ms_median=round(med, 4), ms_min=round(min(times[r]), 4), ms_max=round(max(times[r]), 4),
                                     spread=round((max(times[r]) - min(times[r])) / med, 4), calls_per_block=calls[r],
                                     gb_per_s=round(nbytes / med / 1e6, 1),
                                     roofline_fraction=round(nbytes / (med * 1e-3) / ROOFLINE_BYTES_PER_S, 4))
        med = {r: case["routes"][r]["ms_median"] for r in routes}
        if "a" in med and "b" in med:
            case["a_over_b"] = round(med["a"] / med["b"], 4)
            # a is faster than b by more than the block-to-block spread of either: its slowest block beats b's fastest
            case["a_faster_than_b_beyond_spread"] = bool(case["routes"]["a"]["ms_max"] < case["routes"]["b"]["ms_min"])
        if "a" in med and "c" in med:
            case["a_over_c"] = round(med["a"] / med["c"], 4)
        result["cases"][name] = case
        print(name, json.dumps({r: case["routes"][r]["ms_median"] for r in routes}),
              {key: case[key] for key in ("a_over_b", "a_over_c") if key in case}, flush=True)
    capi.spgpuDestroy(h)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({"wrote": args.out, "cases": list(result["cases"])}))


if __name__ == "__main__":
    main()
