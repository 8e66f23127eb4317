#!/usr/bin/env python3
"""A/B of the fused SpMV + dot for HDIA matrices (include/spgpu/ext/hdia_solver.h) against the calls it replaces, in one process
and on the same matrix, at three sizes in fp64: the 5-point Laplacian on 1024^2 and the 7-point one on 128^3 and 512^3.

  call        spgpuDhdiaspmvDotDevice (2 kernels)  against  spgpuDhdiaspmv + spgpuDdotDevice (3 kernels), each a captured graph
  iteration   the two legs of tools/cg_hdia_amd.c, each two captured graphs that alternate the cells of |r|^2:
              fused    spgpuDhdiaspmvDotDevice, spgpuDaxpbyPairDotDevice, spgpuDaxpbyQuotDevice                            5 kernels
              unfused  spgpuDhdiaspmv, spgpuDdotDevice, 2 x spgpuDaxpbyQuotDevice, spgpuDdotDevice, spgpuDaxpbyQuotDevice   8 kernels

The matrix is written in HBM directly: hackSize 32, every hack stores every diagonal of the stencil (a coefficient whose
neighbour does not exist is 0; the first and last hacks so store a few diagonals cooToHdia would drop).  x0 = 0, b = A * ones.  The
two routes of a set are timed in alternating blocks (fused unfused fused unfused ...) after a warm-up block each; an iteration
block restores the start vectors (untimed) and then replays its iterations between two device events.  Per route the median over
the blocks is the figure and (max - min) / median the spread.  After its warm-up block each leg's x and |r|^2 are kept: the two
must be the same bits, and so must z and p.Ap of the two call routes.

    python tools/bench_hdia_cg.py                       # -> profiles/hdia_cg_ab.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HACK = 32
#: (name, grid, dimensions, iterations or calls per timed block)
SIZES = (("1024^2 5-point", 1024, 2, 200), ("128^3 7-point", 128, 3, 100), ("512^3 7-point", 512, 3, 20))


def _p(t, at=0):
    return C.c_void_p(t.data_ptr() + at * t.element_size()) if t is not None else None


def laplacian_hdia(g, dims):
    """(dM [hacks, diagonals, 32], offsets [hacks * diagonals], hackOffsets [hacks + 1], rows) of the stencil in HBM."""
    import torch
    n = g ** dims
    assert n % HACK == 0
    strides = [g ** k for k in range(dims)]                                           # x fastest
    offs = sorted([-s for s in strides] + [0] + strides)
    i = torch.arange(n, dtype=torch.int64, device="cuda:0")
    dM = torch.empty((n // HACK, len(offs), HACK), dtype=torch.float64, device="cuda:0")
    for d, o in enumerate(offs):
        if o == 0:
            col = torch.full((n,), 2.0 * dims, dtype=torch.float64, device="cuda:0")
        else:
            s = abs(o)
            coord = (i // s) % g
            col = -((coord > 0) if o < 0 else (coord < g - 1)).to(torch.float64)
        dM[:, d, :] = col.view(n // HACK, HACK)
    del i
    hacks = n // HACK
    offsets = torch.tensor(offs, dtype=torch.int32, device="cuda:0").repeat(hacks)
    hack_offsets = (torch.arange(hacks + 1, dtype=torch.int64, device="cuda:0") * len(offs)).to(torch.int32)
    return dM, offsets, hack_offsets, n


def measure(h, side, name, g, dims, per_block, blocks):
    import torch
    from spgpu_amd import capi
    dM, offsets, hack_offsets, n = laplacian_hdia(g, dims)
    one, zero = capi.scalar("D", 1.0), capi.scalar("D", 0.0)
    b, x, res, p, ap_, ap2 = (torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(6))
    cells = torch.zeros(4, dtype=torch.float64, device="cuda:0")                    # |r|^2 twice, p.Ap, p.Ap of the second call route
    RR, PAP = (0, 1), 2
    matrix = (_p(dM), _p(offsets), HACK, _p(hack_offsets), n, n)

    def spmv_dot(out=None, cell=PAP):
        capi.hdiaspmv_dot_device["D"](h, _p(cells, cell), None, _p(ap_ if out is None else out), None, one, *matrix, _p(p), zero)

    def spmv_then_dot(out=None, cell=PAP):
        out = ap_ if out is None else out
        capi.hdiaspmv["D"](h, _p(out), None, one, *matrix, _p(p), zero)
        capi.dot_device["D"](h, _p(cells, cell), n, _p(p), _p(out))

    def fused(old, new):
        spmv_dot()
        capi.axpby_pair_dot_device["D"](h, _p(cells, new), n, _p(x), _p(x), _p(p), _p(res), _p(res), _p(ap_), _p(cells, old), _p(cells, PAP))
        capi.axpby_quot_device["D"](h, _p(p), n, _p(cells, new), _p(cells, old), _p(p), None, None, 0, _p(res))

    def unfused(old, new):
        spmv_then_dot()
        capi.axpby_quot_device["D"](h, _p(x), n, None, None, _p(x), _p(cells, old), _p(cells, PAP), 0, _p(p))
        capi.axpby_quot_device["D"](h, _p(res), n, None, None, _p(res), _p(cells, old), _p(cells, PAP), 1, _p(ap_))
        capi.dot_device["D"](h, _p(cells, new), n, _p(res), _p(res))
        capi.axpby_quot_device["D"](h, _p(p), n, _p(cells, new), _p(cells, old), _p(p), None, None, 0, _p(res))

    def capture(fn, *args):
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            fn(*args)
        torch.cuda.synchronize()
        return graph

    def start():
        """x = 0, r = p = b, |r|^2 in the first cell."""
        with torch.cuda.stream(side):
            x.zero_()
            res.copy_(b)
            p.copy_(b)
            capi.dot_device["D"](h, _p(cells, RR[0]), n, _p(res), _p(res))

    def block(graphs, restore):
        if restore:
            start()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            t0.record(side)
            for i in range(per_block):
                graphs[i % len(graphs)].replay()
            t1.record(side)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / per_block

    def ab(routes, restore):
        """routes: name -> (graphs, kernels); returns the figures and what each route left after its warm-up block."""
        kept, times = {}, {k: [] for k in routes}
        for key, (graphs, _) in routes.items():
            block(graphs, restore)
            kept[key] = (x.clone(), cells.clone(), ap_.clone(), ap2.clone())
        for _ in range(blocks):
            for key, (graphs, _) in routes.items():
                times[key].append(block(graphs, restore))
        out = {}
        for key, (_, kernels) in routes.items():
            med = statistics.median(times[key])
            out[key] = dict(kernels=kernels, us_median=round(med, 2), us_min=round(min(times[key]), 2), us_max=round(max(times[key]), 2),
                            spread=round((max(times[key]) - min(times[key])) / med, 4))
        return out, kept

    # b = A * ones
    with torch.cuda.stream(side):
        p.fill_(1.0)
        capi.hdiaspmv["D"](h, _p(b), None, one, *matrix, _p(p), zero)
    side.synchronize()

    # ---- the call against the two calls it replaces, on p = b
    start()
    side.synchronize()
    calls, kept = ab({"fused": ([capture(spmv_dot, ap_, PAP)], 2), "unfused": ([capture(spmv_then_dot, ap2, PAP + 1)], 3)}, restore=False)
    last = kept["unfused"]
    same_call = bool(torch.equal(last[2].view(torch.int64), last[3].view(torch.int64))
                     and torch.equal(last[1][PAP:PAP + 1].view(torch.int64), last[1][PAP + 1:PAP + 2].view(torch.int64)))

    # ---- the two legs of the iteration
    legs, kept = ab({"fused": ([capture(fused, RR[k], RR[1 - k]) for k in range(2)], 5),
                     "unfused": ([capture(unfused, RR[k], RR[1 - k]) for k in range(2)], 8)}, restore=True)
    same_leg = bool(torch.equal(kept["fused"][0].view(torch.int64), kept["unfused"][0].view(torch.int64))
                    and torch.equal(kept["fused"][1][:3].view(torch.int64), kept["unfused"][1][:3].view(torch.int64)))
    out = dict(matrix=name, rows=n, stored_diagonals_per_hack=2 * dims + 1, per_block=per_block, call=calls,
               call_z_and_result_bit_identical=same_call, iteration=legs, iteration_x_and_scalars_bit_identical=same_leg)
    for key in ("call", "iteration"):
        f_, u_ = out[key]["fused"], out[key]["unfused"]
        out[f"{key}_unfused_over_fused"] = round(u_["us_median"] / f_["us_median"], 3)
        out[f"{key}_fused_faster_beyond_spread"] = bool(f_["us_max"] < u_["us_min"])
        out[f"{key}_fused_slower_beyond_spread"] = bool(f_["us_min"] > u_["us_max"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--sizes", default="0,1,2", help="indices into SIZES")
    ap.add_argument("--commit", default=None, help="recorded in the result; default: git's HEAD where the tree is a checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdia_cg_ab.json"))
    args = ap.parse_args()

    import torch
    from spgpu_amd import capi
    assert torch.cuda.is_available(), "bench_hdia_cg.py measures on the GPU; there is none"
    h = capi.create_handle(0)
    side = torch.cuda.Stream()
    capi.spgpuSetStream(h, C.c_void_p(side.cuda_stream))
    result = dict(device=torch.cuda.get_device_name(0), commit=args.commit or _commit(), type="fp64", hack_size=HACK, blocks=args.blocks,
                  sizes=[])
    for k in (int(s) for s in args.sizes.split(",")):
        name, g, dims, per_block = SIZES[k]
        result["sizes"].append(measure(h, side, name, g, dims, per_block, args.blocks))
        torch.cuda.empty_cache()
    capi.spgpuSetStream(h, None)
    capi.spgpuDestroy(h)
    print(json.dumps(result, indent=1))
    for size in result["sizes"]:
        assert size["call_z_and_result_bit_identical"] and size["iteration_x_and_scalars_bit_identical"], size["matrix"]
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({"wrote": args.out}))


def _commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


if __name__ == "__main__":
    main()
