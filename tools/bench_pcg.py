#!/usr/bin/env python3
"""A/B of one Jacobi-PCG iteration captured as a graph: the fused step of include/spgpu/ext/precond.h against the same iteration
written with the calls the library had before.

  fused     spgpuDhellspmvDotDevice, spgpuDaxpbyPairAxyDotDevice, spgpuDaxpbyQuotDevice                      5 kernels
  unfused   spgpuDhellspmvDotDevice, spgpuDaxpbyPairDotDevice, spgpuDaxy, spgpuDdotDevice, spgpuDaxpbyQuotDevice   8 kernels

The matrix is that of tools/pcg_amd.c at grid 1024: A = S L S, L the 5-point Laplacian, in HELL with hackSize 32; dinv comes from
spgpuDhellDiag.  Both routes replay two graphs that alternate the cells of r.z (as tools/pcg_amd.c does), from the same start.  They
are timed in alternating blocks (fused unfused fused unfused ...) after a warm-up block each; a block restores the start vectors
(untimed) and then replays --iters iterations between two device events.  Per route the median over the blocks is the figure and
(max - min) / median the spread.  After its first block each route's x is kept: the two must be the same bits.  For context the
fused plain-CG iteration of tools/cg_amd.bin on the unscaled Laplacian of the same size is timed too (its own process).

    python tools/bench_pcg.py                       # -> profiles/pcg_ab.json
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(t, at=0):
    return C.c_void_p(t.data_ptr() + at * t.element_size()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=400, help="iterations per timed block (an even number)")
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--commit", default=None, help="recorded in the result; default: git's HEAD where the tree is a checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcg_ab.json"))
    args = ap.parse_args()
    assert args.iters % 2 == 0

    import numpy as np
    import torch
    from spgpu_amd import capi, formats, synth
    assert torch.cuda.is_available(), "bench_pcg.py measures on the GPU; there is none"
    h = capi.create_handle(0)
    side = torch.cuda.Stream()
    capi.spgpuSetStream(h, C.c_void_p(side.cuda_stream))

    g = args.grid
    n, _, r, c, v = synth.laplacian_2d_5pt(g)
    scale = 10.0 ** (3.0 * np.random.default_rng(1).random(n) - 1.5)
    v = (scale[r] * v.astype(np.float64)) * scale[c]
    hell = formats.ell_to_hell(formats.coo_to_ell(n, r, c, v), 32)
    A = formats.DeviceHell(hell)
    b = formats.to_device(np.bincount(r, weights=v, minlength=n))                  # b = A * ones
    dinv, x, res, p, ap_, z = (torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(6))
    cells = torch.zeros(5, dtype=torch.float64, device="cuda:0")                    # (r.z, |r|^2) twice, p.Ap
    RZ = (0, 2)
    PAP = 4
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        capi.hell_diag["D"](h, _p(dinv), _p(A.cM), _p(A.rP), 32, _p(A.hack_offsets), _p(A.rS), n, 0, 1)
    side.synchronize()
    assert bool(torch.equal(dinv, formats.to_device(1.0 / ((scale * 4.0) * scale)))), "spgpuDhellDiag differs from the host's diagonal"

    def spmv_dot():
        capi.hellspmv_dot_device["D"](h, _p(cells, PAP), None, _p(ap_), None, capi.scalar("D", 1.0), _p(A.cM), _p(A.rP), 32, _p(A.hack_offsets),
                                      _p(A.rS), n, _p(p), capi.scalar("D", 0.0), 0)

    def fused(old, new):
        spmv_dot()
        capi.axpby_pair_axy_dot_device["D"](h, _p(cells, new), n, _p(x), _p(x), _p(p), _p(res), _p(res), _p(ap_), _p(z), _p(dinv),
                                            _p(cells, old), _p(cells, PAP))
        capi.axpby_quot_device["D"](h, _p(p), n, _p(cells, new), _p(cells, old), _p(p), None, None, 0, _p(z))

    def unfused(old, new):
        spmv_dot()
        capi.axpby_pair_dot_device["D"](h, _p(cells, new + 1), n, _p(x), _p(x), _p(p), _p(res), _p(res), _p(ap_), _p(cells, old), _p(cells, PAP))
        capi.axy["D"](h, _p(z), n, capi.scalar("D", 1.0), _p(dinv), _p(res))
        capi.dot_device["D"](h, _p(cells, new), n, _p(res), _p(z))
        capi.axpby_quot_device["D"](h, _p(p), n, _p(cells, new), _p(cells, old), _p(p), None, None, 0, _p(z))

    def capture(step):
        graphs = []
        for parity in range(2):
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                step(RZ[parity], RZ[1 - parity])
            graphs.append(graph)
        torch.cuda.synchronize()
        return graphs

    def start():
        """x = 0, r = b, z = dinv o r, p = z, r.z in the first pair of cells."""
        with torch.cuda.stream(side):
            x.zero_()
            res.copy_(b)
            capi.axy_dot_device["D"](h, _p(cells, RZ[0]), n, _p(z), _p(dinv), _p(res))
            p.copy_(z)

    def block(graphs, iters):
        start()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            t0.record(side)
            for i in range(iters):
                graphs[i & 1].replay()
            t1.record(side)
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / iters

    routes = {"fused": (capture(fused), 5), "unfused": (capture(unfused), 8)}
    kept = {}
    for name, (graphs, _) in routes.items():                                        # warm-up, and the iterate each route reaches
        block(graphs, args.iters)
        kept[name] = (x.clone(), cells.clone())
    same = bool(torch.equal(kept["fused"][0].view(torch.int64), kept["unfused"][0].view(torch.int64))
                and torch.equal(kept["fused"][1][:4].view(torch.int64), kept["unfused"][1][:4].view(torch.int64)))
    times = {name: [] for name in routes}
    for _ in range(args.blocks):
        for name, (graphs, _) in routes.items():
            times[name].append(block(graphs, args.iters))
    capi.spgpuSetStream(h, None)
    capi.spgpuDestroy(h)

    result = dict(device=torch.cuda.get_device_name(0), commit=args.commit or _commit(), type="fp64", grid=g, rows=n, iterations_per_block=args.iters,
                  blocks=args.blocks, x_and_scalars_bit_identical=same, routes={})
    for name, (_, kernels) in routes.items():
        med = statistics.median(times[name])
        result["routes"][name] = dict(kernels_per_iteration=kernels, us_per_iteration_median=round(med, 2),
                                      us_min=round(min(times[name]), 2), us_max=round(max(times[name]), 2),
                                      spread=round((max(times[name]) - min(times[name])) / med, 4))
    f_, u_ = result["routes"]["fused"], result["routes"]["unfused"]
    result["speedup_unfused_over_fused"] = round(u_["us_per_iteration_median"] / f_["us_per_iteration_median"], 3)
    result["fused_faster_beyond_spread"] = bool(f_["us_max"] < u_["us_min"])

    # context: the fused plain-CG iteration (5 kernels) on the unscaled Laplacian, in its own process
    exe = os.path.join(ROOT, "tools", "cg_amd.bin")
    done = subprocess.run([exe, str(g), "60", "1e-30", "timing"], capture_output=True, text=True, timeout=300)
    found = re.search(r"fused replay: \d+ iterations, [\d.]+ ms total, ([\d.]+) us per iteration", done.stdout)
    result["plain_cg_fused_us_per_iteration"] = float(found.group(1)) if done.returncode == 0 and found else None
    print(json.dumps(result, indent=1))
    assert same, "the fused and the unfused iteration differ"
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
