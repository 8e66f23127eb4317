#!/usr/bin/env python3
"""A/B of the device-scalar Level-1 calls on pitch multivectors (include/spgpu/ext/device_scalars_mv.h) against what their caller had
before: a loop of `count` single-vector calls (include/spgpu/device_scalars.h) on the same arrays.

One process, three measurements:

  dot      spgpuDmdotDevice against `count` spgpuDdotDevice calls, n = 5 M, count 8 and 16
  update   spgpuDmaxpbyQuotDevice against `count` spgpuDaxpbyQuotDevice calls, same shapes (beta_j != 0: three streams per vector)
  cg       tools/cg_multi_amd.bin at grid 1024 with 8 right-hand sides: us per block iteration of its three legs -- (a) every column
           alone with the single-vector calls, (b) one graph of multivector calls, (c) the same with the fused pair-dot

For dot and update the two routes are timed in alternating blocks (new loop new loop ...), each block a number of back-to-back calls
between two device events; per route the median over the blocks is the figure and (max - min) / median over its blocks the spread.
The multivector reduction shares 1024 workgroups among its vectors where each single-vector call has up to 1024 of its own: at large n
it may well be the slower one.  The figures are recorded as they come.  The tool is run --cg-runs times; the figure of a leg is the
median over the runs and the spread (max - min) / median over them.

    python tools/bench_mv_level1.py                 # -> profiles/mv_level1_ab.json
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
    ap.add_argument("--n", type=int, default=5_000_000)
    ap.add_argument("--counts", default="8,16")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=40.0, help="device time a block aims at (3 to 200 calls)")
    ap.add_argument("--cg-grid", type=int, default=1024)
    ap.add_argument("--cg-iters", type=int, default=60)
    ap.add_argument("--cg-count", type=int, default=8)
    ap.add_argument("--cg-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv_level1_ab.json"))
    args = ap.parse_args()

    import torch
    from spgpu_amd import capi, synth
    assert torch.cuda.is_available(), "bench_mv_level1.py measures on the GPU; there is none"
    h = capi.create_handle(0)
    n = args.n
    pitch = (n + 2) & ~1                    # 16-byte multiple, larger than n
    counts = [int(c) for c in args.counts.split(",")]
    kmax = max(counts)
    result = dict(device=torch.cuda.get_device_name(0), type="fp64", n=n, pitch=pitch, blocks=args.blocks, cases={})

    def block(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    def ab(name, run, nbytes):
        calls = {}
        for r in run:       # warm-up, and the number of calls that fills a block
            block(run[r], 2)
            calls[r] = max(3, min(200, int(args.block_ms / max(block(run[r], 3), 1e-3))))
        times = {r: [] for r in run}
        for _ in range(args.blocks):
            for r in run:
                times[r].append(block(run[r], calls[r]))
        case = dict(algorithmic_bytes=nbytes, routes={})
        for r in run:
            med = statistics.median(times[r])
            case["routes"][r] = dict(ms_median=round(med, 4), ms_min=round(min(times[r]), 4), ms_max=round(max(times[r]), 4),
                                     spread=round((max(times[r]) - min(times[r])) / med, 4), calls_per_block=calls[r],
                                     gb_per_s=round(nbytes / med / 1e6, 1))
        case["speedup_loop_over_new"] = round(case["routes"]["loop"]["ms_median"] / case["routes"]["new"]["ms_median"], 4)
        case["new_faster_beyond_spread"] = bool(case["routes"]["new"]["ms_max"] < case["routes"]["loop"]["ms_min"])
        case["new_slower_beyond_spread"] = bool(case["routes"]["new"]["ms_min"] > case["routes"]["loop"]["ms_max"])
        result["cases"][name] = case
        print(name, json.dumps({r: case["routes"][r]["ms_median"] for r in run}), case["speedup_loop_over_new"], flush=True)

    X = synth.device_vector(pitch * kmax, "D", 3)
    Y = synth.device_vector(pitch * kmax, "D", 4)
    Zn, Zl = torch.empty_like(X), torch.empty_like(X)
    num, den = synth.device_vector(kmax, "D", 5) + 2, synth.device_vector(kmax, "D", 6) + 2
    out_n, out_l = torch.zeros(kmax, dtype=X.dtype, device=X.device), torch.zeros(kmax, dtype=X.dtype, device=X.device)
    for k in counts:
        def dot_new():
            capi.mdot_device["D"](h, _p(out_n), n, _p(X), _p(Y), k, pitch)

        def dot_loop():
            for j in range(k):
                capi.dot_device["D"](h, _p(out_l, j), n, _p(X, j * pitch), _p(Y, j * pitch))

        def upd_new():
            capi.maxpby_quot_device["D"](h, _p(Zn), n, _p(den), _p(num), _p(Y), _p(num), _p(den), 1, _p(X), k, pitch)

        def upd_loop():
            for j in range(k):
                capi.axpby_quot_device["D"](h, _p(Zl, j * pitch), n, _p(den, j), _p(num, j), _p(Y, j * pitch), _p(num, j), _p(den, j), 1,
                                            _p(X, j * pitch))

        dot_new(), dot_loop(), upd_new(), upd_loop()
        torch.cuda.synchronize()
        rows = lambda t: torch.stack([t[j * pitch:j * pitch + n] for j in range(k)]).view(torch.int64)
        assert torch.equal(rows(Zn), rows(Zl)), f"update {k}: the multivector call and the loop differ"
        ab(f"dot_{k}", {"new": dot_new, "loop": dot_loop}, 2 * 8 * n * k)
        result["cases"][f"dot_{k}"]["bits_equal_to_loop"] = bool(torch.equal(out_n[:k].view(torch.int64), out_l[:k].view(torch.int64)))
        ab(f"update_{k}", {"new": upd_new, "loop": upd_loop}, 3 * 8 * n * k)
    del X, Y, Zn, Zl
    torch.cuda.empty_cache()
    capi.spgpuDestroy(h)

    # the block solver: a fresh process per run, its own graphs and events
    exe = os.path.join(ROOT, "tools", "cg_multi_amd.bin")
    line = re.compile(r"per block iteration: reference ([\d.]+) us, multi ([\d.]+) us .*, fused ([\d.]+) us")
    legs = {"reference": [], "multi": [], "fused": []}
    for _ in range(args.cg_runs):
        done = subprocess.run([exe, str(args.cg_grid), str(args.cg_iters), str(args.cg_count)], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0 and "PASSED" in done.stdout, done.stdout + done.stderr
        found = line.search(done.stdout)
        for leg, us in zip(legs, found.groups()):
            legs[leg].append(float(us))
    cg = dict(grid=args.cg_grid, iterations=args.cg_iters, vectors=args.cg_count, runs=args.cg_runs, legs={})
    for leg, us in legs.items():
        med = statistics.median(us)
        cg["legs"][leg] = dict(us_median=round(med, 1), us_min=min(us), us_max=max(us), spread=round((max(us) - min(us)) / med, 4))
    for leg in ("multi", "fused"):
        cg[f"speedup_reference_over_{leg}"] = round(cg["legs"]["reference"]["us_median"] / cg["legs"][leg]["us_median"], 3)
    result["cg"] = cg
    print("cg", json.dumps(cg), flush=True)

    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({"wrote": args.out, "cases": len(result["cases"])}))


if __name__ == "__main__":
    main()
