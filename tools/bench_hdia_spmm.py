#!/usr/bin/env python3
"""A/B of the HDIA SpMM on pitch-layout multivectors (include/spgpu/ext/hdia_spmm.h) against what its caller had before: `count`
calls of spgpu?hdiaspmv, one per vector, on the same arrays.

One process and one set of allocations per matrix.  Matrices: the 7-point Laplacian on 256^3 and (up to 8 vectors) 512^3, the
5-point Laplacian on 1024^2, all HDIA with hackSize 32; fp64 and fp32; 1, 2, 4, 8 and 16 vectors at pitch = rows, beta = 0.  Two
routes:

  new   spgpu?hdiaspmmMv                              one pass over dM per 8 vectors
  loop  spgpu?hdiaspmv, vector by vector              `count` passes over dM: the yardstick

Before any timing the two must agree bit for bit.  Then they are timed in alternating blocks (new loop new loop ...), each block
a number of back-to-back calls between two device events; per route the median over the blocks is the figure and
(max - min) / median over its blocks the spread.  Beside the medians and their ratio every case records the ratio of ALGORITHMIC
bytes: dM + offsets + hackOffsets once per pass of 8 vectors plus count * (x + z), against count times the SpMV's bytes.

    python tools/bench_hdia_spmm.py                                     # all cases -> profiles/hdia_spmm_ab.json
    python tools/bench_hdia_spmm.py --matrices lap7_256 --types D --counts 8 --routes new --blocks 2 --out /dev/null   # under a profiler

A run of some matrices only keeps the other matrices' cases that the output file already holds."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_V = 8      # vectors per pass (spgpu_amd/csrc/hdia_spmm.hip, kHdiaMmMaxV)
HACK = 32
MATRICES = {"lap7_256": ("lap7", 256, 16), "lap7_512": ("lap7", 512, 8), "lap5_1024": ("lap5", 1024, 16)}   # kind, grid, most vectors
SIZEOF = {"S": 4, "D": 8}


def _p(t, at=0):
    return C.c_void_p(t.data_ptr() + at * t.element_size()) if t is not None else None


def build(kind, grid, letter):
    """HDIA arrays in HBM: dict(rows, cols, nnz, height, dM, offsets, hack_offsets)."""
    import numpy as np
    from spgpu_amd import formats, synth
    if kind == "lap7":
        return synth.hdia_laplacian7_on_device(grid, letter, HACK)
    n, m, r, c, v = synth.laplacian_2d_5pt(grid, dtype=np.float64 if letter == "D" else np.float32)
    host = formats.coo_to_hdia(n, m, r, c, v, HACK)
    dev = formats.DeviceHdia(host)
    return dict(rows=n, cols=m, nnz=int(r.size), height=int(host["hack_offsets"][-1]), dM=dev.dM, offsets=dev.offsets,
                hack_offsets=dev.hack_offsets)


def algorithmic_bytes(mat, letter, count):
    """(new, loop): the matrix once per pass resp. once per vector; x and z once per vector (beta == 0: no y)."""
    size = SIZEOF[letter]
    matrix = mat["height"] * HACK * size + mat["height"] * 4 + (mat["rows"] // HACK + 1) * 4
    vectors = (mat["cols"] + mat["rows"]) * size
    passes = (count + MAX_V - 1) // MAX_V
    return passes * matrix + count * vectors, count * (matrix + vectors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default=",".join(MATRICES))
    ap.add_argument("--types", default="D,S")
    ap.add_argument("--counts", default="1,2,4,8,16")
    ap.add_argument("--routes", default="new,loop")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-ms", type=float, default=40.0, help="device time a block aims at (3 to 200 calls)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdia_spmm_ab.json"))
    args = ap.parse_args()

    import torch
    from spgpu_amd import capi, synth
    assert torch.cuda.is_available(), "bench_hdia_spmm.py measures on the GPU; there is none"
    h = capi.create_handle(0)
    routes = args.routes.split(",")
    counts = [int(c) for c in args.counts.split(",")]
    result = dict(device=torch.cuda.get_device_name(0), hack_size=HACK, vectors_per_pass=MAX_V, blocks=args.blocks, beta=0.0, cases={})
    if args.out != os.devnull and os.path.exists(args.out):
        with open(args.out) as f:
            result["cases"] = json.load(f).get("cases", {})

    def block(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / calls

    for name in args.matrices.split(","):
        kind, grid, most = MATRICES[name]
        for letter in args.types.split(","):
            mat = build(kind, grid, letter)
            n, cols = mat["rows"], mat["cols"]
            mine = [c for c in counts if c <= most]
            kmax = max(mine)
            X = synth.device_vector(cols * kmax, letter, 3)     # pitch layout, pitch = the vector's length
            Zn, Zl = torch.empty(n * kmax, dtype=X.dtype, device=X.device), torch.empty(n * kmax, dtype=X.dtype, device=X.device)
            m_args = (_p(mat["dM"]), _p(mat["offsets"]), HACK, _p(mat["hack_offsets"]), n, cols)
            one, zero = capi.scalar(letter, 1.0), capi.scalar(letter, 0.0)
            for k in mine:
                def new():
                    capi.hdiaspmm_mv[letter](h, _p(Zn), None, one, *m_args, _p(X), zero, k, cols, n)

                def loop():
                    for j in range(k):
                        capi.hdiaspmv[letter](h, _p(Zl, j * n), None, one, *m_args, _p(X, j * cols), zero)

                run = {"new": new, "loop": loop}
                Zn.fill_(float("nan"))
                Zl.fill_(float("nan"))
                new()
                loop()
                torch.cuda.synchronize()
                bits = torch.int64 if letter == "D" else torch.int32
                same = torch.equal(Zn[:n * k].view(bits), Zl[:n * k].view(bits)) and not torch.isnan(Zn[:n * k]).any().item()
                assert same, f"{name} {letter} {k}: the SpMM and the loop of SpMVs differ"
                calls = {}
                for r in routes:   # warm-up, and the number of calls that fills a block
                    block(run[r], 2)
                    calls[r] = max(3, min(200, int(args.block_ms / max(block(run[r], 3), 1e-3))))
                times = {r: [] for r in routes}
                for _ in range(args.blocks):
                    for r in routes:
                        times[r].append(block(run[r], calls[r]))
                bytes_new, bytes_loop = algorithmic_bytes(mat, letter, k)
                case = dict(matrix=name, type={"D": "fp64", "S": "fp32"}[letter], rows=n, stored_diagonals=mat["height"], vectors=k,
                            algorithmic_bytes=dict(new=bytes_new, loop=bytes_loop), bytes_ratio_loop_over_new=round(bytes_loop / bytes_new, 4),
                            bits_equal=True, routes={})
                for r in routes:
                    med = statistics.median(times[r])
                    nbytes = bytes_new if r == "new" else bytes_loop
                    case["routes"][r] = dict(ms_median=round(med, 4), ms_min=round(min(times[r]), 4), ms_max=round(max(times[r]), 4),
                                             spread=round((max(times[r]) - min(times[r])) / med, 4), calls_per_block=calls[r],
                                             gb_per_s=round(nbytes / med / 1e6, 1))
                if "new" in times and "loop" in times:
                    rn, rl = case["routes"]["new"], case["routes"]["loop"]
                    case["speedup_loop_over_new"] = round(rl["ms_median"] / rn["ms_median"], 4)
                    case["speedup_over_bytes_ratio"] = round(case["speedup_loop_over_new"] / case["bytes_ratio_loop_over_new"], 4)
                    case["new_faster_beyond_spread"] = bool(rn["ms_max"] < rl["ms_min"])
                    # one vector: not slower than the SpMV beyond the run-to-run spread of the loop itself
                    case["new_not_slower_beyond_loop_spread"] = bool(rn["ms_median"] <= rl["ms_median"] * (1 + rl["spread"]))
                result["cases"][f"{name}_{letter}_{k}"] = case
                print(f"{name} {letter} {k:2d}", json.dumps({r: case["routes"][r]["ms_median"] for r in routes}),
                      {key: case[key] for key in ("speedup_loop_over_new", "bytes_ratio_loop_over_new") if key in case}, flush=True)
            del X, Zn, Zl, mat
            torch.cuda.empty_cache()
    capi.spgpuDestroy(h)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({"wrote": args.out, "cases": len(result["cases"])}))


if __name__ == "__main__":
    main()
