#!/usr/bin/env python3
"""GPU box: what building A^T from a stored HELL matrix costs (include/spgpu/ext/transpose_device.h), against the same sort without
the front end, in one process and on the same allocations:

  transpose   spgpuHellTransposeLengthsDevice + spgpuHellPlanDevice + spgpuHellTransposeDevice on the HELL arrays of A
  coo         spgpuCooRowLengthsDevice + spgpuHellPlanDevice + spgpuCooToHellDevice on the COO listing of A with rows and columns
              swapped, already resident in HBM (include/spgpu/convert_device.h): one stable sort by the new row, no HELL slab read

on  banded     BASELINE.json configs[1]: 10 M rows x 32, banded, fp64
    powerlaw   the power-law matrix of bench.py (lengths of mean 32, longest 2 048, columns near the row, fp64) as the rows come

Per route: the median over --reps repetitions (after --warmup, the routes alternating inside a repetition) of the host clock around
the calls, which end in a device synchronise, and of the last call alone (the fill).  The destination is zeroed by the caller before
every run, outside the clock.  The two results are compared byte for byte.  Reported, not gated.

usage: bench_transpose.py [--rows 10000000] [--reps 5] [--warmup 2] [--out profiles/hell_transpose_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from spgpu_amd import capi, formats, synth  # noqa: E402

DEV = "cuda:0"
HACK = 32


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def measure(handle, name, lengths, pattern, reps, warmup):
    n = int(lengths.size)
    rows, cols, vals = synth.ragged_coo_on_device(lengths, n, pattern, 2048, "D", seed=5, device=DEV)
    nnz = int(rows.numel())
    a = formats.coo_to_ordered_hell_device(handle, n, rows, cols, vals, "D", HACK, order=False)
    i32 = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=DEV)
    t_lens, t_ho = i32(n), i32((n + HACK - 1) // HACK)
    work_t = torch.empty(capi.spgpuHellTransposeWorkBytes(n, n, a["slots"]), dtype=torch.uint8, device=DEV)
    work_c = torch.empty(capi.spgpuCooConvertWorkBytes(n, nnz), dtype=torch.uint8, device=DEV)
    longest, count, height = C.c_int(0), C.c_int(0), C.c_int(0)

    def route_transpose(out_v, out_i):
        t0 = clock()
        ok(capi.spgpuHellTransposeLengthsDevice(handle, p(t_lens), C.byref(longest), C.byref(count), p(a["rP"]), HACK, p(a["hack_offsets"]),
                                                p(a["rS"]), None, n, n, 0, a["slots"], p(work_t)))
        ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(t_ho), HACK, n, p(t_lens), p(work_t)))
        assert out_i is None or HACK * height.value <= out_i.numel()
        t1 = clock()
        if out_i is not None:
            ok(capi.spgpuHellTransposeDevice(handle, p(out_v), p(out_i), p(t_ho), HACK, 0, p(a["cM"]), p(a["rP"]), HACK, p(a["hack_offsets"]),
                                             p(a["rS"]), None, n, n, 0, a["slots"], capi.TYPE_DOUBLE, p(t_lens), p(work_t)))
        t2 = clock()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    def route_coo(out_v, out_i):
        t0 = clock()
        ok(capi.spgpuCooRowLengthsDevice(handle, p(t_lens), C.byref(longest), n, nnz, p(cols), 0, p(work_c)))
        ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(t_ho), HACK, n, p(t_lens), p(work_c)))
        assert HACK * height.value <= out_i.numel()
        t1 = clock()
        ok(capi.spgpuCooToHellDevice(handle, p(out_v), p(out_i), p(t_ho), HACK, 0, n, nnz, p(cols), p(rows), p(vals), 0, capi.TYPE_DOUBLE,
                                     p(t_lens), p(work_c)))
        t2 = clock()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    route_transpose(None, None)          # untimed: the slots of the destination
    t_slots = HACK * height.value
    assert count.value == nnz
    out_v, out_i = torch.empty(t_slots, dtype=torch.float64, device=DEV), torch.empty(t_slots, dtype=torch.int32, device=DEV)
    ref_v, ref_i = torch.empty_like(out_v), torch.empty_like(out_i)
    routes = {"transpose": route_transpose, "coo": route_coo}
    times = {key: [] for key in routes}
    for rep in range(warmup + reps):
        for key, run in routes.items():
            out_v.zero_()
            out_i.zero_()
            sample = run(out_v, out_i)
            if rep >= warmup:
                times[key].append(sample)
    ref_v.zero_()
    ref_i.zero_()
    route_coo(ref_v, ref_i)
    plan = (t_lens.clone(), t_ho.clone())
    out_v.zero_()
    out_i.zero_()
    route_transpose(out_v, out_i)
    same = bool(torch.equal(out_i, ref_i) and torch.equal(out_v.view(torch.int64), ref_v.view(torch.int64))
                and torch.equal(plan[0], t_lens) and torch.equal(plan[1], t_ho))
    entry = dict(matrix=name, rows=n, nnz=nnz, source_slots=a["slots"], transposed_slots=t_slots, longest_transposed_row=longest.value,
                 work_bytes=dict(transpose=int(work_t.numel()), coo=int(work_c.numel())), same_bytes_as_coo_route=same, routes={})
    for key, samples in times.items():
        whole = statistics.median(s[0] for s in samples)
        entry["routes"][key] = dict(ms=round(whole, 3), ms_min=round(min(s[0] for s in samples), 3),
                                    ms_max=round(max(s[0] for s in samples), 3),
                                    fill_ms=round(statistics.median(s[1] for s in samples), 3))
    entry["transpose_over_coo"] = round(entry["routes"]["transpose"]["ms"] / entry["routes"]["coo"]["ms"], 3)
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hell_transpose_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_transpose.py measures on a GPU; none found")
    handle = capi.create_handle(0)
    results = [measure(handle, "banded", np.full(args.rows, 32, np.int32), "band", args.reps, args.warmup)]
    torch.cuda.empty_cache()
    lengths = synth.power_law_lengths(args.rows, mean=32.0, max_len=2048, seed=5)
    results.append(measure(handle, "powerlaw", lengths, "near", args.reps, args.warmup))
    out = dict(tool="tools/bench_transpose.py", device=torch.cuda.get_device_name(0), type="fp64", hack_size=HACK, reps=args.reps,
               warmup=args.warmup, clock="host clock around calls that end in a device synchronise; median",
               routes=dict(transpose="spgpuHellTransposeLengthsDevice + spgpuHellPlanDevice + spgpuHellTransposeDevice",
                           coo="spgpuCooRowLengthsDevice + spgpuHellPlanDevice + spgpuCooToHellDevice on the resident swapped COO listing"),
               matrices=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    capi.spgpuDestroy(handle)


if __name__ == "__main__":
    main()
