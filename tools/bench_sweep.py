#!/usr/bin/env python3
"""GPU box: the multicolour sweep and the residual on CSR arrays (include/spgpu/ext/sweep_device.h), fp64, in one process, on two
whole matrices: a, the 7-point matrix of a 200^3 grid, and b, the 27-point matrix of a 100^3 grid, with random diagonally dominant
coefficients (the matrices of tools/bench_ilu0.py).  Legs per matrix:
  sweep <shape> on A     one FORWARD + one BACKWARD spgpuCsrSweepDevice on A with `order`, through one row shape -- thread, group8,
                         group32 -- with the public call's segmenting
  sweep <shape> on B     the same on the permuted B = A(order, order) with order == NULL
  trsv route on B        the route that exists without the sweep: gather b by order, spgpuCsrTrsvDevice LOWER then UPPER on B, gather
                         back by inverse (a zero-guess application: the same traffic, not the same result)
  residual <shape>       spgpuCsrResidualDevice on A
  hell residual          spgpuDhellspmv on the converted matrix plus spgpuDaxpby
Every sweep leg's x is compared byte for byte with the thread leg's on the same matrix before anything is timed.

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
calls, ended by a device synchronise; minimum and maximum are kept.  THE RULE (ILU(0)'s): a shape counts as fastest only when its
min-max range lies below that of every other shape; otherwise thread.  The file records what the rule would choose beside what
csrc/sweep_rules.h ships; no number is fixed in advance.

usage: bench_sweep.py [--cube7 200] [--cube27 100] [--cases a,b] [--reps 5] [--warmup 1] [--out profiles/csr_sweep_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from spgpu_amd import capi, formats  # noqa: E402
from bench_ilu0 import csr_of, grid_pattern  # noqa: E402  (the same matrices)

DEV = "cuda:0"
SHAPES = {"thread": capi.SWEEP_SHAPE_THREAD, "group8": 8, "group32": 32}
FALLBACK = "thread"


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def summary(samples):
    return dict(ms=round(statistics.median(samples), 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3))


def chosen_by_the_rule(legs, prefix, suffix=""):
    """The fastest shape of the legs `prefix <shape><suffix>` by its median, if its range lies below the range of EVERY other one."""
    mine = {name[len(prefix) + 1:len(name) - len(suffix)]: leg for name, leg in legs.items()
            if name.startswith(prefix + " ") and name.endswith(suffix) and name[len(prefix) + 1:len(name) - len(suffix)] in SHAPES}
    best = min(mine, key=lambda name: mine[name]["ms"])
    clear = all(mine[best]["ms_max"] < leg["ms_min"] for name, leg in mine.items() if name != best)
    return best if clear else FALLBACK


class Swept:
    """One matrix with its sweep Plan; order None: the matrix is in colour order."""

    def __init__(self, handle, n, mat, colours, order, colour_ptr, colour_of):
        self.handle, self.n, self.mat, self.colours, self.order = handle, n, mat, colours, order
        self.diag_pos = torch.empty(n, dtype=torch.int32, device=DEV)
        self.host = np.zeros(colours + 1, np.int32)
        self.at = self.host.ctypes.data_as(C.POINTER(C.c_int))
        entries = C.c_int(0)
        work = torch.empty(capi.spgpuCsrSweepWorkBytes(n), dtype=torch.uint8, device=DEV)
        ok(capi.spgpuCsrSweepPlanDevice(handle, C.byref(entries), p(self.diag_pos), self.at, n, colours, p(order), p(colour_ptr), p(colour_of),
                                        p(mat[0]), p(mat[1]), 0, p(work)))
        self.entries = entries.value

    def sweep(self, x, b, shape):
        ptr, cols, vals = self.mat
        for direction in (capi.SWEEP_FORWARD, capi.SWEEP_BACKWARD):
            ok(capi.spgpuCsrSweepDeviceWith(self.handle, p(x), p(b), self.n, self.colours, p(self.order), self.at, p(self.diag_pos), p(ptr),
                                            p(cols), p(vals), 0, direction, None, capi.TYPE_DOUBLE, self.entries, shape, -1, 0))

    def residual(self, r, b, x, shape):
        ptr, cols, vals = self.mat
        ok(capi.spgpuCsrResidualDeviceWith(self.handle, p(r), p(b), p(x), self.n, p(ptr), p(cols), p(vals), 0, capi.TYPE_DOUBLE, self.entries,
                                           shape, 0))


def trsv_plans(handle, n, mat):
    plans = []
    work = torch.empty(capi.spgpuCsrTrsvWorkBytes(n), dtype=torch.uint8, device=DEV)
    for side in (capi.TRSV_LOWER, capi.TRSV_UPPER):
        levels = C.c_int(0)
        order, level_ptr = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n + 1, dtype=torch.int32, device=DEV)
        host = np.zeros(n + 1, np.int32)
        ok(capi.spgpuCsrTrsvPlanDevice(handle, C.byref(levels), p(order), p(level_ptr), host.ctypes.data_as(C.POINTER(C.c_int)), n, p(mat[0]),
                                       p(mat[1]), 0, side, capi.TRSV_DIAG_STORED, p(work)))
        plans.append((side, levels.value, order, level_ptr, host))
    return plans


def measure(handle, name, n, mat, reps, warmup):
    ptr, cols, vals = mat
    nnz = int(cols.numel())
    colours, rounds = C.c_int(0), C.c_int(0)
    work = torch.empty(capi.spgpuCsrColourWorkBytes(n), dtype=torch.uint8, device=DEV)
    permute_work = torch.empty(capi.spgpuCsrPermuteWorkBytes(n), dtype=torch.uint8, device=DEV)
    colour_of, order, inverse = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
    ok(capi.spgpuCsrColourDevice(handle, C.byref(colours), C.byref(rounds), p(colour_of), n, p(ptr), p(cols), 0, p(work)))
    colour_ptr = torch.empty(colours.value + 1, dtype=torch.int32, device=DEV)
    ok(capi.spgpuCsrColourOrderDevice(handle, p(order), p(inverse), p(colour_ptr), n, colours.value, p(colour_of), p(work)))
    b_mat = (torch.empty_like(ptr), torch.empty_like(cols), torch.empty_like(vals))
    ok(capi.spgpuCsrPermuteDevice(handle, p(b_mat[0]), p(b_mat[1]), p(b_mat[2]), n, p(order), p(inverse), p(ptr), p(cols), p(vals), 0,
                                  capi.TYPE_DOUBLE, p(permute_work)))
    torch.cuda.synchronize()
    sides = {"A": Swept(handle, n, mat, colours.value, order, colour_ptr, colour_of),
             "B": Swept(handle, n, b_mat, colours.value, None, colour_ptr, None)}
    plans = trsv_plans(handle, n, b_mat)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    b, x0 = (torch.randn(n, dtype=torch.float64, device=DEV, generator=gen) for _ in range(2))
    x, r, t, bp, xp = (torch.empty_like(b) for _ in range(5))
    # the HELL copy of A for the residual's baseline (host converters, set-up only)
    row_of = torch.repeat_interleave(torch.arange(n, device=DEV), (ptr[1:] - ptr[:-1]).long()).int().cpu().numpy()
    hell = formats.DeviceHell(formats.ell_to_hell(formats.coo_to_ell(n, row_of, cols.cpu().numpy(), vals.cpu().numpy()), 32))

    # ---- every shape gives the thread leg's bytes, on A and on B ----
    same = True
    for which, side in sides.items():
        start = x0 if which == "A" else x0[order.long()]
        rhs = b if which == "A" else b[order.long()]
        first = None
        for shape in SHAPES.values():
            x.copy_(start)
            side.sweep(x, rhs, shape)
            torch.cuda.synchronize()
            first = x.clone() if first is None else first
            same = same and bool(torch.equal(first.view(torch.int64), x.view(torch.int64)))
    x.copy_(x0)

    def trsv_route():
        capi.gath["D"](handle, p(bp), n, p(order), 0, p(b))
        for (side, levels, row_order, level_ptr, host), (out, rhs) in zip(plans, ((t, bp), (xp, t))):
            ok(capi.spgpuCsrTrsvDevice(handle, p(out), p(rhs), n, levels, p(row_order), p(level_ptr), host.ctypes.data_as(C.POINTER(C.c_int)),
                                       p(b_mat[0]), p(b_mat[1]), p(b_mat[2]), 0, side, capi.TRSV_DIAG_STORED, capi.TYPE_DOUBLE))
        capi.gath["D"](handle, p(r), n, p(inverse), 0, p(xp))

    def hell_residual():
        hell.spmv(handle, t, t, 1.0, x, 0.0)
        capi.axpby["D"](handle, p(r), n, 1.0, p(b), -1.0, p(t))

    legs = {}
    for leg, shape in SHAPES.items():
        legs[f"sweep {leg} on A"] = lambda shape=shape: sides["A"].sweep(x, b, shape)
        legs[f"sweep {leg} on B"] = lambda shape=shape: sides["B"].sweep(x, b, shape)
        legs[f"residual {leg}"] = lambda shape=shape: sides["A"].residual(r, b, x, shape)
    legs["trsv route on B"] = trsv_route
    legs["hell residual"] = hell_residual
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    shipped = [k for k, v in SHAPES.items() if v == capi.csr_sweep_default_shape(n, nnz)]
    entry = dict(matrix=name, rows=n, entries=nnz, mean_row_length=round(nnz / n, 2), colours=colours.value, rounds=rounds.value,
                 launches_a_symmetric_sweep=capi.csr_sweep_launches(sides["A"].at, colours.value, capi.SWEEP_SYMMETRIC, -1),
                 trsv_levels=dict(lower=plans[0][1], upper=plans[1][1]), every_shape_gives_the_same_bytes=same,
                 legs={leg: summary(samples) for leg, samples in times.items()})
    entry.update(chosen_by_the_rule={"sweep on A": chosen_by_the_rule(entry["legs"], "sweep", " on A"),
                                     "sweep on B": chosen_by_the_rule(entry["legs"], "sweep", " on B"),
                                     "residual": chosen_by_the_rule(entry["legs"], "residual")},
                 shipped=shipped[0] if shipped else None)
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cube7", type=int, default=200)
    ap.add_argument("--cube27", type=int, default=100)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_sweep_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sweep.py measures on a GPU; none found")
    handle = capi.create_handle(0)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    results = []
    for case in args.cases.split(","):
        side, full = (args.cube7, False) if case == "a" else (args.cube27, True)
        n, rows, cols = grid_pattern(side, 3, full)
        mat = csr_of(n, rows, cols, gen)
        name = f"{27 if full else 7}-point, {side}^3 grid"
        results.append(measure(handle, name, n, mat, args.reps, args.warmup))
        print(json.dumps(results[-1]), flush=True)
    rule = dict(rule="a shape counts as fastest only when its min-max range lies below that of every other shape; otherwise thread",
                thresholds_shipped="ILU(0)'s (csrc/sweep_rules.h): mean <= 2 thread, <= 16 a group of 8, beyond a group of 32",
                holds=all(e["chosen_by_the_rule"]["sweep on A"] == e["shipped"] for e in results) if results else None)
    out = dict(tool="tools/bench_sweep.py", device=torch.cuda.get_device_name(0), type="fp64", reps=args.reps, warmup=args.warmup,
               clock="host clock around the calls, ended by a device synchronise; median, legs alternating; one run", rule=rule,
               matrices=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
