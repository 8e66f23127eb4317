#!/usr/bin/env python3
"""GPU box: the multicolour ordering on CSR arrays (include/spgpu/ext/colour_device.h), fp64, in one process, on two whole matrices
with random, diagonally dominant coefficients:

  a  the 7-point matrix on a --cube7^3 grid       (6.9 stored entries per row)
  b  the 27-point matrix on a --cube27^3 grid     (26.2 stored entries per row)

Per case:
  colour <shape>     spgpuCsrColourDevice through one row shape -- thread (one thread per row), group8, group32, group64 (that many
                     lanes of one wavefront per row): every round runs in the shape, and the call synchronises once per round
  order              spgpuCsrColourOrderDevice
  permute <shape>    spgpuCsrPermuteDevice, B = A(order, order), through the same shapes
  ilu0 A / ilu0 B    the public spgpuCsrIlu0Device on A in its natural order and on B
  trsv L+U A / B     the lower (unit) and the upper solve with the factor, as a preconditioner applies them
and the colours, the rounds and the level counts of both orders.  Every leg's outputs are compared byte for byte with the first
one's before anything is timed.  What is measured is B against A in the same process and on the same vectors: no number is fixed
in advance.

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  THE RULE: on a and on b the public colouring runs the shape that
measured fastest; a shape counts as fastest only when its min-max range lies below that of every other shape; otherwise thread runs.
The permutation has one shape for every matrix: a group replaces thread only if its range lies below thread's on a and on b.

usage: bench_colour.py [--cube7 200] [--cube27 100] [--cases a,b] [--reps 5] [--warmup 1] [--out profiles/csr_colour_ab.json]"""
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
from spgpu_amd import capi  # noqa: E402
from bench_ilu0 import csr_of, grid_pattern  # noqa: E402  (the same matrices)

DEV = "cuda:0"
SHAPES = {"thread": capi.COLOUR_SHAPE_THREAD, "group8": 8, "group32": 32, "group64": 64}
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


def chosen_by_the_rule(legs, prefix):
    """The fastest shape of the legs `prefix <shape>` by its median, if its range lies below the range of EVERY other one."""
    mine = {name.split()[1]: leg for name, leg in legs.items() if name.startswith(prefix + " ")}
    best = min(mine, key=lambda name: mine[name]["ms"])
    clear = all(mine[best]["ms_max"] < leg["ms_min"] for name, leg in mine.items() if name != best)
    return best if clear else FALLBACK


class Side:
    """The ILU(0) Plan, the upper Plan and the two legs of one matrix; the factor and the vectors are shared by both sides."""

    def __init__(self, handle, n, mat, lu, vectors):
        self.handle, self.n, self.mat, self.lu, self.vectors = handle, n, mat, lu, vectors
        ptr, cols, _ = mat
        self.levels, self.u_levels = C.c_int(0), C.c_int(0)
        work = torch.empty(max(capi.spgpuCsrIlu0WorkBytes(n), capi.spgpuCsrTrsvWorkBytes(n)), dtype=torch.uint8, device=DEV)
        self.order, self.u_order, self.diag_pos = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
        self.level_ptr, self.u_level_ptr = (torch.empty(n + 1, dtype=torch.int32, device=DEV) for _ in range(2))
        self.host, self.u_host = np.zeros(n + 2, np.int32), np.zeros(n + 1, np.int32)
        self.at, self.u_at = (h.ctypes.data_as(C.POINTER(C.c_int)) for h in (self.host, self.u_host))
        ok(capi.spgpuCsrIlu0PlanDevice(handle, C.byref(self.levels), p(self.order), p(self.level_ptr), self.at, p(self.diag_pos), n, p(ptr),
                                       p(cols), 0, p(work)))
        ok(capi.spgpuCsrTrsvPlanDevice(handle, C.byref(self.u_levels), p(self.u_order), p(self.u_level_ptr), self.u_at, n, p(ptr), p(cols), 0,
                                       capi.TRSV_UPPER, capi.TRSV_DIAG_STORED, p(work)))
        torch.cuda.synchronize()

    def factor(self):
        ptr, cols, vals = self.mat
        ok(capi.spgpuCsrIlu0Device(self.handle, p(self.lu), p(vals), self.n, self.levels.value, p(self.order), p(self.level_ptr), self.at,
                                   p(self.diag_pos), p(ptr), p(cols), 0, capi.TYPE_DOUBLE))

    def apply(self):
        ptr, cols, _ = self.mat
        b, y, x = self.vectors
        ok(capi.spgpuCsrTrsvDevice(self.handle, p(y), p(b), self.n, self.levels.value, p(self.order), p(self.level_ptr), self.at, p(ptr), p(cols),
                                   p(self.lu), 0, capi.TRSV_LOWER, capi.TRSV_DIAG_UNIT, capi.TYPE_DOUBLE))
        ok(capi.spgpuCsrTrsvDevice(self.handle, p(x), p(y), self.n, self.u_levels.value, p(self.u_order), p(self.u_level_ptr), self.u_at, p(ptr),
                                   p(cols), p(self.lu), 0, capi.TRSV_UPPER, capi.TRSV_DIAG_STORED, capi.TYPE_DOUBLE))


def measure(handle, name, n, mat, reps, warmup):
    ptr, cols, vals = mat
    nnz = int(cols.numel())
    colours, rounds = C.c_int(0), C.c_int(0)
    work = torch.empty(capi.spgpuCsrColourWorkBytes(n), dtype=torch.uint8, device=DEV)
    permute_work = torch.empty(capi.spgpuCsrPermuteWorkBytes(n), dtype=torch.uint8, device=DEV)
    first_of, of, order, inverse = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(4))
    first_b = (torch.empty(n + 1, dtype=torch.int32, device=DEV), torch.empty(nnz, dtype=torch.int32, device=DEV),
               torch.empty(nnz, dtype=torch.float64, device=DEV))
    b_ptr, b_cols, b_vals = (torch.empty_like(t) for t in first_b)

    def colour(out, shape):
        ok(capi.spgpuCsrColourDeviceWith(handle, C.byref(colours), C.byref(rounds), p(out), n, p(ptr), p(cols), 0, p(work), shape, 0))

    def permute(out, shape):
        ok(capi.spgpuCsrPermuteDeviceWith(handle, p(out[0]), p(out[1]), p(out[2]), n, p(order), p(inverse), p(ptr), p(cols), p(vals), 0,
                                          capi.TYPE_DOUBLE, p(permute_work), shape, 0))

    colour(first_of, SHAPES[FALLBACK])
    colours_found, rounds_taken = colours.value, rounds.value
    colour_ptr = torch.empty(colours_found + 1, dtype=torch.int32, device=DEV)

    def sort():
        ok(capi.spgpuCsrColourOrderDevice(handle, p(order), p(inverse), p(colour_ptr), n, colours_found, p(first_of), p(work)))

    sort()
    permute(first_b, SHAPES[FALLBACK])
    torch.cuda.synchronize()
    same = True
    for shape in SHAPES.values():                                            # every leg against the first, before it is timed
        of.fill_(-7)
        for t in (b_ptr, b_cols):
            t.fill_(-7)
        b_vals.fill_(float("nan"))
        colour(of, shape)
        permute((b_ptr, b_cols, b_vals), shape)
        torch.cuda.synchronize()
        same = same and bool(torch.equal(first_of, of)) and (colours.value, rounds.value) == (colours_found, rounds_taken)
        same = same and bool(torch.equal(first_b[0], b_ptr)) and bool(torch.equal(first_b[1], b_cols))
        same = same and bool(torch.equal(first_b[2].view(torch.int64), b_vals.view(torch.int64)))
    lu = torch.empty(nnz, dtype=torch.float64, device=DEV)
    vectors = tuple(torch.ones(n, dtype=torch.float64, device=DEV) for _ in range(3))
    sides = dict(A=Side(handle, n, mat, lu, vectors), B=Side(handle, n, first_b, lu, vectors))
    legs = {f"colour {leg}": (lambda shape=shape: colour(of, shape)) for leg, shape in SHAPES.items()}
    legs["order"] = sort
    legs.update({f"permute {leg}": (lambda shape=shape: permute((b_ptr, b_cols, b_vals), shape)) for leg, shape in SHAPES.items()})
    for which, side in sides.items():                                        # the solve of a side follows its own factor
        legs[f"ilu0 {which}"] = side.factor
        legs[f"trsv L+U {which}"] = side.apply
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    shipped_shape = capi.csr_colour_default_shape(n, nnz)
    entry = dict(matrix=name, rows=n, entries=nnz, mean_row_length=round(nnz / n, 2), colours=colours_found, rounds=rounds_taken,
                 levels=dict(natural=dict(lower=sides["A"].levels.value, upper=sides["A"].u_levels.value),
                             multicolour=dict(lower=sides["B"].levels.value, upper=sides["B"].u_levels.value)),
                 work_bytes=dict(colour=int(work.numel()), permute=int(permute_work.numel())), every_leg_gives_the_same_bytes=same,
                 legs={leg: summary(s) for leg, s in times.items()})
    below_thread = [leg for leg in SHAPES if leg != FALLBACK and
                    entry["legs"][f"permute {leg}"]["ms_max"] < entry["legs"][f"permute {FALLBACK}"]["ms_min"]]
    entry.update(chosen_by_the_rule=dict(colour=chosen_by_the_rule(entry["legs"], "colour"), permute=chosen_by_the_rule(entry["legs"], "permute")),
                 permute_groups_below_thread=below_thread, shipped=dict(colour=[k for k, v in SHAPES.items() if v == shipped_shape][0]))
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube7", type=int, default=200)
    ap.add_argument("--cube27", type=int, default=100)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_colour_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_colour.py measures on a GPU; none found")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    handle = capi.create_handle(0)
    shapes = dict(a=(f"7-point, {args.cube7}^3", lambda: grid_pattern(args.cube7, 3, False)),
                  b=(f"27-point, {args.cube27}^3", lambda: grid_pattern(args.cube27, 3, True)))
    results = []
    for which in args.cases.split(","):
        name, pattern = shapes[which]
        n, rows, cols = pattern()
        mat = csr_of(n, rows, cols, gen)
        del rows, cols
        results.append(dict(case=which, **measure(handle, name, n, mat, args.reps, args.warmup)))
        del mat
        torch.cuda.empty_cache()
    rule = dict(rule="on a and on b the public colouring runs the shape that measured fastest; a shape counts as fastest only when its "
                     "min-max range lies below that of every other shape; otherwise thread, the fallback, runs; the permutation's one "
                     "shape (csrc/colour_rules.h) leaves thread only for a group whose range lies below thread's on a and on b",
                cases={e["case"]: dict(chosen_by_the_rule=e["chosen_by_the_rule"], shipped=e["shipped"]) for e in results},
                permute_groups_below_thread_on_every_case=sorted(set.intersection(*(set(e["permute_groups_below_thread"]) for e in results)))
                if results else None,
                holds=all(e["chosen_by_the_rule"]["colour"] == e["shipped"]["colour"] for e in results) if results else None)
    out = dict(tool="tools/bench_colour.py", device=torch.cuda.get_device_name(0), type="fp64", reps=args.reps, warmup=args.warmup,
               clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run", rule=rule,
               orderings=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
