#!/usr/bin/env python3
"""GPU box: the ILU(0) factorisation on CSR arrays (include/spgpu/ext/ilu0_device.h), fp64, in one process, on four whole matrices
with random, diagonally dominant coefficients:

  a  the 7-point matrix on a --cube7^3 grid       (3 * (cube - 1) + 1 levels, 6.9 stored entries per row)
  b  the 27-point matrix on a --cube27^3 grid     (about 7 * (cube - 1) + 1 levels, 26.2 stored entries per row)
  c  the 5-point matrix on a --square^2 grid      (2 * (square - 1) + 1 levels of at most `square` rows)
  d  a bidiagonal matrix of --chain rows          (as many levels as rows, one row each; nothing to update)

Per case:
  plan             spgpuCsrIlu0PlanDevice (its own check, then the Plan of the lower triangular solve: about one synchronise per level)
  <shape> plain    spgpuCsrIlu0Device through one row shape -- thread (one thread per row), group8, group32 (that many lanes of one
  <shape> chained  wavefront per row: the widths the rule of spgpu_amd/csrc/ilu0_rules.h can choose) -- with one launch per level, or
                   with every run of levels of at most ILU0_CHAIN_WIDTH rows chained in one launch of one workgroup
  trsv L+U         for context only, no pass mark: one application of the factor, the unit lower and the upper solve of
                   spgpuCsrTrsvDevice on the same arrays
Every forced leg's lu is compared byte for byte with the first one's before anything is timed.

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  THE RULE: on a and on b the public call runs the leg that measured
fastest; a leg counts as fastest only when its min-max range lies below that of every other leg; otherwise thread / plain runs.
tools/vendor_context.py reaches rocSPARSE's csrmv and ellmv but no csrilu0, so none is recorded beside.

usage: bench_ilu0.py [--cube7 200] [--cube27 100] [--square 1024] [--chain 100000] [--cases a,b,c,d] [--reps 5] [--warmup 1]
                     [--out profiles/csr_ilu0_ab.json]"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from spgpu_amd import capi  # noqa: E402

DEV = "cuda:0"
SOLVES = {"plain": capi.TRSV_SOLVE_PLAIN, "chained": capi.TRSV_SOLVE_CHAINED}
SHAPES = {"thread": capi.ILU0_SHAPE_THREAD, f"group{capi.ILU0_GROUP_NARROW}": capi.ILU0_GROUP_NARROW,
          f"group{capi.ILU0_GROUP_WIDE}": capi.ILU0_GROUP_WIDE}
FALLBACK = "thread plain"


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def csr_of(n, rows, cols, gen):
    """0-based COO pattern (int64, on the device) -> (ptr, cols, vals): ascending columns, off-diagonals of magnitude about
    1 / (2 * row length), diagonals in [1, 2)."""
    order = torch.argsort(rows * n + cols)
    rows, cols = rows[order], cols[order]
    lengths = torch.bincount(rows, minlength=n)
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    ptr[1:] = torch.cumsum(lengths, 0)
    vals = torch.randn(rows.numel(), dtype=torch.float64, device=DEV, generator=gen) * 0.5 / lengths[rows].double()
    on_diagonal = rows == cols
    vals[on_diagonal] = 1.0 + torch.rand(int(on_diagonal.sum()), dtype=torch.float64, device=DEV, generator=gen)
    return ptr.int(), cols.int(), vals.contiguous()


def grid_pattern(side, dims, full):
    """The 2 * dims + 1 point stencil, or with `full` the 3^dims point one, on a side^dims grid."""
    n = side ** dims
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    coordinates = [(at // side ** d) % side for d in range(dims)]
    steps = [s for s in itertools.product((-1, 0, 1), repeat=dims) if full or sum(map(abs, s)) <= 1]
    rows, cols = [], []
    for step in steps:
        inside = torch.ones(n, dtype=torch.bool, device=DEV)
        for d in range(dims):
            inside &= (coordinates[d] + step[d] >= 0) & (coordinates[d] + step[d] < side)
        rows.append(at[inside])
        cols.append(at[inside] + sum(step[d] * side ** d for d in range(dims)))
    return n, torch.cat(rows), torch.cat(cols)


def chain_pattern(n):
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    return n, torch.cat([at, at[1:]]), torch.cat([at, at[1:] - 1])


def launches(level_ptr, chained):
    """The rule of trsv_rules.h at the factorisation's width, restated: the number of launches of one factor call."""
    narrow = np.diff(level_ptr) <= capi.ILU0_CHAIN_WIDTH
    if not chained:
        return int(narrow.size)
    starts_a_run = narrow & ~np.concatenate(([False], narrow[:-1]))
    return int((~narrow).sum() + starts_a_run.sum())


def summary(samples):
    return dict(ms=round(statistics.median(samples), 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3))


def chosen_by_the_rule(legs):
    """The fastest leg by its median, if its range lies below the range of EVERY other factor leg; the fallback otherwise."""
    factor = {name: leg for name, leg in legs.items() if name.split()[0] in SHAPES}
    best = min(factor, key=lambda name: factor[name]["ms"])
    clear = all(factor[best]["ms_max"] < leg["ms_min"] for name, leg in factor.items() if name != best)
    return best if clear else FALLBACK


def measure(handle, name, n, mat, reps, warmup):
    ptr, cols, vals = mat
    nnz = int(cols.numel())
    levels, u_levels = C.c_int(0), C.c_int(0)
    work = torch.empty(capi.spgpuCsrIlu0WorkBytes(n), dtype=torch.uint8, device=DEV)
    order, u_order, diag_pos = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))
    level_ptr, u_level_ptr = (torch.empty(n + 1, dtype=torch.int32, device=DEV) for _ in range(2))
    host, u_host = np.zeros(n + 2, np.int32), np.zeros(n + 1, np.int32)
    at, u_at = (h.ctypes.data_as(C.POINTER(C.c_int)) for h in (host, u_host))
    first, lu = (torch.empty(nnz, dtype=torch.float64, device=DEV) for _ in range(2))
    b, y, x = (torch.ones(n, dtype=torch.float64, device=DEV) for _ in range(3))

    def plan():
        ok(capi.spgpuCsrIlu0PlanDevice(handle, C.byref(levels), p(order), p(level_ptr), at, p(diag_pos), n, p(ptr), p(cols), 0, p(work)))

    def factor(out, shape, solve):
        ok(capi.spgpuCsrIlu0DeviceWith(handle, p(out), p(vals), n, levels.value, p(order), p(level_ptr), at, p(diag_pos), p(ptr), p(cols), 0,
                                       capi.TYPE_DOUBLE, shape, solve, 0))

    def apply():
        ok(capi.spgpuCsrTrsvDevice(handle, p(y), p(b), n, levels.value, p(order), p(level_ptr), at, p(ptr), p(cols), p(first), 0, capi.TRSV_LOWER,
                                   capi.TRSV_DIAG_UNIT, capi.TYPE_DOUBLE))
        ok(capi.spgpuCsrTrsvDevice(handle, p(x), p(y), n, u_levels.value, p(u_order), p(u_level_ptr), u_at, p(ptr), p(cols), p(first), 0,
                                   capi.TRSV_UPPER, capi.TRSV_DIAG_STORED, capi.TYPE_DOUBLE))

    plan()
    ok(capi.spgpuCsrTrsvPlanDevice(handle, C.byref(u_levels), p(u_order), p(u_level_ptr), u_at, n, p(ptr), p(cols), 0, capi.TRSV_UPPER,
                                   capi.TRSV_DIAG_STORED, p(work)))
    forced = {f"{shape} {solve}": (SHAPES[shape], SOLVES[solve]) for shape in SHAPES for solve in SOLVES}
    factor(first, *forced[FALLBACK])
    same = True
    for leg, (shape, solve) in forced.items():                               # every forced leg against the first, before it is timed
        lu.fill_(float("nan"))
        factor(lu, shape, solve)
        torch.cuda.synchronize()
        same = same and bool(torch.equal(first.view(torch.int64), lu.view(torch.int64)))
    lu.fill_(float("nan"))
    ok(capi.spgpuCsrIlu0Device(handle, p(lu), p(vals), n, levels.value, p(order), p(level_ptr), at, p(diag_pos), p(ptr), p(cols), 0,
                               capi.TYPE_DOUBLE))
    torch.cuda.synchronize()
    same = same and bool(torch.equal(first.view(torch.int64), lu.view(torch.int64)))
    legs = dict(plan=plan)
    legs.update({leg: (lambda shape=shape, solve=solve: factor(lu, shape, solve)) for leg, (shape, solve) in forced.items()})
    legs["trsv L+U"] = apply
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    widths = np.diff(host[:levels.value + 1])
    shipped_shape = capi.csr_ilu0_default_shape(n, nnz)
    shipped = f"{[k for k, v in SHAPES.items() if v == shipped_shape][0]} {[k for k, v in SOLVES.items() if v == capi.ILU0_SOLVE_DEFAULT][0]}"
    entry = dict(matrix=name, rows=n, entries=nnz, mean_row_length=round(nnz / n, 2), stored_entries_slot=int(host[levels.value + 1]),
                 levels=levels.value, widest_level=int(widths.max()), levels_of_at_most_the_chain_width=int((widths <= capi.ILU0_CHAIN_WIDTH).sum()),
                 work_bytes=int(work.numel()), launches=dict(plain=launches(host[:levels.value + 1], False), chained=launches(host[:levels.value + 1], True)),
                 every_leg_gives_the_same_bytes=same, legs={leg: summary(s) for leg, s in times.items()})
    entry.update(chosen_by_the_rule=chosen_by_the_rule(entry["legs"]), shipped=shipped)
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube7", type=int, default=200)
    ap.add_argument("--cube27", type=int, default=100)
    ap.add_argument("--square", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=100000)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_ilu0_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ilu0.py measures on a GPU; none found")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    handle = capi.create_handle(0)
    shapes = dict(a=(f"7-point, {args.cube7}^3", lambda: grid_pattern(args.cube7, 3, False)),
                  b=(f"27-point, {args.cube27}^3", lambda: grid_pattern(args.cube27, 3, True)),
                  c=(f"5-point, {args.square}^2", lambda: grid_pattern(args.square, 2, False)),
                  d=(f"bidiagonal, {args.chain} rows", lambda: chain_pattern(args.chain)))
    results = []
    for which in args.cases.split(","):
        name, pattern = shapes[which]
        n, rows, cols = pattern()
        mat = csr_of(n, rows, cols, gen)
        del rows, cols
        results.append(dict(case=which, **measure(handle, name, n, mat, args.reps, args.warmup)))
        del mat
        torch.cuda.empty_cache()
    decisive = [e for e in results if e["case"] in ("a", "b")]
    rule = dict(rule="on a and on b the public call runs the leg that measured fastest; a leg counts as fastest only when its min-max range lies "
                     "below that of every other leg; otherwise thread / plain, the fallback, runs",
                cases={e["case"]: dict(chosen_by_the_rule=e["chosen_by_the_rule"], shipped=e["shipped"]) for e in decisive},
                holds=all(e["chosen_by_the_rule"] == e["shipped"] for e in decisive) if decisive else None)
    out = dict(tool="tools/bench_ilu0.py", device=torch.cuda.get_device_name(0), type="fp64", reps=args.reps, warmup=args.warmup,
               chain_width=capi.ILU0_CHAIN_WIDTH, thread_max_mean=capi.ILU0_THREAD_MAX_MEAN, narrow_max_mean=capi.ILU0_NARROW_MAX_MEAN,
               clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run",
               vendor="tools/vendor_context.py reaches no rocSPARSE csrilu0: none recorded", rule=rule, factorisations=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
