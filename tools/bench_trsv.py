#!/usr/bin/env python3
"""GPU box: the sparse triangular solve on CSR arrays (include/spgpu/ext/trsv_device.h), fp64, in one process, the lower solve
x = (D + L)^-1 b of three whole matrices with random, diagonally dominant coefficients:

  a  the 7-point matrix on a --cube^3 grid        (3 * (cube - 1) + 1 levels, the widest of about 3/4 cube^2 rows)
  b  the 5-point matrix on a --square^2 grid      (2 * (square - 1) + 1 levels of at most `square` rows)
  c  a bidiagonal matrix of --chain rows          (as many levels as rows, one row each)

Per case:
  plan      spgpuCsrTrsvPlanDevice (synchronises once per sweep of its analysis)
  plain     spgpuCsrTrsvDevice through the plain solve: one launch per level
  chained   the same through the chained solve: a run of levels of at most TRSV_CHAIN_WIDTH rows is one launch of one workgroup;
            the two results are compared byte for byte
and the launches each solve makes, counted from levelPtrHost by the rule of spgpu_amd/csrc/trsv_rules.h.

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  THE RULE: the public call runs the chained solve if it is faster
on case a with non-overlapping min-max ranges of the two legs, the plain one otherwise.  tools/vendor_context.py reaches rocSPARSE's
csrmv and ellmv but no csrsv, so none is recorded beside.

usage: bench_trsv.py [--cube 200] [--square 1024] [--chain 100000] [--cases a,b,c] [--reps 5] [--warmup 1]
                     [--out profiles/csr_trsv_ab.json]"""
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
import torch  # noqa: E402
from spgpu_amd import capi  # noqa: E402

DEV = "cuda:0"


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
    return ptr.int(), cols.int(), vals.contiguous(), int((cols < rows).sum())


def grid_pattern(side, dims):
    n = side ** dims
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    rows, cols = [at], [at]
    for d in range(dims):
        coordinate = (at // side ** d) % side
        for step in (-1, 1):
            inside = (coordinate + step >= 0) & (coordinate + step < side)
            rows.append(at[inside])
            cols.append(at[inside] + step * side ** d)
    return n, torch.cat(rows), torch.cat(cols)


def chain_pattern(n):
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    return n, torch.cat([at, at[1:]]), torch.cat([at, at[1:] - 1])


def launches(level_ptr, chained):
    """The rule of trsv_rules.h, restated: the number of launches of one solve."""
    narrow = np.diff(level_ptr) <= capi.TRSV_CHAIN_WIDTH
    if not chained:
        return int(narrow.size)
    starts_a_run = narrow & ~np.concatenate(([False], narrow[:-1]))
    return int((~narrow).sum() + starts_a_run.sum())


def summary(samples):
    return dict(ms=round(statistics.median(samples), 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3))


def measure(handle, name, n, mat, gen, reps, warmup):
    ptr, cols, vals, below = mat
    nnz = int(cols.numel())
    levels = C.c_int(0)
    work = torch.empty(capi.spgpuCsrTrsvWorkBytes(n), dtype=torch.uint8, device=DEV)
    order = torch.empty(n, dtype=torch.int32, device=DEV)
    level_ptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    host = np.zeros(n + 1, np.int32)
    at = host.ctypes.data_as(C.POINTER(C.c_int))
    b = torch.randn(n, dtype=torch.float64, device=DEV, generator=gen)
    x = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(2)]

    def plan():
        ok(capi.spgpuCsrTrsvPlanDevice(handle, C.byref(levels), p(order), p(level_ptr), at, n, p(ptr), p(cols), 0, capi.TRSV_LOWER,
                                       capi.TRSV_DIAG_STORED, p(work)))

    def solve(which, k):
        ok(capi.spgpuCsrTrsvDeviceWith(handle, p(x[k]), p(b), n, levels.value, p(order), p(level_ptr), at, p(ptr), p(cols), p(vals), 0,
                                       capi.TRSV_LOWER, capi.TRSV_DIAG_STORED, capi.TYPE_DOUBLE, which, 0))

    legs = dict(plan=plan, plain=lambda: solve(capi.TRSV_SOLVE_PLAIN, 0), chained=lambda: solve(capi.TRSV_SOLVE_CHAINED, 1))
    times = {leg: [] for leg in legs}
    same = True
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
        same = same and bool(torch.equal(x[0].view(torch.int64), x[1].view(torch.int64)))
    widths = np.diff(host[:levels.value + 1])
    # every index array and b read once, the triangle's coefficients and the x they meet read once, x written once
    nbytes = 4 * (n + 1) + 4 * n + 4 * nnz + 8 * (below + n) + 8 * below + 8 * n + 8 * n
    entry = dict(matrix=name, rows=n, entries=nnz, entries_below_the_diagonal=below, levels=levels.value, widest_level=int(widths.max()),
                 levels_of_at_most_the_chain_width=int((widths <= capi.TRSV_CHAIN_WIDTH).sum()), work_bytes=int(work.numel()),
                 launches=dict(plain=launches(host[:levels.value + 1], False), chained=launches(host[:levels.value + 1], True)),
                 the_two_solves_give_the_same_bytes=same, algorithmic_bytes=nbytes, legs={leg: summary(s) for leg, s in times.items()})
    entry["chained_over_plain"] = round(entry["legs"]["chained"]["ms"] / entry["legs"]["plain"]["ms"], 3)
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube", type=int, default=200)
    ap.add_argument("--square", type=int, default=1024)
    ap.add_argument("--chain", type=int, default=100000)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_trsv_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trsv.py measures on a GPU; none found")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    handle = capi.create_handle(0)
    shapes = dict(a=(f"7-point, {args.cube}^3", lambda: grid_pattern(args.cube, 3)), b=(f"5-point, {args.square}^2", lambda: grid_pattern(args.square, 2)),
                  c=(f"bidiagonal, {args.chain} rows", lambda: chain_pattern(args.chain)))
    results = []
    for which in args.cases.split(","):
        name, pattern = shapes[which]
        n, rows, cols = pattern()
        mat = csr_of(n, rows, cols, gen)
        del rows, cols
        results.append(dict(case=which, **measure(handle, name, n, mat, gen, args.reps, args.warmup)))
        del mat
        torch.cuda.empty_cache()
    shipped = {capi.TRSV_SOLVE_PLAIN: "plain", capi.TRSV_SOLVE_CHAINED: "chained"}[capi.TRSV_SOLVE_DEFAULT]
    rule = dict(rule="the public call runs the chained solve if it is faster on case a with non-overlapping min-max ranges of the two legs, the "
                     "plain one otherwise", shipped=shipped)
    first = [e for e in results if e["case"] == "a"]
    if first:
        c, q = first[0]["legs"]["chained"], first[0]["legs"]["plain"]
        chosen = "chained" if c["ms_max"] < q["ms_min"] else "plain"
        rule.update(chained=c, plain=q, ranges_overlap=not (c["ms_max"] < q["ms_min"] or q["ms_max"] < c["ms_min"]), chosen_by_the_rule=chosen,
                    holds=shipped == chosen)
    out = dict(tool="tools/bench_trsv.py", device=torch.cuda.get_device_name(0), type="fp64", reps=args.reps, warmup=args.warmup,
               chain_width=capi.TRSV_CHAIN_WIDTH, clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run",
               vendor="tools/vendor_context.py reaches no rocSPARSE csrsv: none recorded", rule=rule, solves=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
