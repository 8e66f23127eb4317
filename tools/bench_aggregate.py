#!/usr/bin/env python3
"""GPU box: the aggregation on CSR arrays (include/spgpu/ext/aggregate_device.h), fp64, in one process, on two whole matrices with
random, diagonally dominant coefficients:

  a  the 7-point matrix on a --cube7^3 grid       (6.9 stored entries per row)
  b  the 27-point matrix on a --cube27^3 grid     (26.2 stored entries per row)

Per case:
  strength <shape>   spgpuCsrStrengthDevice at theta = 0.25 through one row shape -- thread (one thread per row), group8, group32,
                     group64 (that many lanes of one wavefront per row)
  aggregate <shape>  spgpuCsrAggregateDevice on the strength mask through the same shapes: every round's two max-propagation sweeps
                     run in the shape; the scan, the joining passes and the sizes do not depend on it
and the rounds, the aggregates and the mean aggregate size.  Every leg's outputs are compared byte for byte with the first one's
before anything is timed.

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  THE RULE: on a and on b the public aggregation runs the shape that
measured fastest; a shape counts as fastest only when its min-max range lies below that of every other shape; otherwise thread runs.

usage: bench_aggregate.py [--cube7 200] [--cube27 100] [--cases a,b] [--reps 5] [--warmup 1] [--out profiles/csr_aggregate_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from spgpu_amd import capi  # noqa: E402
from bench_ilu0 import csr_of, grid_pattern  # noqa: E402  (the same matrices)

DEV = "cuda:0"
SHAPES = {"thread": capi.AGG_SHAPE_THREAD, "group8": 8, "group32": 32, "group64": 64}
FALLBACK = "thread"
THETA = 0.25


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


def measure(handle, name, n, mat, reps, warmup):
    ptr, cols, vals = mat
    nnz = int(cols.numel())
    count, rounds = C.c_int(0), C.c_int(0)
    work = torch.empty(capi.spgpuCsrAggregateWorkBytes(n), dtype=torch.uint8, device=DEV)
    first_strong, strong = (torch.empty(nnz, dtype=torch.uint8, device=DEV) for _ in range(2))
    first_diag, diag = (torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(2))
    first_of, of, sizes = (torch.empty(n, dtype=torch.int32, device=DEV) for _ in range(3))

    def strength(out, out_diag, shape):
        ok(capi.spgpuCsrStrengthDeviceWith(handle, p(out), p(out_diag), n, p(ptr), p(cols), p(vals), 0, THETA, capi.TYPE_DOUBLE, shape, 0))

    def aggregate(out, shape):
        ok(capi.spgpuCsrAggregateDeviceWith(handle, C.byref(count), C.byref(rounds), p(out), p(sizes), n, p(ptr), p(cols), p(first_strong), 0,
                                            p(work), shape, 0))

    strength(first_strong, first_diag, SHAPES[FALLBACK])
    aggregate(first_of, SHAPES[FALLBACK])
    torch.cuda.synchronize()
    aggregates, rounds_taken = count.value, rounds.value
    same = True
    for shape in SHAPES.values():                                            # every leg against the first, before it is timed
        strong.fill_(0xA5)
        diag.fill_(float("nan"))
        of.fill_(-1)
        strength(strong, diag, shape)
        aggregate(of, shape)
        torch.cuda.synchronize()
        same = same and bool(torch.equal(first_strong, strong)) and bool(torch.equal(first_diag.view(torch.int64), diag.view(torch.int64)))
        same = same and bool(torch.equal(first_of, of)) and (count.value, rounds.value) == (aggregates, rounds_taken)
    legs = {f"strength {leg}": (lambda shape=shape: strength(strong, diag, shape)) for leg, shape in SHAPES.items()}
    legs.update({f"aggregate {leg}": (lambda shape=shape: aggregate(of, shape)) for leg, shape in SHAPES.items()})
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    shipped_shape = capi.csr_aggregate_default_shape(n, nnz)
    entry = dict(matrix=name, rows=n, entries=nnz, mean_row_length=round(nnz / n, 2), theta=THETA, strong_entries=int(first_strong.sum()),
                 rounds=rounds_taken, aggregates=aggregates, mean_aggregate_size=round(n / max(aggregates, 1), 2), work_bytes=int(work.numel()),
                 every_leg_gives_the_same_bytes=same, legs={leg: summary(s) for leg, s in times.items()})
    entry.update(chosen_by_the_rule=dict(strength=chosen_by_the_rule(entry["legs"], "strength"),
                                         aggregate=chosen_by_the_rule(entry["legs"], "aggregate")),
                 shipped=dict(strength=FALLBACK, aggregate=[k for k, v in SHAPES.items() if v == shipped_shape][0]))
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cube7", type=int, default=200)
    ap.add_argument("--cube27", type=int, default=100)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_aggregate_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aggregate.py measures on a GPU; none found")
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
    rule = dict(rule="on a and on b the public aggregation runs the shape that measured fastest; a shape counts as fastest only when its "
                     "min-max range lies below that of every other shape; otherwise thread, the fallback, runs",
                cases={e["case"]: dict(chosen_by_the_rule=e["chosen_by_the_rule"], shipped=e["shipped"]) for e in results},
                holds=all(e["chosen_by_the_rule"]["aggregate"] == e["shipped"]["aggregate"] for e in results) if results else None)
    out = dict(tool="tools/bench_aggregate.py", device=torch.cuda.get_device_name(0), type="fp64", reps=args.reps, warmup=args.warmup,
               clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run", rule=rule,
               aggregations=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
