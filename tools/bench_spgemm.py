#!/usr/bin/env python3
"""GPU box: the sparse product on CSR arrays (include/spgpu/ext/spgemm_device.h), fp64, in one process, on two cases built from the
7-point pattern of a cube of about --rows grid points (random coefficients):

  a  square     A * A
  b  galerkin   R = P^T * A and A_c = R * P with P the unit aggregation of 2 x 2 x 2 cells (the side of the cube is made even)

Per product:
  analysis        spgpuCsrSpgemmProductsDevice + spgpuCsrSpgemmPlanDevice (both synchronise)
  values_staged   spgpuCsrSpgemmValuesDevice through the staged fill (a wavefront per row of C, the row's accumulators in LDS)
  values_plain    the same through the plain fill, one thread per entry of C; the two results are compared byte for byte

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  THE RULE: the public calls run the fill that is faster on case
a if the min-max ranges of the two legs do not overlap, the plain one otherwise.  tools/vendor_context.py offers no rocSPARSE SpGEMM,
so none is recorded beside.

usage: bench_spgemm.py [--rows 8000000] [--cases a,b] [--reps 5] [--warmup 1] [--out profiles/spgemm_ab.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

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


def csr_of(n_rows, rows, cols, gen):
    """0-based COO (int64, on the device) -> (ptr, cols, vals) int32 / fp64 with ascending columns in every row."""
    order = torch.argsort(rows * (int(cols.max()) + 1) + cols)
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    vals = torch.randn(rows.numel(), dtype=torch.float64, device=DEV, generator=gen)
    return ptr.int(), cols[order].int(), vals


def stencil(side, gen):
    n = side ** 3
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    x, y, z = at % side, (at // side) % side, at // (side * side)
    rows, cols = [], []
    for dx, dy, dz in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        inside = (x + dx >= 0) & (x + dx < side) & (y + dy >= 0) & (y + dy < side) & (z + dz >= 0) & (z + dz < side)
        rows.append(at[inside])
        cols.append(at[inside] + dx + dy * side + dz * side * side)
    return n, csr_of(n, torch.cat(rows), torch.cat(cols), gen)


def aggregation(side, gen):
    """P (side^3 x (side/2)^3, one unit entry per row) and P^T, both CSR."""
    n, half = side ** 3, side // 2
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    x, y, z = at % side, (at // side) % side, at // (side * side)
    agg = (z // 2) * half * half + (y // 2) * half + x // 2
    P = csr_of(n, at, agg, gen)
    PT = csr_of(half ** 3, agg, at, gen)
    ones = lambda m: (m[0], m[1], torch.ones_like(m[2]))
    return half ** 3, ones(P), ones(PT)


def median_of(samples):
    return dict(ms=round(statistics.median(samples), 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3))


def measure(handle, name, a, b, a_rows, a_cols, b_cols, reps, warmup):
    """One product C = A * B: the entry of the report and C as a CSR tuple."""
    products, entries = C.c_int(0), C.c_int(0)
    small = torch.empty(capi.spgpuCsrSpgemmWorkBytes(a_rows, b_cols, 0), dtype=torch.uint8, device=DEV)
    ok(capi.spgpuCsrSpgemmProductsDevice(handle, C.byref(products), a_rows, a_cols, p(a[0]), p(a[1]), p(b[0]), 0, p(small)))
    work_bytes = capi.spgpuCsrSpgemmWorkBytes(a_rows, b_cols, products.value)
    work = torch.empty(work_bytes, dtype=torch.uint8, device=DEV)
    c_ptr = torch.empty(a_rows + 1, dtype=torch.int32, device=DEV)

    def analysis():
        ok(capi.spgpuCsrSpgemmProductsDevice(handle, C.byref(products), a_rows, a_cols, p(a[0]), p(a[1]), p(b[0]), 0, p(small)))
        ok(capi.spgpuCsrSpgemmPlanDevice(handle, C.byref(entries), p(c_ptr), a_rows, a_cols, b_cols, p(a[0]), p(a[1]), p(b[0]), p(b[1]), 0,
                                         products.value, p(work)))

    analysis()
    n = entries.value
    c_cols = torch.empty(max(n, 1), dtype=torch.int32, device=DEV)
    c_vals, other = (torch.empty(max(n, 1), dtype=torch.float64, device=DEV) for _ in range(2))
    ok(capi.spgpuCsrSpgemmDevice(handle, p(c_cols), p(c_vals), n, a_rows, p(a[0]), p(a[1]), p(a[2]), p(b[0]), p(b[1]), p(b[2]), p(c_ptr), 0,
                                 capi.TYPE_DOUBLE, p(work)))

    def values(fill, out):
        ok(capi.spgpuCsrSpgemmValuesDeviceWith(handle, p(out), a_rows, p(a[0]), p(a[1]), p(a[2]), p(b[0]), p(b[1]), p(b[2]), p(c_ptr), p(c_cols), 0,
                                               capi.TYPE_DOUBLE, fill, 0))

    legs = dict(analysis=analysis, values_staged=lambda: values(capi.SPGEMM_FILL_STAGED, c_vals),
                values_plain=lambda: values(capi.SPGEMM_FILL_PLAIN, other))
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    same = bool(torch.equal(c_vals.view(torch.int64), other.view(torch.int64)))
    entry = dict(product=name, a_rows=a_rows, a_columns=a_cols, b_columns=b_cols, a_entries=int(a[1].numel()), b_entries=int(b[1].numel()),
                 products=products.value, c_entries=n, products_per_entry=round(products.value / max(n, 1), 3), work_bytes=work_bytes,
                 the_two_fills_give_the_same_bytes=same, legs={leg: median_of(s) for leg, s in times.items()})
    entry["staged_over_plain"] = round(entry["legs"]["values_staged"]["ms"] / entry["legs"]["values_plain"]["ms"], 3)
    print(json.dumps(entry), flush=True)
    del work, small, other
    return entry, (c_ptr, c_cols, c_vals)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_spgemm.py measures on a GPU; none found")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    handle = capi.create_handle(0)
    side = max(2, round(args.rows ** (1.0 / 3.0)) // 2 * 2)
    n, A = stencil(side, gen)
    results = []
    for which in args.cases.split(","):
        if which == "a":
            entry, C_ = measure(handle, "A * A", A, A, n, n, n, args.reps, args.warmup)
            results.append(dict(case="square", **entry))
            del C_
        else:
            coarse, P, PT = aggregation(side, gen)
            entry, R = measure(handle, "R = P^T * A", PT, A, coarse, n, n, args.reps, args.warmup)
            results.append(dict(case="galerkin", **entry))
            entry, Ac = measure(handle, "A_c = R * P", R, P, coarse, n, coarse, args.reps, args.warmup)
            results.append(dict(case="galerkin", **entry))
            del R, Ac, P, PT
        torch.cuda.empty_cache()
    shipped = {capi.SPGEMM_FILL_PLAIN: "plain", capi.SPGEMM_FILL_STAGED: "staged"}[capi.SPGEMM_FILL_DEFAULT]
    rule = dict(rule="the public calls run the fill that is faster on A * A if the min-max ranges of the two legs do not overlap, the plain one "
                     "otherwise", shipped=shipped)
    square = [e for e in results if e["case"] == "square"]
    if square:
        s, q = square[0]["legs"]["values_staged"], square[0]["legs"]["values_plain"]
        faster = "staged" if s["ms_max"] < q["ms_min"] else "plain"
        rule.update(staged=s, plain=q, ranges_overlap=not (s["ms_max"] < q["ms_min"] or q["ms_max"] < s["ms_min"]), chosen_by_the_rule=faster,
                    holds=shipped == faster)
    out = dict(tool="tools/bench_spgemm.py", device=torch.cuda.get_device_name(0), type="fp64", side=side, rows=n, reps=args.reps,
               warmup=args.warmup, row_cap=capi.SPGEMM_ROW_CAP,
               clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run", rule=rule, products=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
