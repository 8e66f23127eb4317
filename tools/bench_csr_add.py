#!/usr/bin/env python3
"""GPU box: the sparse sum on CSR arrays (include/spgpu/ext/add_device.h), fp64, in one process, on two cases built on a cube of
about --rows grid points (random coefficients):

  a  timestep    M + dt * K: K on the 7-point pattern, M on the tridiagonal-in-x subset of it
  b  symmetrise  A + A^T of a one-sided (upwind) 4-point stencil -- the diagonal and the neighbours at -x, -y, -z: the two
                 patterns share the diagonal only

Per case:
  plan            spgpuCsrAddPlanDevice (synchronises)
  full_staged     spgpuCsrAddDevice through the staged fill (a workgroup per tile of C, the column slices of its rows in LDS)
  full_plain      the same through the plain fill, one thread per stored entry of A and of B
  values_staged   spgpuCsrAddValuesDevice through the staged fill
  values_plain    the same through the plain fill; the columns and values of the two fills are compared byte for byte

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, ended by a device synchronise; minimum and maximum are kept.  Beside each leg the algorithmic bytes -- every input array read
once, every output array written once -- and the rate they imply at the median.  THE RULE: the public calls run the fill that is
faster on case a (values pass) if the min-max ranges of the two legs do not overlap, the plain one otherwise.
tools/vendor_context.py reaches no rocSPARSE csrgeam, so none is recorded beside.

usage: bench_csr_add.py [--rows 8000000] [--cases a,b] [--reps 5] [--warmup 1] [--out profiles/csr_add_ab.json]"""
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


def csr_of(n_rows, rows, cols, vals):
    """0-based COO (int64 indices, on the device) -> (ptr, cols, vals) int32 / fp64 with ascending columns in every row."""
    order = torch.argsort(rows * n_rows + cols)
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=DEV)
    ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
    return ptr.int(), cols[order].int(), vals[order].contiguous()


def stencil(side, offsets, gen):
    """The COO list of the stencil's entries inside the cube: (rows, cols, vals)."""
    n = side ** 3
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    x, y, z = at % side, (at // side) % side, at // (side * side)
    rows, cols = [], []
    for dx, dy, dz in offsets:
        inside = (x + dx >= 0) & (x + dx < side) & (y + dy >= 0) & (y + dy < side) & (z + dz >= 0) & (z + dz < side)
        rows.append(at[inside])
        cols.append(at[inside] + dx + dy * side + dz * side * side)
    rows, cols = torch.cat(rows), torch.cat(cols)
    return rows, cols, torch.randn(rows.numel(), dtype=torch.float64, device=DEV, generator=gen)


def median_of(samples, nbytes):
    ms = statistics.median(samples)
    return dict(ms=round(ms, 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3), algorithmic_bytes=nbytes,
                gb_per_s=round(nbytes / ms / 1e6, 1))


def measure(handle, name, a, b, n, alpha, beta, reps, warmup):
    """One sum C = alpha * A + beta * B of two n x n matrices: the entry of the report."""
    entries = C.c_int(0)
    work = torch.empty(capi.spgpuCsrAddWorkBytes(n), dtype=torch.uint8, device=DEV)
    c_ptr = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    h_alpha, h_beta = C.c_double(alpha), C.c_double(beta)
    at = lambda s: C.cast(C.pointer(s), C.c_void_p)

    def plan():
        ok(capi.spgpuCsrAddPlanDevice(handle, C.byref(entries), p(c_ptr), n, n, p(a[0]), p(a[1]), p(b[0]), p(b[1]), 0, p(work)))

    plan()
    nnz = entries.value
    cols = [torch.empty(max(nnz, 1), dtype=torch.int32, device=DEV) for _ in range(2)]
    vals = [torch.empty(max(nnz, 1), dtype=torch.float64, device=DEV) for _ in range(2)]
    matrices = (at(h_alpha), p(a[0]), p(a[1]), p(a[2]), at(h_beta), p(b[0]), p(b[1]), p(b[2]), p(c_ptr), 0, capi.TYPE_DOUBLE)

    def full(fill, k):
        ok(capi.spgpuCsrAddDeviceWith(handle, p(cols[k]), p(vals[k]), nnz, n, *matrices, fill, 0))

    def values(fill, k):
        ok(capi.spgpuCsrAddValuesDeviceWith(handle, p(vals[k]), n, *matrices, fill, 0))

    in_a, in_b = int(a[1].numel()), int(b[1].numel())
    pointers = 4 * (n + 1)
    plan_bytes = 3 * pointers + 4 * (in_a + in_b)
    values_bytes = 3 * pointers + 12 * (in_a + in_b) + 8 * nnz
    full_bytes = values_bytes + 4 * nnz
    legs = dict(plan=(plan, plan_bytes),
                full_staged=(lambda: full(capi.ADD_FILL_STAGED, 0), full_bytes), full_plain=(lambda: full(capi.ADD_FILL_PLAIN, 1), full_bytes),
                values_staged=(lambda: values(capi.ADD_FILL_STAGED, 0), values_bytes),
                values_plain=(lambda: values(capi.ADD_FILL_PLAIN, 1), values_bytes))
    times = {leg: [] for leg in legs}
    same = True
    for rep in range(warmup + reps):
        for leg, (run, _) in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
            if leg in ("full_plain", "values_plain"):
                same = same and bool(torch.equal(cols[0], cols[1])) and bool(torch.equal(vals[0].view(torch.int64), vals[1].view(torch.int64)))
    entry = dict(sum=name, rows=n, a_entries=in_a, b_entries=in_b, c_entries=nnz, work_bytes=int(work.numel()),
                 the_two_fills_give_the_same_bytes=same, legs={leg: median_of(s, legs[leg][1]) for leg, s in times.items()})
    for kind in ("full", "values"):
        entry[f"{kind}_staged_over_plain"] = round(entry["legs"][f"{kind}_staged"]["ms"] / entry["legs"][f"{kind}_plain"]["ms"], 3)
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=8_000_000)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_add_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_csr_add.py measures on a GPU; none found")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    handle = capi.create_handle(0)
    side = max(2, round(args.rows ** (1.0 / 3.0)))
    n = side ** 3
    in_x = ((0, 0, 0), (1, 0, 0), (-1, 0, 0))
    results = []
    for which in args.cases.split(","):
        if which == "a":
            K = csr_of(n, *stencil(side, in_x + ((0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)), gen))
            M = csr_of(n, *stencil(side, in_x, gen))
            results.append(dict(case="timestep", **measure(handle, "M + dt * K", M, K, n, 1.0, 0.01, args.reps, args.warmup)))
            del K, M
        else:
            rows, cols, vals = stencil(side, ((0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)), gen)
            A, AT = csr_of(n, rows, cols, vals), csr_of(n, cols, rows, vals)
            del rows, cols, vals
            results.append(dict(case="symmetrise", **measure(handle, "A + A^T", A, AT, n, 1.0, 1.0, args.reps, args.warmup)))
            del A, AT
        torch.cuda.empty_cache()
    shipped = {capi.ADD_FILL_PLAIN: "plain", capi.ADD_FILL_STAGED: "staged"}[capi.ADD_FILL_DEFAULT]
    rule = dict(rule="the public calls run the fill that is faster on M + dt * K (values pass) if the min-max ranges of the two legs do not "
                     "overlap, the plain one otherwise", shipped=shipped)
    first = [e for e in results if e["case"] == "timestep"]
    if first:
        s, q = first[0]["legs"]["values_staged"], first[0]["legs"]["values_plain"]
        faster = "staged" if s["ms_max"] < q["ms_min"] else "plain"
        rule.update(staged=s, plain=q, ranges_overlap=not (s["ms_max"] < q["ms_min"] or q["ms_max"] < s["ms_min"]), chosen_by_the_rule=faster,
                    holds=shipped == faster)
    out = dict(tool="tools/bench_csr_add.py", device=torch.cuda.get_device_name(0), type="fp64", side=side, rows=n, reps=args.reps,
               warmup=args.warmup, tile=capi.ADD_TILE, row_cap=capi.ADD_ROW_CAP,
               clock="host clock around a call, ended by a device synchronise; median, legs alternating; one run",
               vendor="tools/vendor_context.py reaches no rocSPARSE csrgeam: none recorded", rule=rule, sums=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
