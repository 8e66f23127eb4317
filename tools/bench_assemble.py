#!/usr/bin/env python3
"""GPU box: assembly of a COO list with duplicates (include/spgpu/ext/assemble_device.h), fp64, in one process and on one set of
allocations, on two lists:

  a  stencil   the element-by-element listing of a 3-D 7-point pattern on a cube of about --rows grid points: every matrix entry
               (a point and itself or one of its six neighbours) is listed 5 or 6 times, as the tetrahedra around an edge list it;
               shuffled
  b  once      --rows x 32 banded (BASELINE.json configs[1], 320 M nonzeros at 10 M rows), every entry listed once; shuffled

Per list:
  plan            spgpuCooAssemblePlanDevice, beside the existing COO route on the same list, which also sorts once:
  coo_route       spgpuCooRowLengthsDevice + spgpuHellPlanDevice + spgpuCooToHellDevice (every duplicate becomes a slot)
  values_staged   spgpuCooAssembleValuesDevice through the staged fill (a workgroup per 256 entries, the gathers landed in LDS)
  values_plain    the same through the plain fill, one thread per matrix entry; the two results are compared byte for byte
  spmv_assembled  (list a) one spgpuDhellspmv on the assembled matrix (spgpuCsrToHellDevice of the assembled CSR)
  spmv_kept       (list a) one spgpuDhellspmv on the spgpuCooToHellDevice matrix of the same list: what assembly saves per multiply

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around the
call, which ends in a device synchronise.  The values legs are also given as bytes per second of their algorithmic traffic,
4 nnz + 4 unique + 8 nnz + 8 unique.  THE RULE: the fill the public calls run is the one that is faster on list a.

usage: bench_assemble.py [--rows 10000000] [--lists a,b] [--reps 5] [--warmup 1] [--out profiles/assemble_ab.json]"""
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
HACK = 32


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def stencil_list(rows):
    """(n, n, coo rows, coo cols) of list a, shuffled, int32 on the device."""
    side = max(2, round(rows ** (1.0 / 3.0)))
    n = side ** 3
    at = torch.arange(n, dtype=torch.int64, device=DEV)
    x, y, z = at % side, (at // side) % side, at // (side * side)
    pairs = []
    for k, (dx, dy, dz) in enumerate(((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))):
        inside = (x + dx >= 0) & (x + dx < side) & (y + dy >= 0) & (y + dy < side) & (z + dz >= 0) & (z + dz < side)
        r = at[inside]
        pairs.append((r, r + dx + dy * side + dz * side * side, 5 + (r + k) % 2))
    r = torch.cat([q[0] for q in pairs])
    c = torch.cat([q[1] for q in pairs])
    times = torch.cat([q[2] for q in pairs])
    del pairs, x, y, z, at
    r, c = torch.repeat_interleave(r, times), torch.repeat_interleave(c, times)
    del times
    order = torch.randperm(r.numel(), device=DEV)
    return n, n, r[order].int(), c[order].int()


def once_list(rows):
    """(n, columns, coo rows, coo cols) of list b, shuffled, int32 on the device."""
    width = 32
    r = torch.repeat_interleave(torch.arange(rows, dtype=torch.int64, device=DEV), width)
    c = r + torch.arange(width, dtype=torch.int64, device=DEV).repeat(rows)
    order = torch.randperm(r.numel(), device=DEV)
    return rows, rows + width, r[order].int(), c[order].int()


def median_of(samples):
    return dict(ms=round(statistics.median(samples), 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3))


def measure(handle, name, n, n_cols, coo_r, coo_c, with_spmv, reps, warmup):
    nnz = int(coo_r.numel())
    assert nnz < 2 ** 31
    i32 = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    coo_v = torch.randn(nnz, dtype=torch.float64, device=DEV, generator=gen)
    row_ptr, perm, seg_ptr = i32(n + 1), i32(nnz), i32(nnz + 1)
    work = torch.empty(capi.spgpuCooAssembleWorkBytes(n, n_cols, nnz), dtype=torch.uint8, device=DEV)
    coo_work = torch.empty(capi.spgpuCooConvertWorkBytes(n, nnz), dtype=torch.uint8, device=DEV)
    plan_work = torch.empty(capi.spgpuCooConvertWorkBytes(n, 0), dtype=torch.uint8, device=DEV)
    unique, longest, height = C.c_int(0), C.c_int(0), C.c_int(0)
    # the duplicate-keeping matrix: sized once, untimed
    kept_rs, kept_ho = i32(n), i32((n + HACK - 1) // HACK)
    ok(capi.spgpuCooRowLengthsDevice(handle, p(kept_rs), C.byref(longest), n, nnz, p(coo_r), 0, p(coo_work)))
    ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(kept_ho), HACK, n, p(kept_rs), p(coo_work)))
    kept_slots = HACK * height.value
    kept_cm = torch.zeros(kept_slots, dtype=torch.float64, device=DEV)
    kept_rp = torch.zeros(kept_slots, dtype=torch.int32, device=DEV)

    def plan():
        ok(capi.spgpuCooAssemblePlanDevice(handle, C.byref(unique), p(row_ptr), p(perm), p(seg_ptr), n, n_cols, nnz, p(coo_r), p(coo_c), 0, 0,
                                           p(work)))

    def coo_route():
        ok(capi.spgpuCooRowLengthsDevice(handle, p(kept_rs), C.byref(longest), n, nnz, p(coo_r), 0, p(coo_work)))
        ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(kept_ho), HACK, n, p(kept_rs), p(coo_work)))
        ok(capi.spgpuCooToHellDevice(handle, p(kept_cm), p(kept_rp), p(kept_ho), HACK, 0, n, nnz, p(coo_r), p(coo_c), p(coo_v), 0,
                                     capi.TYPE_DOUBLE, p(kept_rs), p(coo_work)))

    plan()
    entries = unique.value
    csr_cols, csr_vals, other = i32(entries), torch.empty(entries, dtype=torch.float64, device=DEV), torch.empty(entries, dtype=torch.float64, device=DEV)
    ok(capi.spgpuCooAssembleDevice(handle, p(csr_cols), p(csr_vals), entries, nnz, p(coo_c), p(coo_v), 0, 0, capi.TYPE_DOUBLE, p(perm), p(seg_ptr)))

    def values(fill, out):
        ok(capi.spgpuCooAssembleValuesDeviceWith(handle, p(out), entries, nnz, p(coo_v), capi.TYPE_DOUBLE, p(perm), p(seg_ptr), fill, 0))

    legs = dict(plan=plan, coo_route=coo_route, values_staged=lambda: values(capi.ASSEMBLE_FILL_STAGED, csr_vals),
                values_plain=lambda: values(capi.ASSEMBLE_FILL_PLAIN, other))
    if with_spmv:
        rs, ho = i32(n), i32((n + HACK - 1) // HACK)
        ok(capi.spgpuCsrRowLengthsDevice(handle, p(rs), C.byref(longest), n, p(row_ptr), 0))
        ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(ho), HACK, n, p(rs), p(plan_work)))
        slots = HACK * height.value
        cm, rp = torch.zeros(slots, dtype=torch.float64, device=DEV), torch.zeros(slots, dtype=torch.int32, device=DEV)
        ok(capi.spgpuCsrToHellDevice(handle, p(cm), p(rp), p(ho), HACK, 0, n, p(row_ptr), p(csr_cols), p(csr_vals), 0, capi.TYPE_DOUBLE, None))
        coo_route()
        x = torch.randn(n_cols, dtype=torch.float64, device=DEV, generator=gen)
        z_a, z_k = torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)

        def spmv(z, values_, indices, offsets, lengths):
            capi.hellspmv["D"](handle, p(z), p(z), capi.scalar("D", 1.0), p(values_), p(indices), HACK, p(offsets), p(lengths), None, 0, n, p(x),
                               capi.scalar("D", 0.0), 0)

        legs["spmv_assembled"] = lambda: spmv(z_a, cm, rp, ho, rs)
        legs["spmv_kept"] = lambda: spmv(z_k, kept_cm, kept_rp, kept_ho, kept_rs)
    times = {leg: [] for leg in legs}
    for rep in range(warmup + reps):
        for leg, run in legs.items():
            t0 = clock()
            run()
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
    same = bool(torch.equal(csr_vals.view(torch.int64), other.view(torch.int64)))
    entry = dict(list=name, rows=n, columns=n_cols, contributions=nnz, entries=entries, contributions_per_entry=round(nnz / entries, 3),
                 the_two_fills_give_the_same_bytes=same, kept_slots=kept_slots, legs={leg: median_of(s) for leg, s in times.items()})
    traffic = 12 * nnz + 12 * entries
    for leg in ("values_staged", "values_plain"):
        entry["legs"][leg]["algorithmic_bytes"] = traffic
        entry["legs"][leg]["effective_GBps"] = round(traffic / entry["legs"][leg]["ms"] * 1e-6, 1)
    entry["plan_over_coo_route"] = round(entry["legs"]["plan"]["ms"] / entry["legs"]["coo_route"]["ms"], 3)
    entry["staged_over_plain"] = round(entry["legs"]["values_staged"]["ms"] / entry["legs"]["values_plain"]["ms"], 3)
    if with_spmv:
        entry["assembled_slots"] = slots
        entry["spmv_assembled_over_kept"] = round(entry["legs"]["spmv_assembled"]["ms"] / entry["legs"]["spmv_kept"]["ms"], 3)
        # the products agree to rounding: the kept matrix adds the contributions inside the row sum
        entry["spmv_max_difference"] = float((z_a - z_k).abs().max())
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--lists", default="a,b")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_assemble.py measures on a GPU; none found")
    torch.manual_seed(5)
    handle = capi.create_handle(0)
    results = []
    for which in args.lists.split(","):
        name, (n, n_cols, r, c) = ("stencil", stencil_list(args.rows)) if which == "a" else ("once", once_list(args.rows))
        results.append(measure(handle, name, n, n_cols, r, c, which == "a", args.reps, args.warmup))
        del r, c
        torch.cuda.empty_cache()
    shipped = {capi.ASSEMBLE_FILL_PLAIN: "plain", capi.ASSEMBLE_FILL_STAGED: "staged"}[capi.ASSEMBLE_FILL_DEFAULT]
    rule = dict(rule="the public calls run the fill that is faster on the stencil list, same arrays, same process", shipped=shipped)
    stencil = [e for e in results if e["list"] == "stencil"]
    if stencil:
        ratio = stencil[0]["staged_over_plain"]
        rule.update(staged_over_plain=ratio, faster="staged" if ratio < 1 else "plain", holds=(shipped == "staged") == (ratio < 1))
    out = dict(tool="tools/bench_assemble.py", device=torch.cuda.get_device_name(0), type="fp64", hack_size=HACK, rows=args.rows, reps=args.reps,
               warmup=args.warmup, tile=capi.ASSEMBLE_TILE, chunk=capi.ASSEMBLE_CHUNK,
               clock="host clock around a call that ends in a device synchronise; median, legs alternating; one run",
               algorithmic_bytes="values legs: 4 nnz of perm + 4 unique of segPtr + 8 nnz gathered + 8 unique written", rule=rule, lists=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(rule), flush=True)
    capi.spgpuDestroy(handle)
    return 0 if rule.get("holds", True) else 1


if __name__ == "__main__":
    sys.exit(main())
