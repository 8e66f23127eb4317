#!/usr/bin/env python3
"""GPU box: a CSR holder's way to a HELL matrix, three routes on the same matrices and the same allocations, in one process:

  coo            today's route: expand csrRowPtr into a row index per nonzero, spgpuCooRowLengthsDevice (a stable sort of all
                 nonzeros), spgpuHellPlanDevice, spgpuCooToHellDevice; with a row order also spgpuOellOrderAlignedDevice,
                 spgpuCooPermuteRowsDevice and the second spgpuCooRowLengthsDevice (include/spgpu/convert_device.h, oell_device.h)
  csr_plain      spgpuCsrRowLengthsDevice, (spgpuOellOrderAlignedDevice,) spgpuHellPlanDevice and the fill of
                 include/spgpu/ext/csr_device.h run as one thread per row
  csr_transpose  the same calls with the fill that transposes through LDS, a wavefront per 32 rows

on  banded     BASELINE.json configs[1]: 10 M rows x 32, banded, fp64
    powerlaw   the north_star matrix (power-law lengths, mean 32, longest 2 048, fp64) as the rows come
    powerlaw_aligned   the same matrix with the aligned order (windows of 2 048, rows longer than 256 set aside)

Per route: the median over --reps repetitions (after --warmup, the routes alternating inside a repetition) of the host clock
around the calls, which end in a device synchronise; of the last call alone (the fill); and the effective GB/s of the whole route
over the ALGORITHMIC bytes -- the CSR arrays read once plus every stored entry written once.  The destination is zeroed by the
caller before every run, outside the clock, for all routes alike.  The three results are compared byte for byte.

usage: bench_convert_csr.py [--rows 10000000] [--reps 7] [--warmup 2] [--out profiles/csr_convert_ab.json]"""
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
from spgpu_amd import capi, synth  # noqa: E402

DEV = "cuda:0"
HACK = 32
WINDOW, LONG_ROWS = 2048, 256


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Matrix:
    """CSR arrays in HBM (row-major generator: they are the COO arrays too) and every scratch and result array the routes need."""

    def __init__(self, handle, lengths, pattern):
        self.h, self.n = handle, int(lengths.size)
        n = self.n
        rows, self.cols, self.vals = synth.ragged_coo_on_device(lengths, n, pattern, 2048, "D", seed=5, device=DEV)
        del rows
        self.nnz = int(self.cols.numel())
        row_ptr = np.zeros(n + 1, np.int64)
        np.cumsum(lengths, out=row_ptr[1:])
        assert row_ptr[-1] == self.nnz < 2 ** 31
        self.row_ptr = torch.from_numpy(row_ptr.astype(np.int32)).to(DEV)
        self.lengths = torch.from_numpy(np.ascontiguousarray(lengths, np.int32)).to(DEV)       # the expansion's repeat counts
        self.arange = torch.arange(n, dtype=torch.int32, device=DEV)
        i32 = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=DEV)
        self.lens, self.sorted, self.r_idx, self.inverse = i32(n), i32(n), i32(n), i32(n)
        self.ho = i32((n + HACK - 1) // HACK)
        self.work = torch.empty(capi.spgpuCooConvertWorkBytes(n, self.nnz), dtype=torch.uint8, device=DEV)
        self.plan_work = torch.empty(capi.spgpuCooConvertWorkBytes(n, 0), dtype=torch.uint8, device=DEV)
        self.order_work = torch.empty(capi.spgpuOellOrderWorkBytes(n), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def slots(self, ordered):
        """Slots of the destination (an untimed run of the CSR route's plan)."""
        longest, height = C.c_int(0), C.c_int(0)
        ok(capi.spgpuCsrRowLengthsDevice(self.h, p(self.lens), C.byref(longest), self.n, p(self.row_ptr), 0))
        dest = self.lens
        if ordered:
            ok(capi.spgpuOellOrderAlignedDevice(self.h, p(self.r_idx), p(self.sorted), p(self.lens), self.n, WINDOW, LONG_ROWS, p(self.order_work)))
            dest = self.sorted
        ok(capi.spgpuHellPlanDevice(self.h, C.byref(height), p(self.ho), HACK, self.n, p(dest), p(self.plan_work)))
        return HACK * height.value

    def route_coo(self, ordered, out_v, out_i):
        """(ms of the whole route, ms of spgpuCooToHellDevice alone)."""
        longest, height = C.c_int(0), C.c_int(0)
        t0 = clock()
        rows = torch.repeat_interleave(self.arange, self.lengths, output_size=self.nnz)     # csrRowPtr expanded: a row index per nonzero
        torch.cuda.synchronize()
        ok(capi.spgpuCooRowLengthsDevice(self.h, p(self.lens), C.byref(longest), self.n, self.nnz, p(rows), 0, p(self.work)))
        if ordered:
            ok(capi.spgpuOellOrderAlignedDevice(self.h, p(self.r_idx), p(self.sorted), p(self.lens), self.n, WINDOW, LONG_ROWS, p(self.order_work)))
            ok(capi.spgpuCooPermuteRowsDevice(self.h, p(rows), p(rows), self.nnz, p(self.r_idx), self.n, 0, p(self.inverse)))
            ok(capi.spgpuCooRowLengthsDevice(self.h, p(self.lens), C.byref(longest), self.n, self.nnz, p(rows), 0, p(self.work)))
        ok(capi.spgpuHellPlanDevice(self.h, C.byref(height), p(self.ho), HACK, self.n, p(self.lens), p(self.work)))
        assert HACK * height.value <= out_i.numel()
        t1 = clock()
        ok(capi.spgpuCooToHellDevice(self.h, p(out_v), p(out_i), p(self.ho), HACK, 0, self.n, self.nnz, p(rows), p(self.cols), p(self.vals), 0,
                                     capi.TYPE_DOUBLE, p(self.lens), p(self.work)))
        t2 = clock()
        del rows
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    def route_csr(self, fill, ordered, out_v, out_i):
        """(ms of the whole route, ms of the fill alone)."""
        longest, height = C.c_int(0), C.c_int(0)
        t0 = clock()
        ok(capi.spgpuCsrRowLengthsDevice(self.h, p(self.lens), C.byref(longest), self.n, p(self.row_ptr), 0))
        dest, r_idx = self.lens, None
        if ordered:
            ok(capi.spgpuOellOrderAlignedDevice(self.h, p(self.r_idx), p(self.sorted), p(self.lens), self.n, WINDOW, LONG_ROWS, p(self.order_work)))
            dest, r_idx = self.sorted, self.r_idx
        ok(capi.spgpuHellPlanDevice(self.h, C.byref(height), p(self.ho), HACK, self.n, p(dest), p(self.plan_work)))
        assert HACK * height.value <= out_i.numel()
        t1 = clock()
        ok(capi.spgpuCsrToHellDeviceWith(self.h, p(out_v), p(out_i), p(self.ho), HACK, 0, self.n, p(self.row_ptr), p(self.cols), p(self.vals), 0,
                                         capi.TYPE_DOUBLE, p(r_idx), fill, 0))
        t2 = clock()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3


def measure(handle, name, lengths, pattern, ordered, reps, warmup, matrix=None):
    m = matrix or Matrix(handle, lengths, pattern)
    slots = m.slots(ordered)
    out_v, out_i = torch.empty(slots, dtype=torch.float64, device=DEV), torch.empty(slots, dtype=torch.int32, device=DEV)
    ref_v, ref_i = torch.empty_like(out_v), torch.empty_like(out_i)
    routes = {"coo": lambda v, i: m.route_coo(ordered, v, i),
              "csr_plain": lambda v, i: m.route_csr(capi.CSR_FILL_PLAIN, ordered, v, i),
              "csr_transpose": lambda v, i: m.route_csr(capi.CSR_FILL_TRANSPOSE, ordered, v, i)}
    times = {key: [] for key in routes}
    for rep in range(warmup + reps):
        for key, run in routes.items():
            out_v.zero_()
            out_i.zero_()
            whole, last = run(out_v, out_i)
            if rep >= warmup:
                times[key].append((whole, last))
    # the bytes of the three results: the COO route's into the second pair of arrays, each CSR fill into the first
    ref_v.zero_()
    ref_i.zero_()
    routes["coo"](ref_v, ref_i)
    plan = [t.clone() for t in ((m.lens, m.ho) + ((m.r_idx,) if ordered else ()))]
    same = {}
    for key in ("csr_plain", "csr_transpose"):
        out_v.zero_()
        out_i.zero_()
        routes[key](out_v, out_i)
        now = (m.sorted if ordered else m.lens, m.ho) + ((m.r_idx,) if ordered else ())
        same[key] = bool(torch.equal(out_i, ref_i) and torch.equal(out_v.view(torch.int64), ref_v.view(torch.int64))
                         and all(torch.equal(a, b) for a, b in zip(plan, now)))
    algorithmic = (m.n + 1) * 4 + m.nnz * 12 + m.nnz * 12 + (m.n * 4 if ordered else 0)
    entry = dict(matrix=name, rows=m.n, nnz=m.nnz, slots=slots, slots_per_nnz=round(slots / m.nnz, 4), ordered=ordered,
                 algorithmic_bytes=algorithmic, same_bytes_as_coo_route=same, routes={})
    for key, samples in times.items():
        whole = statistics.median(s[0] for s in samples)
        last = statistics.median(s[1] for s in samples)
        entry["routes"][key] = dict(ms=round(whole, 3), ms_min=round(min(s[0] for s in samples), 3), ms_max=round(max(s[0] for s in samples), 3),
                                    fill_ms=round(last, 3), effective_GBps=round(algorithmic / whole * 1e-6, 1),
                                    fill_effective_GBps=round(algorithmic / last * 1e-6, 1))
    print(json.dumps(entry), flush=True)
    del out_v, out_i, ref_v, ref_i
    torch.cuda.empty_cache()
    return entry, m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_convert_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_convert_csr.py measures on a GPU; none found")
    handle = capi.create_handle(0)
    results = []
    entry, m = measure(handle, "banded", np.full(args.rows, 32, np.int32), "band", False, args.reps, args.warmup)
    results.append(entry)
    del m
    torch.cuda.empty_cache()
    lengths = synth.power_law_lengths(args.rows, mean=32.0, max_len=2048, seed=5)
    entry, m = measure(handle, "powerlaw", lengths, "near", False, args.reps, args.warmup)
    results.append(entry)
    entry, m = measure(handle, "powerlaw_aligned", lengths, "near", True, args.reps, args.warmup, matrix=m)
    results.append(entry)
    out = dict(tool="tools/bench_convert_csr.py", device=torch.cuda.get_device_name(0), type="fp64", hack_size=HACK, reps=args.reps,
               warmup=args.warmup, clock="host clock around calls that end in a device synchronise; median",
               algorithmic_bytes="(rows + 1) * 4 + nnz * 12 read, nnz * 12 written (+ rows * 4 of rIdx with an order)",
               chunk_columns=capi.CSR_FILL_CHUNK, default_fill={capi.CSR_FILL_PLAIN: "csr_plain", capi.CSR_FILL_TRANSPOSE: "csr_transpose"}[capi.CSR_FILL_DEFAULT],
               matrices=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    capi.spgpuDestroy(handle)


if __name__ == "__main__":
    main()
