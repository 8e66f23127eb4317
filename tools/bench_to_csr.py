#!/usr/bin/env python3
"""GPU box: the way back from a HELL matrix to CSR arrays (include/spgpu/ext/to_csr_device.h), both fills behind the calls on the
same matrices and the same allocations, in one process, beside the opposite conversion as the yardstick:

  to_csr_plain      spgpuHellToCsrRowPtrDevice, then the fill run as one thread per storage row
  to_csr_transpose  the same row-pointer call, then the fill that transposes through LDS, a wavefront per 32 storage rows
  csr_to_hell       spgpuCsrToHellDevice (include/spgpu/ext/csr_device.h) on the same arrays: the same bytes moved the other way

on  banded     BASELINE.json configs[1]: 10 M rows x 32, banded, fp64
    powerlaw   the north_star matrix (power-law lengths, mean 32, longest 2 048, fp64) as the rows come
    powerlaw_aligned   the same matrix stored in the aligned order (windows of 2 048, rows longer than 256 set aside), with rIdx

Per route: the median over --reps repetitions (after --warmup, the routes alternating inside a repetition) of the host clock
around the calls, which end in a device synchronise: row pointers + fill, and the fill alone; and the effective GB/s over the
ALGORITHMIC bytes -- every stored entry read once, the CSR arrays written once.  The CSR arrays each fill gives are compared byte
for byte with the arrays the HELL matrix was built from.

THE DEFAULT FILL follows from the numbers (rule of DESIGN.md 3.13): the fill that is faster on `powerlaw`, provided it is no more
than 10 % slower than the other on `banded`; if neither fill satisfies both, the transposing fill.  The tool writes the choice the
rule gives beside the fill the library was built with.

usage: bench_to_csr.py [--rows 10000000] [--reps 7] [--warmup 2] [--out profiles/hell_to_csr_ab.json]"""
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
SPREAD = 1.10       # the box-to-box spread README.md states
FILLS = {"to_csr_plain": capi.TO_CSR_FILL_PLAIN, "to_csr_transpose": capi.TO_CSR_FILL_TRANSPOSE}


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


class Matrix:
    """The caller's CSR arrays in HBM (row-major generator), the HELL matrix spgpuCsrToHellDevice builds from them -- the source of
    the timed calls -- and the destination CSR arrays."""

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
        i32 = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=DEV)
        self.lens, self.sorted, self.r_idx_buf = i32(n), i32(n), i32(n)
        self.ho = i32((n + HACK - 1) // HACK)
        self.out_ptr, self.out_cols = i32(n + 1), i32(self.nnz)
        self.out_vals = torch.empty(max(self.nnz, 1), dtype=torch.float64, device=DEV)
        self.work = torch.empty(capi.spgpuToCsrWorkBytes(n), dtype=torch.uint8, device=DEV)
        self.r_idx, self.rs, self.slots, self.cM, self.rP = None, None, 0, None, None
        torch.cuda.synchronize()

    def store(self, ordered):
        """The HELL source (untimed): row lengths, the order if asked for, the plan, the arrays zeroed and filled."""
        plan_work = torch.empty(capi.spgpuCooConvertWorkBytes(self.n, 0), dtype=torch.uint8, device=DEV)
        longest, height = C.c_int(0), C.c_int(0)
        ok(capi.spgpuCsrRowLengthsDevice(self.h, p(self.lens), C.byref(longest), self.n, p(self.row_ptr), 0))
        self.rs, self.r_idx = self.lens, None
        if ordered:
            order_work = torch.empty(capi.spgpuOellOrderWorkBytes(self.n), dtype=torch.uint8, device=DEV)
            ok(capi.spgpuOellOrderAlignedDevice(self.h, p(self.r_idx_buf), p(self.sorted), p(self.lens), self.n, WINDOW, LONG_ROWS, p(order_work)))
            self.rs, self.r_idx = self.sorted, self.r_idx_buf
        ok(capi.spgpuHellPlanDevice(self.h, C.byref(height), p(self.ho), HACK, self.n, p(self.rs), p(plan_work)))
        self.slots = HACK * height.value
        self.cM, self.rP = None, None
        torch.cuda.empty_cache()
        self.cM = torch.zeros(max(self.slots, 1), dtype=torch.float64, device=DEV)
        self.rP = torch.zeros(max(self.slots, 1), dtype=torch.int32, device=DEV)
        self.csr_to_hell(self.cM, self.rP)

    def csr_to_hell(self, out_v, out_i):
        """ms of spgpuCsrToHellDevice alone (the fill the library ships), into arrays the caller zeroed."""
        t0 = clock()
        ok(capi.spgpuCsrToHellDevice(self.h, p(out_v), p(out_i), p(self.ho), HACK, 0, self.n, p(self.row_ptr), p(self.cols), p(self.vals), 0,
                                     capi.TYPE_DOUBLE, p(self.r_idx)))
        t1 = clock()
        return (t1 - t0) * 1e3

    def to_csr(self, fill):
        """(ms of row pointers + fill, ms of the fill alone)."""
        nnz, longest = C.c_int(0), C.c_int(0)
        t0 = clock()
        ok(capi.spgpuHellToCsrRowPtrDevice(self.h, p(self.out_ptr), C.byref(nnz), C.byref(longest), 0, HACK, p(self.ho), p(self.rs),
                                           p(self.r_idx), self.n, self.slots, p(self.work)))
        assert nnz.value == self.nnz
        t1 = clock()
        ok(capi.spgpuHellToCsrDeviceWith(self.h, p(self.out_cols), p(self.out_vals), p(self.out_ptr), 0, p(self.cM), p(self.rP), HACK,
                                         p(self.ho), p(self.rs), p(self.r_idx), self.n, 0, capi.TYPE_DOUBLE, fill, 0))
        t2 = clock()
        return (t2 - t0) * 1e3, (t2 - t1) * 1e3

    def same_as_the_callers(self):
        return bool(torch.equal(self.out_ptr, self.row_ptr) and torch.equal(self.out_cols, self.cols)
                    and torch.equal(self.out_vals.view(torch.int64), self.vals.view(torch.int64)))


def measure(handle, name, lengths, pattern, ordered, reps, warmup, matrix=None):
    m = matrix or Matrix(handle, lengths, pattern)
    m.store(ordered)
    back_v, back_i = torch.empty_like(m.cM), torch.empty_like(m.rP)
    times = {key: [] for key in list(FILLS) + ["csr_to_hell"]}
    for rep in range(warmup + reps):
        for key, fill in FILLS.items():
            m.out_cols.fill_(-1)
            m.out_vals.fill_(-1.0)
            sample = m.to_csr(fill)
            if rep >= warmup:
                times[key].append(sample)
        back_v.zero_()
        back_i.zero_()
        sample = m.csr_to_hell(back_v, back_i)
        if rep >= warmup:
            times["csr_to_hell"].append((sample, sample))
    same = {}
    for key, fill in FILLS.items():
        m.out_ptr.fill_(-1)
        m.out_cols.fill_(-1)
        m.out_vals.fill_(-1.0)
        m.to_csr(fill)
        same[key] = m.same_as_the_callers()
    same["csr_to_hell"] = bool(torch.equal(back_i, m.rP) and torch.equal(back_v.view(torch.int64), m.cM.view(torch.int64)))
    algorithmic = m.nnz * 12 + m.nnz * 12 + (m.n + 1) * 4 + m.n * 4 + (m.n * 4 if ordered else 0)
    entry = dict(matrix=name, rows=m.n, nnz=m.nnz, slots=m.slots, slots_per_nnz=round(m.slots / m.nnz, 4), ordered=ordered,
                 algorithmic_bytes=algorithmic, same_bytes_as_the_callers_csr=same, routes={})
    for key, samples in times.items():
        whole = statistics.median(s[0] for s in samples)
        last = statistics.median(s[1] for s in samples)
        entry["routes"][key] = dict(ms=round(whole, 3), ms_min=round(min(s[0] for s in samples), 3), ms_max=round(max(s[0] for s in samples), 3),
                                    fill_ms=round(last, 3), fill_ms_min=round(min(s[1] for s in samples), 3),
                                    fill_ms_max=round(max(s[1] for s in samples), 3), fill_effective_GBps=round(algorithmic / last * 1e-6, 1))
    yard = entry["routes"]["csr_to_hell"]["fill_ms"]
    for key in FILLS:
        entry["routes"][key]["fill_over_csr_to_hell_fill"] = round(entry["routes"][key]["fill_ms"] / yard, 3)
    print(json.dumps(entry), flush=True)
    del back_v, back_i
    torch.cuda.empty_cache()
    return entry, m


def choose(results):
    """The rule: the faster fill on `powerlaw`, if it is within the spread of the other on `banded`; else the transposing fill."""
    fill_ms = {e["matrix"]: {key: e["routes"][key]["fill_ms"] for key in FILLS} for e in results}
    ragged, banded = fill_ms["powerlaw"], fill_ms["banded"]
    fastest = min(FILLS, key=lambda key: ragged[key])
    other = next(key for key in FILLS if key != fastest)
    holds = banded[fastest] <= SPREAD * banded[other]
    return dict(faster_on_powerlaw=fastest, within_spread_on_banded=holds, banded_ratio_to_the_other=round(banded[fastest] / banded[other], 3),
                choice=fastest if holds else "to_csr_transpose",
                rule="faster fill on powerlaw, no more than 10 % slower than the other on banded; else the transposing fill")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hell_to_csr_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_to_csr.py measures on a GPU; none found")
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
    names = {fill: key for key, fill in FILLS.items()}
    out = dict(tool="tools/bench_to_csr.py", device=torch.cuda.get_device_name(0), type="fp64", hack_size=HACK, rows=args.rows, reps=args.reps,
               warmup=args.warmup, clock="host clock around calls that end in a device synchronise; median",
               algorithmic_bytes="nnz * 12 read, nnz * 12 + (rows + 1) * 4 written, rows * 4 of rS (+ rows * 4 of rIdx with an order)",
               chunk_columns=capi.TO_CSR_FILL_CHUNK, default_fill_of_this_build=names[capi.TO_CSR_FILL_DEFAULT], decision=choose(results),
               matrices=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["decision"]), flush=True)
    capi.spgpuDestroy(handle)


if __name__ == "__main__":
    main()
