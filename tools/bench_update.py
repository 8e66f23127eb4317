#!/usr/bin/env python3
"""GPU box: new coefficients for a stored HELL matrix (include/spgpu/ext/update_device.h) beside the call a solver had to use
before -- the full fill spgpuCsrToHellDevice (include/spgpu/ext/csr_device.h) on the same arrays -- in one process and on one set
of allocations:

  csr_to_hell    spgpuCsrToHellDevice: values and column indices, 24 bytes per fp64 entry
  refill         spgpuCsrToHellValuesDevice: values only, 16 bytes per entry (the transposing refill, 16-byte stores)
  refill_plain   the same through the plain refill, one thread per row
  hellcsput      spgpuDhellcsput with the WHOLE matrix as a row-sorted list (aI, aJ, aVal: 16 bytes per entry read, a bisection over
                 the row's stored indices per entry, 8 bytes written)

on  banded             BASELINE.json configs[1]: 10 M rows x 32, banded, fp64, rows as they come
    powerlaw_aligned   the north_star matrix (power-law lengths, mean 32, longest 2 048) stored in the aligned order (windows of
                       2 048, rows longer than 256 set aside) with rIdx; hellcsput finds the storage row through rowOf

Per leg: the median over --reps repetitions (after --warmup, the legs alternating inside a repetition) of the host clock around
the call, which ends in a device synchronise.  After every leg the value array is compared, byte for byte, with the one the full
fill gives.  THE GATE: on `banded` the refill's median lies below the full fill's (by bytes moved it should be about two thirds).
hellcsput is recorded, not gated.

usage: bench_update.py [--rows 10000000] [--reps 7] [--warmup 2] [--out profiles/hell_update_ab.json]"""
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
LEGS = ("csr_to_hell", "refill", "refill_plain", "hellcsput")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ok(status):
    if status != capi.SPGPU_SUCCESS:
        raise RuntimeError(f"status {status}")


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def measure(handle, name, lengths, pattern, ordered, reps, warmup):
    n = int(lengths.size)
    i32 = lambda count: torch.empty(max(count, 1), dtype=torch.int32, device=DEV)
    _, cols, vals = synth.ragged_coo_on_device(lengths, n, pattern, 2048, "D", seed=5, device=DEV)
    nnz = int(cols.numel())
    row_ptr_host = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=row_ptr_host[1:])
    assert row_ptr_host[-1] == nnz < 2 ** 31
    row_ptr = torch.from_numpy(row_ptr_host.astype(np.int32)).to(DEV)
    # the list of hellcsput: the matrix row of every entry, and -- its bisection wants them -- columns that ascend within a row
    a_i = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=DEV), torch.from_numpy(lengths.astype(np.int64)).to(DEV))
    inside = a_i[1:] == a_i[:-1]
    if not bool(((cols[1:] >= cols[:-1]) | ~inside).all()):
        key, _ = torch.sort((a_i.long() << 32) | cols.long())
        cols = (key & 0xFFFFFFFF).int()
        del key
    del inside
    lens, sorted_lens, r_idx_buf, row_of = i32(n), i32(n), i32(n), None
    ho = i32((n + HACK - 1) // HACK)
    plan_work = torch.empty(capi.spgpuCooConvertWorkBytes(n, 0), dtype=torch.uint8, device=DEV)
    longest, height = C.c_int(0), C.c_int(0)
    ok(capi.spgpuCsrRowLengthsDevice(handle, p(lens), C.byref(longest), n, p(row_ptr), 0))
    rs, r_idx = lens, None
    if ordered:
        order_work = torch.empty(capi.spgpuOellOrderWorkBytes(n), dtype=torch.uint8, device=DEV)
        ok(capi.spgpuOellOrderAlignedDevice(handle, p(r_idx_buf), p(sorted_lens), p(lens), n, WINDOW, LONG_ROWS, p(order_work)))
        rs, r_idx = sorted_lens, r_idx_buf
        row_of = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        ok(capi.spgpuInvertRowOrderDevice(handle, p(row_of), p(r_idx), n))
        del order_work
    ok(capi.spgpuHellPlanDevice(handle, C.byref(height), p(ho), HACK, n, p(rs), p(plan_work)))
    slots = HACK * height.value
    want_v = torch.zeros(max(slots, 1), dtype=torch.float64, device=DEV)      # what the full fill gives for `vals`
    r_p = torch.zeros(max(slots, 1), dtype=torch.int32, device=DEV)
    ok(capi.spgpuCsrToHellDevice(handle, p(want_v), p(r_p), p(ho), HACK, 0, n, p(row_ptr), p(cols), p(vals), 0, capi.TYPE_DOUBLE, p(r_idx)))
    c_m = torch.empty_like(want_v)                                           # the matrix the update legs work on (its indices: r_p)
    scratch_i = torch.empty_like(r_p)
    torch.cuda.synchronize()

    def run(leg):
        if leg == "csr_to_hell":
            ok(capi.spgpuCsrToHellDevice(handle, p(c_m), p(scratch_i), p(ho), HACK, 0, n, p(row_ptr), p(cols), p(vals), 0, capi.TYPE_DOUBLE,
                                         p(r_idx)))
        elif leg == "hellcsput":
            capi.hellcsput["D"](handle, capi.scalar("D", 1.0), p(c_m), p(r_p), HACK, p(ho), p(rs), p(row_of), n, nnz, p(a_i), p(cols), p(vals), 0)
        else:
            fill = capi.UPDATE_FILL_PLAIN if leg == "refill_plain" else -1
            ok(capi.spgpuCsrToHellValuesDeviceWith(handle, p(c_m), p(ho), HACK, n, p(row_ptr), p(vals), 0, capi.TYPE_DOUBLE, p(r_idx), fill, 0))

    times = {leg: [] for leg in LEGS}
    same = {leg: True for leg in LEGS}
    for rep in range(warmup + reps):
        for leg in LEGS:
            c_m.zero_()                                                      # as the caller of the full fill zeroes its arrays; untimed
            scratch_i.zero_()
            t0 = clock()
            run(leg)
            t1 = clock()
            if rep >= warmup:
                times[leg].append((t1 - t0) * 1e3)
            if rep in (0, warmup + reps - 1):
                same[leg] = same[leg] and bool(torch.equal(c_m.view(torch.int64), want_v.view(torch.int64)))
    moved = dict(csr_to_hell=nnz * 24, refill=nnz * 16, refill_plain=nnz * 16, hellcsput=nnz * 24)
    for leg in moved:
        moved[leg] += (n + 1) * 4 + (n * 4 if ordered else 0)
    entry = dict(matrix=name, rows=n, nnz=nnz, slots=slots, slots_per_nnz=round(slots / nnz, 4), ordered=ordered,
                 value_array_equals_the_full_fills=same, legs={})
    for leg, samples in times.items():
        median = statistics.median(samples)
        entry["legs"][leg] = dict(ms=round(median, 3), ms_min=round(min(samples), 3), ms_max=round(max(samples), 3),
                                  algorithmic_bytes=moved[leg], effective_GBps=round(moved[leg] / median * 1e-6, 1))
    yard = entry["legs"]["csr_to_hell"]["ms"]
    for leg in LEGS[1:]:
        entry["legs"][leg]["over_csr_to_hell"] = round(entry["legs"][leg]["ms"] / yard, 3)
    print(json.dumps(entry), flush=True)
    return entry


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hell_update_ab.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_update.py measures on a GPU; none found")
    handle = capi.create_handle(0)
    results = [measure(handle, "banded", np.full(args.rows, 32, np.int32), "band", False, args.reps, args.warmup)]
    torch.cuda.empty_cache()
    lengths = synth.power_law_lengths(args.rows, mean=32.0, max_len=2048, seed=5)
    results.append(measure(handle, "powerlaw_aligned", lengths, "near", True, args.reps, args.warmup))
    banded = results[0]["legs"]
    gate = dict(rule="on banded the refill's median lies below spgpuCsrToHellDevice's, same arrays, same process",
                refill_ms=banded["refill"]["ms"], csr_to_hell_ms=banded["csr_to_hell"]["ms"], ratio=banded["refill"]["over_csr_to_hell"],
                holds=banded["refill"]["ms"] < banded["csr_to_hell"]["ms"])
    out = dict(tool="tools/bench_update.py", device=torch.cuda.get_device_name(0), type="fp64", hack_size=HACK, rows=args.rows, reps=args.reps,
               warmup=args.warmup, clock="host clock around a call that ends in a device synchronise; median, legs alternating",
               algorithmic_bytes="per entry: full fill 12 read + 12 written, refill 8 + 8, hellcsput 16 read (list) + 8 written, the bisection's "
                                 "index reads not counted; + (rows + 1) * 4 of csrRowPtr (+ rows * 4 of rIdx / rowOf with an order)",
               gate=gate, matrices=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(gate), flush=True)
    capi.spgpuDestroy(handle)
    return 0 if gate["holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
