#!/usr/bin/env python3
"""GPU box: counters of the HDIA kernel on BASELINE configs[3] (7-point Laplacian 512^3, fp64) -> gpurun_out/profile_<tag>/<tag>_hdia_pmc.json.
    python tools/profile_hdia.py <tag> [grid]     (the profiled workload: python tools/profile_hdia.py --run [grid])
Separate rocprofv3 --pmc passes (a pass that names a counter the card does not have is reported and skipped):
FETCH_SIZE | WRITE_SIZE | TCC_HIT_sum TCC_MISS_sum | TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum | TCC_EA0_RDREQ_sum TCC_EA0_RDREQ_DRAM_sum |
TA_BUSY_avr TCP_PENDING_STALL_CYCLES_sum; the question they answer: is the x traffic beyond "once" served by L2, by the Infinity Cache or by HBM,
and would an LDS slice of x (reference: hdia_spmv_base_template.cuh:94-148 stages offsets per warp) take anything off the fabric?"""
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(m):
    """The workload: 5 rounds of 10 timed launches of the HDIA SpMV on the 7-point Laplacian m^3 (fp64, hack size 32)."""
    import ctypes as C
    sys.path.insert(0, ROOT)
    import torch
    from spgpu_amd import capi, synth
    handle = capi.create_handle(0)
    stream = torch.cuda.Stream()
    capi.spgpuSetStream(handle, C.c_void_p(stream.cuda_stream))
    p = lambda t: C.c_void_p(t.data_ptr())
    d = synth.hdia_laplacian7_on_device(m, "D", 32)
    n = d["rows"]
    x, z = synth.device_vector(n, "D", 3), torch.empty(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    alg = 32 * d["height"] * 8 + d["height"] * 4 + (n // 32 + 1) * 4 + 2 * n * 8
    call = lambda: capi.hdiaspmv["D"](handle, p(z), None, 1.0, p(d["dM"]), p(d["offsets"]), 32, p(d["hack_offsets"]), n, n, p(x), 0.0)
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            call()
            a.record(stream)
            for _ in range(10):
                call()
            b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b) / 10)
    t = sorted(times)[len(times) // 2]
    print(f"median {t:.4f} ms  min {min(times):.4f}  {alg / t * 1e-6:7.1f} GB/s  {alg / t * 1e-6 / 8000:6.1%}", flush=True)


if sys.argv[1] == "--run":
    run(int(sys.argv[2]) if len(sys.argv) > 2 else 512)
    sys.exit(0)
tag = sys.argv[1]
grid = sys.argv[2] if len(sys.argv) > 2 else "512"
out = os.path.join(ROOT, "gpurun_out", f"profile_{tag}")
os.makedirs(out, exist_ok=True)
env = dict(os.environ, TMPDIR="/tmp")
cmd = ["python3", os.path.abspath(__file__), "--run", grid]
passes = [["FETCH_SIZE"], ["WRITE_SIZE"], ["TCC_HIT_sum", "TCC_MISS_sum"], ["TCP_TCC_READ_REQ_sum", "TCP_TOTAL_CACHE_ACCESSES_sum"],
          ["TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_DRAM_sum"], ["TCC_EA0_RDREQ_32B_sum"], ["TA_BUSY_avr", "TCP_PENDING_STALL_CYCLES_sum"], ["TCC_REQ_sum", "TCC_READ_sum"]]
result = {"command": "rocprofv3 --pmc <counters> --kernel-trace -- python3 tools/profile_hdia.py --run " + grid, "counters_mean_per_launch": {}, "skipped": {}}
said = None
for counters in passes:
    d = os.path.join(out, "hdia_" + "_".join(c.lower() for c in counters))
    r = subprocess.run(["rocprofv3", "--pmc"] + counters + ["--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--"] + cmd, cwd="/tmp", env=env,
                       capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if "median" in ln]
    said = said or (lines[0] if lines else None)
    got = {}
    for path in glob.glob(os.path.join(d, "*counter_collection.csv")):
        for row in csv.DictReader(open(path)):
            if "hdiaSpmvKernel" in row["Kernel_Name"]:
                got.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    if not got:
        result["skipped"][" ".join(counters)] = (r.stderr.strip().splitlines() or ["no rows"])[-1][:300]
    for name, values in got.items():
        result["counters_mean_per_launch"][name] = dict(mean=sum(values) / len(values), launches=len(values))
    for path in glob.glob(os.path.join(d, "*.csv")):
        if os.path.getsize(path) > (1 << 20):
            os.remove(path)
c = result["counters_mean_per_launch"]
n = int(grid) ** 3
if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
    read_b, write_b = 2 * c["FETCH_SIZE"]["mean"] * 1024, c["WRITE_SIZE"]["mean"] * 1024
    result["fabric_read_bytes_x2_corrected"] = read_b
    result["fabric_write_bytes"] = write_b
    result["x_and_z_once_bytes"] = 2 * n * 8
result["timing_under_the_profiler"] = said
with open(os.path.join(out, f"{tag}_hdia_pmc.json"), "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(result, indent=1))
