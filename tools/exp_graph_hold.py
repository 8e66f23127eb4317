#!/usr/bin/env python3
"""GPU box experiment: what a hold (include/spgpu/ext/graph.h) buys a captured graph on the north_star target -- HELL fp64, 10 M rows,
power-law lengths (mean 32, max 2 048), the rows as they come, ADOPTED (spgpuHellSpmvAdopt) -- with columns as a band and within
+-2 048 of the row (bench.py bench_powerlaw's matrices, built the same way).  Per pattern, on one side stream of one handle:

    eager          the adopted call (spgpuDhellspmv on the caller's arrays, no rIdx: runs on the library's ordered copy), median
                   of --reps calls timed one by one with events
    replay unheld  one SpMV captured without a hold (the plain kernel on the caller's arrays), the graph replayed --reps times
    replay held    the same capture under spgpuSpmvHold (the ordered copy), replayed --reps times
    cg unheld/held one CG iteration with the scalars on the device (SpMV, dot, three quotient updates, dot) captured per parity and
                   replayed --iters times (the matrix is not symmetric: the iteration is timed, not solved)

and whether the held replay's z is the eager call's bit for bit.

    python tools/exp_graph_hold.py [--rows 10000000] [--reps 200] [--iters 100] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from spgpu_amd import capi, formats, synth  # noqa: E402


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rows, letter = args.rows, "D"
    handle = capi.create_handle(0)
    side = torch.cuda.Stream()
    capi.spgpuSetStream(handle, C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    say(f"exp_graph_hold: HELL fp64, {rows} rows, power-law lengths mean 32 / max 2048, rows as they come, adopted; "
        f"{args.reps} replays / calls, {args.iters} CG iterations; device {torch.cuda.get_device_name(0)}")
    lengths = synth.power_law_lengths(rows, mean=32.0, max_len=2048, seed=5)

    def timed(fn, count):
        """median and mean ms of `count` runs of fn on the side stream, each between two events"""
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(count)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(count)]
        with torch.cuda.stream(side):
            for i in range(count):
                starts[i].record(side)
                fn()
                ends[i].record(side)
        side.synchronize()
        ms = [s.elapsed_time(e) for s, e in zip(starts, ends)]
        return statistics.median(ms), statistics.fmean(ms)

    def capture(fn):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        torch.cuda.synchronize()
        return g

    for pattern in ("band", "near"):
        coo = synth.ragged_coo_on_device(lengths, rows, pattern, 2048, letter, seed=5, device="cuda:0")
        plain = formats.coo_to_ordered_hell_device(handle, rows, *coo, letter, 32, 0, 0, order=False)
        del coo
        torch.cuda.empty_cache()
        key = plain["rP"]
        x = torch.rand(rows, dtype=torch.float64, device="cuda:0")
        z = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
        z_eager = torch.zeros_like(z)

        def spmv(out=z, p=x):
            capi.hellspmv[letter](handle, _dp(out), None, capi.scalar(letter, 1.0), _dp(plain["cM"]), _dp(key), 32, _dp(plain["hack_offsets"]),
                                  _dp(plain["rS"]), None, 32, rows, _dp(p), capi.scalar(letter, 0.0), 0)

        said = capi.spgpuHellSpmvAdopt(handle, capi.TYPE_CODE[letter], _dp(plain["cM"]), _dp(key), 32, _dp(plain["hack_offsets"]), _dp(plain["rS"]), rows, 0)
        say(f"[{pattern}] slots/nnz {plain['slots'] / plain['nnz']:.3f}  adopt {said}  copy {capi.spgpuSpmvFrozenBytes(handle) / 1e9:.3f} GB")
        if said != capi.SPGPU_SUCCESS:
            say(f"[{pattern}] not adopted: skipped")
            continue
        graphs = []
        try:
            for _ in range(5):
                with torch.cuda.stream(side):
                    spmv(z_eager)
            side.synchronize()
            eager = timed(lambda: spmv(z_eager), args.reps)
            say(f"[{pattern}] eager adopted call       median {eager[0]:.4f} ms  mean {eager[1]:.4f} ms")
            uses = capi.spgpuSpmvAdoptedUses(handle)
            g = capture(spmv)
            graphs.append(g)
            said_uses = capi.spgpuSpmvAdoptedUses(handle) - uses
            g.replay()
            unheld = timed(g.replay, args.reps)
            say(f"[{pattern}] captured SpMV, no hold   median {unheld[0]:.4f} ms  mean {unheld[1]:.4f} ms  (AdoptedUses at capture +{said_uses})")
            assert capi.spgpuSpmvHold(handle, _dp(key)) == capi.SPGPU_SUCCESS
            uses = capi.spgpuSpmvAdoptedUses(handle)
            g = capture(spmv)
            graphs.append(g)
            said_uses = capi.spgpuSpmvAdoptedUses(handle) - uses
            z.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            same = torch.equal(z, z_eager)
            held = timed(g.replay, args.reps)
            say(f"[{pattern}] captured SpMV, held      median {held[0]:.4f} ms  mean {held[1]:.4f} ms  (AdoptedUses at capture +{said_uses}; "
                f"z {'bit-identical to' if same else 'DIFFERS from'} the eager adopted call)")

            # one CG iteration, scalars on the device, a graph per parity of the |r|^2 cell
            r, p, w = torch.rand_like(x), torch.rand_like(x), torch.zeros_like(x)
            xs = torch.zeros_like(x)
            s = torch.ones(3, dtype=torch.float64, device="cuda:0")

            def iteration(rr_old, rr_new):
                spmv(w, p)
                capi.dot_device[letter](handle, _dp(s[2:]), rows, _dp(p), _dp(w))
                capi.axpby_quot_device[letter](handle, _dp(xs), rows, None, None, _dp(xs), _dp(rr_old), _dp(s[2:]), 0, _dp(p))
                capi.axpby_quot_device[letter](handle, _dp(r), rows, None, None, _dp(r), _dp(rr_old), _dp(s[2:]), 1, _dp(w))
                capi.dot_device[letter](handle, _dp(rr_new), rows, _dp(r), _dp(r))
                capi.axpby_quot_device[letter](handle, _dp(p), rows, _dp(rr_new), _dp(rr_old), _dp(p), None, None, 0, _dp(r))

            for tag, hold in (("no hold", False), ("held", True)):
                if not hold:
                    assert capi.spgpuSpmvRelease(handle, _dp(key)) == capi.SPGPU_SUCCESS
                else:
                    assert capi.spgpuSpmvHold(handle, _dp(key)) == capi.SPGPU_SUCCESS
                pair = [capture(lambda par=par: iteration(s[par:], s[1 - par:])) for par in range(2)]
                graphs.extend(pair)
                pair[0].replay()
                pair[1].replay()
                side_ms = timed(lambda: [pair[i & 1].replay() for i in range(args.iters)], 1)[0] / args.iters
                say(f"[{pattern}] graph CG iteration, {tag:8s} {side_ms * 1e3:.1f} us per iteration")
                if not hold:
                    assert capi.spgpuSpmvHold(handle, _dp(key)) == capi.SPGPU_SUCCESS  # the held single-SpMV graph still lives
        finally:
            for g in graphs:
                g.reset()
            torch.cuda.synchronize()
            while capi.spgpuSpmvHolds(handle, _dp(key)) > 0:
                capi.spgpuSpmvRelease(handle, _dp(key))
            capi.spgpuSpmvThaw(handle, _dp(key))
        del plain, key, x, z, z_eager
        torch.cuda.empty_cache()
    capi.spgpuSetStream(handle, None)
    capi.spgpuDestroy(handle)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
