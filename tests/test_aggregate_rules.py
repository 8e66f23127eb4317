"""CPU: spgpu_amd/csrc/aggregate_rules.h -- the one place where the aggregation picks the lanes that own a row and sizes its grids --
executed.  tests/aggregate_rules_cases.cpp is a stand-alone program around that header (g++, undefined-behaviour sanitizer on); its
answers are compared with the rules as the header's text states them, restated here: the shape follows the mean row length
nnz / rows through two thresholds, a launch over r rows of a shape of L lanes has ceil(r L / 256) workgroups up to the cap, and the
library's exported rule is the header's.  The thresholds are ILU(0)'s until tools/bench_aggregate.py has run, and the header says so."""
import os
import subprocess

import pytest

from spgpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
THREADS = 256


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aggregate_rules") / "aggregate_rules_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "aggregate_rules_cases.cpp"), "-o", exe], check=True)
    return exe


def run(program, lines):
    """Input lines -> per line the answer, and the constants."""
    done = subprocess.run([program], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, (done.returncode, done.stderr[-2000:])
    out, constants = [], None
    for line in done.stdout.splitlines():
        if line.startswith("case "):
            assert int(line.split()[1]) == len(out)
            out.append(None)
        elif line.startswith("constants "):
            constants = tuple(int(v) for v in line.split()[1:])
        else:
            out[-1] = int(line)
    assert len(out) == len(lines) and None not in out
    return out, constants


def test_the_constants_are_whole_groups_and_ilu0s_until_measured(program):
    _, (threads, thread, narrow, wide, t1, t2, widest) = run(program, [])
    assert threads == THREADS and thread == capi.AGG_SHAPE_THREAD == 1 and 2 <= narrow < wide <= widest == 64 and 0 < t1 < t2
    for L in (narrow, wide):
        assert L & (L - 1) == 0 and 64 % L == 0 and THREADS % L == 0          # whole groups in a wavefront and in a workgroup
    with open(os.path.join(CSRC, "aggregate_rules.h")) as f:
        rules = f.read()
    assert "hip/" not in rules and '#include "ilu0_rules.h"' in rules         # plain host C++
    if not os.path.exists(os.path.join(ROOT, "profiles", "csr_aggregate_ab.json")):
        assert "NOT MEASURED" in rules and "ILU(0)'s" in rules
        assert (narrow, wide, t1, t2) == (capi.ILU0_GROUP_NARROW, capi.ILU0_GROUP_WIDE, capi.ILU0_THREAD_MAX_MEAN, capi.ILU0_NARROW_MAX_MEAN)


def test_the_shape_follows_the_mean_row_length_around_every_threshold(program):
    _, (_, thread, narrow, wide, t1, t2, _) = run(program, [])

    def restated(rows, nnz):
        if rows <= 0 or nnz <= t1 * rows:
            return thread
        return narrow if nnz <= t2 * rows else wide

    cases = []
    for rows in (1, 7, 1000, 8_000_000, 2 ** 31 - 1):
        for threshold in (t1, t2):
            for nnz in (threshold * rows - 1, threshold * rows, threshold * rows + 1):
                cases.append((rows, nnz))
        cases += [(rows, rows), (rows, 0), (rows, 7 * rows), (rows, 27 * rows)]
    cases += [(0, 0), (0, 5), (-3, 100), (5, -1)]
    got, _ = run(program, [f"shape {rows} {nnz}" for rows, nnz in cases])
    for (rows, nnz), answer in zip(cases, got):
        assert answer == restated(rows, nnz), (rows, nnz)
        if 0 <= nnz < 2 ** 31 and -2 ** 31 <= rows < 2 ** 31:
            assert capi.csr_aggregate_default_shape(rows, nnz) == answer          # the library runs this header
    assert restated(1000, t1 * 1000) == thread and restated(1000, t1 * 1000 + 1) == narrow
    assert restated(1000, t2 * 1000) == narrow and restated(1000, t2 * 1000 + 1) == wide
    known, _ = run(program, [f"known {s}" for s in range(-2, 130)])
    assert [s for s, k in zip(range(-2, 130), known) if k == 1] == [1, 2, 4, 8, 16, 32, 64]


def test_the_grid_covers_the_rows_up_to_the_cap(program):
    cases = [(rows, shape, cap) for rows in (0, 1, 255, 256, 257, 1025, 5 * THREADS, 8_000_000, 2 ** 31 - 1) for shape in (1, 8, 32, 64)
             for cap in (0, 1, 3)]
    got, _ = run(program, [f"grid {rows} {shape} {cap}" for rows, shape, cap in cases])
    for (rows, shape, cap), grid in zip(cases, got):
        assert grid == max(1, min((rows * shape + THREADS - 1) // THREADS, cap if cap > 0 else 1048576)), (rows, shape, cap)
    corners, _ = run(program, ["grid 1280 1 0", "grid 1280 8 0", "grid 1280 32 2", "grid 1 64 0", f"grid {2 ** 31 - 1} 64 0"])
    assert corners == [5, 40, 2, 1, 1048576]                                  # rows * lanes does not wrap
