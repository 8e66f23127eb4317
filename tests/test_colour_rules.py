"""CPU: spgpu_amd/csrc/colour_rules.h -- the one place where the multicolour ordering picks the lanes that own a row and sizes its
grids -- executed.  tests/colour_rules_cases.cpp is a stand-alone program around that header (g++, undefined-behaviour sanitizer on);
its answers are compared with the rules as the header's text states them, restated here: the colouring runs one thread per row
whatever the mean row length, a launch over r rows of a shape of L lanes has ceil(r L / 256) workgroups up to the cap, the
permutation runs one fixed shape, and the library's exported rule is the header's.  The shapes are the ones
profiles/csr_colour_ab.json backs, and the test reads that file."""
import json
import os
import subprocess

import pytest

from spgpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
THREADS = 256


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("colour_rules") / "colour_rules_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "colour_rules_cases.cpp"), "-o", exe], check=True)
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


def test_the_constants_are_whole_groups_and_the_measured_shapes(program):
    _, (threads, thread, widest, permute) = run(program, [])
    assert threads == THREADS and thread == capi.COLOUR_SHAPE_THREAD == 1 and widest == 64
    assert permute & (permute - 1) == 0 and 64 % permute == 0 and THREADS % permute == 0      # whole groups in a wavefront and a workgroup
    with open(os.path.join(CSRC, "colour_rules.h")) as f:
        rules = f.read()
    assert "hip/" not in rules and '#include "csr_host.h"' in rules and "cappedGrid(" in rules      # plain host C++, the shared grid rule
    profile = os.path.join(ROOT, "profiles", "csr_colour_ab.json")
    if not os.path.exists(profile):
        assert "NOT MEASURED" in rules and permute == thread                  # the fallback
        return
    # the shipped shapes are the ones the file backs: thread colours fastest on both matrices with its range below every other
    # shape's, and the permutation's one shape lies below thread on both
    with open(profile) as f:
        measured = json.load(f)
    assert "MEASURED" in rules and "NOT MEASURED" not in rules and len(measured["orderings"]) == 2
    name = {1: "thread", 8: "group8", 32: "group32", 64: "group64"}
    for entry in measured["orderings"]:
        legs = entry["legs"]
        assert entry["every_leg_gives_the_same_bytes"] and entry["chosen_by_the_rule"]["colour"] == "thread"
        assert capi.csr_colour_default_shape(entry["rows"], entry["entries"]) == thread
        assert all(legs["colour thread"]["ms_max"] < legs[f"colour {other}"]["ms_min"] for other in ("group8", "group32", "group64"))
        assert legs[f"permute {name[permute]}"]["ms_max"] < legs["permute thread"]["ms_min"]
        assert entry["levels"]["multicolour"]["lower"] == entry["colours"] < entry["levels"]["natural"]["lower"]


def test_the_colouring_runs_one_thread_per_row_whatever_the_mean_row_length(program):
    """Measured at the means 6.97 and 26.46, the fallback everywhere else: there is no threshold to stand on either side of."""
    _, (_, thread, _, _) = run(program, [])
    cases = []
    for rows in (1, 7, 1000, 8_000_000, 2 ** 31 - 1):
        cases += [(rows, nnz) for nnz in (0, rows, 2 * rows, 2 * rows + 1, 7 * rows, 16 * rows, 16 * rows + 1, 27 * rows, 64 * rows, 1000 * rows)]
    cases += [(0, 0), (0, 5), (-3, 100), (5, -1)]
    got, _ = run(program, [f"shape {rows} {nnz}" for rows, nnz in cases])
    for (rows, nnz), answer in zip(cases, got):
        assert answer == thread, (rows, nnz)
        if 0 <= nnz < 2 ** 31 and -2 ** 31 <= rows < 2 ** 31:
            assert capi.csr_colour_default_shape(rows, nnz) == answer         # the library runs this header
    known, _ = run(program, [f"known {s}" for s in range(-2, 130)])
    assert [s for s, k in zip(range(-2, 130), known) if k == 1] == [1, 2, 4, 8, 16, 32, 64]


def test_the_grid_covers_the_rows_up_to_the_cap(program):
    cases = [(rows, shape, cap) for rows in (0, 1, 255, 256, 257, 1025, 5 * THREADS, 8_000_000, 2 ** 31 - 1) for shape in (1, 8, 32, 64)
             for cap in (0, 1, 3)]
    got, _ = run(program, [f"grid {rows} {shape} {cap}" for rows, shape, cap in cases])
    for (rows, shape, cap), grid in zip(cases, got):
        assert grid == max(1, min((rows * shape + THREADS - 1) // THREADS, cap if cap > 0 else 1048576)), (rows, shape, cap)
    corners, _ = run(program, ["grid 1280 1 0", "grid 1280 8 0", "grid 1280 32 2", "grid 1 64 0", f"grid {2 ** 31 - 1} 64 0",
                               f"grid {1048576 * THREADS} 1 0", f"grid {1048576 * THREADS + 1} 1 0", f"grid {1048575 * THREADS + 1} 1 0"])
    assert corners == [5, 40, 2, 1, 1048576, 1048576, 1048576, 1048576]       # rows * lanes does not wrap; the cap is reached, not passed
