"""CPU: spgpu_amd/csrc/sweep_rules.h -- the one place where the multicolour sweep and the residual pick the lanes that own a row,
cut the colour passes into launches and size their grids -- executed.  tests/sweep_rules_cases.cpp is a stand-alone program around
that header (g++ alone, undefined-behaviour sanitizer on); its answers are compared with the rules as the header's text states them,
restated here: the segments of the forward and of the reversed list, the shape thresholds at their edges, the grids with and
without a cap; and the library's exported rules are the header's."""
import ctypes as C
import os
import subprocess

import pytest

from spgpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
THREADS, WIDTH, PASSES = 256, 256, 64
PLAIN, CHAINED = 0, 1


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_rules") / "sweep_rules_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "sweep_rules_cases.cpp"), "-o", exe], check=True)
    return exe


def run(program, lines):
    """Input lines -> per line the list of its answer lines, and the constants."""
    done = subprocess.run([program], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, (done.returncode, done.stderr[-2000:])
    out, constants = [], None
    for line in done.stdout.splitlines():
        if line.startswith("case "):
            assert int(line.split()[1]) == len(out)
            out.append([])
        elif line.startswith("constants "):
            constants = tuple(int(v) for v in line.split()[1:])
        else:
            out[-1].append(line)
    assert len(out) == len(lines)
    return out, constants


def segments_restated(sizes, step, solve):
    """The rule in words: the colours in the order of the visit; chained, a maximal run of colours of at most WIDTH rows is one
    segment, every other colour one of its own -> ([(firstColour, colours, step, chained)], launches)."""
    visit = list(range(len(sizes))) if step > 0 else list(range(len(sizes) - 1, -1, -1))
    out = []
    for c in visit:
        narrow = solve == CHAINED and sizes[c] <= WIDTH
        if narrow and out and out[-1][3] == 1 and out[-1][0] + step * out[-1][1] == c:
            out[-1] = (out[-1][0], out[-1][1] + 1, step, 1)
        else:
            out.append((c, 1, step, 1 if narrow else 0))
    return out, sum(-(-g[1] // PASSES) if g[3] else 1 for g in out)


def test_the_constants_and_the_header(program):
    _, constants = run(program, [])
    assert constants == (THREADS, WIDTH, PASSES, 1, 8, 32, 64, 2, 16)
    assert constants[7:] == (capi.ILU0_THREAD_MAX_MEAN, capi.ILU0_NARROW_MAX_MEAN) and constants[4:6] == (capi.ILU0_GROUP_NARROW, capi.ILU0_GROUP_WIDE)
    assert (capi.SWEEP_CHAIN_WIDTH, capi.SWEEP_CHAIN_PASSES, capi.SWEEP_SHAPE_THREAD) == (WIDTH, PASSES, 1)
    with open(os.path.join(CSRC, "sweep_rules.h")) as f:
        rules = f.read()
    assert "hip/" not in rules and '#include "ilu0_rules.h"' in rules and "forEachTrsvSegment(" in rules and "NOT MEASURED" in rules
    with open(os.path.join(CSRC, "trsv_rules.h")) as f:
        assert "sweep" not in f.read().lower()                                # included, not changed


SIZES = ([5], [300], [3, 2], [300, 300], [3, 2, 300, 300, 4, 3], [300, 2, 0, 7, 300, 256, 257, 1], [0], [256] * 3, [1] * 64, [1] * 65,
         [2] * 130 + [400] + [1] * 3)


@pytest.mark.parametrize("solve", [PLAIN, CHAINED])
@pytest.mark.parametrize("step", [1, -1])
def test_the_segments_of_the_forward_and_of_the_reversed_list(program, step, solve):
    lines = []
    for sizes in SIZES:
        ptr = [0]
        for s in sizes:
            ptr.append(ptr[-1] + s)
        lines.append(f"segments {step} {solve} {len(sizes)} " + " ".join(map(str, ptr)))
    got, _ = run(program, lines)
    for sizes, answer in zip(SIZES, got):
        want, launches = segments_restated(sizes, step, solve)
        assert [tuple(int(v) for v in line.split()) for line in answer[:-1]] == want, (sizes, step, solve)
        assert answer[-1] == f"launches {launches}"
        # every colour is visited once, in the order of the direction
        visited = [g[0] + g[2] * k for g in want for k in range(g[1])]
        assert visited == (list(range(len(sizes))) if step > 0 else list(range(len(sizes) - 1, -1, -1)))
        # the library counts the launches of a call by the same rule
        ptr = [0]
        for s in sizes:
            ptr.append(ptr[-1] + s)
        host = (C.c_int * len(ptr))(*ptr)
        assert capi.csr_sweep_launches(host, len(sizes), capi.SWEEP_FORWARD if step > 0 else capi.SWEEP_BACKWARD, solve) == launches
        both = segments_restated(sizes, 1, solve)[1] + segments_restated(sizes, -1, solve)[1]
        assert capi.csr_sweep_launches(host, len(sizes), capi.SWEEP_SYMMETRIC, solve) == both


def test_a_symmetric_sweep_of_narrow_colours_is_two_launches(program):
    host = (C.c_int * 8)(0, 3, 5, 9, 12, 200, 456, 457)
    assert capi.SWEEP_SOLVE_DEFAULT == CHAINED
    assert capi.csr_sweep_launches(host, 7, capi.SWEEP_SYMMETRIC, -1) == 2 and capi.csr_sweep_launches(host, 7, capi.SWEEP_FORWARD, -1) == 1
    assert capi.csr_sweep_launches(host, 7, capi.SWEEP_SYMMETRIC, PLAIN) == 14
    assert capi.csr_sweep_launches(host, 7, 3, -1) == 0 and capi.csr_sweep_launches(None, 7, 0, -1) == 0


def test_the_shape_thresholds_at_their_edges(program):
    """ILU(0)'s rule with ILU(0)'s thresholds: a mean of at most 2 THREAD, of at most 16 a group of 8, beyond a group of 32."""
    cases = []
    for rows in (1, 7, 1000, 8_000_000):
        cases += [(rows, nnz) for nnz in (0, rows, 2 * rows, 2 * rows + 1, 3 * rows, 16 * rows, 16 * rows + 1, 17 * rows, 27 * rows)]
    cases += [(0, 0), (0, 5), (-3, 100), (5, -1), (2 ** 31 - 1, 2 ** 40)]
    got, _ = run(program, [f"shape {rows} {nnz}" for rows, nnz in cases])
    for (rows, nnz), answer in zip(cases, got):
        want = 1 if rows <= 0 or nnz <= 2 * rows else (8 if nnz <= 16 * rows else 32)
        assert int(answer[0]) == want, (rows, nnz)
        if 0 <= nnz < 2 ** 31 and -2 ** 31 <= rows < 2 ** 31:
            assert capi.csr_sweep_default_shape(rows, nnz) == want == capi.csr_ilu0_default_shape(rows, nnz)
    means = {mean: capi.csr_sweep_default_shape(1000, mean * 1000) for mean in (2, 3, 16, 17)}
    assert means == {2: 1, 3: 8, 16: 8, 17: 32}
    known, _ = run(program, [f"known {s}" for s in range(-2, 130)])
    assert [s for s, k in zip(range(-2, 130), known) if int(k[0]) == 1] == [1, 2, 4, 8, 16, 32, 64]


def test_the_grid_covers_the_rows_up_to_the_cap(program):
    cases = [(rows, shape, cap) for rows in (0, 1, 255, 256, 257, 300, 1025, 8_000_000, 2 ** 31 - 1) for shape in (1, 8, 32, 64)
             for cap in (0, 1, 3)]
    got, _ = run(program, [f"grid {rows} {shape} {cap}" for rows, shape, cap in cases])
    for (rows, shape, cap), grid in zip(cases, got):
        assert int(grid[0]) == max(1, min((rows * shape + THREADS - 1) // THREADS, cap if cap > 0 else 1048576)), (rows, shape, cap)
