"""CPU: spgpu_amd/csrc/ilu0_rules.h -- the one place where the ILU(0) factorisation cuts its list of levels into launches and picks
the lanes that own a row -- executed.  tests/ilu0_rules_cases.cpp is a stand-alone program around that header (g++,
undefined-behaviour sanitizer on); its answers are compared with the rules as the header's text states them, restated here: plain --
every level a launch; chained -- a level wider than the factorisation's chain width a launch of its own, a MAXIMAL run of narrower
levels one launch of one workgroup; a launch over r rows of a shape of L lanes has ceil(r L / 256) workgroups up to the cap; the shape
follows the mean row length nnz / rows through two thresholds."""
import os
import subprocess

import pytest

from spgpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
PLAIN, CHAINED = capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED
THREADS = 256
W = capi.ILU0_CHAIN_WIDTH
THREAD, NARROW, WIDE = capi.ILU0_SHAPES
T1, T2 = capi.ILU0_THREAD_MAX_MEAN, capi.ILU0_NARROW_MAX_MEAN


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ilu0_rules") / "ilu0_rules_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "ilu0_rules_cases.cpp"), "-o", exe], check=True)
    return exe


def run(program, lines):
    """Input lines -> per line the list of answer tuples, and the constants."""
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
            out[-1].append(tuple(int(v) for v in line.split()))
    assert len(out) == len(lines)
    return out, constants


def segments_line(solve, shape, cap, widths):
    return f"segments {solve} {shape} {cap} {len(widths)} " + " ".join(map(str, widths))


def restated_segments(solve, shape, cap, widths):
    """The rule of the header's text."""
    grid = lambda rows: max(1, min((rows * shape + THREADS - 1) // THREADS, cap if cap > 0 else 1048576))
    out, l = [], 0
    while l < len(widths):
        if solve != CHAINED or widths[l] > W:
            out.append((l, 1, 0, grid(widths[l])))
            l += 1
            continue
        end = l
        while end < len(widths) and widths[end] <= W:
            end += 1
        out.append((l, end - l, 1, 1))
        l = end
    return out


def restated_shape(rows, nnz):
    if rows <= 0 or nnz <= T1 * rows:
        return THREAD
    return NARROW if nnz <= T2 * rows else WIDE


SHAPES = {
    "zero levels": [],
    "w-1 alone": [W - 1],
    "w alone": [W],
    "w+1 alone": [W + 1],
    "w-1, w, w+1": [W - 1, W, W + 1],
    "w+1, w, w-1": [W + 1, W, W - 1],
    "alternating wide and narrow": [W + 1, 1, W + 1, W, 3 * W, W - 1, W + 1],
    "alternating narrow and wide": [1, W + 1, W, 3 * W, 2, W + 1, 1],
    "narrow runs at the start, in the middle and at the end": [1, 1, 2 * W, 7, W, W - 1, 3 * W, W + 1, 2, 1],
    "a bidiagonal chain": [1] * 3000,
    "the largest level": [1, 2 ** 31 - 1 - 2, 1],
}


def test_the_constants_are_the_librarys(program):
    _, constants = run(program, [])
    assert constants == (THREADS, W, THREAD, NARROW, WIDE, T1, T2, 64)
    assert THREAD == capi.ILU0_SHAPE_THREAD == 1 and 2 <= NARROW < WIDE <= 64 and 0 < T1 < T2
    for L in (NARROW, WIDE):
        assert L & (L - 1) == 0 and 64 % L == 0 and THREADS % L == 0              # whole groups in a wavefront and in a workgroup
    assert W >= 64 and W % 64 == 0 and capi.ILU0_SOLVE_DEFAULT in (PLAIN, CHAINED)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_level_is_covered_exactly_once_and_in_order(program, name):
    widths = SHAPES[name]
    cases = [(solve, shape, cap, widths) for solve in (PLAIN, CHAINED) for shape in (THREAD, NARROW, WIDE, 64) for cap in (0, 1, 3)]
    got, _ = run(program, [segments_line(*case) for case in cases])
    for case, segments in zip(cases, got):
        at = 0
        for first, count, _, grid in segments:
            assert first == at and count >= 1 and grid >= 1
            at += count
        assert at == len(widths)
        assert segments == restated_segments(*case), (name, case[:3])
        if case[0] == CHAINED:
            for (first, count, chained, _), nxt in zip(segments, segments[1:] + [None]):
                assert (max(widths[first:first + count]) <= W) == bool(chained)
                assert not (chained and nxt and nxt[2]), "two chained segments in a row: the run was not maximal"


def test_the_written_expectations_at_the_corners(program):
    got, _ = run(program, [segments_line(CHAINED, THREAD, 0, SHAPES["w-1, w, w+1"]), segments_line(CHAINED, NARROW, 0, SHAPES["a bidiagonal chain"]),
                           segments_line(PLAIN, THREAD, 0, [5 * THREADS]), segments_line(PLAIN, NARROW, 0, [5 * THREADS]),
                           segments_line(PLAIN, WIDE, 2, [5 * THREADS]), segments_line(PLAIN, 64, 0, [1]),
                           segments_line(PLAIN, 64, 0, [2 ** 31 - 1])])
    assert got[0] == [(0, 2, 1, 1), (2, 1, 0, 2)]
    assert got[1] == [(0, 3000, 1, 1)]
    assert got[2] == [(0, 1, 0, 5)] and got[3] == [(0, 1, 0, 5 * NARROW)] and got[4] == [(0, 1, 0, 2)] and got[5] == [(0, 1, 0, 1)]
    assert got[6] == [(0, 1, 0, 1048576)]                                     # rows * lanes does not wrap


def test_the_shape_follows_the_mean_row_length_around_every_threshold(program):
    cases = []
    for rows in (1, 7, 1000, 8_000_000, 2 ** 31 - 1):
        for threshold in (T1, T2):
            for nnz in (threshold * rows - 1, threshold * rows, threshold * rows + 1):
                cases.append((rows, nnz))
        cases += [(rows, rows), (rows, 0), (rows, 7 * rows), (rows, 27 * rows)]
    cases += [(0, 0), (0, 5), (-3, 100), (5, -1)]
    got, _ = run(program, [f"shape {rows} {nnz}" for rows, nnz in cases])
    for (rows, nnz), answer in zip(cases, got):
        assert answer == [(restated_shape(rows, nnz),)], (rows, nnz)
        if 0 <= nnz < 2 ** 31 and -2 ** 31 <= rows < 2 ** 31:
            assert capi.csr_ilu0_default_shape(rows, nnz) == answer[0][0]
    assert restated_shape(1000, T1 * 1000) == THREAD and restated_shape(1000, T1 * 1000 + 1) == NARROW
    assert restated_shape(1000, T2 * 1000) == NARROW and restated_shape(1000, T2 * 1000 + 1) == WIDE
    known, _ = run(program, [f"known {s}" for s in range(-2, 130)])
    assert [s for s, k in zip(range(-2, 130), known) if k == [(1,)]] == [1, 2, 4, 8, 16, 32, 64]
