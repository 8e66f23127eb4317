"""CPU: spgpu_amd/csrc/trsv_rules.h -- the one place where the triangular solve cuts its list of levels into launches -- executed.
tests/trsv_rules_cases.cpp is a stand-alone program around that header (g++, undefined-behaviour sanitizer on); its segments are
compared with the rule as the header's text states it, restated here: plain -- every level a launch; chained -- a level wider than
the chain width a launch of its own, a MAXIMAL run of narrower levels one launch of one workgroup.  Every level must be covered
exactly once and in order."""
import os
import subprocess

import pytest

from spgpu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
PLAIN, CHAINED = 0, 1
THREADS = 256


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trsv_rules") / "trsv_rules_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "trsv_rules_cases.cpp"), "-o", exe], check=True)
    return exe


def run(program, cases):
    """cases: (solve, width, maxBlocks, [level widths]) -> per case the list of (firstLevel, levels, chained, grid)."""
    text = "".join(f"{s} {w} {cap} {len(widths)} " + " ".join(map(str, widths)) + "\n" for s, w, cap, widths in cases)
    done = subprocess.run([program], input=text, capture_output=True, text=True)
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
    assert len(out) == len(cases)
    return out, constants


def restated(solve, width, cap, widths):
    """The rule of the header's text."""
    grid = lambda rows: max(1, min((rows + THREADS - 1) // THREADS, cap if cap > 0 else 1048576))
    out, l = [], 0
    while l < len(widths):
        if solve != CHAINED or widths[l] > width:
            out.append((l, 1, 0, grid(widths[l])))
            l += 1
            continue
        end = l
        while end < len(widths) and widths[end] <= width:
            end += 1
        out.append((l, end - l, 1, 1))
        l = end
    return out


def covered_once_and_in_order(segments, levels):
    at = 0
    for first, count, _, grid in segments:
        assert first == at and count >= 1 and grid >= 1
        at += count
    assert at == levels


W = capi.TRSV_CHAIN_WIDTH
SHAPES = {
    "zero levels": [],
    "a single narrow level": [5],
    "a single level at the width": [W],
    "a single wide level": [W + 1],
    "all wide": [W + 1, 3 * W, 10 * W, W + 1],
    "all narrow": [1, 2, W, W - 1, 1],
    "a narrow run at the start": [1, 2, 3, 4 * W, 5 * W],
    "a narrow run in the middle": [4 * W, 1, W, 2, 5 * W],
    "a narrow run at the end": [4 * W, 5 * W, 3, 2, 1],
    "narrow runs at the start, in the middle and at the end": [1, 1, 2 * W, 7, W, W - 1, 3 * W, W + 1, 2, 1],
    "w-1, w, w+1": [W - 1, W, W + 1],
    "w+1, w, w-1": [W + 1, W, W - 1],
    "alternating": [W + 1, 1, W + 1, 1, W + 1],
    "a stencil's wavefront": list(range(1, 3 * W, 37)) + list(range(3 * W, 0, -41)),
    "a bidiagonal chain": [1] * 3000,
    "the largest level": [1, 2 ** 31 - 1 - 2, 1],
}


def test_the_constants_are_the_librarys(program):
    _, constants = run(program, [])
    assert constants == (THREADS, W, capi.TRSV_SOLVE_PLAIN, capi.TRSV_SOLVE_CHAINED) and (PLAIN, CHAINED) == constants[2:]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_every_level_is_covered_exactly_once_and_in_order(program, name):
    widths = SHAPES[name]
    cases = [(solve, width, cap, widths) for solve in (PLAIN, CHAINED) for width in (W, 1, 64, 1024) for cap in (0, 1, 3)]
    got, _ = run(program, cases)
    for case, segments in zip(cases, got):
        covered_once_and_in_order(segments, len(widths))
        assert segments == restated(*case), (name, case[:3])
        if case[0] == PLAIN:
            assert [s[:3] for s in segments] == [(l, 1, 0) for l in range(len(widths))]
        else:
            for (first, count, chained, _), nxt in zip(segments, segments[1:] + [None]):
                span = widths[first:first + count]
                assert (max(span) <= case[1]) == bool(chained)
                assert not (chained and nxt and nxt[2]), "two chained segments in a row: the run was not maximal"


def test_the_written_expectations_at_the_corners(program):
    got, _ = run(program, [(CHAINED, W, 0, SHAPES["w-1, w, w+1"]), (CHAINED, W, 0, SHAPES["a bidiagonal chain"]),
                           (CHAINED, W, 0, SHAPES["narrow runs at the start, in the middle and at the end"]),
                           (PLAIN, W, 2, [5 * THREADS]), (CHAINED, W, 0, []), (CHAINED, W, 0, SHAPES["the largest level"])])
    assert got[0] == [(0, 2, 1, 1), (2, 1, 0, 2)]
    assert got[1] == [(0, 3000, 1, 1)]                                        # one launch instead of 3 000
    assert got[2] == [(0, 2, 1, 1), (2, 1, 0, 2), (3, 3, 1, 1), (6, 1, 0, 3), (7, 1, 0, 2), (8, 2, 1, 1)]
    assert got[3] == [(0, 1, 0, 2)] and got[4] == []
    assert got[5] == [(0, 1, 1, 1), (1, 1, 0, 1048576), (2, 1, 1, 1)]
