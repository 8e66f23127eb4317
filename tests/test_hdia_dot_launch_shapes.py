"""CPU: the case table of tests/test_gpu_stencil_dot.py reaches every instantiation of hdiaSpmvDotKernel and every branch of its host
dispatch (spgpu_amd/csrc/fused_hdia.hip over level1_grid.h) and of the kernel's control flow, each case reaches the branches it is
there for, the restated dispatch (tests/hdia_dot_launch_shapes.py) states the constants the sources state and decides as
level1_grid.h itself does (tests/hdia_dot_grid_cases.cpp, a stand-alone program around that header), and the integer inputs of
every case that claims exact sums satisfy the condition under which they are exact."""
import os
import re
import subprocess

import numpy as np
import pytest

import exact_ref as X
import hdia_dot_launch_shapes as M
import hdia_launch_shapes as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cap = re.search(r"#define SPGPU_REDUCE_MAX_BLOCKS (\d+)\b", _source("spgpu_internal.h")).group(1)
    exe = str(tmp_path_factory.mktemp("hdia_dot_grid") / "hdia_dot_grid_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    f"-DSPGPU_REDUCE_MAX_BLOCKS={cap}", os.path.join(ROOT, "tests", "hdia_dot_grid_cases.cpp"), "-o", exe], check=True)
    return exe


def _ask(program, lines):
    """(wide, blocks, nt, packed) of level1_grid.h per (elemBytes, rows, hackSizeOrPitch, offW, offZ, offDM)."""
    text = "".join(" ".join(str(v) for v in line) + "\n" for line in lines)
    done = subprocess.run([program], input=text, capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, (done.returncode, done.stderr[-2000:])
    out = [tuple(int(v) for v in line.split()) for line in done.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _restated(letter, rows, hack, off_w, off_z, off_dM):
    got = M.launch(letter, rows, hack, off_w, off_z, off_dM)
    return (0, 0, 0, 0) if got is None else (int(got["path"] != "narrow"), got["blocks"], 0, int(got["path"] == "packed"))


def test_the_constants_are_those_of_the_sources():
    grid, internal, numeric, kernel = (_source(n) for n in ("level1_grid.h", "spgpu_internal.h", "numeric.hip.h", "fused_hdia.hip"))
    assert f"constexpr int kL1Threads = {M.kL1Threads};" in grid and f"constexpr int kL1Unroll = {M.kL1Unroll};" in grid
    assert re.search(rf"#define SPGPU_REDUCE_MAX_BLOCKS {M.SPGPU_REDUCE_MAX_BLOCKS}\b", internal)
    assert f"constexpr int kWave = {M.kWave};" in numeric and f"constexpr int kStage = {M.kStage};" in kernel
    assert M.WIDE == {"S": 4, "D": 2} and M.TILE == 1024
    assert "inline bool packedStrips(size_t elemBytes, bool wide, int hackSizeOrPitch, const void* dM)" in grid
    # the call site asks the header, once
    assert len(re.findall(r"hipLaunchKernelGGL\(\(hdiaSpmvDotKernel<", kernel)) == 1
    assert "reduceGrid(sizeof(T), rows, 1, 0, a.w, z, false, SPGPU_REDUCE_MAX_BLOCKS)" in kernel
    assert "packedStrips(sizeof(T), g.wide, hackSize, dM)" in kernel


def test_the_header_decides_as_the_restated_dispatch_on_every_case(program):
    lines, want = [], []
    for letter in M.LETTERS:
        eb = M.SIZEOF[letter]
        for c in M.cases(letter).values():
            off = c["off"]
            args = (c["rows"], c["hp"], (off["x"] if c["w_null"] else off["w"]) * eb, off["z"] * eb, off["dM"] * eb)
            lines.append((eb,) + args)
            want.append(_restated(letter, *args))
    assert len(lines) > 80
    assert _ask(program, lines) == want


def test_the_header_decides_as_the_restated_dispatch_on_the_boundaries_of_each_rule(program):
    lines, want = [], []
    for letter in M.LETTERS:
        eb, W, cap = M.SIZEOF[letter], M.WIDE[letter], M.SPGPU_REDUCE_MAX_BLOCKS
        sizes = [1, W - 1, W, W + 1, M.TILE * W - 1, M.TILE * W, M.TILE * W + 1, M.TILE, M.TILE + 1, cap * M.TILE * W, cap * M.TILE * W + 1,
                 cap * M.TILE, cap * M.TILE + 1, 2**31 - 1, 0, -1]
        for rows in sizes:
            for hack in (0, 1, 2, 3, 4, 30, 31, 32, 33, 4128):
                for offs in ((0, 0, 0), (eb, 0, 0), (0, eb, 0), (0, 0, eb), (0, 0, 4), (8, 0, 0), (0, 0, 8)):
                    lines.append((eb, rows, hack) + offs)
                    want.append(_restated(letter, rows, hack, *offs))
    assert _ask(program, lines) == want
    # written out, not only restated
    assert _restated("D", 100, 30, 0, 0, 0) == (1, 1, 0, 1) and _restated("S", 100, 30, 0, 0, 0) == (1, 1, 0, 0)
    assert _restated("D", 100, 31, 0, 0, 0)[3] == 0 and _restated("S", 100, 32, 0, 0, 4)[3] == 0 and _restated("D", 100, 32, 0, 0, 8)[3] == 0
    assert _restated("D", 100, 32, 8, 0, 0) == (0, 1, 0, 0) and _restated("S", 100, 32, 0, 4, 0) == (0, 1, 0, 0)
    assert _restated("D", 2_102_500, 32, 0, 0, 0)[1] == 1024 and _restated("S", 2_102_500, 32, 0, 0, 0)[1] == 514


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_case_reaches_the_branches_it_names(letter):
    walk = set(M.WALK)
    for cid, case in M.cases(letter).items():
        got = M.reached(case)
        assert case["want"] <= got, (letter, cid, "not reached", sorted(case["want"] - got))
        assert got - case["want"] <= walk, (letter, cid, "dispatch branches the case does not name", sorted(got - case["want"] - walk))


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_branch_is_reached_by_a_case_that_names_it(letter):
    named = set()
    for case in M.cases(letter).values():
        named |= case["want"]
    assert named == set(M.BRANCHES), sorted(named ^ set(M.BRANCHES))


def test_every_instantiation_has_a_case():
    """hdiaSpmvDotKernel<T, VEC, PACKED, HAS_BETA>: 2 types x (narrow, wide, packed) x 2 = twelve, each through both entry points."""
    count = 0
    for letter in M.LETTERS:
        table = M.cases(letter)
        for inst in M.INSTANTIATIONS:
            assert any(inst in c["want"] for c in table.values()), (letter, inst)
            count += 1
    assert count == 24


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_launches_are_what_the_table_says(letter):
    W, cap, eb = M.WIDE[letter], M.SPGPU_REDUCE_MAX_BLOCKS, M.SIZEOF[letter]
    for path, off_w, hack in (("packed", 0, 32), ("wide", 0, 31), ("narrow", eb, 32)):
        rows = M.second_trip_rows(letter, path)
        got = M.launch(letter, rows, hack, off_w=off_w)
        assert got["path"] == path and got["blocks"] == cap and got["cap_binds"] and got["trips"] == 2
        assert got["packs"] == cap * M.TILE + M.TILE + 5 and got["last_trip_partial"] and got["tail"] == (1 if path == "narrow" else W) - 1
    assert M.second_trip_rows("D", "wide") > 2_097_152 and M.second_trip_rows("S", "wide") > 4_194_304
    assert M.second_trip_rows(letter, "narrow") > 1_048_576
    assert M.launch(letter, 1, 32)["trips"] == 0 and M.launch(letter, 1, 32)["tail"] == 1
    assert M.launch(letter, 33, 32)["packs"] == 33 // W and M.launch(letter, 4097, 32)["tail"] == 1
    assert M.launch(letter, 100, 30)["path"] == ("packed" if letter == "D" else "wide") and M.launch(letter, 100, 31)["path"] == "wide"
    assert M.launch(letter, 100, 32, off_dM=eb)["path"] == "wide"
    assert M.launch(letter, 100, 32, off_w=eb)["path"] == M.launch(letter, 100, 32, off_z=eb)["path"] == "narrow"
    assert M.launch(letter, 0, 32) is None and M.launch(letter, 70, 0) is None


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_walk_on_matrices_small_enough_to_read(letter):
    """One wavefront of packs and one pack more, hand-made offsets."""
    W = M.WIDE[letter]
    n = (M.kWave + 1) * W
    hacks = -(-n // 32)
    diag = M.walk(H.hdia_matrix(letter, n, n, 32, [[0]] * hacks), letter, "packed")
    assert diag["x-strip"] == 2 and diag["x-elements"] == 0 and diag["dead-lanes"] == 63 and diag["stage-guarded"] == 2
    assert diag["mask-col-low"] == diag["mask-col-high"] == 0 and diag["stage-whole"] == 0
    low = M.walk(H.hdia_matrix(letter, n, n, 32, [[-1, 0]] * hacks), letter, "packed")
    assert (low["x-strip"], low["x-elements"], low["one-lane-crosses"], low["mask-col-low"]) == (1, 1, 1, 1)
    high = M.walk(H.hdia_matrix(letter, n, n, 32, [[0, 1]] * hacks), letter, "packed")       # the last pack is wavefront 1's only lane
    assert (high["x-strip"], high["x-elements"], high["one-lane-crosses"], high["mask-col-high"]) == (1, 1, 1, 1)
    four = M.walk(H.dia_matrix(letter, n, n, H.dia_alloc_pitch(n), [-2, 0, 2, 4, 6]), letter, "packed")
    assert four["stage-whole"] == 1 and four["stage-guarded"] == 3 and four["second-stage"] == 2     # the one-lane wavefront is never whole
    assert M.walk(H.hdia_matrix(letter, n, n, 32, [[0]] + [[]] * (hacks - 1)), letter, "packed")["hack-no-diags"] == n - 32
    odd = M.walk(H.hdia_matrix(letter, n, n, 31, [[0]] * (-(-n // 31))), letter, "wide")
    assert odd["pack-in-two-hacks"] == sum(1 for p in range(n // W) if p * W // 31 != (p * W + W - 1) // 31) > 0
    assert M.walk(H.hdia_matrix(letter, 2 * W, 1, 32, [[0]]), letter, "packed")["x-small-cols"] == 1


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_capped_matrix_is_laid_out_as_the_hand_built_ones(letter):
    """uniform_hdia against hdia_launch_shapes.hdia_matrix on the same offsets: the same slots hold values, the same hold NaN."""
    for rows, cols, hack in ((100, 100, 32), (67, 70, 31), (5, 5, 32)):
        a = M.uniform_hdia(letter, rows, cols, hack, M.BAND)
        b = H.hdia_matrix(letter, rows, cols, hack, [list(M.BAND)] * (-(-rows // hack)))
        assert np.array_equal(np.isnan(a["values"]), np.isnan(b["values"])) and a["values"].dtype == b["values"].dtype
        for key in ("offsets", "hack_offsets"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key
        assert np.array_equal(a["coo"][0], b["coo"][0]) and np.array_equal(a["coo"][1], b["coo"][1])
        r, c, v = a["coo"]                                  # diagonal d of the band has offset d - 1: slot (first + d) * hack + r % hack
        at = (a["hack_offsets"][r // hack].astype(np.int64) + (c - r + 1)) * hack + r % hack
        assert np.array_equal(a["values"][at], v)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_exact_cases_add_exactly(letter):
    """Every case that claims integer results: the sums of term magnitudes stay below 2^24 (fp32) / 2^53 (fp64), so every product and
    partial sum is exact in any order; and the vectors are not so sparse that the dot has nothing to lose.  Each path has one."""
    paths = set()
    for cid, case in M.cases(letter).items():
        if not case["exact"] or case["rows"] <= 0 or case["hp"] <= 0:
            continue
        m, x, w, y = M.inputs(case)
        z, dot, sums = M.exact(case, m, x, w, y)
        X.assert_sums_exact(letter, sums)
        assert sums["dot_terms"] > 0 and np.count_nonzero(z) >= min(case["rows"], 2), cid
        finite = m["values"][~np.isnan(m["values"])]
        assert np.array_equal(finite, np.rint(finite)), cid
        paths.add(case["path"])
    assert paths == set(M.PATHS)
