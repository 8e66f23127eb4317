"""CPU: the case table of tests/test_gpu_fused_shapes.py reaches every branch of the host dispatch of the fused CG steps
(spgpu_amd/csrc/fused_solver.hip over level1_grid.h) and of the strip choice inside rowSums, each case reaches the branches it is there for, the
restated dispatch (tests/fused_launch_shapes.py) still states the constants the sources state, and the integer inputs of every
case that claims exact sums satisfy the condition under which they are exact."""
import os
import re

import numpy as np
import pytest

import exact_ref as X
import fused_launch_shapes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", name)) as f:
        return f.read()


def test_the_constants_are_those_of_the_sources():
    grid, internal, numeric = (_source(n) for n in ("level1_grid.h", "spgpu_internal.h", "numeric.hip.h"))
    assert f"constexpr int kL1Threads = {M.kL1Threads};" in grid and f"constexpr int kL1Unroll = {M.kL1Unroll};" in grid
    assert re.search(rf"#define SPGPU_REDUCE_MAX_BLOCKS {M.SPGPU_REDUCE_MAX_BLOCKS}\b", internal)
    assert re.search(rf"constexpr int kWave = {M.kWave};", numeric)
    assert "constexpr int wideOf(size_t elemBytes) { return (int)(16 / elemBytes); }" in grid
    assert M.WIDE == {"S": 4, "D": 2} and M.TILE == 1024
    # the conditions the restated dispatch repeats (`wide` of w and z resp. of z2, `packed`) are those of level1_grid.h's reduceGrid and
    # packedRows, which tests/test_level1_grid.py runs on every case of this table and compares with spmv_dot_launch / pair_dot_launch


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_case_reaches_the_branches_it_names(letter):
    for cid, case in M.cases(letter).items():
        assert M.reached(case) == case["want"], (letter, cid, sorted(M.reached(case) ^ case["want"]))


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_branch_is_reached(letter):
    seen = set()
    for case in M.cases(letter).values():
        seen |= M.reached(case)
    assert seen == set(M.BRANCHES), sorted(seen ^ set(M.BRANCHES))


def test_every_instantiation_has_a_case():
    """hellSpmvDotKernel<T, VEC, PACKED, HAS_BETA>: 2 types x (narrow, wide, packed) x 2 = twelve; axpbyPairDotKernel<T, VEC>: four."""
    count = 0
    for letter in M.LETTERS:
        table = M.cases(letter)
        for inst in M.INSTANTIATIONS:
            assert any(inst in M.reached(c) for c in table.values()), (letter, inst)
            count += 1
    assert count == 16 and sum(i.startswith("spmv") for i in M.INSTANTIATIONS) * len(M.LETTERS) == 12


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_launches_are_what_the_table_says(letter):
    W, cap = M.WIDE[letter], M.SPGPU_REDUCE_MAX_BLOCKS
    for path, off_w, hack in (("packed", 0, 32), ("wide", 0, 33), ("narrow", M.SIZEOF[letter], 32)):
        rows = M.second_trip_rows(letter, path)
        got = M.spmv_dot_launch(letter, rows, hack, off_w=off_w)
        vec = 1 if path == "narrow" else W
        assert got["path"] == path and got["blocks"] == cap and got["cap_binds"] and got["trips"] == 2
        assert got["packs"] == cap * M.TILE + M.TILE + 5 and got["last_trip_partial"] and got["tail"] == vec - 1
    # the sizes the parent's suite reaches pass the cap for fp64 only
    assert M.spmv_dot_launch(letter, 2_102_500, 32)["cap_binds"] == (letter == "D")
    assert M.pair_dot_launch(letter, 2_500_003)["cap_binds"] == (letter == "D")
    # each of the matrix arrays alone takes the call off the packed kernel, w or z alone off the wide ones
    assert M.spmv_dot_launch(letter, 100, 32)["path"] == "packed"
    for k in ("off_cM", "off_rP", "off_rS"):
        assert M.spmv_dot_launch(letter, 100, 32, **{k: 4 if k != "off_cM" else M.SIZEOF[letter]})["path"] == "wide"
    assert M.spmv_dot_launch("D", 100, 32, off_rP=8)["path"] == "packed" and M.spmv_dot_launch("S", 100, 32, off_rP=8)["path"] == "wide"
    assert M.spmv_dot_launch(letter, 100, 32, off_w=8)["path"] == M.spmv_dot_launch(letter, 100, 32, off_z=8)["path"] == "narrow"
    assert M.spmv_dot_launch(letter, 0, 32) is None and M.pair_dot_launch(letter, 0) is None
    assert M.spmv_dot_launch(letter, W - 1, 32)["trips"] == 0 and M.spmv_dot_launch(letter, W - 1, 32)["tail"] == W - 1
    assert M.pair_dot_launch(letter, 100, off_z2=M.SIZEOF[letter])["path"] == "narrow"


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_strip_profile_on_matrices_small_enough_to_read(letter):
    """One wavefront of packs with hand-made columns."""
    from spgpu_amd import formats
    W = M.WIDE[letter]
    n = M.kWave * W
    i = np.arange(n, dtype=np.int32)
    hell = lambda r, c, base=0: formats.ell_to_hell(formats.coo_to_ell(n, r + base, c + base, np.ones(r.size, X.REAL_OF[letter]),
                                                                       coo_base=base, ell_base=base), 32)
    assert M.strip_profile(hell(i, i), letter) == {"all-strip"}                           # the diagonal
    assert M.strip_profile(hell(i, i, 1), letter) == {"all-strip"}
    assert M.strip_profile(hell(i, i, 1), letter, base=2) == {"all-gather", "one-lane-refuses"}   # column 0 falls below the base
    assert M.strip_profile(hell(i, i[::-1].copy()), letter) == {"all-gather"}             # descending columns
    c = i.copy()
    c[W] = 0                                                                              # the second pack breaks the run
    assert M.strip_profile(hell(i, c), letter) == {"all-gather", "one-lane-refuses"}
    r2, c2 = np.concatenate([i, i[1:]]), np.concatenate([i, i[1:]])                       # a second entry in every row but row 0
    order = np.argsort(r2, kind="stable")
    assert M.strip_profile(hell(r2[order], c2[order]), letter) == {"mixed-k", "one-lane-refuses", "unequal-lengths-in-pack"}


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_capped_matrix_is_what_the_converters_produce(letter):
    for n, hack in ((1000, 32), (1001, 33), (67, 4), (5, 32)):
        a, b = M.uniform2_hell(letter, n, hack), M.uniform2_through_converters(letter, n, hack)
        for key in ("values", "indices", "hack_offsets", "row_lengths"):
            assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), (n, hack, key)
        assert (a["rows"], a["hack_size"], a["height"], a["base"]) == (b["rows"], b["hack_size"], b["height"], b["base"])
    assert set(np.unique(M.uniform2_rows(1000)[0])) == {0, 1, 2}


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_exact_cases_add_exactly(letter):
    """Every case that claims integer results: the sums of term magnitudes stay below 2^24 (fp32) / 2^53 (fp64), so every product and
    partial sum is exact in any order; and the vectors are not so sparse that the dot has nothing to lose."""
    for cid, case in M.cases(letter).items():
        if case["call"] == "pair":
            if case["n"] == 0:
                continue
            x1, y1, x2, y2 = M.pair_inputs(case)
            _, z2, dot, sums = M.pair_exact(case, x1, y1, x2, y2)
            X.assert_sums_exact(letter, sums)
            assert dot > 0 and np.count_nonzero(z2) >= min(case["n"], 8), cid
        elif case["exact"] and case["rows"] > 0:
            hell, x, w, y = M.spmv_inputs(case)
            z, dot, sums = M.spmv_exact(case, hell, x, w, y)
            X.assert_sums_exact(letter, sums)
            if case["matrix"] != "empty":
                assert sums["dot_terms"] > 0, cid
    # every capped case and every alignment case is of this kind
    for cid, case in M.cases(letter).items():
        if case["call"] == "spmv" and (any(case["off"].values()) or "spmv-cap-binds" in case["want"]):
            assert case["exact"] or case["matrix"] == "ragged" and set(k for k, v in case["off"].items() if v) == {"w"}, cid
