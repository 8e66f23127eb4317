"""CPU: the case table of tests/test_gpu_device_scalars_mv.py reaches every branch of the host dispatch behind
include/spgpu/ext/device_scalars_mv.h, each case reaches the branches it is there for, and the restated dispatch
(tests/device_scalars_mv_launch_shapes.py) still states the constants the sources state."""
import os
import re

import pytest

import device_scalars_mv_launch_shapes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name):
    with open(os.path.join(ROOT, "spgpu_amd", "csrc", name)) as f:
        return f.read()


def test_the_constants_are_those_of_the_sources():
    reduce_h, internal, grid = _source("reduce.hip.h"), _source("spgpu_internal.h"), _source("level1_grid.h")
    assert f"constexpr int kL1Threads = {M.THREADS};" in grid and f"constexpr int kL1Unroll = {M.UNROLL};" in grid
    assert re.search(rf"#define SPGPU_REDUCE_MAX_BLOCKS {M.REDUCE_MAX_BLOCKS}\b", internal)
    assert "constexpr int kReduceMaxVectorsPerPass = SPGPU_REDUCE_MAX_BLOCKS;" in reduce_h
    assert f"constexpr int kL1MaxBlocks = {M.L1_MAX_BLOCKS};" in grid


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


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_special_cases_are_what_the_table_says(letter):
    c = M.cases(letter)
    n = M.CAP_N[letter]
    (cap,) = M.reduce_passes(letter, n, M.CAP_COUNT, M.pitch_of(letter, "rounded", n))
    assert cap == dict(vectors=64, wide=True, blocks=16, cap_binds=True) and not M.cap_free(letter, n, M.CAP_COUNT)
    two = M.reduce_passes(letter, **M.TWO_PASS)
    assert [(p["vectors"], p["blocks"]) for p in two] == [(1024, 1), (1, 1)] and all(p["wide"] for p in two)
    assert M.reduce_passes(letter, 0, 3, 4) == [dict(vectors=3, wide=None, blocks=0, cap_binds=False)]
    assert M.reduce_passes(letter, 5, 0, 8) == [] and M.update_launch(letter, 5, 0, 8) is None
    # the odd pitch is the narrow path for more than one vector, and the pitch plays no part for one
    for count in M.COUNTS:
        want = {"wide"} if count == 1 else {"narrow"}
        assert {"wide", "narrow"} & c[f"n1025-c{count}-odd-aligned"]["want"] == want
    # at 4099 elements a vector takes more than one workgroup on both paths; at 2049 only on the narrow one (fp64: on both)
    assert M.reduce_passes(letter, 4099, 8, M.pitch_of(letter, "rounded", 4099))[0]["blocks"] == (2 if letter == "S" else 3)
    assert M.reduce_passes(letter, 4099, 8, M.pitch_of(letter, "odd", 4099))[0]["blocks"] == 5


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_per_vector_choice_of_y(letter):
    assert [M.has_beta("quot-mixed", j) for j in range(4)] == [True, False, True, True]
    assert [M.has_beta("plain-mixed", j) for j in range(3)] == [False, True, False]
    assert M.beta_branches("plain-null", 8) == {"beta-null"} and M.beta_branches("quot-ones", 8) == {"beta-nonzero"}
    # y counts for the alignment only where it may be read
    assert M.update_launch(letter, 100, 2, 104, 0, 0, M.SIZEOF[letter], beta_given=True)["wide"] is False
    assert M.update_launch(letter, 100, 2, 104, 0, 0, M.SIZEOF[letter], beta_given=False)["wide"] is True
    assert M.update_launch(letter, 100, 2, 104, 0, 0, None)["wide"] is True
