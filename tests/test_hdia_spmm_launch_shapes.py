"""CPU: the case table of tests/test_gpu_hdia_spmm.py (tests/hdia_spmm_launch_shapes.py) against the dispatch of
spgpu_amd/csrc/hdia_spmm.hip.  The constants restated there are the ones the source sets, on the lines named; every case's arguments
select the passes it is there for; the table reaches every instantiation of hdiaSpmmMvKernel, the wide ones with wideIO on and off,
and every composition of passes; and it holds the shapes, counts, pitches, placements and scalars it was asked to hold."""
import os
import re

import numpy as np
import pytest

import hdia_launch_shapes as H
import hdia_spmm_launch_shapes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "spgpu_amd", "csrc", "hdia_spmm.hip")
TABLE = {L: M.cases(L) for L in M.LETTERS}


def _lines():
    with open(SOURCE) as f:
        return [""] + f.read().split("\n")      # 1-based


def test_the_constants_are_the_ones_the_source_sets_on_the_lines_named():
    src = _lines()
    assert re.search(r"constexpr int kHdiaMmThreads = (\d+);", src[49]).group(1) == str(M.THREADS)
    assert re.search(r"constexpr int kHdiaMmMaxV = (\d+);", src[50]).group(1) == str(M.MAX_V)
    assert "return V <= 2 ? 4 : V <= 4 || sizeof(T) == 8 ? 2 : 1;" in src[55]
    assert M.UNROLL == {"S": {1: 4, 2: 4, 4: 2, 8: 1}, "D": {1: 4, 2: 4, 4: 2, 8: 2}}
    body = "\n".join(src[229:240])
    assert [int(v) for v in re.findall(r"launchHdiaMm<T, RPL, (\d+)>", body)] == [1, 2, 4] and "kHdiaMmMaxV>" in body
    assert [int(v) for v in re.findall(r"a\.nvec <= (\d+)", body)] == [1, 2, 4]
    assert "constexpr int WIDE = 16 / (int)sizeof(T);" in src[259]
    assert "hackSize % WIDE == 0 && ((uintptr_t)dM % 16 == 0)" in src[260]
    assert "(uintptr_t)z % 16 == 0" in src[262] and "(uintptr_t)y % 16 == 0" in src[262] and "pitchYZ * sizeof(T)) % 16 == 0" in src[262]
    assert "first += kHdiaMmMaxV" in src[265]
    entry = "\n".join(src[282:333])
    assert entry.count("if (count <= 0 || rows <= 0 ||") == 4 and entry.count("if (count == 1)") == 4
    assert M.WIDE == {"S": 4, "D": 2}
    assert M.THREADS == H.THREADS


def test_the_source_instantiates_exactly_the_sixteen_kernels():
    names = [M.kernel_name(*k) for k in M.every_instantiation()]
    assert len(set(names)) == 16
    assert M.kernel_name("D", 2, 8) == "hdiaSpmmMvKernel<double, 2, 8>"


@pytest.mark.parametrize("count", sorted(M.PASSES))
def test_the_passes_of_a_count_written_out_are_the_dispatch_s(count):
    for letter in M.LETTERS:
        got = M.dispatch(letter, 32, M.ALIGNED, 64, count)
        assert tuple((v, n) for _, v, _, n in got) == M.PASSES[count]
        assert sum(n for _, _, _, n in got) == count
        assert all(v == M.SPMV or (n <= v and (v == 1 or n > v // 2)) for _, v, _, n in got), "the smallest kernel that holds them"
    assert M.dispatch("D", 32, M.ALIGNED, 64, 0) == [] and M.dispatch("D", 0, M.ALIGNED, 64, 4) == []


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_case_selects_the_passes_it_is_there_for(letter):
    for cid, case in TABLE[letter].items():
        assert M.case_dispatch(case) == case["want"], cid
        rows, cols = case["shape"]
        assert M.pitch_of(letter, case["pitch"], rows) >= rows and M.pitch_of(letter, case["pitch"], cols) >= cols


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_table_reaches_every_instantiation_with_wide_io_on_and_off(letter):
    for fmt in ("hdia", "dia"):
        seen = {(rpl, v, io) for case in TABLE[letter].values() if case["fmt"] == fmt for rpl, v, io, _ in case["want"]}
        for _, rpl, v in (k for k in M.every_instantiation() if k[0] == letter):
            assert (rpl, v, 1) in seen, (fmt, rpl, v, "wideIO on")
            if rpl > 1:
                assert (rpl, v, 0) in seen, (fmt, rpl, v, "wideIO off")
        assert {rpl for rpl, v, _ in seen if v == M.SPMV} == {M.WIDE[letter], 1}, "count == 1, on both of the SpMV's kernels"


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_table_reaches_every_composition_of_passes(letter):
    for fmt in ("hdia", "dia"):
        for rpl in (M.WIDE[letter], 1):
            shapes = {tuple((v, n) for _, v, _, n in case["want"]) for case in TABLE[letter].values()
                      if case["fmt"] == fmt and case["want"][0][0] == rpl}
            for name, holds in M.COMPOSITIONS.items():
                if fmt == "dia" and rpl == 1 and name not in ("single partial pass", "full + remainder 1", "two full passes + remainder",
                                                               "the SpMV itself"):
                    continue        # the narrow kernels' full set of compositions is run on HDIA; DIA is the same launch code
                assert any(holds(p) for p in shapes), (fmt, rpl, name)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_table_holds_what_it_was_asked_to_hold(letter):
    t = TABLE[letter].values()
    hdia = [c for c in t if c["fmt"] == "hdia"]
    dia = [c for c in t if c["fmt"] == "dia"]
    assert {c["shape"] for c in t} == {(H.N, H.N)} | set(H.RECT_SHAPES) | set(M.SMALL_SHAPES)
    assert {(c["hp"], c["prog"]) for c in hdia if c["shape"] == (H.N, H.N)} >= {(h, p) for h in M.HACKS for p in ("cycle", "runs", "interior")}
    assert M.HACKS == (1, 2, 30, 32, 33, 64, 4512)
    assert {c["hp"] for c in dia if c["shape"] == (H.N, H.N)} == set(H.dia_pitches(letter, H.N))
    assert {c["prog"][0] for c in dia} == {"edge", "interior"}
    assert M.COUNTS == (1, 2, 7, 8, 9, 19)
    for family in (hdia, dia):
        assert {c["count"] for c in family} >= set(M.COUNTS)
        assert {c["pitch"] for c in family} == set(M.PITCHES)
        assert {c["scalars_kind"] for c in family} == set(M.SCALARS)
        assert {c["shift_kind"] for c in family} >= {"aligned", "z-shifted", "y-shifted", "x-shifted"}
    assert {c["shift_kind"] for c in hdia} == set(M.SHIFTS)
    # the tight pitch of the big shapes is odd: every second vector is off a 16-byte boundary
    assert H.N % 2 == 1 and M.pitch_of(letter, "tight", H.N) == H.N
    for kind in ("rounded", "rounded+5"):
        assert (M.pitch_of(letter, kind, H.N) * H.SIZEOF[letter] % 16 == 0) == (kind == "rounded")
    # every hack size meets every count but 1 (which is the SpMV's own test's) and every pitch
    assert {c["count"] for c in hdia if c["hp"] in M.HACKS and c["shape"] == (H.N, H.N)} >= set(M.COUNTS[1:])
    for hack in M.HACKS:
        mine = [c for c in hdia if c["hp"] == hack and c["shape"] == (H.N, H.N)]
        assert len({c["count"] for c in mine}) >= 3 and len({c["pitch"] for c in mine}) >= 2, hack


def test_the_operands_differ_from_vector_to_vector_and_vector_0_is_the_spmv_test_s():
    x0, y0 = M.operands("D", 300, 3, 0)
    hx, hy = H.operands("D", 300, 3)
    assert x0.tobytes() == hx.tobytes() and y0.tobytes() == hy.tobytes()
    x1, y1 = M.operands("D", 300, 3, 1)
    assert not np.array_equal(x0, x1) and not np.array_equal(y0, y1)
