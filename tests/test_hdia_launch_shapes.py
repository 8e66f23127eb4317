"""CPU: the hand-built matrices and the case table of tests/test_gpu_hdia_shapes.py (tests/hdia_launch_shapes.py) are what that
module needs them to be -- the table names all seven instantiations of hdiaSpmvKernel for HDIA and for DIA and both values of
wideIO, every case takes the branches it is in the table for (the kernel's control flow walked on the CPU), the table as a whole
takes every branch every instantiation can reach, and on every matrix the oracle, reading the NaN-poisoned arrays, returns no NaN
and agrees with the extended-precision sum of the matrix' COO triplets: fixtures and references agree before a GPU is involved."""
import zlib

import numpy as np
import pytest

import exact_ref as X
import hdia_launch_shapes as H
import oracle_api as O
from test_gpu_fuzz import _complex_scalars


def test_constants_give_the_launch_shapes_the_source_states():
    assert H.WIDE == {"S": 4, "D": 2, "C": 2, "Z": 1}
    assert H.THREADS * H.WIDE["S"] == 2048 and H.N == 2 * 2048 + 256 + 151 and H.N % 4 == 3
    assert H.N == 4 * 1024 + 3 * 128 + 23
    assert len(H.every_instantiation()) == 7 and H.kernel_name("C", 2) == "hdiaSpmvKernel<spgpu::Cx<float>, 2>"
    assert H.dia_alloc_pitch(H.N) == 4512 and H.dia_pitches("S", H.N) == (4512, 4544, 4503, 4504)
    assert H.dia_pitches("Z", H.N)[3] == H.N


def test_dispatch_restated_on_a_few_hand_worked_calls():
    assert H.dispatch("S", 32) == (4, 1) and H.dispatch("S", 30) == (1, 1) and H.dispatch("D", 30) == (2, 1)
    assert H.dispatch("S", 32, dict(H.ALIGNED, dM=4)) == (1, 1)
    assert H.dispatch("D", 32, dict(H.ALIGNED, z=8)) == (2, 0) and H.dispatch("C", 32, dict(H.ALIGNED, y=8)) == (2, 0)
    assert H.dispatch("C", 32, dict(H.ALIGNED, y=8), has_y=False) == (2, 1)
    assert H.dispatch("S", 32, dict(H.ALIGNED, x=4)) == (4, 1)
    assert H.dispatch("Z", 32) == (1, 1) and H.dispatch("Z", 32, H.offsets_of("Z", ("dM", "z"))) == (1, 1)
    assert H.dispatch("S", 4503) == (1, 1) and H.dispatch("S", 4504) == (4, 1) and H.dispatch("D", 4503) == (1, 1)
    for letter in "SDC":
        for hack in H.HACKS:
            assert (H.dispatch(letter, hack)[0] > 1) == (hack in H.WIDE_HACKS[letter])


def test_builders_poison_exactly_the_slots_no_product_uses():
    m = H.hdia_matrix("D", 11, 9, 4, [[-2, 0, 3], [], [-10, 1]])
    assert m["hack_offsets"].tolist() == [0, 3, 3, 5] and m["offsets"].tolist() == [-2, 0, 3, -10, 1]
    v = m["values"].reshape(5, 4)
    # hack 0 (rows 0-3): offset -2 leaves rows 0, 1 outside; hack 2 (rows 8-10 and a row past the matrix): -10 leaves only row 10,
    # +1 leaves none of rows 8-10 inside 9 columns
    assert np.isnan(v).tolist() == [[True, True, False, False], [False] * 4, [False] * 4, [True, True, False, True], [True] * 4]
    r, c, vals = m["coo"]
    assert r.tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 10] and c.tolist() == [0, 3, 1, 4, 0, 2, 5, 1, 3, 6, 0]
    assert vals.tolist() == [v[1, 0], v[2, 0], v[1, 1], v[2, 1], v[0, 2], v[1, 2], v[2, 2], v[0, 3], v[1, 3], v[2, 3], v[3, 2]]
    d = H.dia_matrix("C", 5, 4, 7, [-1, 2])
    w = d["values"].reshape(2, 7)
    assert np.isnan(w).tolist() == [[True, False, False, False, False, True, True], [False, False, True, True, True, True, True]]
    assert d["coo"][0].tolist() == [0, 1, 1, 2, 3, 4] and d["coo"][1].tolist() == [2, 0, 3, 1, 2, 3]
    assert np.array_equal(d["coo"][2], [w[1, 0], w[0, 1], w[1, 1], w[0, 2], w[0, 3], w[0, 4]])
    assert np.isnan(w[0, 0].imag) and np.isnan(w[0, 0].real)


def test_branch_walk_on_a_call_worked_by_hand():
    """Double, wide (two rows per lane), 11 x 9, hack 4, hacks of 3, 0 and 2 diagonals: one wavefront of six live lanes."""
    m = H.hdia_matrix("D", 11, 9, 4, [[-2, 0, 3], [], [-10, 1]])
    n = H.branches(m, "D", 2, 1, True)
    assert n["wave_exit"] == 7 and n["dead_lanes"] == 58 and n["wave_no_diags"] == 0 and n["wave_mixed_counts"] == 1
    assert (n["stages"], n["stage_whole"], n["stage_guarded"], n["wave_three_stages"]) == (1, 0, 1, 0)
    assert (n["x_wide"], n["x_elem_edge"], n["x_elem_small_cols"]) == (0, 1, 0)
    assert (n["store_wide"], n["store_elem_partial_strip"], n["store_elem_no_wideio"]) == (5, 1, 0)
    # col < 0: rows 0, 1 at -2 and rows 8, 9 at -10; col >= cols: rows 8, 9, 10, (11) at +1; row 11 at both diagonals of its hack
    assert (n["mask_col_low"], n["mask_col_high"], n["mask_row"]) == (2 + 2, 4, 2)
    n = H.branches(m, "D", 2, 0, False)
    assert (n["store_wide"], n["store_elem_partial_strip"], n["store_elem_no_wideio"], n["y_read"]) == (0, 0, 6, 0)
    n = H.branches(m, "D", 1, 1, True)
    assert n["wave_exit"] == 7 and n["dead_lanes"] == 53 and n["mask_row"] == 0 and n["store_narrow"] == 11
    # an interior wavefront: rows 128 .. 255 of a 600-row band, offsets odd and even
    band = H.dia_matrix("D", 600, 600, 608, [-3, 0, 2, 5])
    n = H.branches(band, "D", 2, 1, False)
    assert n["stage_whole"] == 4 and n["stage_guarded"] == 1                  # five wavefronts, the last with dead lanes
    assert n["x_wide"] == 3 and n["x_wide_unaligned"] == 3 and n["x_elem_edge"] == 2   # the first and the last touch an edge
    even = H.dia_matrix("D", 600, 600, 608, [-4, 0, 2])
    assert H.branches(even, "D", 2, 1, False)["x_wide_unaligned"] == 0
    assert H.branches(even, "D", 2, 1, False, x_off=8)["x_wide_unaligned"] == 3


@pytest.mark.parametrize("letter", "SDCZ")
def test_every_case_takes_the_route_and_the_branches_it_claims(letter):
    table = H.cases(letter)
    kinds = {(c["fmt"], c["kind"]) for c in table.values()}
    assert kinds >= {(fmt, kind) for fmt in ("hdia", "dia") for kind in H.PLACEMENTS}
    for cid, c in table.items():
        off = H.offsets_of(letter, c["shift"])
        y_off = off["z"] if c["y_mode"] == "z" else off["y"]
        assert H.dispatch(letter, c["hp"], dict(off, y=y_off), c["y_mode"] != "null") == c["want"], cid
        assert c["want"] == H.route_rpl_io(letter, c["route"])
        n = H.case_branches(c)
        for claim in c["claims"]:
            assert n[claim] > 0, (cid, claim)
        assert c["claims"], cid
        assert all(claim in H.reachable(c["fmt"], c["want"][0]) for claim in c["claims"]), cid


def test_table_names_every_instantiation_and_both_kinds_of_store():
    for fmt in ("hdia", "dia"):
        seen = {(H.kernel_name(L, c["want"][0]), c["want"][1]) for L in "SDCZ" for c in H.cases(L).values() if c["fmt"] == fmt}
        assert {name for name, _ in seen} == set(H.every_instantiation()), fmt
        for letter in "SDC":
            assert {io for name, io in seen if name == H.kernel_name(letter, H.WIDE[letter])} == {0, 1}, (fmt, letter)


@pytest.mark.parametrize("letter", "SDCZ")
def test_table_reaches_every_branch_every_instantiation_can_reach(letter):
    """Per format and instantiation, every branch of H.BRANCHES but those H.NARROW_HAS_NO and H.DIA_HAS_NO name is taken by at
    least one case; and those the lists name are taken by none, so the lists say no more than is true."""
    taken = {}
    for c in H.cases(letter).values():
        n = H.case_branches(c)
        taken.setdefault((c["fmt"], c["want"][0]), set()).update(b for b in H.BRANCHES if n[b] > 0)
    assert set(taken) == {(fmt, rpl) for fmt in ("hdia", "dia") for rpl in {H.WIDE[letter], 1}}
    for (fmt, rpl), got in taken.items():
        assert got == set(H.reachable(fmt, rpl)), (fmt, rpl, set(H.reachable(fmt, rpl)) ^ got)


def test_hack_programmes_hold_the_counts_and_offsets_the_issue_lists():
    for hack in H.HACKS[:-1]:
        counts = [len(o) for o in H.programme("cycle", H.N, H.N, hack)]
        assert set(counts) == set(H.CYCLE) if len(counts) >= 9 * 5 else set(counts) <= set(H.CYCLE)
        runs = H.programme("runs", H.N, H.N, hack)
        for run, want in enumerate(H.RUN_COUNTS):
            first, last = -(-run * H.RUN // hack), ((run + 1) * H.RUN - 1) // hack
            assert {len(o) for o in runs[first:last + 1]} == {want}
            assert (last + 1) * hack - first * hack >= 256 + 255       # a whole S wavefront lies inside, wherever it starts
        inner = H.programme("interior", H.N, H.N, hack)
        assert {len(o) for o in inner} == set(H.INTERIOR_COUNTS) or hack > 96
        assert any(o % 2 for one in inner for o in one) and max(abs(o) for one in inner for o in one) <= 41
    cand = H.candidates(H.N, H.N)
    assert set(range(-3, 4)) <= set(cand) and {-(H.N - 1), H.N - 1, 100, 101} <= set(cand) and len(cand) >= 13
    assert len(H.programme("cycle", H.N, H.N, 4512)[0]) == 13
    edge = H.dia_offsets(("edge", 13), H.N, H.N)
    assert len(edge) == 13 and {-(H.N - 1), H.N - 1, 1, -1} <= set(edge)


@pytest.mark.parametrize("letter", "SDCZ")
def test_oracle_on_the_poisoned_arrays_is_finite_and_within_the_bound_of_the_exact_sums(letter):
    done = set()
    for c in H.cases(letter).values():
        key = H.matrix_key(c)
        if key in done:
            continue
        done.add(key)
        m = H.matrix_of(c)
        rows, cols = c["shape"]
        x, y = H.operands(letter, rows, cols)
        r, cc, v = m["coo"]
        stored = m["values"][:(m["height"] * m["hack_size"]) if c["fmt"] == "hdia" else (m["diags"] * m["pitch"])]
        assert np.count_nonzero(~np.isnan(stored)) == v.size and (v != 0).all()
        alpha, beta = _complex_scalars(zlib.crc32(repr(key).encode()), letter, *H.WITH_Y)
        got = (O.hdia_spmv if c["fmt"] == "hdia" else O.dia_spmv)(m, x, y, alpha, beta)
        assert not np.isnan(got).any(), key
        want, scale = X.spmv(rows, r, cc, v, x, y, alpha, beta)
        X.assert_within(got, want, scale, letter, key)
        if c["fmt"] == "dia":
            assert O.hdia_spmv(H.as_one_hack(m), x, y, alpha, beta).tobytes() == got.tobytes(), key
    assert len(done) > 60
