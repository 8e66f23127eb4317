"""CPU: the matrices and the case table of tests/test_gpu_spmm_shapes.py (tests/spmm_launch_shapes.py) are what that module needs
them to be -- the column windows lie on the intended side of every tile size, the table names every instantiation either dispatch
can return, and the extended-precision reference of every matrix is finite with few elements of zero scale."""
import numpy as np
import pytest

import exact_ref as X
import spmm_launch_shapes as S

MATRICES = [(name, base) for name in S.NAMED for base in (0, 1)]


@pytest.fixture(scope="module")
def made():
    return {key: S.matrix(*key) for key in MATRICES}


def test_constants_give_the_tile_sizes_the_source_states():
    assert S.strip_tile_rows("D", 2) == 320 and S.strip_tile_rows("S", 1) == 1280
    assert S.tiled_tile_rows("D") == 344 and S.tiled_tile_rows("S") == 688
    assert S.mv_strip_tile_rows("D", 2) == 319 and S.mv_strip_tile_rows("S", 1) == 1277
    assert S.ROWS == 613 and len(S.workgroups()) == 3 and S.workgroups()[-1] == (512, 613)


@pytest.mark.parametrize("base", [0, 1])
def test_shape_of_the_rows(made, base):
    for name in ("mixed", "band", "narrow"):
        m = made[name, base]
        L = m["lengths"]
        assert L.shape == (S.ROWS,) and L.min() == 0 and S.SLAB_HEAD < L.max() <= S.MAX_LEN
        assert int(L.sum()) == m["rows"].size == m["cols"].size
        assert np.array_equal(m["rows"], np.repeat(np.arange(S.ROWS), L))
        assert not L[S.EMPTY_WAVE * S.WAVE:(S.EMPTY_WAVE + 1) * S.WAVE].any()
        assert np.all(L[S.UNIFORM_WAVE * S.WAVE:(S.UNIFORM_WAVE + 1) * S.WAVE] == S.UNIFORM_LEN)
        assert np.count_nonzero(L == 0) > S.WAVE                      # empty rows sprinkled beside the empty wavefront
        if name != "band":
            assert {int(n) % 4 for n in L} == {0, 1, 2, 3}             # a ragged last trip for every UNROLL
        assert m["cols"].min() >= 1 and m["cols"].max() < S.COLS       # column 0 is named nowhere
        assert m["hole"].any() == (base == 1)
        if base == 1:
            first = np.cumsum(L) - L
            assert not m["hole"][first[L > 0]].any()
            assert not m["hole"][m["rows"] // S.WAVE == S.UNIFORM_WAVE].any()


@pytest.mark.parametrize("base", [0, 1])
def test_windows_lie_on_the_intended_side_of_every_tile(made, base):
    smallest, largest = S.all_tile_rows()[0], S.all_tile_rows()[-1]
    assert S.NARROW_WINDOW < smallest and S.WIDE_SPREAD > largest and S.PROBE_SPREAD < smallest
    for name, patterns in S.NAMED.items():
        m = made[name, base]
        for g, kind in enumerate(patterns):
            w, first = S.window_of(m, g), S.window_of(m, g, first_only=True)
            if kind == "empty":
                assert w is None
            elif kind in ("narrow", "band"):
                assert w[1] - w[0] + 16 // 4 - 1 < smallest, (name, g, w)   # + the rounding of the pitch layout's low end
            else:
                assert w[1] - w[0] > S.WIDE_SPREAD > largest, (name, g, w)
                if kind == "wide_after_scan":
                    assert first[1] - first[0] < S.PROBE_SPREAD, (name, g, first)
                    # and what the strip kernel sees before it scans, the first SLAB_HEAD slab columns, fits too
                    lo, hi = S.workgroups()[g]
                    k = np.arange(m["rows"].size) - np.repeat(np.cumsum(m["lengths"]) - m["lengths"], m["lengths"])
                    sel = (m["rows"] >= lo) & (m["rows"] < hi) & (k < S.SLAB_HEAD)
                    assert np.ptp(m["cols"][sel]) < smallest
                    assert np.ptp(m["cols"][sel & ~m["hole"]]) < smallest
                else:
                    assert first[1] - first[0] > S.WIDE_SPREAD, (name, g, first)


def test_band_wavefronts_are_bands(made):
    """Whole wavefronts of equal rows, a multiple of 8 and at most 32 long, row r + 1 = row r shifted by one -- in both bases (the
    holes stay out of them) -- beside ragged ones."""
    for base in (0, 1):
        m = made["band", base]
        bands = 0
        for w0 in range(0, S.ROWS - S.WAVE + 1, S.WAVE):
            L = m["lengths"][w0:w0 + S.WAVE]
            sel = (m["rows"] >= w0) & (m["rows"] < w0 + S.WAVE)
            if L[0] > 0 and np.all(L == L[0]) and L[0] % 8 == 0 and L[0] <= S.SLAB_HEAD and not m["hole"][sel].any():
                c = m["cols"][sel].reshape(S.WAVE, L[0])
                assert np.array_equal(c, c[0, 0] + np.arange(S.WAVE)[:, None] + np.arange(L[0])[None, :])
                bands += 1
        assert bands >= 5
        assert len({int(m["lengths"][w0]) for w0 in range(0, S.ROWS, S.WAVE)}) >= 4


@pytest.mark.parametrize("letter", "SD")
def test_case_table_names_every_instantiation(letter):
    seen = set()
    for cid, c in S.interleaved_cases(letter).items():
        for beta in c["betas"]:
            got = S.interleaved_passes(letter, c["hack"], c["count"], c["ldx"], c["ldyz"], False, S.offsets(letter, c["shift"]), beta != 0)
            assert got == S.expected_passes(letter, c), (cid, beta)
            seen.update(got)
    for name in S.every_interleaved_instantiation(letter):
        flags = {flag for n, flag in seen if n == name}
        assert flags == ({True, False} if "Strip" in name else {None}), name
    for cid in S.ONE_EACH:
        assert cid in S.interleaved_cases(letter)
    one_each = {S.expected_passes(letter, S.interleaved_cases(letter)[cid])[0][0] for cid in S.ONE_EACH}
    assert one_each == set(S.every_interleaved_instantiation(letter))
    seen = set()
    for cid, c in S.mv_cases(letter).items():
        px, pz = S.mv_pitches(letter, c)
        assert px >= S.COLS and pz >= S.ROWS
        for beta in c["betas"]:
            got = S.mv_passes(letter, c["hack"], c["count"], px, pz, c["r_idx"], S.offsets(letter, c["shift"]), beta != 0)
            assert got == S.expected_passes(letter, c, pitch=True), (cid, beta)
            seen.update(got)
    for name in S.every_mv_instantiation(letter):
        assert {flag for n, flag in seen if n == name} == {True, False}, name


def test_dispatch_restated_on_a_few_hand_worked_calls():
    assert S.interleaved_passes("D", 32, 21, 21, 21) == [(S.plain_name("D", 16, 1, 2), None), (S.strip_name("D", 1), False)]
    assert S.interleaved_passes("S", 48, 6, 6, 6) == [(S.plain_name("S", 4, 2, 4), None)]
    assert S.interleaved_passes("S", 32, 16, 16, 16, off=dict(S.ALIGNED, Y=4), has_y=False) == [(S.strip_name("S", 2), True)]
    assert S.mv_passes("D", 32, 16, 4000, 616, r_idx=True) == [(S.strip_name("D", 2, True), False)]


@pytest.mark.parametrize("letter", "SD")
def test_exact_reference_is_finite_and_rarely_without_scale(made, letter):
    count = 5
    for (name, base), m in made.items():
        r, c = S.used(m)
        v = S.values(letter, 1, m["rows"].size)[~m["hole"]]
        Xk = S.values(letter, 2, S.COLS * count).reshape(S.COLS, count)
        Yk = S.values(letter, 3, S.ROWS * count).reshape(S.ROWS, count)
        has_entries = np.zeros(S.ROWS, bool)
        has_entries[r] = True
        for beta in (0.0, 0.5):
            exact, scale = X.spmm(S.ROWS, r, c, v, Xk, Yk if beta else None, -1.5, beta, count)
            assert np.isfinite(exact.astype(np.float64)).all() and np.isfinite(scale).all()
            zero = scale == 0
            # no scale only where a row has no entries and no beta*y: there the result is an exact zero and `tiny` is the bound
            assert np.array_equal(zero, np.broadcast_to((~has_entries)[:, None] & (beta == 0), zero.shape)), (name, base, beta)
            if "empty" not in S.NAMED[name]:
                assert zero.mean() <= S.ZERO_SCALE_CAP, (name, base, beta, zero.mean())
