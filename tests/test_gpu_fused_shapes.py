"""GPU: the fused CG steps (include/spgpu/device_scalars.h, spgpu_amd/csrc/fused_solver.hip: spgpu{S,D}hellspmvDotDevice and
spgpu{S,D}axpbyPairDotDevice) on every kernel shape and branch their dispatch can choose.  The case table, the dispatch restated and the
inputs are tests/fused_launch_shapes.py; tests/test_fused_launch_shapes.py checks on the CPU that the table reaches every branch.

Each case asserts
  * the library's own bit contract: z byte for byte the oracle's one-phase HELL SpMV (whichever of strip or gather ran), z1 and z2
    byte for byte what two spgpu?axpbyQuotDevice calls leave, *result byte for byte spgpu?dotDevice on the stored vectors;
  * a reference that shares no code with the library: the inputs are integer-valued (matrix values in -2 ... 2, vectors from
    exact_ref.integer_vector, integer coefficients, an exact integer quotient), every product and partial sum is exact in any order
    while the sum of term magnitudes stays below 2^24 / 2^53 (asserted on the inputs), so z, z1, z2 and *result must EQUAL int64
    arithmetic in numpy;
  * for the ragged, real-valued matrices instead: z within exact_ref's bound of the long double product;
  * around every output the elements before its start and after its end keep a sentinel."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import fused_launch_shapes as M
import oracle_api as O

pytestmark = pytest.mark.gpu

TABLE = {L: M.cases(L) for L in M.LETTERS}
SENTINEL = -12345.0
LEAD, TRAIL = 8, 8             # sentinel elements around every device array; 8 elements keep the 16-byte boundary where it was
_RAISED = []                   # a call or a synchronisation that raised: no later case touches the GPU


def _ids(call):
    return [pytest.param(L, cid, id=f"{L}-{cid}") for L in M.LETTERS for cid, c in TABLE[L].items() if c["call"] == call]


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _start():
    if _RAISED:
        pytest.fail(f"not started: {_RAISED[0]} raised on the GPU before")


def _guard(cid, fn, *args):
    """One library call, then a synchronisation; whatever either raises stops every later case."""
    import torch
    try:
        fn(*args)
        torch.cuda.synchronize()
    except BaseException:
        _RAISED.append(cid)
        raise


def _place(host, off):
    """A host array on the device `off` elements past a 16-byte boundary, sentinels before and after: (whole buffer, the array)."""
    import torch
    host = np.ascontiguousarray(host)
    whole = np.full(LEAD + off + host.size + TRAIL, SENTINEL, host.dtype)
    whole[LEAD + off:LEAD + off + host.size] = host
    buf = torch.from_numpy(whole).to("cuda:0")
    view = buf[LEAD + off:LEAD + off + host.size]
    assert view.data_ptr() % 16 == off * host.dtype.itemsize % 16, "the allocator moved the 16-byte boundary"
    return buf, view


def _assert_margins(buf, off, n, what):
    whole = buf.cpu().numpy()
    assert np.all(whole[:LEAD + off] == SENTINEL), f"{what}: written before its start"
    assert np.all(whole[LEAD + off + n:] == SENTINEL), f"{what}: written past its end"
    return whole[LEAD + off:LEAD + off + n]


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        word = np.uint32 if got.dtype.itemsize == 4 else np.uint64
        at = int(np.flatnonzero(got.view(word) != want.view(word))[0])
        raise AssertionError(f"{what}: differs at element {at} of {got.size}: got {got[at]!r}, want {want[at]!r}")


def _real(letter, seed, n):
    return np.random.default_rng(seed).standard_normal(n, dtype=X.REAL_OF[letter])


def _equals_integers(got, want, what):
    got = np.asarray(got)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: {np.count_nonzero(got != want)} of {got.size} differ from int64 arithmetic, first at {at}: "
                             f"got {got[at]!r}, want {want[at]}")


@pytest.mark.parametrize("letter,cid", _ids("spmv"))
def test_hellspmv_dot_device(gpu, letter, cid):
    import torch
    from spgpu_amd import capi
    _start()
    case = TABLE[letter][cid]
    n, hack, base, off = case["rows"], case["hack"], case["base"], case["off"]
    real = X.REAL_OF[letter]
    out = torch.full((1,), float("nan"), dtype=getattr(torch, np.dtype(real).name), device="cuda:0")
    if n == 0:                                       # no first stage: *result = 0, nothing else is touched
        z_buf, dz = _place(np.zeros(4, real), 0)
        dz.fill_(SENTINEL)
        _guard(cid, capi.hellspmv_dot_device[letter], gpu, _p(out), _p(dz), _p(dz), _p(dz), capi.scalar(letter, M.ALPHA), _p(dz),
               _p(dz), hack, _p(dz), _p(dz), 0, _p(dz), capi.scalar(letter, M.BETA), base)
        assert out.cpu().numpy()[0] == 0 and np.all(z_buf.cpu().numpy() == SENTINEL)
        return
    hell, x, w, y = M.spmv_inputs(case)
    alpha, beta = M.coefficients(case)
    assert M.reached(case) == case["want"]
    _, cM = _place(hell["values"], off["cM"])
    _, rP = _place(hell["indices"], off["rP"])
    _, rS = _place(hell["row_lengths"], off["rS"])
    hack_offsets = torch.from_numpy(np.ascontiguousarray(hell["hack_offsets"])).to("cuda:0")

    def run(x, w, y, alpha, beta, what):
        """One call on operands placed as the case says; the margins and the library's bit contract; (z, *result)."""
        _, dx = _place(x, off["x"])
        dw = None if w is None else _place(w, off["w"])[1]
        y_dev = y if case["beta"] else np.full(n, np.nan, real)          # beta == 0: y is full of NaN and must not be read
        if case["z_is_y"]:
            z_buf, dz = _place(y_dev, off["z"])
            dy = dz
        else:
            z_buf, dz = _place(np.full(n, SENTINEL, real), off["z"])
            dy = _place(y_dev, off["y"])[1]
        out.fill_(float("nan"))
        _guard(cid, capi.hellspmv_dot_device[letter], gpu, _p(out), _p(dw), _p(dz), _p(dy), capi.scalar(letter, alpha), _p(cM), _p(rP),
               hack, _p(hack_offsets), _p(rS), n, _p(dx), capi.scalar(letter, beta), base)
        got_z = _assert_margins(z_buf, off["z"], n, f"{what}: z")
        got = out.cpu().numpy()[0]
        _same_bytes(got_z, O.hell_spmv(hell, x, y, alpha, beta, phases=1), f"{what}: z against the one-phase oracle")
        ref = torch.full_like(out, float("nan"))
        _guard(cid, capi.dot_device[letter], gpu, _p(ref), n, _p(dx if dw is None else dw), _p(dz))
        assert got.tobytes() == ref.cpu().numpy()[0].tobytes(), f"{what}: *result {got!r}, spgpu?dotDevice(w, z) {ref.cpu().numpy()[0]!r}"
        return got_z, got

    got_z, got = run(x, w, y, alpha, beta, cid)
    if case["exact"]:
        # a reference outside the library
        z_int, dot_int, sums = M.spmv_exact(case, hell, x, w, y)
        X.assert_sums_exact(letter, sums)
        _equals_integers(got_z, z_int, f"{cid}: z")
        assert float(got) == dot_int, f"{cid}: *result {got!r}, the integer is {dot_int}"
        if n <= M.REAL_PASS_MAX:
            # the bit contract once more on vectors that round (integers add to the same bits on any grid); the capped sizes leave
            # this to the cost of a second oracle product
            rx, rw, ry = (_real(letter, 7 + i, n) for i in range(3))
            run(rx, None if w is None else rw, ry if case["beta"] else None, M.RAGGED_ALPHA, M.RAGGED_BETA if case["beta"] else 0.0,
                f"{cid} (real vectors)")
    else:
        want, scale = X.spmv(n, *X.hell_coo(hell), x, y, alpha, beta, base=hell["base"])
        X.assert_within(got_z, want, scale, letter, case=cid)
        ww = (x if w is None else w).astype(np.longdouble)
        zz = got_z.astype(np.longdouble)
        assert abs(np.longdouble(got) - np.sum(ww * zz)) <= n * X.EPS[letter] * np.sum(np.abs(ww * zz)) + X.TINY, f"{cid}: *result"


@pytest.mark.parametrize("letter,cid", _ids("pair"))
def test_axpby_pair_dot_device(gpu, letter, cid):
    import torch
    from spgpu_amd import capi, formats
    _start()
    case = TABLE[letter][cid]
    n, off = case["n"], case["off"]
    real = X.REAL_OF[letter]
    out = torch.full((1,), float("nan"), dtype=getattr(torch, np.dtype(real).name), device="cuda:0")
    num, den = M.QUOTIENTS[case["form"]]
    scal = formats.to_device(np.array([num or 0.0, den or 0.0], real))
    p_num, p_den = (_p(scal[0:]) if num is not None else None), (_p(scal[1:]) if den is not None else None)
    if n == 0:
        z_buf, dz = _place(np.full(4, SENTINEL, real), 0)
        _guard(cid, capi.axpby_pair_dot_device[letter], gpu, _p(out), 0, _p(dz), _p(dz), _p(dz), _p(dz), _p(dz), _p(dz), p_num, p_den)
        assert out.cpu().numpy()[0] == 0 and np.all(z_buf.cpu().numpy() == SENTINEL)
        return
    assert M.reached(case) == case["want"]

    def run(x1, y1, x2, y2, what):
        """One call on operands placed as the case says; the margins and the library's bit contract; (z1, z2, *result)."""
        # what the separate calls leave (element-wise: the same bits wherever the operands lie)
        ax1, ay1, ax2, ay2 = (formats.to_device(v) for v in (x1, y1, x2, y2))
        want1, want2 = torch.empty_like(ax1), torch.empty_like(ax1)
        _guard(cid, capi.axpby_quot_device[letter], gpu, _p(want1), n, None, None, _p(ay1), p_num, p_den, 0, _p(ax1))
        _guard(cid, capi.axpby_quot_device[letter], gpu, _p(want2), n, None, None, _p(ay2), p_num, p_den, 1, _p(ax2))
        dx1, dx2 = _place(x1, off["x1"])[1], _place(x2, off["x2"])[1]
        if case["in_place"]:
            z1_buf, dz1 = _place(y1, off["z1"])
            z2_buf, dz2 = _place(y2, off["z2"])
            dy1, dy2 = dz1, dz2
        else:
            z1_buf, dz1 = _place(np.full(n, SENTINEL, real), off["z1"])
            z2_buf, dz2 = _place(np.full(n, SENTINEL, real), off["z2"])
            dy1, dy2 = _place(y1, off["y1"])[1], _place(y2, off["y2"])[1]
        out.fill_(float("nan"))
        _guard(cid, capi.axpby_pair_dot_device[letter], gpu, _p(out), n, _p(dz1), _p(dy1), _p(dx1), _p(dz2), _p(dy2), _p(dx2), p_num, p_den)
        got1 = _assert_margins(z1_buf, off["z1"], n, f"{what}: z1")
        got2 = _assert_margins(z2_buf, off["z2"], n, f"{what}: z2")
        got = out.cpu().numpy()[0]
        _same_bytes(got1, want1.cpu().numpy(), f"{what}: z1 against spgpu?axpbyQuotDevice")
        _same_bytes(got2, want2.cpu().numpy(), f"{what}: z2 against spgpu?axpbyQuotDevice")
        ref = torch.full_like(out, float("nan"))
        _guard(cid, capi.dot_device[letter], gpu, _p(ref), n, _p(dz2), _p(dz2))
        assert got.tobytes() == ref.cpu().numpy()[0].tobytes(), f"{what}: *result {got!r}, spgpu?dotDevice(z2, z2) {ref.cpu().numpy()[0]!r}"
        return got1, got2, got

    x1, y1, x2, y2 = M.pair_inputs(case)
    got1, got2, got = run(x1, y1, x2, y2, cid)
    # a reference outside the library
    z1_int, z2_int, dot_int, sums = M.pair_exact(case, x1, y1, x2, y2)
    X.assert_sums_exact(letter, sums)
    _equals_integers(got1, z1_int, f"{cid}: z1")
    _equals_integers(got2, z2_int, f"{cid}: z2")
    assert float(got) == dot_int, f"{cid}: *result {got!r}, the integer is {dot_int}"
    # the bit contract once more on vectors that round: integers add to the same bits on any grid, these do not
    run(*(_real(letter, 11 + i, n) for i in range(4)), f"{cid} (real vectors)")
