"""GPU: the Jacobi steps of PCG fused into the device-scalar calls (include/spgpu/ext/precond.h, spgpu_amd/csrc/fused_solver.hip:
spgpu{S,D}axyDotDevice, spgpu{S,D}axpbyPairAxyDotDevice and their m-forms on pitch multivectors).

Each single-vector case asserts
  * the header's bit contract against the existing calls run on the GPU on the same inputs: z (w) byte for byte spgpu?axy at
    alpha = 1, z1 / z2 / result[1] byte for byte spgpu?axpbyPairDotDevice, *result (result[0]) byte for byte spgpu?dotDevice on the
    stored vectors -- for a w off the 16-byte boundary under an aligned z2, on a copy of the stored w that lies as z2 does, which is
    what the header promises there;
  * a reference that shares no code with the library: integer-valued inputs (exact_ref.integer_vector), an exact integer
    quotient, the sums of term magnitudes asserted below 2^24 / 2^53, so every vector and result must EQUAL int64 arithmetic;
  * sentinels around every output.
The multivector cases assert every vector byte for byte against the single-vector call on that vector, result[] against
spgpu?mdotDevice / spgpu?maxpbyPairDotDevice, and the sentinels in the gaps between the vectors and behind the last one; the cases
with hundreds of vectors use integer inputs and int64 arithmetic for the vectors instead of a call per vector."""
import numpy as np
import pytest

import exact_ref as X
import fused_launch_shapes as M
import test_gpu_fused_shapes as F            # _start / _guard / _place / _assert_margins / _same_bytes: one list of raised calls for both files

pytestmark = pytest.mark.gpu

LETTERS = "SD"
TILE = {L: M.kL1Threads * M.kL1Unroll * M.WIDE[L] for L in LETTERS}        # elements of one Level-1 tile of 16-byte accesses
SIZES = {L: [1, 255, TILE[L], TILE[L] + 1, 3 * TILE[L] + 5] for L in LETTERS}
NUM, DEN = 6.0, -3.0                                                       # a = -2: z1 = y1 - 2 x1, z2 = y2 + 2 x2
A = int(NUM / DEN)
# operand -> elements past the 16-byte boundary
AXY_PLACES = {"aligned": {}, "d-off": {"d": 1}, "z-off": {"z": 1}, "dot-off": {"r": 1, "z": 1}}
PAIR_PLACES = {"aligned": {}, "d-off": {"d": 1}, "w-off": {"w": 1}, "dot-off": {"z2": 1, "y2": 1}, "all-off": {k: 1 for k in ("z1", "y1", "x1", "z2", "y2", "x2", "w", "d")}}
_p = F._p


def _torch_dtype(letter):
    import torch
    return torch.float32 if letter == "S" else torch.float64


def _scalars(letter, values):
    import torch
    return torch.tensor(values, dtype=_torch_dtype(letter), device="cuda:0")


def _result(letter, cells):
    import torch
    return torch.full((cells + 2,), F.SENTINEL, dtype=_torch_dtype(letter), device="cuda:0")   # two sentinel cells behind the results


def _cells(out, cells, what):
    got = out.cpu().numpy()
    assert np.all(got[cells:] == F.SENTINEL), f"{what}: result written past its {cells} cells"
    return got[:cells]


# ---- one vector ------------------------------------------------------------------------------------------------------------------
def _axy_dot(gpu, letter, cid, n, off, d, r):
    """One spgpu?axyDotDevice on operands placed as `off` says; the margins and the bit contract; (z, *result)."""
    from spgpu_amd import capi
    real = X.REAL_OF[letter]
    dd, dr = F._place(d, off.get("d", 0))[1], F._place(r, off.get("r", 0))[1]
    z_buf, dz = F._place(np.full(n, F.SENTINEL, real), off.get("z", 0))
    out = _result(letter, 1)
    F._guard(cid, capi.axy_dot_device[letter], gpu, _p(out), n, _p(dz), _p(dd), _p(dr))
    got_z, got = F._assert_margins(z_buf, off.get("z", 0), n, f"{cid}: z"), _cells(out, 1, cid)
    want_z, ref = F._place(np.full(n, F.SENTINEL, real), 0)[1], _result(letter, 1)
    F._guard(cid, capi.axy[letter], gpu, _p(want_z), n, capi.scalar(letter, 1.0), _p(dd), _p(dr))
    F._same_bytes(got_z, want_z.cpu().numpy(), f"{cid}: z against spgpu?axy")
    F._guard(cid, capi.dot_device[letter], gpu, _p(ref), n, _p(dr), _p(dz))
    F._same_bytes(got, _cells(ref, 1, cid), f"{cid}: *result against spgpu?dotDevice(r, z)")
    return got_z, got[0]


@pytest.mark.parametrize("place", AXY_PLACES)
@pytest.mark.parametrize("size", range(5))
@pytest.mark.parametrize("letter", LETTERS)
def test_axy_dot_device(gpu, letter, size, place):
    F._start()
    n, off = SIZES[letter][size], AXY_PLACES[place]
    cid = f"{letter}-axyDot-n{n}-{place}"
    d, r = X.integer_vector(letter, 31, n, density=0.5), X.integer_vector(letter, 32, n, density=0.5)
    got_z, got = _axy_dot(gpu, letter, cid, n, off, d, r)
    di, ri = X._ints(d)[0], X._ints(r)[0]
    X.assert_sums_exact(letter, dict(dot_terms=int(np.sum(np.abs(ri * ri * di)))))
    F._equals_integers(got_z, di * ri, f"{cid}: z")
    assert float(got) == int(np.sum(ri * ri * di)), f"{cid}: *result {got!r}"
    _axy_dot(gpu, letter, f"{cid} (real vectors)", n, off, F._real(letter, 41, n), F._real(letter, 42, n))


def _pair(gpu, letter, cid, n, off, in_place, x1, y1, x2, y2, d, num=NUM, den=DEN):
    """One spgpu?axpbyPairAxyDotDevice; the margins and the bit contract; (z1, z2, w, result[0], result[1])."""
    from spgpu_amd import capi
    real = X.REAL_OF[letter]
    o = lambda k: off.get(k, 0)
    scal = _scalars(letter, [num, den])
    p_num, p_den = _p(scal[0:]), _p(scal[1:])
    dx1, dx2, dd = F._place(x1, o("x1"))[1], F._place(x2, o("x2"))[1], F._place(d, o("d"))[1]
    if in_place:
        (z1_buf, dz1), (z2_buf, dz2) = F._place(y1, o("z1")), F._place(y2, o("z2"))
        dy1, dy2 = dz1, dz2
    else:
        (z1_buf, dz1), (z2_buf, dz2) = F._place(np.full(n, F.SENTINEL, real), o("z1")), F._place(np.full(n, F.SENTINEL, real), o("z2"))
        dy1, dy2 = F._place(y1, o("y1"))[1], F._place(y2, o("y2"))[1]
    w_buf, dw = F._place(np.full(n, F.SENTINEL, real), o("w"))
    out = _result(letter, 2)
    F._guard(cid, capi.axpby_pair_axy_dot_device[letter], gpu, _p(out), n, _p(dz1), _p(dy1), _p(dx1), _p(dz2), _p(dy2), _p(dx2), _p(dw),
             _p(dd), p_num, p_den)
    got1, got2 = F._assert_margins(z1_buf, o("z1"), n, f"{cid}: z1"), F._assert_margins(z2_buf, o("z2"), n, f"{cid}: z2")
    got_w, got = F._assert_margins(w_buf, o("w"), n, f"{cid}: w"), _cells(out, 2, cid)
    # spgpu?axpbyPairDotDevice on operands that lie the same way
    (_, rz1), (_, rz2), ref = F._place(y1, o("z1")), F._place(y2, o("z2")), _result(letter, 1)
    F._guard(cid, capi.axpby_pair_dot_device[letter], gpu, _p(ref), n, _p(rz1), _p(rz1), _p(dx1), _p(rz2), _p(rz2), _p(dx2), p_num, p_den)
    F._same_bytes(got1, rz1.cpu().numpy(), f"{cid}: z1 against spgpu?axpbyPairDotDevice")
    F._same_bytes(got2, rz2.cpu().numpy(), f"{cid}: z2 against spgpu?axpbyPairDotDevice")
    F._same_bytes(got[1:], _cells(ref, 1, cid), f"{cid}: result[1] against spgpu?axpbyPairDotDevice")
    want_w = F._place(np.full(n, F.SENTINEL, real), 0)[1]
    F._guard(cid, capi.axy[letter], gpu, _p(want_w), n, capi.scalar(letter, 1.0), _p(dd), _p(dz2))
    F._same_bytes(got_w, want_w.cpu().numpy(), f"{cid}: w against spgpu?axy")
    # spgpu?dotDevice(z2, w): on w itself unless w alone left the boundary (the header: then on a copy of w that lies as z2 does)
    w_ref = dw if not (o("z2") == 0 and o("w") != 0) else F._place(got_w, 0)[1]
    ref0 = _result(letter, 1)
    F._guard(cid, capi.dot_device[letter], gpu, _p(ref0), n, _p(dz2), _p(w_ref))
    F._same_bytes(got[:1], _cells(ref0, 1, cid), f"{cid}: result[0] against spgpu?dotDevice(z2, w)")
    return got1, got2, got_w, got[0], got[1]


def _pair_integers(letter, n, seed=500):
    k = dict(density=0.5)
    return (X.integer_vector(letter, seed, n, **k), X.integer_vector(letter, seed + 1, n, **k),
            X.integer_vector(letter, seed + 2, n, support_seed=seed + 4, **k), X.integer_vector(letter, seed + 3, n, support_seed=seed + 4, **k),
            X.integer_vector(letter, seed + 5, n, support_seed=seed + 4, **k))


def _pair_exact(letter, x1, y1, x2, y2, d):
    """(z1, z2, w, z2 . w, z2 . z2) in int64, the sums of term magnitudes asserted below the type's limit."""
    i = lambda v: X._ints(v)[0]
    z1, z2 = i(y1) + A * i(x1), i(y2) - A * i(x2)
    w = i(d) * z2
    m2 = np.abs(i(y2)) + abs(A) * np.abs(i(x2))
    X.assert_sums_exact(letter, dict(asum=int(max(m2.max(initial=0) * np.abs(i(d)).max(initial=0), (np.abs(i(y1)) + abs(A) * np.abs(i(x1))).max(initial=0))),
                                     nrm2sq=int(np.sum(m2 * m2)), dot_terms=int(np.sum(m2 * m2 * np.abs(i(d))))))
    return z1, z2, w, int(np.sum(z2 * w)), int(np.sum(z2 * z2))


@pytest.mark.parametrize("place", PAIR_PLACES)
@pytest.mark.parametrize("size", range(5))
@pytest.mark.parametrize("letter", LETTERS)
def test_axpby_pair_axy_dot_device(gpu, letter, size, place):
    F._start()
    n, off = SIZES[letter][size], PAIR_PLACES[place]
    in_place = size % 2 == 0
    cid = f"{letter}-pairAxyDot-n{n}-{place}"
    vectors = _pair_integers(letter, n)
    got1, got2, got_w, zw, zz = _pair(gpu, letter, cid, n, off, in_place, *vectors)
    z1, z2, w, zw_int, zz_int = _pair_exact(letter, *vectors)
    F._equals_integers(got1, z1, f"{cid}: z1")
    F._equals_integers(got2, z2, f"{cid}: z2")
    F._equals_integers(got_w, w, f"{cid}: w")
    assert float(zw) == zw_int and float(zz) == zz_int, f"{cid}: result {zw!r}, {zz!r}; the integers are {zw_int}, {zz_int}"
    # the bit contract once more on vectors that round: integers add to the same bits on any grid, these do not
    _pair(gpu, letter, f"{cid} (real vectors)", n, off, in_place, *(F._real(letter, 51 + i, n) for i in range(5)), num=0.75, den=-1.25)


@pytest.mark.parametrize("letter", LETTERS)
def test_no_elements_leave_zero_results(gpu, letter):
    from spgpu_amd import capi
    F._start()
    z_buf, dz = F._place(np.full(4, F.SENTINEL, X.REAL_OF[letter]), 0)
    one, two, many = _result(letter, 1), _result(letter, 2), _result(letter, 6)
    F._guard("axyDot-n0", capi.axy_dot_device[letter], gpu, _p(one), 0, _p(dz), _p(dz), _p(dz))
    F._guard("pairAxyDot-n0", capi.axpby_pair_axy_dot_device[letter], gpu, _p(two), 0, *([_p(dz)] * 8), None, None)
    F._guard("mpairAxyDot-n0", capi.maxpby_pair_axy_dot_device[letter], gpu, _p(many), 0, *([_p(dz)] * 8), None, None, 3, 4)
    for out, cells in ((one, 1), (two, 2), (many, 6)):
        got = _cells(out, cells, "n = 0")
        assert np.all(got == 0) and not np.any(np.signbit(got))
    assert np.all(z_buf.cpu().numpy() == F.SENTINEL)


def test_the_cap_on_workgroups_binds(gpu):
    """fp32, n = 1024 * 4096 + 4096: 1025 tiles of 16-byte accesses for 1024 workgroups, about 17 MB per stream."""
    import torch
    from spgpu_amd import capi
    F._start()
    letter, n = "S", 1024 * 4096 + 4096
    assert M.SPGPU_REDUCE_MAX_BLOCKS == 1024 and -(-(n // M.WIDE[letter]) // (M.kL1Threads * M.kL1Unroll)) > M.SPGPU_REDUCE_MAX_BLOCKS
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    x, r0, ap, p, d = (torch.randn(n, dtype=torch.float32, device="cuda:0", generator=gen) for _ in range(5))
    d = d.abs() + 0.5
    scal = _scalars(letter, [0.75, -1.25])
    r, xx, w, out = r0.clone(), x.clone(), torch.empty_like(r0), _result(letter, 2)
    F._guard("cap", capi.axpby_pair_axy_dot_device[letter], gpu, _p(out), n, _p(xx), _p(xx), _p(p), _p(r), _p(r), _p(ap), _p(w), _p(d),
             _p(scal[0:]), _p(scal[1:]))
    got = _cells(out, 2, "cap")
    r_ref, x_ref, ref1, ref0 = r0.clone(), x.clone(), _result(letter, 1), _result(letter, 1)
    F._guard("cap", capi.axpby_pair_dot_device[letter], gpu, _p(ref1), n, _p(x_ref), _p(x_ref), _p(p), _p(r_ref), _p(r_ref), _p(ap),
             _p(scal[0:]), _p(scal[1:]))
    F._guard("cap", capi.dot_device[letter], gpu, _p(ref0), n, _p(r), _p(w))
    assert torch.equal(r.view(torch.int32), r_ref.view(torch.int32)) and torch.equal(xx.view(torch.int32), x_ref.view(torch.int32))
    assert torch.equal(w.view(torch.int32), (d * r).view(torch.int32))           # one IEEE multiplication per element
    F._same_bytes(got[1:], _cells(ref1, 1, "cap"), "cap: result[1] against spgpu?axpbyPairDotDevice")
    F._same_bytes(got[:1], _cells(ref0, 1, "cap"), "cap: result[0] against spgpu?dotDevice(z2, w)")


# ---- pitch multivectors ------------------------------------------------------------------------------------------------------------
def _mv_n(letter):
    return TILE[letter] + 6          # two workgroups per vector; pitch = n keeps D on the 16-byte boundary and takes S off it


def _pitches(letter):
    n = _mv_n(letter)
    return {"n": n, "n+1": n + 1, "padded": -(-n // 4) * 4}


def _mv_place(vectors, pitch):
    """(count, n) on the host -> a pitch multivector on the device, sentinels in the gaps and around: (whole buffer, the multivector)."""
    count, n = vectors.shape
    whole = np.full(count * pitch, F.SENTINEL, vectors.dtype)
    whole.reshape(count, pitch)[:, :n] = vectors
    return F._place(whole, 0)


def _mv_read(buf, count, n, pitch, what):
    whole = F._assert_margins(buf, 0, count * pitch, what).reshape(count, pitch)
    assert np.all(whole[:, n:] == F.SENTINEL), f"{what}: a gap between the vectors, or behind the last, was written"
    return np.ascontiguousarray(whole[:, :n])


def _mv_reals(letter, seed, count, n):
    return np.stack([F._real(letter, seed + 17 * j, n) for j in range(count)])


def _mv_integers(letter, seed, count, n, support):
    return np.stack([X.integer_vector(letter, seed + 17 * j, n, support_seed=support + j, density=0.5) for j in range(count)])


MV_SMALL = [(count, kind) for count in (1, 3, 8) for kind in ("n", "n+1", "padded")]


@pytest.mark.parametrize("count,kind", MV_SMALL + [(1025, "two passes")])
@pytest.mark.parametrize("letter", LETTERS)
def test_maxy_dot_device(gpu, letter, count, kind):
    from spgpu_amd import capi
    F._start()
    real = X.REAL_OF[letter]
    n, pitch = (5, 8) if count > 8 else (_mv_n(letter), _pitches(letter)[kind])
    cid = f"{letter}-maxyDot-count{count}-n{n}-pitch{pitch}"
    exact = count > 8
    d, r = (_mv_integers(letter, s, count, n, 900) if exact else _mv_reals(letter, s, count, n) for s in (61, 62))
    (_, dd), (_, dr), (z_buf, dz) = _mv_place(d, pitch), _mv_place(r, pitch), _mv_place(np.full((count, n), F.SENTINEL, real), pitch)
    out, ref = _result(letter, count), _result(letter, count)
    F._guard(cid, capi.maxy_dot_device[letter], gpu, _p(out), n, _p(dz), _p(dd), _p(dr), count, pitch)
    got_z, got = _mv_read(z_buf, count, n, pitch, f"{cid}: z"), _cells(out, count, cid)
    F._guard(cid, capi.mdot_device[letter], gpu, _p(ref), n, _p(dr), _p(dz), count, pitch)
    F._same_bytes(got, _cells(ref, count, cid), f"{cid}: result[] against spgpu?mdotDevice(r, z)")
    if exact:
        di, ri = X._ints(d)[0], X._ints(r)[0]
        F._equals_integers(got_z, di * ri, f"{cid}: z")
        F._equals_integers(got, np.sum(ri * ri * di, axis=1), f"{cid}: result[]")
        return
    for j in range(count):
        z_j, _ = _axy_dot(gpu, letter, f"{cid} vector {j}", n, {}, d[j], r[j])
        F._same_bytes(got_z[j], z_j, f"{cid}: vector {j} against the single-vector call")


@pytest.mark.parametrize("count,kind", MV_SMALL + [(512, "one launch"), (513, "two launches"), (1025, "two passes")])
@pytest.mark.parametrize("letter", LETTERS)
def test_maxpby_pair_axy_dot_device(gpu, letter, count, kind):
    """512 vectors: the last count whose two sets of partials go through one launch; 513: the pass runs as two (fused_solver.hip
    kPairAxyMaxVectorsPerLaunch); 1025: a second pass of spgpu?mdotDevice's 1024."""
    from spgpu_amd import capi
    F._start()
    real = X.REAL_OF[letter]
    n, pitch = (5, 8) if count > 8 else (_mv_n(letter), _pitches(letter)[kind])
    cid = f"{letter}-mpairAxyDot-count{count}-n{n}-pitch{pitch}"
    exact = count > 8
    if exact:
        x1, y1 = (_mv_integers(letter, s, count, n, 910 + s) for s in (71, 72))
        x2, y2, d = (_mv_integers(letter, s, count, n, 920) for s in (73, 74, 75))
        num, den = np.full(count, NUM, real), np.full(count, DEN, real)
    else:
        x1, y1, x2, y2, d = (_mv_reals(letter, s, count, n) for s in (71, 72, 73, 74, 75))
        num, den = F._real(letter, 76, count), F._real(letter, 77, count) + real(3)
    scal = _scalars(letter, np.concatenate([num, den]))
    p_num, p_den = _p(scal[0:]), _p(scal[count:])
    dx1, dx2, dd = _mv_place(x1, pitch)[1], _mv_place(x2, pitch)[1], _mv_place(d, pitch)[1]
    (z1_buf, dz1), (z2_buf, dz2) = _mv_place(y1, pitch), _mv_place(y2, pitch)                     # in place: z1 = y1, z2 = y2
    w_buf, dw = _mv_place(np.full((count, n), F.SENTINEL, real), pitch)
    out = _result(letter, 2 * count)
    F._guard(cid, capi.maxpby_pair_axy_dot_device[letter], gpu, _p(out), n, _p(dz1), _p(dz1), _p(dx1), _p(dz2), _p(dz2), _p(dx2), _p(dw),
             _p(dd), p_num, p_den, count, pitch)
    got1, got2 = _mv_read(z1_buf, count, n, pitch, f"{cid}: z1"), _mv_read(z2_buf, count, n, pitch, f"{cid}: z2")
    got_w, got = _mv_read(w_buf, count, n, pitch, f"{cid}: w"), _cells(out, 2 * count, cid)
    # result[count + j]: spgpu?maxpbyPairDotDevice on operands that lie the same way; result[j]: spgpu?mdotDevice(z2, w)
    (_, rz1), (_, rz2), ref1, ref0 = _mv_place(y1, pitch), _mv_place(y2, pitch), _result(letter, count), _result(letter, count)
    F._guard(cid, capi.maxpby_pair_dot_device[letter], gpu, _p(ref1), n, _p(rz1), _p(rz1), _p(dx1), _p(rz2), _p(rz2), _p(dx2), p_num, p_den,
             count, pitch)
    F._guard(cid, capi.mdot_device[letter], gpu, _p(ref0), n, _p(dz2), _p(dw), count, pitch)
    F._same_bytes(got[count:], _cells(ref1, count, cid), f"{cid}: result[count + j] against spgpu?maxpbyPairDotDevice")
    F._same_bytes(got[:count], _cells(ref0, count, cid), f"{cid}: result[j] against spgpu?mdotDevice(z2, w)")
    if exact:
        i = lambda v: X._ints(v)[0]
        z1, z2 = i(y1) + A * i(x1), i(y2) - A * i(x2)
        F._equals_integers(got1, z1, f"{cid}: z1")
        F._equals_integers(got2, z2, f"{cid}: z2")
        F._equals_integers(got_w, i(d) * z2, f"{cid}: w")
        F._equals_integers(got[:count], np.sum(z2 * z2 * i(d), axis=1), f"{cid}: result[j]")
        F._equals_integers(got[count:], np.sum(z2 * z2, axis=1), f"{cid}: result[count + j]")
        return
    for j in range(count):
        z1_j, z2_j, w_j, _, _ = _pair(gpu, letter, f"{cid} vector {j}", n, {}, True, x1[j], y1[j], x2[j], y2[j], d[j], num=num[j], den=den[j])
        for name, mine, single in (("z1", got1, z1_j), ("z2", got2, z2_j), ("w", got_w, w_j)):
            F._same_bytes(mine[j], single, f"{cid}: {name} of vector {j} against the single-vector call")
