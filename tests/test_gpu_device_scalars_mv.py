"""GPU: the device-scalar Level-1 calls on pitch multivectors (include/spgpu/ext/device_scalars_mv.h) on every case of
tests/device_scalars_mv_launch_shapes.py.  The reductions against spgpu?mdot / spgpu?mnrm2 (the contracted bits), against the
single-vector device calls where the header's three conditions hold, and against exact integer sums; the updates and the pair-dot
against the single-vector device calls vector by vector and against numpy on data where every operation is exact.  Every
multivector carries a NaN pattern between its vectors and behind the last one: inputs must come back unchanged, outputs must keep
the pattern there and hold no NaN elsewhere; results sit between guard cells."""
import ctypes as C

import numpy as np
import pytest

import device_scalars_mv_launch_shapes as M
import exact_ref as X

pytestmark = pytest.mark.gpu

NP = {"S": np.float32, "D": np.float64}
BITS = {"S": np.uint32, "D": np.uint64}
GAP_IN = {"S": 0x7FC0DEAD, "D": 0x7FF8DEAD0000BEEF}     # quiet NaNs that no arithmetic produces: between the vectors of an input ...
GAP_OUT = {"S": 0x7FC0FACE, "D": 0x7FF8FACE0000F00D}    # ... and everywhere in an output before the call
GUARD = 3
CASES = [pytest.param(L, cid, id=f"{L}-{cid}") for L in M.LETTERS for cid in M.cases(L)]


def _addr(t, element=0):
    return C.c_void_p(t.data_ptr() + element * t.element_size()) if t is not None else None


class Layout:
    """Where the vectors of a case lie in a flat buffer: vector j at off + j*pitch; 5 elements behind the last pitch."""

    def __init__(self, case):
        self.letter, self.n, self.count, self.pitch = case["letter"], case["n"], case["count"], case["pitch"]
        self.off = case["off"] // M.SIZEOF[self.letter]
        self.size = self.off + self.count * self.pitch + 5

    def host(self, vectors, fill):
        """Flat host array: `fill` bits everywhere, row j of `vectors` [count, n] (or None) at vector j."""
        flat = np.full(self.size, fill[self.letter], BITS[self.letter]).view(NP[self.letter])
        if vectors is not None:
            for j in range(self.count):
                flat[self.off + j * self.pitch:self.off + j * self.pitch + self.n] = vectors[j]
        return flat

    def vectors(self, flat):
        return np.stack([flat[self.off + j * self.pitch:self.off + j * self.pitch + self.n] for j in range(self.count)])

    def device(self, flat):
        import torch
        t = torch.from_numpy(flat.copy()).to("cuda:0")
        assert t.data_ptr() % 16 == 0
        return t

    def base(self, t):
        return _addr(t, self.off)

    def vector(self, t, j):
        return _addr(t, self.off + j * self.pitch)


def _values(letter, seed, count, n):
    from spgpu_amd import synth
    return synth.values_for(letter, seed, max(count * n, 1))[:count * n].reshape(count, n)


def _integers(letter, seed, count, n):
    return np.random.default_rng(seed).integers(-3, 4, (count, n)).astype(NP[letter])


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _results(letter, count):
    """Device array of count results between GUARD cells on each side, all holding the output pattern."""
    import torch
    host = np.full(count + 2 * GUARD, GAP_OUT[letter], BITS[letter]).view(NP[letter])
    return torch.from_numpy(host.copy()).to("cuda:0"), host


def _checked(res, host, count):
    """The results of a call, after the guard cells were found unchanged."""
    got = res.cpu().numpy()
    assert _same(got[:GUARD], host[:GUARD]) and _same(got[GUARD + count:], host[GUARD + count:]), "a guard cell was written"
    return got[GUARD:GUARD + count]


# ---- reductions ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("letter,cid", CASES)
def test_mdot_and_mnrm2_device(gpu, letter, cid):
    import torch
    from spgpu_amd import capi
    case = M.cases(letter)[cid]
    lay = Layout(case)
    n, count, pitch = lay.n, lay.count, lay.pitch
    a_h, b_h = lay.host(_values(letter, 1, count, n), GAP_IN), lay.host(_values(letter, 2, count, n), GAP_IN)
    da, db = lay.device(a_h), lay.device(b_h)

    res, res_h = _results(letter, count)
    capi.mdot_device[letter](gpu, _addr(res, GUARD), n, lay.base(da), lay.base(db), count, pitch)
    want = np.full(count, np.nan, NP[letter])
    capi.mdot[letter](gpu, C.c_void_p(want.ctypes.data), n, lay.base(da), lay.base(db), count, pitch)   # synchronises
    dot = _checked(res, res_h, count).copy()
    assert _same(dot, want), f"mdotDevice {dot} != mdot {want}"

    res, res_h = _results(letter, count)
    capi.mnrm2_device[letter](gpu, _addr(res, GUARD), n, lay.base(da), count, pitch)
    want = np.full(count, np.nan, NP[letter])
    capi.mnrm2[letter](gpu, C.c_void_p(want.ctypes.data), n, lay.base(da), count, pitch)
    nrm = _checked(res, res_h, count).copy()
    assert _same(nrm, want), f"mnrm2Device {nrm} != mnrm2 {want}"
    if n <= 0:
        assert _same(dot, np.zeros(count, NP[letter])) and _same(nrm, np.zeros(count, NP[letter]))      # +0, not -0

    # the single-vector calls on vector j alone, where the header's three conditions hold
    if n > 0 and M.repeats_single_vector_call(letter, n, count, pitch, case["off"]):
        single = torch.zeros(2 * count, dtype=da.dtype, device="cuda:0")
        for j in range(count):
            capi.dot_device[letter](gpu, _addr(single, j), n, lay.vector(da, j), lay.vector(db, j))
            capi.nrm2_device[letter](gpu, _addr(single, count + j), n, lay.vector(da, j))
        torch.cuda.synchronize()
        single = single.cpu().numpy()
        assert _same(single[:count], dot) and _same(single[count:], nrm)
    assert _same(da.cpu().numpy(), a_h) and _same(db.cpu().numpy(), b_h), "an input was written"

    # independent of every order of addition: small integers, whose sums are exact (9 * n < 2^24)
    ai, bi = _integers(letter, 11, count, n), _integers(letter, 12, count, n)
    da, db = lay.device(lay.host(ai, GAP_IN)), lay.device(lay.host(bi, GAP_IN))
    res, res_h = _results(letter, count)
    capi.mdot_device[letter](gpu, _addr(res, GUARD), n, lay.base(da), lay.base(db), count, pitch)
    torch.cuda.synchronize()
    dot = _checked(res, res_h, count).copy()
    res, res_h = _results(letter, count)
    capi.mnrm2_device[letter](gpu, _addr(res, GUARD), n, lay.base(da), count, pitch)
    torch.cuda.synchronize()
    nrm = _checked(res, res_h, count)
    for j in range(count):
        sums = X.integer_sums(letter, ai[j], bi[j])
        X.assert_sums_exact(letter, sums)
        assert dot[j] == sums["dot"][0], (j, dot[j], sums["dot"])
        assert nrm[j] == X.rounded_sqrt(letter, sums["nrm2sq"]), (j, nrm[j], sums["nrm2sq"])


# ---- updates --------------------------------------------------------------------------------------------------------------------

def _coefficients(letter, mode, count, exact=False):
    """Host arrays (or None = NULL) betaNum, betaDen, alphaNum, alphaDen and negateAlpha of a mode of
    tests/device_scalars_mv_launch_shapes.py; the plain modes use betaNum as beta and alphaNum as alpha.  exact: powers of two."""
    from spgpu_amd import synth
    dt = NP[letter]
    j = np.arange(count)
    if exact:
        b_num, b_den, a_num, a_den = ((2.0 ** ((j + s) % 3 - 1)).astype(dt) for s in range(4))
    else:
        b_num, b_den, a_num, a_den = ((synth.values_for(letter, 20 + s, count) + 2).astype(dt) for s in range(4))
    zero_where = [not M.has_beta(mode, int(k)) for k in j]
    if mode in ("quot-mixed", "in-place"):
        b_num = np.where(zero_where, dt(0), b_num).astype(dt)
        return b_num, b_den, a_num, a_den, 1
    if mode == "quot-ones":
        return None, None, None, a_den, 0
    if mode == "plain-mixed":
        return np.where(zero_where, dt(0), b_num).astype(dt), None, a_num, None, 0
    assert mode == "plain-null"
    return None, None, a_num, None, 0


def _run_update(gpu, lay, mode, coeff, dz, dy, dx, single):
    """The multivector call (single False) or the single-vector call on every vector in turn, on the same device buffers."""
    from spgpu_amd import capi, formats
    L, n, count, pitch = lay.letter, lay.n, lay.count, lay.pitch
    b_num, b_den, a_num, a_den = (formats.to_device(c) if c is not None and c.size else None for c in coeff[:4])
    negate = coeff[4]
    plain = mode.startswith("plain")
    if not single:
        if plain:
            capi.maxpby_device[L](gpu, lay.base(dz), n, _addr(b_num), lay.base(dy), _addr(a_num), lay.base(dx), count, pitch)
        else:
            capi.maxpby_quot_device[L](gpu, lay.base(dz), n, _addr(b_num), _addr(b_den), lay.base(dy), _addr(a_num), _addr(a_den),
                                       negate, lay.base(dx), count, pitch)
        return
    at = lambda t, j: _addr(t, j) if t is not None else None
    for j in range(count):
        if plain:
            capi.axpby_device[L](gpu, lay.vector(dz, j), n, at(b_num, j), lay.vector(dy, j), at(a_num, j), lay.vector(dx, j))
        else:
            capi.axpby_quot_device[L](gpu, lay.vector(dz, j), n, at(b_num, j), at(b_den, j), lay.vector(dy, j), at(a_num, j),
                                      at(a_den, j), negate, lay.vector(dx, j))


@pytest.mark.parametrize("letter,cid", CASES)
def test_maxpby_device_and_quot(gpu, letter, cid):
    import torch
    case = M.cases(letter)[cid]
    lay = Layout(case)
    n, count = lay.n, lay.count
    x_h = lay.host(_values(letter, 3, count, n), GAP_IN)
    dx = lay.device(x_h)
    for mode in M.MODES:
        coeff = _coefficients(letter, mode, count)
        y = _values(letter, 4, count, n).copy()
        for j in range(count):
            if not M.has_beta(mode, j):
                y[j] = np.nan                                   # a vector whose beta is 0 (or NULL) must stay unread
        y_h = lay.host(y, GAP_IN)
        if mode == "in-place":
            got, want = lay.device(y_h), lay.device(y_h)
            _run_update(gpu, lay, mode, coeff, got, got, dx, single=False)
            _run_update(gpu, lay, mode, coeff, want, want, dx, single=True)
        else:
            dy = lay.device(y_h)
            got, want = lay.device(lay.host(None, GAP_OUT)), lay.device(lay.host(None, GAP_OUT))
            _run_update(gpu, lay, mode, coeff, got, dy, dx, single=False)
            _run_update(gpu, lay, mode, coeff, want, dy, dx, single=True)
        torch.cuda.synchronize()
        got_h, want_h = got.cpu().numpy(), want.cpu().numpy()
        assert _same(got_h, want_h), f"{mode}: differs from the single-vector calls (or wrote between the vectors)"
        blank = lay.host(None, GAP_IN if mode == "in-place" else GAP_OUT)
        keep = np.ones(lay.size, bool)
        for j in range(count):
            keep[lay.off + j * lay.pitch:lay.off + j * lay.pitch + n] = False
        assert _same(got_h[keep], blank[keep]), f"{mode}: an element between the vectors or behind the last one was written"
        assert not np.isnan(lay.vectors(got_h)).any(), f"{mode}: a NaN of a gap or of an unread y reached z"
        assert _same(dx.cpu().numpy(), x_h) and (mode == "in-place" or _same(dy.cpu().numpy(), y_h)), f"{mode}: an input was written"

    # every operation exact: small integers, coefficients that are quotients of powers of two -> numpy's values
    xi, yi = _integers(letter, 13, count, n), _integers(letter, 14, count, n)
    for mode in ("quot-mixed", "plain-mixed"):
        b_num, b_den, a_num, a_den, negate = coeff = _coefficients(letter, mode, count, exact=True)
        beta = b_num / b_den if b_den is not None else b_num
        alpha = (a_num / a_den if a_den is not None else a_num) * (-1 if negate else 1)
        got = lay.device(lay.host(None, GAP_OUT))
        _run_update(gpu, lay, mode, coeff, got, lay.device(lay.host(yi, GAP_IN)), lay.device(lay.host(xi, GAP_IN)), single=False)
        torch.cuda.synchronize()
        want = alpha[:, None] * xi + beta[:, None] * yi
        assert want.dtype == NP[letter] and np.array_equal(lay.vectors(got.cpu().numpy()), want), mode


# ---- pair-dot -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("letter,cid", CASES)
def test_maxpby_pair_dot_device(gpu, letter, cid):
    import torch
    from spgpu_amd import capi, formats, synth
    case = M.cases(letter)[cid]
    lay = Layout(case)
    n, count, pitch = lay.n, lay.count, lay.pitch
    hosts = [lay.host(_values(letter, 5 + k, count, n), GAP_IN) for k in range(4)]
    x1, y1, x2, y2 = (lay.device(h) for h in hosts)
    num = formats.to_device((synth.values_for(letter, 30, count) + 2).astype(NP[letter]))
    den = formats.to_device((synth.values_for(letter, 31, count) + 2).astype(NP[letter]))

    want1, want2 = lay.device(lay.host(None, GAP_OUT)), lay.device(lay.host(None, GAP_OUT))
    scratch = torch.zeros(1, dtype=x1.dtype, device="cuda:0")
    for j in range(count):
        capi.axpby_pair_dot_device[letter](gpu, _addr(scratch), n, lay.vector(want1, j), lay.vector(y1, j), lay.vector(x1, j),
                                           lay.vector(want2, j), lay.vector(y2, j), lay.vector(x2, j), _addr(num, j), _addr(den, j))
    want_rr, want_rr_h = _results(letter, count)
    capi.mdot_device[letter](gpu, _addr(want_rr, GUARD), n, lay.base(want2), lay.base(want2), count, pitch)

    got1, got2 = lay.device(lay.host(None, GAP_OUT)), lay.device(lay.host(None, GAP_OUT))
    got_rr, got_rr_h = _results(letter, count)
    capi.maxpby_pair_dot_device[letter](gpu, _addr(got_rr, GUARD), n, lay.base(got1), lay.base(y1), lay.base(x1), lay.base(got2),
                                        lay.base(y2), lay.base(x2), _addr(num), _addr(den), count, pitch)
    torch.cuda.synchronize()
    assert _same(got1.cpu().numpy(), want1.cpu().numpy()) and _same(got2.cpu().numpy(), want2.cpu().numpy())
    rr = _checked(got_rr, got_rr_h, count).copy()
    assert _same(rr, _checked(want_rr, want_rr_h, count)), "result differs from mdotDevice on the stored z2"
    assert not np.isnan(rr).any() and not np.isnan(lay.vectors(got2.cpu().numpy())).any()
    for t, h in zip((x1, y1, x2, y2), hosts):
        assert _same(t.cpu().numpy(), h), "an input was written"

    # aliased: z1 == y1, z2 == y2 (the x += alpha p, r -= alpha Ap of CG)
    a, b = lay.device(hosts[1]), lay.device(hosts[3])
    got_rr, got_rr_h = _results(letter, count)
    capi.maxpby_pair_dot_device[letter](gpu, _addr(got_rr, GUARD), n, lay.base(a), lay.base(a), lay.base(x1), lay.base(b),
                                        lay.base(b), lay.base(x2), _addr(num), _addr(den), count, pitch)
    torch.cuda.synchronize()
    a_h, b_h = a.cpu().numpy(), b.cpu().numpy()
    if n > 0:
        assert _same(lay.vectors(a_h), lay.vectors(want1.cpu().numpy())) and _same(lay.vectors(b_h), lay.vectors(want2.cpu().numpy()))
    keep = np.ones(lay.size, bool)
    for j in range(count):
        keep[lay.off + j * lay.pitch:lay.off + j * lay.pitch + n] = False
    assert _same(a_h[keep], hosts[1][keep]) and _same(b_h[keep], hosts[3][keep]), "an element between the vectors was written"
    assert _same(_checked(got_rr, got_rr_h, count), rr)


# ---- division -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("letter", M.LETTERS)
@pytest.mark.parametrize("count", [1, 8, 257])
def test_mdiv_device(gpu, letter, count):
    import torch
    from spgpu_amd import capi, formats, synth
    dt = NP[letter]
    num_h, den_h = synth.values_for(letter, 40, count).astype(dt), (synth.values_for(letter, 41, count) + 2).astype(dt)
    if count > 1:
        num_h[1], den_h[1] = 0, 0                      # 0/0: NaN, as in spgpu?divDevice
    num, den = formats.to_device(num_h), formats.to_device(den_h)
    for negate in (0, 1):
        res, res_h = _results(letter, count)
        capi.mdiv_device[letter](gpu, _addr(res, GUARD), _addr(num), _addr(den), negate, count)
        single = torch.zeros(count, dtype=num.dtype, device="cuda:0")
        for j in range(count):
            capi.div_device[letter](gpu, _addr(single, j), _addr(num, j), _addr(den, j), negate)
        torch.cuda.synchronize()
        got = _checked(res, res_h, count)
        assert _same(got, single.cpu().numpy())
        ok = np.arange(count) != 1
        with np.errstate(invalid="ignore"):
            want = (num_h / den_h) * (-1 if negate else 1)
        assert np.array_equal(got[ok], want[ok].astype(dt)) and (count == 1 or np.isnan(got[1]))
    # a NULL array stands for 1
    res, res_h = _results(letter, count)
    capi.mdiv_device[letter](gpu, _addr(res, GUARD), None, _addr(den), 0, count)
    torch.cuda.synchronize()
    with np.errstate(divide="ignore"):
        assert np.array_equal(_checked(res, res_h, count)[ok], (dt(1) / den_h)[ok])
