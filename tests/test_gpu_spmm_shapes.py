"""GPU: spgpu?hellspmm and spgpu?hellspmmMv on every kernel instantiation their dispatches can choose (hellSpmm, hell_spmm.hip) and
on the workgroup-uniform branches inside the kernels that no argument names: window fits the LDS tile or not, decided at the probe
or after the scan, a workgroup without entries, direct or staged tile fill, 16-byte runs or single elements in the pitch layout,
wavefronts of uniform rows, band wavefronts.  The constants, both dispatches restated, the case tables and the 613-row matrices
are in tests/spmm_launch_shapes.py; tests/test_spmm_launch_shapes.py checks them without a GPU.

Every call is checked three ways: the oracle's bits (O.hell_spmm; for the pitch layout also interleave -> hellspmm ->
deinterleave on the device), the exact sums of exact_ref.spmm within the project's TOL, and the bytes of Z that are no vector
element (padding columns, the elements in front of a shifted base and behind the buffer), which hold a sentinel.  Before it
launches, every case asserts from the addresses it is about to pass that the dispatch restated in spmm_launch_shapes selects the
instantiation the case is there for: a case fails rather than run another kernel."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O
import spmm_launch_shapes as S
from test_gpu_spmm_mv import SENTINEL, _Mv, _via_interleaved

pytestmark = pytest.mark.gpu
RAN = set()   # node ids of the tests of this file that were run (test_zz_no_case_was_skipped)
ALPHA = -1.5
MATRICES = (("mixed", 1), ("band", 0))   # the holes of base 1 ride along with `mixed`

_IL_IDS = [(L, cid) for L in "SD" for cid in S.interleaved_cases(L)]
_MV_IDS = [(L, cid) for L in "SD" for cid in S.mv_cases(L)]


@pytest.fixture(autouse=True)
def _ran(request):
    """A test skipped by a mark or a condition is never set up, so it never gets here; no test of this file skips itself."""
    RAN.add(request.node.nodeid)
    yield


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- matrices -------------------------------------------------------------------------------------------------------------------
_HOST, _DEV, _REF = {}, {}, {}


def _host_matrix(name, base, letter, hack):
    """Host HELL of S.matrix(name, base) with the holes planted, and the COO of the entries a product uses."""
    key = (name, base, letter, hack)
    if key not in _HOST:
        from spgpu_amd import formats
        m = S.matrix(name, base)
        v = S.values(letter, 1, m["rows"].size)
        hell = formats.ell_to_hell(formats.coo_to_ell(S.ROWS, m["rows"], m["cols"], v, ell_base=base), hack)
        assert hell["hack_size"] == hack and np.array_equal(hell["row_lengths"][:S.ROWS], m["lengths"])
        r, c, vv = X.hell_coo(hell)      # slab order is the generator's order
        assert np.array_equal(r - base, m["rows"]) and np.array_equal(c - base, m["cols"]) and np.array_equal(vv, v)
        if m["hole"].any():
            k = np.arange(m["rows"].size) - np.repeat(np.cumsum(m["lengths"]) - m["lengths"], m["lengths"])
            slots = hell["hack_offsets"].astype(np.int64)[m["rows"] // hack] + m["rows"] % hack + k * hack
            hell["indices"][slots[m["hole"]]] = 0       # column -1 of a 1-based matrix: never used
        ur, uc = S.used(m)
        _HOST[key] = dict(hell=hell, m=m, r=ur, c=uc, v=v[~m["hole"]], empty=np.flatnonzero(m["lengths"] == 0))
    return _HOST[key]


class _DevMatrix:
    """The HELL arrays in HBM; cM and rP each optionally one element past a 16-byte boundary."""

    def __init__(self, hell, shift_cm=False, shift_rp=False, r_idx=None):
        import torch
        from spgpu_amd import formats

        def place(a, shift):
            buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a[:1]).dtype, device="cuda:0")
            assert buf.data_ptr() % 16 == 0
            view = buf[int(shift):int(shift) + a.size]
            view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
            return buf, view

        self._cm, self.cM = place(hell["values"], shift_cm)
        self._rp, self.rP = place(hell["indices"], shift_rp)
        self.hack_offsets = formats.to_device(hell["hack_offsets"])
        self.rS = formats.to_device(hell["row_lengths"])
        self.rIdx = formats.to_device(r_idx)
        self.hack_size, self.base, self.rows, self.letter = hell["hack_size"], hell["base"], hell["rows"], hell["letter"]


def _dev_matrix(name, base, letter, hack, shift=(), r_idx=None):
    key = (name, base, letter, hack, "cM" in shift, "rP" in shift, None if r_idx is None else r_idx.tobytes())
    if key not in _DEV:
        _DEV[key] = _DevMatrix(_host_matrix(name, base, letter, hack)["hell"], "cM" in shift, "rP" in shift, r_idx)
    return _DEV[key]


def _operands(letter, count):
    """X [COLS, count] and Y [ROWS, count], the same for every case of one count."""
    key = ("xy", letter, count)
    if key not in _REF:
        _REF[key] = (S.values(letter, 100 + count, S.COLS * count).reshape(S.COLS, count),
                     S.values(letter, 200 + count, S.ROWS * count).reshape(S.ROWS, count))
    return _REF[key]


def _exact(name, base, letter, count, beta, perm=None):
    """exact_ref.spmm of one (matrix, count, beta, row order), computed once and left unchanged."""
    key = ("exact", name, base, letter, count, beta, None if perm is None else perm.tobytes())
    if key not in _REF:
        h = _host_matrix(name, base, letter, 32)
        Xk, Yk = _operands(letter, count)
        _REF[key] = X.spmm(S.ROWS, h["r"], h["c"], h["v"], Xk, Yk if beta != 0 else None, ALPHA, beta, count, r_idx=perm)
    return _REF[key]


# ---- interleaved multivectors ------------------------------------------------------------------------------------------------------
class _Il:
    """[n, count] in the interleaved layout inside one device buffer: `shift` elements in front of the base, rows of `ld` elements,
    5 elements behind; everything that is no vector element holds `gap`."""

    def __init__(self, rows2d, ld, shift=0, gap=np.nan):
        from spgpu_amd import formats
        n, count = rows2d.shape
        assert ld >= count
        self.n, self.count, self.ld, self.shift = n, count, ld, shift
        host = np.full(shift + n * ld + 5, gap, dtype=rows2d.dtype)
        self.is_gap = np.ones(host.size, dtype=bool)
        body = host[shift:shift + n * ld].reshape(n, ld)
        body[:, :count] = rows2d
        self.is_gap[shift:shift + n * ld].reshape(n, ld)[:, :count] = False
        self.before = host.copy()
        self.dev = formats.to_device(host)
        assert self.dev.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + self.shift * self.dev.element_size())

    @property
    def off16(self):
        return (self.dev.data_ptr() + self.shift * self.dev.element_size()) % 16

    def vectors(self):
        """[n, count] host array; asserts that nothing outside the vector elements changed, bit for bit."""
        host = self.dev.cpu().numpy()
        assert host[self.is_gap].tobytes() == self.before[self.is_gap].tobytes(), "elements outside the vectors were written"
        return np.ascontiguousarray(host[self.shift:self.shift + self.n * self.ld].reshape(self.n, self.ld)[:, :self.count])


def _shift_of(shift, name):
    return 2 if name == "X" and "X2" in shift else int(name in shift)


def _same_bits(got, want, case=""):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), case


def _run_interleaved(gpu, letter, name, base, c, beta, perm=None, z_init=None, alias=False, x_rows=None, alpha=ALPHA):
    """One spgpu?hellspmm call of case `c`; returns (Z as [ROWS, count], the oracle's Z).  alias: Z is Y."""
    import torch
    from spgpu_amd import capi
    count, shift = c["count"], c["shift"]
    Xk, Yk = _operands(letter, count)
    if x_rows is not None:
        Xk = x_rows
    h = _host_matrix(name, base, letter, c["hack"])
    mat = _dev_matrix(name, base, letter, c["hack"], shift, perm)
    x = _Il(Xk, c["ldx"], _shift_of(shift, "X"))
    if alias:
        z = _Il(Yk if z_init is None else z_init, c["ldyz"], _shift_of(shift, "Z"), gap=SENTINEL)
        y = z
    else:
        z = _Il(np.full_like(Yk, np.nan), c["ldyz"], _shift_of(shift, "Z"), gap=SENTINEL)
        y = _Il(Yk, c["ldyz"], _shift_of(shift, "Y")) if beta != 0 else None
    off = dict(cM=mat.cM.data_ptr() % 16, rP=mat.rP.data_ptr() % 16, X=x.off16, Z=z.off16, Y=y.off16 if y is not None else 0)
    assert off == dict(S.offsets(letter, shift), Y=off["Y"]) and (y is None or alias or off["Y"] == S.offsets(letter, shift)["Y"])
    chosen = S.interleaved_passes(letter, c["hack"], count, c["ldx"], c["ldyz"], perm is not None, off, y is not None)
    assert chosen == S.expected_passes(letter, c), "the arguments of this case select another instantiation"
    capi.hellspmm[letter](gpu, z.ptr, y.ptr if y is not None else None, capi.scalar(letter, alpha), _p(mat.cM), _p(mat.rP),
                          mat.hack_size, _p(mat.hack_offsets), _p(mat.rS), _p(mat.rIdx), 0, mat.rows, x.ptr,
                          capi.scalar(letter, beta), mat.base, count, c["ldx"], c["ldyz"])
    torch.cuda.synchronize()
    got = z.vectors()
    y_host = None if beta == 0 else (Yk if z_init is None else z_init)
    want = O.hell_spmm(h["hell"], Xk, y_host, alpha, beta, r_idx=perm, in_place=alias)
    return got, want


def _check(got, want, name, base, letter, count, beta, case, perm=None):
    _same_bits(got, want, (case, "oracle"))
    exact, scale = _exact(name, base, letter, count, beta, perm)
    X.assert_within(got, exact, scale, letter, case)


@pytest.mark.parametrize("name,base", MATRICES)
@pytest.mark.parametrize("letter,cid", _IL_IDS, ids=[f"{L}-{cid}" for L, cid in _IL_IDS])
def test_interleaved_instantiation(gpu, letter, cid, name, base):
    """Every row of the case table (spmm_launch_shapes.interleaved_cases): alpha = -1.5, Y == NULL and beta = 0.5, on the matrix
    whose workgroups are narrow / wide after the scan / wide at the probe (1-based, with holes) and on the band matrix."""
    c = S.interleaved_cases(letter)[cid]
    for beta in c["betas"]:
        got, want = _run_interleaved(gpu, letter, name, base, c, beta)
        _check(got, want, name, base, letter, c["count"], beta, (letter, cid, name, beta))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("letter,cid", [(L, cid) for L in "SD" for cid in ("strip2-direct-h32", "strip1-count7", "tiled-count10-h48",
                                                                            "k8x1-count5-h48")])
def test_workgroup_without_entries(gpu, letter, cid, base):
    """A whole workgroup whose rows have no entries (hi < lo in the window search) between one that misses the tile and one that
    fits it: with Y == NULL its rows of Z are zeros, with beta they are beta * Y."""
    c = S.interleaved_cases(letter)[cid]
    for beta in (0.0, 0.5):
        got, want = _run_interleaved(gpu, letter, "empty_group", base, c, beta)
        _check(got, want, "empty_group", base, letter, c["count"], beta, (letter, cid, base, beta))
        lo, hi = S.workgroups()[1]
        Yk = _operands(letter, c["count"])[1]
        assert np.array_equal(got[lo:hi], Yk[lo:hi] * Yk.dtype.type(beta)), "the empty workgroup"


@pytest.mark.parametrize("alias", [False, True], ids=["out-of-place", "z-is-y"])
@pytest.mark.parametrize("cid", S.ONE_EACH)
@pytest.mark.parametrize("letter", "SD")
def test_row_order_on_every_instantiation(gpu, letter, cid, alias):
    """rIdx, a random permutation: row i of the matrix is written to Z[rIdx[i]] and Y is read there."""
    c = S.interleaved_cases(letter)[cid]
    perm = np.random.default_rng(4).permutation(S.ROWS).astype(np.int32)
    got, want = _run_interleaved(gpu, letter, "mixed", 1, c, 0.5, perm=perm, alias=alias)
    _check(got, want, "mixed", 1, letter, c["count"], 0.5, (letter, cid, alias), perm=perm)


@pytest.mark.parametrize("cid", S.ONE_EACH)
@pytest.mark.parametrize("letter", "SD")
def test_in_place_sum_on_every_instantiation(gpu, letter, cid):
    """Z += alpha*A*X (Y == Z, beta == 1): rows without entries keep their bytes -- half of them hold -0.0, half NaN -- and the
    rest equals the oracle called the same way.  What the sharded driver's "rest" product is made of."""
    c = S.interleaved_cases(letter)[cid]
    h = _host_matrix("mixed", 1, letter, c["hack"])
    Z0 = _operands(letter, c["count"])[1].copy()
    empty = h["empty"]
    assert empty.size > S.WAVE
    Z0[empty[0::2]] = -0.0
    Z0[empty[1::2]] = np.nan
    # alpha > 0: a kernel that did compute these rows would turn -0.0 into alpha * 0 + -0.0 = +0.0
    got, want = _run_interleaved(gpu, letter, "mixed", 1, c, 1.0, z_init=Z0, alias=True, alpha=0.5)
    _same_bits(got[empty], Z0[empty], "rows without entries")
    _same_bits(got, want, (letter, cid, "oracle"))
    # rows whose entries are all holes (none by construction) would be zero-scale rows with entries: the exact sums cover the rest
    full = np.setdiff1d(np.arange(S.ROWS), empty)
    Xk = _operands(letter, c["count"])[0]
    exact, scale = X.spmm(S.ROWS, h["r"], h["c"], h["v"], Xk, np.where(np.isnan(Z0), 0, Z0), 0.5, 1.0, c["count"])
    X.assert_within(got[full], exact[full], scale[full], letter, (letter, cid))


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("cid", S.ONE_EACH)
@pytest.mark.parametrize("letter", "SD")
def test_nan_in_row_0_of_x_reaches_nothing(gpu, letter, cid, base):
    """Absent entries -- past a row's length, and the holes of the 1-based matrix -- read row 0 of X and discard the product
    (spmmAccumulate's global-memory loop, spmm_rows.hip.h).  The matrix names column 0 nowhere, row 0 of X holds NaN: none may reach Z."""
    c = S.interleaved_cases(letter)[cid]
    Xk = _operands(letter, c["count"])[0].copy()
    Xk[0] = np.nan
    got, want = _run_interleaved(gpu, letter, "mixed", base, c, 0.5, x_rows=Xk)
    assert not np.isnan(got).any()
    _check(got, want, "mixed", base, letter, c["count"], 0.5, (letter, cid, base))


# ---- the pitch layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,base", MATRICES)
@pytest.mark.parametrize("letter,cid", _MV_IDS, ids=[f"{L}-{cid}" for L, cid in _MV_IDS])
def test_mv_instantiation(gpu, letter, cid, name, base):
    """spgpu?hellspmmMv: both strip kernels with 16-byte runs and with single elements (a shifted base, a pitch that is no multiple
    of 16 bytes, a row order), and the one-row-per-lane kernel by hack size 48 and by a shifted cM or rP."""
    import torch
    from spgpu_amd import capi
    c = S.mv_cases(letter)[cid]
    count, shift = c["count"], c["shift"]
    px, pz = S.mv_pitches(letter, c)
    Xk, Yk = _operands(letter, count)
    perm = np.random.default_rng(5).permutation(S.ROWS).astype(np.int32) if c["r_idx"] else None
    h = _host_matrix(name, base, letter, c["hack"])
    mat = _dev_matrix(name, base, letter, c["hack"], shift, perm)
    x = _Mv(Xk, px, shift=int("X" in shift))
    for beta in c["betas"]:
        y = _Mv(Yk, pz, shift=int("Y" in shift)) if beta != 0 else None
        z = _Mv(np.full_like(Yk, np.nan), pz, shift=int("Z" in shift), gap=SENTINEL)
        off16 = lambda mv: (mv.dev.data_ptr() + mv.shift * mv.dev.element_size()) % 16
        off = dict(cM=mat.cM.data_ptr() % 16, rP=mat.rP.data_ptr() % 16, X=off16(x), Z=off16(z), Y=off16(y) if y is not None else 0)
        chosen = S.mv_passes(letter, c["hack"], count, px, pz, c["r_idx"], off, y is not None)
        assert chosen == S.expected_passes(letter, c, pitch=True), "the arguments of this case select another instantiation"
        capi.hellspmm_mv[letter](gpu, z.ptr, y.ptr if y is not None else None, capi.scalar(letter, ALPHA), _p(mat.cM), _p(mat.rP),
                                 mat.hack_size, _p(mat.hack_offsets), _p(mat.rS), _p(mat.rIdx), 0, mat.rows, x.ptr,
                                 capi.scalar(letter, beta), mat.base, count, px, pz)
        torch.cuda.synchronize()
        got = z.vectors()   # checks the sentinels
        _check(got, O.hell_spmm(h["hell"], Xk, Yk if beta != 0 else None, ALPHA, beta, r_idx=perm), name, base, letter, count, beta,
               (letter, cid, name, beta), perm=perm)
        _same_bits(got, _via_interleaved(gpu, letter, mat, z, y, ALPHA, x, beta, count), (letter, cid, name, beta, "interleaved"))


def test_zz_no_case_was_skipped(request):
    """Every case above is mandatory.  This test is the last of the file: of the tests of this file selected for the run, each
    one before it must have been run (a failed one has; a skipped one has not)."""
    mine = [item.nodeid for item in request.session.items
            if item.fspath == request.node.fspath and item.nodeid != request.node.nodeid]
    skipped = [nodeid for nodeid in mine if nodeid not in RAN]
    assert not skipped, skipped
    if not request.config.getoption("keyword") and not any("::" in arg for arg in request.config.args):
        n_il, n_mv, one = len(_IL_IDS), len(_MV_IDS), len(S.ONE_EACH)
        assert len(mine) == 2 * n_il + 2 * 8 + 2 * 2 * one + 2 * one + 2 * 2 * one + 2 * n_mv, len(mine)
