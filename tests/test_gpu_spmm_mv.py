"""GPU: spgpu?hellspmmMv (include/spgpu/ext/spmm_mv.h) -- the HELL SpMM on the reference's multivector layout, vector j at
base + j*pitch.  Its contract is spgpu?hellspmm's with the layout changed, so it is checked three ways: against the oracle
(whose orc_?hellspmm works on interleaved arrays: transposed here in numpy), bit for bit; against spgpu?mvInterleave ->
spgpu?hellspmm -> spgpu?mvDeinterleave on the device, bit for bit (the header's claim); and against exact sums
(exact_ref.spmm), a bound that does not restate the kernel's order of additions.

Every multivector is built by _Mv: the elements between the end of a vector and the next pitch, those behind the last vector
and those in front of a shifted base hold NaN where the call may only read (X, Y) and a sentinel where it may write (Z),
and every call checks that the sentinel is still there."""
import ctypes as C
import os

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -7777.25
RAN = set()   # node ids of the tests of this file that were run (test_zz_no_case_was_skipped)


@pytest.fixture(autouse=True)
def _ran(request):
    """A test skipped by a mark or a condition is never set up, so it never gets here; no test of this file skips itself."""
    RAN.add(request.node.nodeid)
    yield


def _hell(name):
    with np.load(os.path.join(GOLD, name + ".npz")) as f:
        g = {k: f[k] for k in f.files}
    letter = O.LETTER_OF[g["coo_vals"].dtype]
    hell = dict(letter=letter, rows=int(g["n_rows"]), values=g["hell_values"], indices=g["hell_indices"],
                hack_offsets=g["hell_hack_offsets"], hack_size=int(g["hack_size"]), row_lengths=g["row_lengths"],
                base=int(g["base"]), height=int(g["hell_height"]))
    return g, letter, hell


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Mv:
    """`count` vectors of `n` elements in the pitch layout inside one device buffer: `shift` elements in front of the base,
    vector j at base + j*pitch, 5 elements behind the last vector; everything that is not a vector holds `gap`."""

    def __init__(self, cols2d, pitch, shift=0, gap=np.nan):
        from spgpu_amd import formats
        n, count = cols2d.shape
        assert pitch >= n
        self.n, self.count, self.pitch, self.shift = n, count, pitch, shift
        host = np.full(shift + count * pitch + 5, gap, dtype=cols2d.dtype)
        self.is_gap = np.ones(host.size, dtype=bool)
        for j in range(count):
            host[shift + j * pitch:shift + j * pitch + n] = cols2d[:, j]
            self.is_gap[shift + j * pitch:shift + j * pitch + n] = False
        self.before = host.copy()
        self.dev = formats.to_device(host)

    @property
    def ptr(self):
        return C.c_void_p(self.dev.data_ptr() + self.shift * self.dev.element_size())

    def vectors(self):
        """[n, count] host array of the vectors; asserts that nothing outside them changed, bit for bit."""
        host = self.dev.cpu().numpy()
        assert host[self.is_gap].tobytes() == self.before[self.is_gap].tobytes(), "elements outside the vectors were written"
        s, p, n = self.shift, self.pitch, self.n
        return np.stack([host[s + j * p:s + j * p + n] for j in range(self.count)], axis=1)


def _call(gpu, letter, mat, z, y, alpha, x, beta, count):
    from spgpu_amd import capi
    capi.hellspmm_mv[letter](gpu, z.ptr, y.ptr if y is not None else None, capi.scalar(letter, alpha), _p(mat.cM), _p(mat.rP),
                             mat.hack_size, _p(mat.hack_offsets), _p(mat.rS), _p(mat.rIdx), 0, mat.rows, x.ptr,
                             capi.scalar(letter, beta), mat.base, count, x.pitch, z.pitch)


def _via_interleaved(gpu, letter, mat, z, y, alpha, x, beta, count):
    """What the header promises the same bits as: mvInterleave -> spgpu?hellspmm -> mvDeinterleave, on the device, on the same
    data.  Returns Z as an [n, count] host array."""
    import torch
    from spgpu_amd import capi
    dt = x.dev.dtype
    xi = torch.empty(x.n * count, dtype=dt, device="cuda:0")
    zi = torch.full((z.n * count,), float("nan"), dtype=dt, device="cuda:0")
    capi.mv_interleave[letter](gpu, _p(xi), count, x.ptr, x.pitch, x.n, count)
    yi = None
    if y is not None:
        yi = zi if y is z else torch.empty_like(zi)
        capi.mv_interleave[letter](gpu, _p(yi), count, y.ptr, y.pitch, y.n, count)
    capi.hellspmm[letter](gpu, _p(zi), _p(yi), capi.scalar(letter, alpha), _p(mat.cM), _p(mat.rP), mat.hack_size,
                          _p(mat.hack_offsets), _p(mat.rS), _p(mat.rIdx), 0, mat.rows, _p(xi), capi.scalar(letter, beta), mat.base,
                          count, count, count)
    back = torch.empty_like(zi)
    capi.mv_deinterleave[letter](gpu, _p(back), z.n, _p(zi), count, z.n, count)
    torch.cuda.synchronize()
    return np.ascontiguousarray(back.cpu().numpy().reshape(count, z.n).T)


def _same_bits(got, want, case=""):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), case


@pytest.mark.parametrize("count", [1, 3, 4, 7, 8, 16, 21, 32])
@pytest.mark.parametrize("name", ["powerlaw_d_b0_h32", "powerlaw_s_b1_h64", "lap3d_16_d", "ctest_s"])
def test_mv_matches_oracle_and_the_interleaved_call(gpu, name, count):
    """Both types, both index bases, hack sizes 32 and 64, ragged and regular rows; Z holds NaN before the call.  pitch =
    the vector length rounded up to 16 bytes' worth, bases as the allocator gives them: the fast shape."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, hell = _hell(name)
    rows, n_cols = hell["rows"], int(g["n_cols"])
    Xk = synth.values_for(letter, 100 + count, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for(letter, 200 + count, rows * count).reshape(rows, count)
    mat = formats.DeviceHell(hell)
    px, pz = (n_cols + 3) // 4 * 4, (rows + 3) // 4 * 4
    x, y = _Mv(Xk, px), _Mv(Yk, pz)
    for beta in (0.0, -0.5):
        z = _Mv(np.full_like(Yk, np.nan), pz, gap=SENTINEL)
        _call(gpu, letter, mat, z, y, 1.25, x, beta, count)
        torch.cuda.synchronize()
        got = z.vectors()
        _same_bits(got, O.hell_spmm(hell, Xk, Yk if beta != 0 else None, 1.25, beta), (name, count, beta, "oracle"))
        _same_bits(got, _via_interleaved(gpu, letter, mat, z, y if beta != 0 else None, 1.25, x, beta, count),
                   (name, count, beta, "interleaved"))


def test_mv_within_exact_sums_with_row_order_in_place(gpu):
    """The independent bound: exact sums of the products (exact_ref), as test_spmm_leading_dimensions_row_reorder_and_in_place
    has it for the interleaved call -- here with pitches larger than the vectors, a row order and Z == Y."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, hell = _hell("powerlaw_d_b1_h64")
    n_cols, rows, count = int(g["n_cols"]), hell["rows"], 6
    Xk = synth.values_for("D", 1, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for("D", 2, rows * count).reshape(rows, count)
    perm = np.random.default_rng(4).permutation(rows).astype(np.int32)
    mat = formats.DeviceHell(hell, r_idx=perm)
    x, z = _Mv(Xk, n_cols + 10), _Mv(Yk, rows + 6, gap=SENTINEL)
    _call(gpu, letter, mat, z, z, 2.0, x, 0.75, count)
    torch.cuda.synchronize()
    got = z.vectors()
    _same_bits(got, O.hell_spmm(hell, Xk, Yk, 2.0, 0.75, r_idx=perm), "oracle")
    r, c, v = X.hell_coo(hell)
    exact, scale = X.spmm(rows, r, c, v, Xk, Yk, 2.0, 0.75, count, r_idx=perm, base=hell["base"])
    X.assert_within(got, exact, scale, "D", "pitch layout, rIdx, in place")


@pytest.mark.parametrize("count", [16, 5])
@pytest.mark.parametrize("name", ["powerlaw_d_b0_h32", "powerlaw_s_b1_h64"])
def test_mv_pitches_larger_than_the_vectors(gpu, name, count):
    """pitchX != pitchYZ, both larger than the vector lengths (multiples of 16 bytes: the fast shape): the gaps and the elements
    behind the last vector hold NaN in X and Y -- none may reach Z -- and a sentinel in Z, found unchanged."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, hell = _hell(name)
    rows, n_cols = hell["rows"], int(g["n_cols"])
    Xk = synth.values_for(letter, 11, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for(letter, 12, rows * count).reshape(rows, count)
    mat = formats.DeviceHell(hell)
    x, y = _Mv(Xk, (n_cols + 3) // 4 * 4 + 64), _Mv(Yk, (rows + 3) // 4 * 4 + 12)
    for beta in (0.0, 0.5):
        z = _Mv(np.full_like(Yk, np.nan), y.pitch, gap=SENTINEL)
        _call(gpu, letter, mat, z, y, -1.5, x, beta, count)
        torch.cuda.synchronize()
        got = z.vectors()   # checks the sentinels
        assert not np.isnan(got).any()
        _same_bits(got, O.hell_spmm(hell, Xk, Yk if beta != 0 else None, -1.5, beta), (name, count, beta))


@pytest.mark.parametrize("beta", [0.75, 1.0])
@pytest.mark.parametrize("name", ["powerlaw_d_b0_h32", "powerlaw_s_b1_h64"])
def test_mv_row_order_and_in_place(gpu, name, beta):
    """rIdx (a random permutation) with Z == Y; with beta == 1 on a matrix some of whose rows are emptied (rS zeroed): their Z
    entries hold NaN before the call and after it -- neither read nor written.  Then the same without rIdx (16-byte runs)."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, hell = _hell(name)
    rows, n_cols, count = hell["rows"], int(g["n_cols"]), 16
    rng = np.random.default_rng(7)
    if beta == 1.0:
        hell = dict(hell, row_lengths=hell["row_lengths"].copy())
        hell["row_lengths"][rng.choice(rows, size=rows // 3, replace=False)] = 0
    empty = np.flatnonzero(hell["row_lengths"][:rows] == 0)
    assert beta != 1.0 or empty.size >= rows // 3
    Xk = synth.values_for(letter, 21, n_cols * count).reshape(n_cols, count)
    perm = rng.permutation(rows).astype(np.int32)
    for r_idx in (perm, None):
        Z0 = synth.values_for(letter, 22, rows * count).reshape(rows, count).copy()
        if beta == 1.0:
            Z0[empty if r_idx is None else perm[empty]] = np.nan
        mat = formats.DeviceHell(hell, r_idx=r_idx)
        x, z = _Mv(Xk, (n_cols + 3) // 4 * 4), _Mv(Z0, (rows + 3) // 4 * 4 + 4, gap=SENTINEL)
        _call(gpu, letter, mat, z, z, 0.5, x, beta, count)
        torch.cuda.synchronize()
        got = z.vectors()
        want = O.hell_spmm(hell, Xk, Z0, 0.5, beta, r_idx=r_idx, in_place=True)
        _same_bits(got, want, (name, beta, r_idx is not None))
        if beta == 1.0:
            out_rows = empty if r_idx is None else perm[empty]
            assert np.isnan(got[out_rows]).all()
            keep = np.ones(rows, dtype=bool)
            keep[out_rows] = False
            assert not np.isnan(got[keep]).any()


def test_mv_matrix_without_entries(gpu):
    """empty_d: every rS is 0.  beta == 0 writes zeros, Z == Y with beta == 1 touches nothing (NaN stays), beta == -2 scales."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, hell = _hell("empty_d")
    rows, n_cols, count = hell["rows"], int(g["n_cols"]), 5
    Xk = synth.values_for("D", 1, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for("D", 2, rows * count).reshape(rows, count)
    mat = formats.DeviceHell(hell)
    x, y = _Mv(Xk, n_cols), _Mv(Yk, rows)
    z = _Mv(np.full_like(Yk, np.nan), rows + 2, gap=SENTINEL)
    y2 = _Mv(Yk, rows + 2)
    _call(gpu, "D", mat, z, None, 1.0, x, 0.0, count)
    torch.cuda.synchronize()
    _same_bits(z.vectors(), O.hell_spmm(hell, Xk, None, 1.0, 0.0), "beta 0")
    _call(gpu, "D", mat, z, y2, 1.0, x, -2.0, count)
    torch.cuda.synchronize()
    _same_bits(z.vectors(), O.hell_spmm(hell, Xk, Yk, 1.0, -2.0), "beta -2")
    zn = _Mv(np.full_like(Yk, np.nan), rows, gap=SENTINEL)
    _call(gpu, "D", mat, zn, zn, 1.0, x, 1.0, count)
    torch.cuda.synchronize()
    assert np.isnan(zn.vectors()).all()
    del y


@pytest.mark.parametrize("count", [16, 9, 3])
@pytest.mark.parametrize("name,hs", [("powerlaw_d_b0_h32", 48), ("powerlaw_s_b0_h32", 80), ("powerlaw_d_b0_h32", 32)])
def test_mv_fallback_shape(gpu, name, hs, count):
    """What the fast shape does not take: bases one element off 16-byte alignment, odd pitches, and a hackSize that is not a
    multiple of 32 (rebuilt with the host converters from the golden COO; hackSize 32 keeps the strip kernel but with
    element-wise fill and stores).  Same bits as the oracle and as the interleaved call."""
    import torch
    from spgpu_amd import formats, synth
    g, letter, _ = _hell(name)
    rows, n_cols = int(g["n_rows"]), int(g["n_cols"])
    hell = formats.ell_to_hell(formats.coo_to_ell(rows, g["coo_rows"], g["coo_cols"], g["coo_vals"], coo_base=int(g["base"]),
                                                  ell_base=1), hs)
    assert hell["hack_size"] == hs and hell["rows"] == rows
    Xk = synth.values_for(letter, 31, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for(letter, 32, rows * count).reshape(rows, count)
    mat = formats.DeviceHell(hell)
    x = _Mv(Xk, n_cols + 1 + n_cols % 2, shift=1)          # odd pitch
    y = _Mv(Yk, rows + 3 + rows % 2, shift=1)
    assert x.pitch % 2 == 1 and y.pitch % 2 == 1
    for beta in (0.0, 0.25):
        z = _Mv(np.full_like(Yk, np.nan), y.pitch, shift=1, gap=SENTINEL)
        _call(gpu, letter, mat, z, y, 2.0, x, beta, count)
        torch.cuda.synchronize()
        got = z.vectors()
        _same_bits(got, O.hell_spmm(hell, Xk, Yk if beta != 0 else None, 2.0, beta), (name, hs, count, beta, "oracle"))
        _same_bits(got, _via_interleaved(gpu, letter, mat, z, y if beta != 0 else None, 2.0, x, beta, count),
                   (name, hs, count, beta, "interleaved"))


@pytest.mark.parametrize("count", [16, 8])
@pytest.mark.parametrize("pattern", ["banded", "window", "random"])
def test_mv_many_workgroups_against_the_interleaved_call(gpu, pattern, count):
    """262 144 rows x 32: a thousand workgroups, X far wider than one LDS tile.  banded: every workgroup stages its window (tile
    boundaries, band wavefronts and -- the columns wrap -- their neighbours); window / random: the columns of a workgroup
    miss the tile and come as one gather per vector.  Bit for bit spgpu?hellspmm on the interleaved copy of the same data."""
    import torch
    from spgpu_amd import capi, synth
    n, L = 262_144, 32
    h = synth.hell_uniform_on_device(n, L, pattern, "D", 32, seed=11)
    Xp = synth.device_vector(n * count, "D", 12)      # vector j at j*n
    Yp = synth.device_vector(n * count, "D", 13)
    Zp = torch.full_like(Yp, float("nan"))
    Xi = Xp.view(count, n).t().contiguous()
    Yi = Yp.view(count, n).t().contiguous()
    Zi = torch.full_like(Yi, float("nan"))
    torch.cuda.synchronize()
    for beta in (0.0, -0.25):
        capi.hellspmm_mv["D"](gpu, _p(Zp), _p(Yp), 1.5, _p(h["cM"]), _p(h["rP"]), 32, _p(h["hack_offsets"]), _p(h["rS"]), None, L, n,
                              _p(Xp), beta, 0, count, n, n)
        capi.hellspmm["D"](gpu, _p(Zi), _p(Yi), 1.5, _p(h["cM"]), _p(h["rP"]), 32, _p(h["hack_offsets"]), _p(h["rS"]), None, L, n,
                           _p(Xi), beta, 0, count, count, count)
        torch.cuda.synchronize()
        got = Zp.view(count, n).t().contiguous()
        assert not torch.isnan(got).any()
        assert torch.equal(got.view(torch.int64), Zi.view(torch.int64)), (pattern, count, beta)
        Zp.fill_(float("nan"))
        Zi.fill_(float("nan"))


def test_mv_captured_into_a_graph(gpu):
    """No allocation, no state, no host synchronisation: captured on the handle's stream and replayed twice, the eager bits --
    with new X values between the replays, so that a replay is seen to compute."""
    import torch
    from spgpu_amd import capi, formats, synth
    g, letter, hell = _hell("lap3d_16_d")
    rows, n_cols, count = hell["rows"], int(g["n_cols"]), 16
    Xk = synth.values_for("D", 41, n_cols * count).reshape(n_cols, count)
    Yk = synth.values_for("D", 42, rows * count).reshape(rows, count)
    mat = formats.DeviceHell(hell)
    x, y = _Mv(Xk, n_cols), _Mv(Yk, rows)
    z = _Mv(np.full_like(Yk, np.nan), rows, gap=SENTINEL)
    stream = torch.cuda.Stream()
    capi.spgpuSetStream(gpu, C.c_void_p(stream.cuda_stream))
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(stream):
            _call(gpu, "D", mat, z, y, 1.25, x, -0.5, count)
        stream.synchronize()
        eager = z.vectors()
        _same_bits(eager, O.hell_spmm(hell, Xk, Yk, 1.25, -0.5), "eager")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            _call(gpu, "D", mat, z, y, 1.25, x, -0.5, count)
        torch.cuda.synchronize()
        for replay in range(2):
            z.dev[~torch.from_numpy(z.is_gap).to("cuda:0")] = float("nan")
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            _same_bits(z.vectors(), eager, f"replay {replay}")
        x.dev.mul_(0.5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(z.vectors(), O.hell_spmm(hell, Xk * 0.5, Yk, 1.25, -0.5), "replay on new X")
        del graph
    finally:
        capi.spgpuSetStream(gpu, None)


def test_zz_no_case_was_skipped(request):
    """Every case above is mandatory.  This test is the last of the file: of the tests of this file selected for the run, each
    one before it must have been run (a failed one has; a skipped one has not)."""
    mine = [item.nodeid for item in request.session.items
            if item.fspath == request.node.fspath and item.nodeid != request.node.nodeid]
    skipped = [nodeid for nodeid in mine if nodeid not in RAN]
    assert not skipped, skipped
    if not request.config.getoption("keyword") and not any("::" in arg for arg in request.config.args):
        assert len(mine) == 32 + 1 + 4 + 4 + 1 + 9 + 6 + 1, len(mine)   # the whole file was asked for: the whole file ran
