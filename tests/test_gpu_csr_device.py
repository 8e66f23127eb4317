"""GPU: device-side CSR -> ELL / HELL construction (include/spgpu/ext/csr_device.h): the bytes of the COO route
(include/spgpu/convert_device.h) and of the host converters (byte-identical to the reference's) for the same matrix, with no sort:
entry order of the CSR, duplicates, both index bases on either side, all four value types, hack sizes that are and are not
multiples of 32, rows of any length, a row order through rIdx, and the two fills behind the calls (one thread per row; a
wavefront per 32 rows transposing through LDS) giving the same bytes.

Every conversion of the small matrices here runs THREE times -- the public call and each fill through the unexported
spgpuCsrTo{Ell,Hell}DeviceWith -- and the three results must be the same bytes (_csr_convert)."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O
from test_gpu_convert_device import _hosts, _same

pytestmark = pytest.mark.gpu


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _upload(a, offset=0):
    """numpy array -> HBM at `offset` bytes behind the start of an allocation of its own; (the allocation, the address)."""
    import torch
    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    buf = torch.zeros(offset + max(raw.size, 16), dtype=torch.uint8, device="cuda:0")
    if raw.size:
        buf[offset:offset + raw.size] = torch.from_numpy(raw.copy()).to("cuda:0")
    return buf, buf.data_ptr() + offset


def _zeros(n, dtype):
    from spgpu_amd import formats
    return formats.to_device(np.zeros(max(n, 1), dtype))


def _row_lengths(gpu, n_rows, d_ptr, csr_base):
    """spgpuCsrRowLengthsDevice: (status, longest row, device lengths)."""
    import torch
    from spgpu_amd import capi
    rs = torch.full((max(n_rows, 1),), -7, dtype=torch.int32, device="cuda:0")
    longest = C.c_int(-1)
    torch.cuda.synchronize()
    st = capi.spgpuCsrRowLengthsDevice(gpu, _p(rs), C.byref(longest), n_rows, _p(d_ptr), csr_base)
    return st, longest.value, rs


def _hell_plan(gpu, n_rows, hack_size, dest_lengths):
    """spgpuHellPlanDevice on the lengths in destination order, with the `work` the header promises is enough."""
    import torch
    from spgpu_amd import capi
    work = torch.empty(capi.spgpuCooConvertWorkBytes(n_rows, 0), dtype=torch.uint8, device="cuda:0")
    hacks = (n_rows + hack_size - 1) // hack_size
    ho = torch.zeros(max(hacks, 1), dtype=torch.int32, device="cuda:0")
    height = C.c_int(-1)
    assert capi.spgpuHellPlanDevice(gpu, C.byref(height), _p(ho), hack_size, n_rows, _p(dest_lengths), _p(work)) == capi.SPGPU_SUCCESS
    return height.value, ho


def _to_hell(gpu, which, hv, hi, ho, hack_size, out_base, n_rows, d_ptr, cols_at, vals_at, csr_base, code, d_ridx, max_blocks=0):
    """which None: the public call; else the fill of that number through the unexported entry point."""
    from spgpu_amd import capi
    args = (gpu, _p(hv), _p(hi), _p(ho), hack_size, out_base, n_rows, _p(d_ptr), C.c_void_p(cols_at), C.c_void_p(vals_at), csr_base,
            code, _p(d_ridx))
    return capi.spgpuCsrToHellDevice(*args) if which is None else capi.spgpuCsrToHellDeviceWith(*args, which, max_blocks)


def _csr_convert(gpu, n_rows, row_ptr, cols, vals, csr_base, out_base, hack_size, r_idx=None, misalign=False, ell=True):
    """Runs the device calls on host CSR arrays; returns (ell dict, hell dict) of numpy arrays with the keys of the host converters.
    misalign: the column and value arrays start one element (8 bytes for the 16-byte type) behind a 16-byte boundary."""
    import torch
    from spgpu_amd import capi, formats
    vals = np.ascontiguousarray(vals)
    code = capi.TYPE_CODE[formats.LETTER_OF[np.dtype(vals.dtype)]]
    d_ptr = formats.to_device(np.ascontiguousarray(row_ptr, np.int32))
    cols_buf, cols_at = _upload(np.ascontiguousarray(cols, np.int32), 4 if misalign else 0)
    vals_buf, vals_at = _upload(vals, min(vals.dtype.itemsize, 8) if misalign else 0)
    st, longest, rs = _row_lengths(gpu, n_rows, d_ptr, csr_base)
    assert st == capi.SPGPU_SUCCESS
    d_ridx = None if r_idx is None else formats.to_device(np.ascontiguousarray(r_idx, np.int32))
    dest = rs if r_idx is None else rs[d_ridx.long()].contiguous()      # plumbing: the lengths in destination order
    height, ho = _hell_plan(gpu, n_rows, hack_size, dest)
    slots, hacks = hack_size * height, (n_rows + hack_size - 1) // hack_size
    pitch = capi.computeEllAllocPitch(n_rows)
    results = []
    for which in (None, capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE):
        hv, hi = _zeros(slots, vals.dtype), _zeros(slots, np.int32)
        torch.cuda.synchronize()
        assert _to_hell(gpu, which, hv, hi, ho, hack_size, out_base, n_rows, d_ptr, cols_at, vals_at, csr_base, code,
                        d_ridx) == capi.SPGPU_SUCCESS
        got = dict(hell_values=hv.cpu().numpy()[:slots], hell_indices=hi.cpu().numpy()[:slots])
        if ell:
            ev, ei = _zeros(longest * pitch, vals.dtype), _zeros(longest * pitch, np.int32)
            torch.cuda.synchronize()
            args = (gpu, _p(ev), _p(ei), pitch, pitch, out_base, n_rows, _p(d_ptr), C.c_void_p(cols_at), C.c_void_p(vals_at), csr_base,
                    code, _p(d_ridx))
            st = capi.spgpuCsrToEllDevice(*args) if which is None else capi.spgpuCsrToEllDeviceWith(*args, which, 0)
            assert st == capi.SPGPU_SUCCESS
            got.update(ell_values=ev.cpu().numpy()[:longest * pitch], ell_indices=ei.cpu().numpy()[:longest * pitch])
        results.append(got)
    for other in results[1:]:       # the plain and the transposing fill, and whichever of them the public call runs
        for key, a in results[0].items():
            assert a.tobytes() == other[key].tobytes(), key
    pub = results[0]
    ell_d = dict(max_row=longest, pitch=pitch, row_lengths=dest.cpu().numpy()[:n_rows], values=pub.get("ell_values"),
                 indices=pub.get("ell_indices"))
    hell_d = dict(height=height, hack_offsets=ho.cpu().numpy()[:hacks], values=pub["hell_values"], indices=pub["hell_indices"])
    del cols_buf, vals_buf
    return ell_d, hell_d


def _against_hosts(ell_d, hell_d, n_rows, r, c, v, csr_base, out_base, hack_size):
    """The three reference sets of test_gpu_convert_device.py on the COO form of the same matrix."""
    for _, host in _hosts():
        ell_h = host.coo_to_ell(n_rows, r, c, v, coo_base=csr_base, ell_base=out_base)
        hell_h = host.ell_to_hell(ell_h, hack_size)
        _same(ell_d, ell_h, ("max_row", "pitch", "row_lengths", "indices", "values"))
        _same(hell_d, hell_h, ("height", "hack_offsets", "indices", "values"))


# ---- 1. random matrices ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_random_csr_matches_host_converters(gpu, letter):
    """Shuffled COO with duplicates made CSR by a stable sort: the host converters on the COO give the bytes to match; the two
    index bases are drawn independently, the hack size from {32, 64, 96} with one case of 48."""
    from spgpu_amd import synth
    from test_oracle_vs_reference import _random_coo
    rng = np.random.default_rng(700 + ord(letter))
    for trial in range(10):
        csr_base, out_base = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        hs = 48 if trial == 3 else int(rng.choice([32, 64, 96]))
        n_rows, n_cols, r, c, v = _random_coo(rng, letter, csr_base)
        row_ptr, cc, vv = synth.coo_to_csr(n_rows, r, c, v, csr_base)
        ell_d, hell_d = _csr_convert(gpu, n_rows, row_ptr, cc, vv, csr_base, out_base, hs)
        _against_hosts(ell_d, hell_d, n_rows, r, c, v, csr_base, out_base, hs)


# ---- 2. chunk edges ---------------------------------------------------------------------------------------------------
_EDGE_ROWS = 97
_EDGE_EMPTY = (0, 31, 32, 47, 48, 63, 64, 91, 95, 96)     # first and last rows of hacks of 32, 48 and 64, and of the matrix


def _edge_lengths():
    lengths = np.arange(_EDGE_ROWS, dtype=np.int64)       # row i has i entries for i < 90 ...
    lengths[90:] = (5, 0, 1000, 2, 40, 0, 0)              # ... one row of 1 000 entries among the last few
    lengths[list(_EDGE_EMPTY)] = 0
    return lengths


def _edge_matrix(letter, base):
    from spgpu_amd import synth
    lengths = _edge_lengths()
    n, m, r, c, v = synth.random_rows_coo(_EDGE_ROWS, 1500, lengths, seed=17, letter=letter, base=base)
    return lengths, r, c, v


@pytest.mark.parametrize("letter", "SDCZ")
def test_chunk_edges_and_unaligned_runs(gpu, letter):
    """97 rows (no multiple of 32 or of a hack size used), row i of length i, empty rows at both ends of hacks, one row of 1 000
    entries, lengths K-1, K, K+1 and 2K+1 around the transposing fill's chunk width K -- read from the library, so a new K
    fails the assertion here instead of leaving its edges untested.

    ALIGNMENT.  With row i of length i the runs start at every element offset, so no choice of the first row keeps all of them
    off 16-byte boundaries for the 4- and 8-byte types.  What is pinned instead: the column and value arrays themselves start
    one element (8 bytes for complex fp64) behind a 16-byte boundary, so the first run is unaligned, the runs of complex fp64
    are ALL unaligned, and for the other types the run starts take every residue an element-aligned address has."""
    from spgpu_amd import capi, synth
    K = capi.CSR_FILL_CHUNK
    lengths = _edge_lengths()
    present = set(lengths.tolist())
    assert {K - 1, K, K + 1, 2 * K + 1} <= present, (K, sorted(present))
    assert 1000 in present and lengths[0] == 0 and lengths[-1] == 0
    size = np.dtype(O.NP_DTYPE[letter]).itemsize
    starts = (np.cumsum(lengths) - lengths)[lengths > 0] * size + min(size, 8)     # byte addresses past a 16-byte boundary
    assert set((starts % 16).tolist()) == {(min(size, 8) + size * j) % 16 for j in range(4)}
    assert starts[0] % 16 != 0 and (size < 16 or (starts % 16 != 0).all())
    for base, out_base, hs in ((0, 1, 32), (1, 0, 48), (1, 1, 64)):
        _, r, c, v = _edge_matrix(letter, base)
        row_ptr, cc, vv = synth.coo_to_csr(_EDGE_ROWS, r, c, v, base)
        assert (np.diff(row_ptr) == lengths).all()
        ell_d, hell_d = _csr_convert(gpu, _EDGE_ROWS, row_ptr, cc, vv, base, out_base, hs, misalign=True)
        _against_hosts(ell_d, hell_d, _EDGE_ROWS, r, c, v, base, out_base, hs)


# ---- 3. bits, not numbers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_values_are_moved_as_bits(gpu, letter):
    """Random 32-, 64- and 128-bit patterns viewed as the type -- NaNs with payloads, denormals, -0 among them and planted: every
    stored value is its CSR entry's bytes (placed here by the slot formula, independently of any converter), every other slot
    the caller's zero bytes; and the host converters agree."""
    from spgpu_amd import synth
    rng = np.random.default_rng(900 + ord(letter))
    dtype = np.dtype(O.NP_DTYPE[letter])
    n_rows, hs = 150, 32
    lengths = rng.integers(0, 40, n_rows)
    nnz = int(lengths.sum())
    words = rng.integers(0, 1 << 32, size=nnz * dtype.itemsize // 4, dtype=np.uint64).astype(np.uint32)
    words[0:8] = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FF80000, 0xFFF00001)
    v = words.view(dtype)
    assert v.size == nnz
    r = np.repeat(np.arange(n_rows), lengths).astype(np.int32)
    c = rng.integers(0, 500, nnz).astype(np.int32)
    row_ptr, cc, vv = synth.coo_to_csr(n_rows, r, c, v, 0)
    assert vv.tobytes() == v.tobytes()
    ell_d, hell_d = _csr_convert(gpu, n_rows, row_ptr, cc, vv, 0, 0, hs)
    k = np.arange(nnz) - np.repeat(row_ptr[:-1].astype(np.int64), lengths)
    slot = hell_d["hack_offsets"].astype(np.int64)[r // hs] + r % hs + k * hs
    want = np.zeros((hell_d["values"].size, dtype.itemsize), np.uint8)
    want[slot] = v.view(np.uint8).reshape(nnz, dtype.itemsize)
    assert hell_d["values"].tobytes() == want.tobytes()
    want_ell = np.zeros((ell_d["values"].size, dtype.itemsize), np.uint8)
    want_ell[r + k * ell_d["pitch"]] = v.view(np.uint8).reshape(nnz, dtype.itemsize)
    assert ell_d["values"].tobytes() == want_ell.tobytes()
    _against_hosts(ell_d, hell_d, n_rows, r, c, v, 0, 0, hs)


# ---- 4. row order -------------------------------------------------------------------------------------------------------
_ORDERED = {}


def _ordered_case(gpu):
    """Power-law lengths (50 000 rows, mean 12, longest 2 048) ordered with spgpuOellOrderAlignedDevice(2048, 256): the CSR route of
    the header's five calls and, on the same matrix as COO, the route of INTEGRATION.md for COO holders.  Built once."""
    if _ORDERED:
        return _ORDERED
    import torch
    from spgpu_amd import capi, formats, synth
    n = 50_000
    lengths = synth.power_law_lengths(n, 12.0, 2048, seed=11)
    rows_t, cols_t, vals_t = synth.ragged_coo_on_device(lengths, n, "near", 1024, "D", seed=12)
    r, c, v = rows_t.cpu().numpy(), cols_t.cpu().numpy(), vals_t.cpu().numpy()
    row_ptr, cc, vv = synth.coo_to_csr(n, r, c, v, 0)
    assert cc.tobytes() == c.tobytes()                    # the generator is row-major: the CSR arrays are the COO arrays
    d_ptr = formats.to_device(row_ptr)
    st, longest, rs = _row_lengths(gpu, n, d_ptr, 0)
    assert st == capi.SPGPU_SUCCESS and longest == int(lengths.max()) and rs.cpu().numpy().tobytes() == lengths.tobytes()
    order_work = torch.empty(capi.spgpuOellOrderWorkBytes(n), dtype=torch.uint8, device="cuda:0")
    r_idx = torch.empty(n, dtype=torch.int32, device="cuda:0")
    sorted_lengths = torch.empty(n, dtype=torch.int32, device="cuda:0")
    assert capi.spgpuOellOrderAlignedDevice(gpu, _p(r_idx), _p(sorted_lengths), _p(rs), n, 2048, 256, _p(order_work)) == capi.SPGPU_SUCCESS
    height, ho = _hell_plan(gpu, n, 32, sorted_lengths)
    slots = 32 * height
    code = capi.TYPE_CODE["D"]
    fills = {}
    for which in (None, capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE):
        hv, hi = _zeros(slots, np.float64), _zeros(slots, np.int32)
        torch.cuda.synchronize()
        assert _to_hell(gpu, which, hv, hi, ho, 32, 0, n, d_ptr, cols_t.data_ptr(), vals_t.data_ptr(), 0, code, r_idx) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        fills[which] = (hv, hi)
    coo = formats.coo_to_ordered_hell_device(gpu, n, rows_t, cols_t, vals_t, "D", 32, 2048, 256, aligned=True)
    _ORDERED.update(n=n, lengths=lengths, coo_host=(r, c, v), r_idx=r_idx, sorted_lengths=sorted_lengths, height=height, ho=ho,
                    slots=slots, fills=fills, coo=coo)
    return _ORDERED


def test_row_order_equals_the_coo_route_on_the_gpu(gpu):
    import torch
    case = _ordered_case(gpu)
    coo, slots = case["coo"], case["slots"]
    hv, hi = case["fills"][None]
    assert coo["slots"] == slots
    assert torch.equal(coo["rIdx"][:case["n"]], case["r_idx"]) and torch.equal(coo["rS"][:case["n"]], case["sorted_lengths"])
    assert torch.equal(coo["hack_offsets"], case["ho"])
    assert torch.equal(coo["rP"][:slots], hi[:slots])
    assert torch.equal(coo["cM"][:slots].view(torch.int64), hv[:slots].view(torch.int64))


def test_row_order_equals_the_host_converters_on_renumbered_rows(gpu):
    from spgpu_amd import formats
    case = _ordered_case(gpu)
    n, (r, c, v) = case["n"], case["coo_host"]
    r_idx = case["r_idx"].cpu().numpy()
    want_idx, want_len = formats.oell_order(case["lengths"], 2048, 256, aligned=True)
    assert r_idx.tobytes() == want_idx.tobytes() and case["sorted_lengths"].cpu().numpy().tobytes() == want_len.tobytes()
    inverse = np.empty(n, np.int64)
    inverse[r_idx] = np.arange(n)
    hv, hi = case["fills"][None]
    hell_d = dict(height=case["height"], hack_offsets=case["ho"].cpu().numpy()[:(n + 31) // 32],
                  values=hv.cpu().numpy()[:case["slots"]], indices=hi.cpu().numpy()[:case["slots"]], row_lengths=want_len)
    for _, host in _hosts():
        hell_h = host.ell_to_hell(host.coo_to_ell(n, inverse[r], c, v), 32)
        _same(hell_d, hell_h, ("height", "hack_offsets", "row_lengths", "indices", "values"))


def test_spmv_on_the_csr_built_arrays(gpu):
    """spgpuDhellspmv with rIdx on the CSR-built arrays: the bits of the same call on the COO-built arrays, and within the bound of
    the extended-precision product of the matrix as its rows come (tests/exact_ref.py, as test_gpu_adopt.py)."""
    import torch
    from spgpu_amd import capi, formats, synth
    case = _ordered_case(gpu)
    n, coo = case["n"], case["coo"]
    hv, hi = case["fills"][None]
    x, y = synth.values_for("D", 41, n), synth.values_for("D", 42, n)
    dx, dy = formats.to_device(x), formats.to_device(y)
    alpha, beta = -0.5, 2.0
    out = []
    for cM, rP, ho, rs, ridx in ((hv, hi, case["ho"], case["sorted_lengths"], case["r_idx"]),
                                 (coo["cM"], coo["rP"], coo["hack_offsets"], coo["rS"], coo["rIdx"])):
        dz = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        capi.hellspmv["D"](gpu, _p(dz), _p(dy), capi.scalar("D", alpha), _p(cM), _p(rP), 32, _p(ho), _p(rs), _p(ridx), 12, n, _p(dx),
                           capi.scalar("D", beta), 0)
        torch.cuda.synchronize()
        out.append(dz.cpu().numpy())
    assert out[0].tobytes() == out[1].tobytes()
    r, c, v = case["coo_host"]
    exact, scale = X.spmv(n, r, c, v, x, y, alpha, beta, base=0)
    X.assert_within(out[0], exact, scale, "D", "csr-built ordered HELL")


@pytest.mark.parametrize("letter", "SZ")
def test_ell_with_a_random_permutation(gpu, letter):
    """70 rows, rIdx a random permutation, ELL (and HELL with a hack of 48) with both fills: destination row i is CSR row rIdx[i],
    i.e. the host converters on the COO whose row r has become row inverse[r]."""
    from spgpu_amd import synth
    rng = np.random.default_rng(55)
    n = 70
    lengths = rng.integers(0, 45, n)
    _, _, r, c, v = synth.random_rows_coo(n, 300, lengths, seed=23, letter=letter, base=1)
    row_ptr, cc, vv = synth.coo_to_csr(n, r, c, v, 1)
    r_idx = rng.permutation(n).astype(np.int32)
    inverse = np.empty(n, np.int64)
    inverse[r_idx] = np.arange(n)
    ell_d, hell_d = _csr_convert(gpu, n, row_ptr, cc, vv, 1, 0, 48, r_idx=r_idx)
    assert ell_d["row_lengths"].tolist() == lengths[r_idx].tolist()
    _against_hosts(ell_d, hell_d, n, (inverse[r - 1] + 1).astype(np.int32), c, v, 1, 0, 48)


# ---- 5. both fills agree ----------------------------------------------------------------------------------------------
def test_both_fills_give_the_same_bytes(gpu):
    """The plain and the transposing fill on the matrices above.  _csr_convert compares them for every small matrix (tests 1 to 3);
    here explicitly: the chunk-edge matrix with a hack of 48, and the ordered power-law matrix.  Neither is the result of the
    other's code path: the public call runs exactly one of them (capi.CSR_FILL_DEFAULT)."""
    import torch
    from spgpu_amd import capi, synth
    assert capi.CSR_FILL_DEFAULT in (capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE)
    _, r, c, v = _edge_matrix("C", 0)
    row_ptr, cc, vv = synth.coo_to_csr(_EDGE_ROWS, r, c, v, 0)
    _csr_convert(gpu, _EDGE_ROWS, row_ptr, cc, vv, 0, 0, 48, misalign=True)         # asserts the three results equal
    case = _ordered_case(gpu)
    slots = case["slots"]
    pv, pi = case["fills"][capi.CSR_FILL_PLAIN]
    tv, ti = case["fills"][capi.CSR_FILL_TRANSPOSE]
    assert int((pi[:slots] != 0).sum()) > 0
    assert torch.equal(pi[:slots], ti[:slots]) and torch.equal(pv[:slots].view(torch.int64), tv[:slots].view(torch.int64))
    dv, di = case["fills"][None]
    assert torch.equal(di[:slots], ti[:slots]) and torch.equal(dv[:slots].view(torch.int64), tv[:slots].view(torch.int64))


# ---- 6. scale and grid stride -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "DS")
def test_300k_banded_rows_equal_the_coo_route(gpu, letter):
    """300 000 rows x 32, banded: 9 375 row groups -- more workgroups than the chip holds at once -- and, with the grid capped at 48
    workgroups through the unexported entry point, the grid stride of both fills; against the COO route on the GPU."""
    import torch
    from spgpu_amd import capi, formats, synth
    n, L = 300_000, 32
    rows_t, cols_t, vals_t = synth.ragged_coo_on_device(np.full(n, L), n, "band", 0, letter, seed=3)
    coo = formats.coo_to_ordered_hell_device(gpu, n, rows_t, cols_t, vals_t, letter, 32, order=False)
    d_ptr = torch.arange(0, (n + 1) * L, L, dtype=torch.int32, device="cuda:0")
    st, longest, rs = _row_lengths(gpu, n, d_ptr, 0)
    assert st == capi.SPGPU_SUCCESS and longest == L and torch.equal(rs, coo["rS"][:n])
    height, ho = _hell_plan(gpu, n, 32, rs)
    assert height * 32 == coo["slots"] and torch.equal(ho, coo["hack_offsets"])
    slots = coo["slots"]
    bits = torch.int64 if letter == "D" else torch.int32
    for which, max_blocks in ((None, 0), (capi.CSR_FILL_PLAIN, 0), (capi.CSR_FILL_TRANSPOSE, 0), (capi.CSR_FILL_PLAIN, 48),
                              (capi.CSR_FILL_TRANSPOSE, 48)):
        hv, hi = torch.zeros_like(coo["cM"]), torch.zeros_like(coo["rP"])
        torch.cuda.synchronize()
        assert _to_hell(gpu, which, hv, hi, ho, 32, 0, n, d_ptr, cols_t.data_ptr(), vals_t.data_ptr(), 0, capi.TYPE_CODE[letter], None,
                        max_blocks) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(hi[:slots], coo["rP"][:slots]), (which, max_blocks)
        assert torch.equal(hv[:slots].view(bits), coo["cM"][:slots].view(bits)), (which, max_blocks)


# ---- 7. degenerate and bad input ----------------------------------------------------------------------------------------
def test_degenerate_and_bad_input(gpu):
    import torch
    from spgpu_amd import capi, formats
    # no entries at all: nothing is written (the destination keeps what the caller put there)
    for base in (0, 1):
        d_ptr = formats.to_device(np.full(71, base, np.int32))
        st, longest, rs = _row_lengths(gpu, 70, d_ptr, base)
        assert st == capi.SPGPU_SUCCESS and longest == 0 and not rs.cpu().numpy().any()
        height, ho = _hell_plan(gpu, 70, 32, rs)
        assert height == 0 and not ho.cpu().numpy().any()
        spare_v, spare_i = torch.full((64,), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((64,), 7, dtype=torch.int32, device="cuda:0")
        none = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        for which in (None, capi.CSR_FILL_PLAIN, capi.CSR_FILL_TRANSPOSE):
            assert _to_hell(gpu, which, spare_v, spare_i, ho, 32, base, 70, d_ptr, none.data_ptr(), none.data_ptr(), base,
                            capi.TYPE_DOUBLE, None) == capi.SPGPU_SUCCESS
        assert capi.spgpuCsrToEllDevice(gpu, _p(spare_v), _p(spare_i), 128, 128, base, 70, _p(d_ptr), _p(none), _p(none), base,
                                        capi.TYPE_DOUBLE, None) == capi.SPGPU_SUCCESS
        torch.cuda.synchronize()
        assert (spare_v == 7.0).all() and (spare_i == 7).all()
    # one row
    for letter in "SZ":
        v = np.arange(1, 20).astype(O.NP_DTYPE[letter])
        r, c = np.zeros(19, np.int32), np.arange(19, dtype=np.int32)[::-1].copy()
        ell_d, hell_d = _csr_convert(gpu, 1, np.array([0, 19], np.int32), c, v, 0, 1, 32)
        _against_hosts(ell_d, hell_d, 1, r, c, v, 0, 1, 32)
    # a row pointer array that does not start at the base, and one that descends: reported
    for bad, base in (([1, 3, 5, 9], 0), ([0, 3, 5, 9], 1), ([0, 4, 3, 9], 0), ([1, 1, 1, 0], 1)):
        st, longest, _ = _row_lengths(gpu, 3, formats.to_device(np.array(bad, np.int32)), base)
        assert st == capi.SPGPU_UNSUPPORTED and longest == 0, bad
    st, longest, rs = _row_lengths(gpu, 3, formats.to_device(np.array([1, 3, 5, 9], np.int32)), 1)
    assert st == capi.SPGPU_SUCCESS and longest == 4 and rs.cpu().numpy()[:3].tolist() == [2, 2, 4]
    # an element size that is not 4, 8 or 16 (no such type code): refused before anything is launched
    d_ptr = formats.to_device(np.array([0, 1, 2], np.int32))
    for code in (5, -1):
        assert capi.spgpuSizeOf(code) == 0
        assert capi.spgpuCsrToHellDevice(gpu, None, None, None, 32, 0, 2, _p(d_ptr), None, None, 0, code, None) == capi.SPGPU_UNSUPPORTED
        assert capi.spgpuCsrToEllDevice(gpu, None, None, 32, 32, 0, 2, _p(d_ptr), None, None, 0, code, None) == capi.SPGPU_UNSUPPORTED
