"""GPU: the device-side transpose of a stored HELL or ELL matrix (include/spgpu/ext/transpose_device.h).

Every case builds the source arrays on the host with the ORACLE's converters, poisons their padding slots (column indices far
outside the matrix, NaN values), builds the expected arrays with the oracle's cooToEll -> ellToHell on the transposed COO listing of
spgpu_amd.formats (pinned in test_transpose_device_surface.py), and compares tLengths, the two host scalars, tHackOffsets,
tIndices and tValues byte for byte.  Destinations are zeroed inside an allocation with guard words on both sides; the guards must
be unchanged.  A padding slot that is read shows as SPGPU_UNSUPPORTED (its column is outside the matrix) or as a wrong byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 16          # guard words of 16 bytes on each side of a destination
POISON_COLUMN = 0x7F000000


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Guarded:
    """`count` zeroed elements of `dtype` in HBM between two runs of GUARD 16-byte words of 0xA5."""

    def __init__(self, count, dtype):
        import torch
        self.bytes = max(count, 1) * np.dtype(dtype).itemsize
        self.count, self.dtype = count, np.dtype(dtype)
        self.buf = torch.full((self.bytes + 2 * GUARD * 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.buf[GUARD * 16:GUARD * 16 + self.bytes] = 0

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD * 16)

    def host(self):
        raw = self.buf.cpu().numpy()
        assert (raw[:GUARD * 16] == 0xA5).all() and (raw[GUARD * 16 + self.bytes:] == 0xA5).all(), "a guard word was written"
        return raw[GUARD * 16:GUARD * 16 + self.count * self.dtype.itemsize].copy().view(self.dtype)


def _stored_mask(mat):
    """True for the slots rS covers, HELL or ELL host dict."""
    lengths = np.asarray(mat["row_lengths"][:mat["rows"]], np.int64)
    r = np.repeat(np.arange(mat["rows"], dtype=np.int64), lengths)
    k = np.arange(int(lengths.sum()), dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    if "hack_size" in mat:
        hs = mat["hack_size"]
        slots = np.asarray(mat["hack_offsets"], np.int64)[r // hs] + r % hs + k * hs
    else:
        slots = r + k * mat["pitch"]
    mask = np.zeros(mat["indices"].size, bool)
    mask[slots] = True
    return mask


def _poisoned(mat):
    """A copy of the host arrays whose padding slots hold a column far outside the matrix and NaN."""
    mask = _stored_mask(mat)
    indices, values = mat["indices"].copy(), mat["values"].copy()
    indices[~mask] = POISON_COLUMN
    values[~mask] = np.nan if values.dtype.kind == "f" else complex(np.nan, np.nan)
    return dict(mat, indices=indices, values=values)


def _source(n_rows, r, c, v, base, hack_size=32, ell=False):
    ell_h = O.oracle_converters.coo_to_ell(n_rows, r, c, v, coo_base=base, ell_base=base)
    return _poisoned(ell_h if ell else O.oracle_converters.ell_to_hell(ell_h, hack_size))


def _transpose(gpu, src, n_cols, t_hack, t_base, r_idx=None, values_pitch=None, fill_after_refusal=False):
    """The three device calls on a host HELL or ELL dict.  Returns dict(status, longest, nnz, row_lengths, height, hack_offsets,
    indices, values) of numpy arrays; the guards of all four destinations are checked."""
    import torch
    from spgpu_amd import capi, formats
    n_rows, is_ell = src["rows"], "hack_size" not in src
    code = capi.TYPE_CODE[src["letter"]]
    d_idx = formats.to_device(src["indices"] if src["indices"].size else np.zeros(1, np.int32))
    values = src["values"] if src["values"].size else np.zeros(1, src["values"].dtype)
    slots = int(src["indices"].size)
    ip = vp = src.get("pitch", 0)
    if is_ell and values_pitch:                      # the values laid out again with a pitch of their own
        vp = values_pitch
        wide = np.full(vp * src["max_row"], np.nan, values.dtype)
        wide.reshape(src["max_row"], vp)[:, :n_rows] = values.reshape(src["max_row"], ip)[:, :n_rows]
        values = wide
    d_val = formats.to_device(values)
    d_rs = formats.to_device(np.ascontiguousarray(src["row_lengths"], np.int32))
    d_ridx = None if r_idx is None else formats.to_device(np.ascontiguousarray(r_idx, np.int32))
    d_ho = None if is_ell else formats.to_device(np.ascontiguousarray(src["hack_offsets"], np.int32))
    work_bytes = capi.spgpuHellTransposeWorkBytes(n_rows, n_cols, slots)
    assert work_bytes > 0
    work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda:0")
    lengths = _Guarded(n_cols, np.int32)
    longest, nnz, height = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    if is_ell:
        st = capi.spgpuEllTransposeLengthsDevice(gpu, lengths.ptr, C.byref(longest), C.byref(nnz), _p(d_idx), ip, _p(d_rs), _p(d_ridx),
                                                 n_rows, n_cols, src["base"], slots, _p(work))
    else:
        st = capi.spgpuHellTransposeLengthsDevice(gpu, lengths.ptr, C.byref(longest), C.byref(nnz), _p(d_idx), src["hack_size"],
                                                  _p(d_ho), _p(d_rs), _p(d_ridx), n_rows, n_cols, src["base"], slots, _p(work))
    out = dict(status=st, longest=longest.value, nnz=nnz.value)
    hacks = (n_cols + t_hack - 1) // t_hack
    offsets = _Guarded(hacks, np.int32)
    if st == capi.SPGPU_SUCCESS:
        assert capi.spgpuHellPlanDevice(gpu, C.byref(height), offsets.ptr, t_hack, n_cols, lengths.ptr, _p(work)) == capi.SPGPU_SUCCESS
        t_slots = t_hack * height.value
    elif fill_after_refusal:
        t_slots, height = 4096, C.c_int(4096 // t_hack)    # a caller who goes on regardless: nothing may be written
    else:
        torch.cuda.synchronize()
        out.update(row_lengths=lengths.host())
        return out
    t_val, t_idx = _Guarded(t_slots, src["values"].dtype), _Guarded(t_slots, np.int32)
    torch.cuda.synchronize()
    if is_ell:
        st2 = capi.spgpuEllTransposeDevice(gpu, t_val.ptr, t_idx.ptr, offsets.ptr, t_hack, t_base, _p(d_val), _p(d_idx), vp, ip,
                                           _p(d_rs), _p(d_ridx), n_rows, n_cols, src["base"], slots, code, lengths.ptr, _p(work))
    else:
        st2 = capi.spgpuHellTransposeDevice(gpu, t_val.ptr, t_idx.ptr, offsets.ptr, t_hack, t_base, _p(d_val), _p(d_idx),
                                            src["hack_size"], _p(d_ho), _p(d_rs), _p(d_ridx), n_rows, n_cols, src["base"], slots, code,
                                            lengths.ptr, _p(work))
    assert st2 == capi.SPGPU_SUCCESS
    torch.cuda.synchronize()
    out.update(row_lengths=lengths.host(), height=height.value, hack_offsets=offsets.host(), indices=t_idx.host(), values=t_val.host(),
               device=dict(cM=t_val, rP=t_idx, hack_offsets=offsets, rS=lengths))
    return out


def _expected(src, n_cols, t_hack, t_base, r_idx=None):
    """The oracle's cooToEll -> ellToHell on the transposed listing."""
    from spgpu_amd import formats
    listing = formats.ell_transposed_coo if "hack_size" not in src else formats.hell_transposed_coo
    t_rows, t_cols, t_vals = listing(src, r_idx)
    ell = O.oracle_converters.coo_to_ell(n_cols, t_rows, t_cols, t_vals, coo_base=0, ell_base=t_base)
    return ell, O.oracle_converters.ell_to_hell(ell, t_hack), (t_rows, t_cols, t_vals)


def _check(gpu, src, n_cols, t_hack, t_base, r_idx=None, values_pitch=None):
    from spgpu_amd import capi
    got = _transpose(gpu, src, n_cols, t_hack, t_base, r_idx, values_pitch)
    ell, want, listing = _expected(src, n_cols, t_hack, t_base, r_idx)
    assert got["status"] == capi.SPGPU_SUCCESS
    assert got["longest"] == ell["max_row"] and got["nnz"] == listing[0].size and got["height"] == want["height"]
    assert got["row_lengths"].tobytes() == np.ascontiguousarray(ell["row_lengths"][:n_cols], np.int32).tobytes()
    assert got["hack_offsets"].tobytes() == want["hack_offsets"].tobytes()
    assert got["indices"].tobytes() == want["indices"].tobytes()
    assert got["values"].tobytes() == want["values"].tobytes()
    return got, want, listing


def _random_rows(rng, n_rows, n_cols, max_len, letter, base, first_col=0, end_col=None, empty=()):
    """Row-major COO: row lengths 0 .. max_len, the columns of a row distinct and ascending."""
    end_col = n_cols if end_col is None else end_col
    lengths = rng.integers(0, max_len + 1, n_rows)
    lengths[list(empty)] = 0
    r = np.repeat(np.arange(n_rows), lengths).astype(np.int32)
    c = np.concatenate([np.sort(rng.choice(np.arange(first_col, end_col), int(l), replace=False)) for l in lengths] +
                       [np.zeros(0, np.int64)]).astype(np.int32)
    v = rng.standard_normal(r.size)
    if letter in "CZ":
        v = v + 1j * rng.standard_normal(r.size)
    return r + base, c + base, v.astype(O.NP_DTYPE[letter])


# ---- 1. rectangular, partial hacks, destination hack sizes ------------------------------------------------------------------
@pytest.mark.parametrize("t_hack", [32, 64, 24])
@pytest.mark.parametrize("shape", [(70, 45), (45, 70)])
def test_rectangular_with_a_partial_hack(gpu, shape, t_hack):
    """70 x 45 and 45 x 70, source hackSize 32 (three hacks, the last partial); destination hack 32, 64 and 24."""
    n_rows, n_cols = shape
    rng = np.random.default_rng(n_rows * 100 + t_hack)
    r, c, v = _random_rows(rng, n_rows, n_cols, 12, "D", 0)
    src = _source(n_rows, r, c, v, 0)
    assert src["hack_offsets"].size == (3 if n_rows == 70 else 2) and n_rows % 32 != 0
    _check(gpu, src, n_cols, t_hack, 0)


# ---- 2. empty rows and columns ------------------------------------------------------------------------------------------------
def test_empty_rows_and_columns_at_both_ends(gpu):
    """Rows 0, 1, 68, 69 empty; columns 0 .. 2 and 64 .. 69 of 70 empty: zeros at the edges of tLengths, the last destination hack
    (rows 64 .. 69 of A^T) empty."""
    rng = np.random.default_rng(2)
    r, c, v = _random_rows(rng, 70, 70, 9, "D", 0, first_col=3, end_col=64, empty=(0, 1, 68, 69))
    src = _source(70, r, c, v, 0)
    got, want, _ = _check(gpu, src, 70, 32, 0)
    assert not got["row_lengths"][:3].any() and not got["row_lengths"][64:].any() and got["row_lengths"].any()
    assert got["hack_offsets"][2] == got["indices"].size      # the third hack stores nothing
    # no entries at all: only tLengths is written (zeros); the scalars are 0
    none = _source(70, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0)
    got = _transpose(gpu, none, 45, 32, 0)
    assert (got["longest"], got["nnz"], got["height"]) == (0, 0, 0) and not got["row_lengths"].any() and not got["hack_offsets"].any()


# ---- 3. a dense column, a dense row -----------------------------------------------------------------------------------------
def test_a_dense_column_and_a_dense_row(gpu):
    """Column 7 is hit by every one of the 70 rows (a row of A^T longer than a hack is tall); row 5 of A holds all 45 columns."""
    rng = np.random.default_rng(3)
    r, c, v = _random_rows(rng, 70, 45, 6, "D", 0)
    keep = (c != 7) & (r != 5)
    r, c, v = r[keep], c[keep], v[keep]
    r = np.concatenate([r, np.arange(70), np.full(44, 5)]).astype(np.int32)
    c = np.concatenate([c, np.full(70, 7), np.delete(np.arange(45), 7)]).astype(np.int32)
    v = np.concatenate([v, rng.standard_normal(114)])
    order = np.argsort(r, kind="stable")
    src = _source(70, r[order], c[order], v[order], 0)
    got, _, _ = _check(gpu, src, 45, 32, 0)
    assert got["row_lengths"][7] == 70 and got["longest"] == 70 and src["row_lengths"][5] == 45
    _check(gpu, src, 45, 24, 1)


# ---- 4. duplicates --------------------------------------------------------------------------------------------------------------
def test_duplicates_are_kept_in_slot_order(gpu):
    rng = np.random.default_rng(4)
    r, c, v = _random_rows(rng, 70, 45, 8, "S", 0)
    r = np.concatenate([r, [10, 10, 10, 40, 40]]).astype(np.int32)      # (10, 3) three times, (40, 44) twice, different values
    c = np.concatenate([c, [3, 3, 3, 44, 44]]).astype(np.int32)
    v = np.concatenate([v, [101.0, 102.0, 103.0, 104.0, 105.0]]).astype(np.float32)
    order = np.argsort(r, kind="stable")
    src = _source(70, r[order], c[order], v[order], 0)
    got, want, (t_rows, t_cols, t_vals) = _check(gpu, src, 45, 32, 0)
    planted = t_vals[(t_vals > 100)]
    assert planted.tolist() == [101.0, 102.0, 103.0, 104.0, 105.0]     # ascending slot inside (10, 3) and inside (40, 44)
    assert sorted(got["values"][got["values"] > 100].tolist()) == planted.tolist()


# ---- 5. base indices --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,t_base", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_base_indices(gpu, base, t_base):
    rng = np.random.default_rng(5)
    r, c, v = _random_rows(rng, 70, 45, 10, "D", base)
    src = _source(70, r, c, v, base)
    got, _, _ = _check(gpu, src, 45, 32, t_base)
    stored = got["indices"][got["indices"] != 0] if t_base else got["indices"]
    assert stored.min() >= t_base and stored.max() <= 69 + t_base


# ---- 6. row order -------------------------------------------------------------------------------------------------------------
def _permuted_source(letter="D", base=0):
    """70 x 45 with rIdx a random permutation: storage row s holds matrix row rIdx[s] (the COO rows renumbered, then converted)."""
    rng = np.random.default_rng(6)
    r, c, v = _random_rows(rng, 70, 45, 10, letter, 0)
    r_idx = rng.permutation(70).astype(np.int32)
    inverse = np.empty(70, np.int64)
    inverse[r_idx] = np.arange(70)
    s = inverse[r]
    order = np.argsort(s, kind="stable")
    return _source(70, (s[order] + base).astype(np.int32), c[order] + base, v[order], base), r_idx, (r, c, v)


def test_row_order_through_ridx(gpu):
    src, r_idx, (r, c, v) = _permuted_source()
    got, want, (t_rows, t_cols, t_vals) = _check(gpu, src, 45, 32, 0, r_idx=r_idx)
    order = np.lexsort((r, c))             # the matrix itself by column, then by matrix row (its rows have distinct columns)
    assert t_rows.tolist() == c[order].tolist() and t_cols.tolist() == r[order].tolist() and t_vals.tobytes() == v[order].tobytes()
    assert t_cols.tolist() != np.sort(t_cols).tolist()


@pytest.mark.parametrize("fault", ["rIdx", "column", "rS"])
def test_bad_input_is_reported_and_nothing_is_written(gpu, fault):
    """An rIdx entry outside [0, rows), a stored column outside [base, base + cols), an rS that reaches beyond the stored slots:
    SPGPU_UNSUPPORTED, the scalars 0, and no destination byte written -- not by the lengths call and not by a fill that follows."""
    from spgpu_amd import capi
    src, r_idx, _ = _permuted_source(base=1)
    r_idx = r_idx.copy()
    if fault == "rIdx":
        r_idx[33] = 70
    elif fault == "column":
        mask = _stored_mask(src)
        src["indices"][np.flatnonzero(mask)[17]] = 46 + 1          # base 1: columns 1 .. 45 are inside
    else:
        src["row_lengths"] = src["row_lengths"].copy()
        src["row_lengths"][69] = 1000
    for fill in (False, True):
        got = _transpose(gpu, src, 45, 32, 0, r_idx=r_idx, fill_after_refusal=fill)
        assert got["status"] == capi.SPGPU_UNSUPPORTED and (got["longest"], got["nnz"]) == (0, 0)
        assert not got["row_lengths"].any()
        if fill:
            assert not got["indices"].any() and not got["values"].view(np.uint8).any() and not got["hack_offsets"].any()
    # one below the base is outside as well
    src, r_idx, _ = _permuted_source(base=1)
    src["indices"][np.flatnonzero(_stored_mask(src))[0]] = 0
    assert _transpose(gpu, src, 45, 32, 0, r_idx=r_idx)["status"] == capi.SPGPU_UNSUPPORTED


# ---- 7. element sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDZ")
def test_values_are_moved_as_words(gpu, letter):
    """4-, 8- and 16-byte elements with NaN payloads, -0 and denormals among the real parts: every word arrives intact."""
    rng = np.random.default_rng(7)
    r, c, v = _random_rows(rng, 70, 45, 10, letter, 0)
    words = v.view(np.uint32).copy()
    per = v.dtype.itemsize // 4
    planted = (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FF80000, 0xFFF00001)
    for n, word in enumerate(planted):
        words[(3 * n + 1) * per + (per - 1 if letter != "Z" else 1)] = word      # the high word of a real part
    v = words.view(v.dtype)
    assert np.isnan(v.real).sum() >= 2        # 0x7FF80000 and 0xFFF00001 head NaNs in either width, three more do in fp32
    src = _source(70, r, c, v, 0)
    got, _, _ = _check(gpu, src, 45, 32, 0)
    assert set(planted) <= set(got["values"].view(np.uint32).tolist())


# ---- 8. ELL source ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_order", [False, True])
def test_ell_source_with_two_pitches(gpu, with_order):
    """The 70 x 45 case stored as ELL, the values with a pitch (128) other than the indices' (the converter's); with and without rIdx."""
    if with_order:
        src, r_idx, _ = _permuted_source()
        ell = O.oracle_converters.coo_to_ell(70, *_ell_coo(src), coo_base=0, ell_base=0)
    else:
        rng = np.random.default_rng(8)
        r, c, v = _random_rows(rng, 70, 45, 12, "D", 0)
        ell, r_idx = O.oracle_converters.coo_to_ell(70, r, c, v, coo_base=0, ell_base=0), None
    src = _poisoned(ell)
    assert src["pitch"] != 128 and src["pitch"] >= 70
    _check(gpu, src, 45, 32, 0, r_idx=r_idx, values_pitch=128)
    _check(gpu, src, 45, 24, 1, r_idx=r_idx)


def _ell_coo(hell):
    """Storage-row COO of a host HELL dict (row-major, slots ascending)."""
    mask = _stored_mask(hell)
    lengths = np.asarray(hell["row_lengths"][:hell["rows"]], np.int64)
    r = np.repeat(np.arange(hell["rows"], dtype=np.int64), lengths)
    k = np.arange(int(lengths.sum()), dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    slots = np.asarray(hell["hack_offsets"], np.int64)[r // hell["hack_size"]] + r % hell["hack_size"] + k * hell["hack_size"]
    assert mask[slots].all()
    return r.astype(np.int32), hell["indices"][slots] - hell["base"], hell["values"][slots]


# ---- 9. one larger case -------------------------------------------------------------------------------------------------------
_LARGE = {}


def _large_case():
    """5 000 x 3 000, power-law row lengths (longest >= 300), the rows ordered by the oracle's ellToOell: built once."""
    if not _LARGE:
        from spgpu_amd import synth
        lengths = synth.power_law_lengths(5000, 12.0, 512, seed=21)
        assert lengths.max() >= 300
        _, _, r, c, v = synth.random_rows_coo(5000, 3000, lengths, seed=22, letter="D")
        ell = O.oracle_converters.coo_to_ell(5000, r, c, v)
        oell, r_idx = O.oracle_converters.ell_to_oell(ell)
        src = _poisoned(O.oracle_converters.ell_to_hell(oell, 32))
        _LARGE.update(src=src, r_idx=r_idx, coo=(r, c, v))
    return _LARGE


def test_larger_ordered_power_law_matrix(gpu):
    case = _large_case()
    assert sorted(case["r_idx"].tolist()) == list(range(5000)) and case["r_idx"].tolist() != list(range(5000))
    got, want, _ = _check(gpu, case["src"], 3000, 32, 0, r_idx=case["r_idx"])
    assert got["nnz"] == case["coo"][0].size > 40000
    case["got"] = got


def test_two_streams_give_the_same_bytes(gpu):
    """The larger case again on a second stream of the same handle: identical bytes (and the handle's stream restored)."""
    from spgpu_amd import capi
    case = _large_case()
    first = case.get("got") or _transpose(gpu, case["src"], 3000, 32, 0, r_idx=case["r_idx"])
    mine = capi.spgpuGetStream(gpu)
    other = C.c_void_p()
    capi.spgpuStreamCreate(gpu, C.byref(other))
    try:
        capi.spgpuSetStream(gpu, other)
        second = _transpose(gpu, case["src"], 3000, 32, 0, r_idx=case["r_idx"])
    finally:
        capi.spgpuSetStream(gpu, mine)
        capi.spgpuStreamDestroy(other)
    for key in ("row_lengths", "hack_offsets", "indices", "values"):
        assert first[key].tobytes() == second[key].tobytes(), key
    assert (first["longest"], first["nnz"], first["height"]) == (second["longest"], second["nnz"], second["height"])


# ---- 10. round trip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hack,base", [(32, 0), (24, 1)])
def test_transposing_twice_gives_the_source_back(gpu, hack, base):
    """Rows column-sorted, no duplicates, no rIdx: (A^T)^T with the source's hackSize and base is the source, byte for byte."""
    rng = np.random.default_rng(10)
    r, c, v = _random_rows(rng, 70, 45, 10, "D", base, empty=(0, 69))
    ell = O.oracle_converters.coo_to_ell(70, r, c, v, coo_base=base, ell_base=base)
    clean = O.oracle_converters.ell_to_hell(ell, hack)
    once = _transpose(gpu, _poisoned(clean), 45, hack, base)
    middle = dict(letter="D", rows=45, hack_size=hack, base=base, row_lengths=once["row_lengths"], hack_offsets=once["hack_offsets"],
                  indices=once["indices"], values=once["values"])
    twice = _transpose(gpu, _poisoned(middle), 70, hack, base)
    assert twice["row_lengths"].tobytes() == np.ascontiguousarray(clean["row_lengths"][:70], np.int32).tobytes()
    assert twice["hack_offsets"].tobytes() == clean["hack_offsets"].tobytes()
    assert twice["indices"].tobytes() == clean["indices"].tobytes() and twice["values"].tobytes() == clean["values"].tobytes()
    assert (twice["longest"], twice["nnz"], twice["height"]) == (ell["max_row"], r.size, clean["height"])


# ---- 11. the product ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "DS")
def test_the_product_on_the_transposed_arrays_is_exact(gpu, letter):
    """Small-integer values and an integer x: every sum is exact in either precision, so spgpu?hellspmv on the arrays of A^T must give
    the exact A^T x of tests/exact_ref.py bit for bit -- as built, and after spgpuHellSpmvAdopt (A^T has power-law rows: A's columns
    were drawn that way)."""
    import torch
    from spgpu_amd import capi, formats, synth
    n_rows, n_cols = 3000, 5000
    lengths = synth.power_law_lengths(n_cols, 12.0, 512, seed=31)
    _, _, tr, tc, _ = synth.random_rows_coo(n_cols, n_rows, lengths, seed=32, letter=letter)      # the rows of A^T: columns of A
    order = np.argsort(tc, kind="stable")
    r, c = tc[order].astype(np.int32), tr[order].astype(np.int32)
    rng = np.random.default_rng(33)
    v = rng.integers(-3, 4, r.size).astype(O.NP_DTYPE[letter])
    x = rng.integers(-4, 5, n_rows).astype(O.NP_DTYPE[letter])
    src = _source(n_rows, r, c, v, 0)
    got, _, _ = _check(gpu, src, n_cols, 32, 0)
    exact, _ = X.spmv(n_cols, c, r, v, x, None, 1.0, 0.0)
    want = np.asarray(exact).astype(O.NP_DTYPE[letter])
    assert (want.astype(np.longdouble) == exact).all() and np.abs(want).max() > 8       # representable: the comparison is of bits
    dev = got["device"]
    dx = formats.to_device(x)
    dz = torch.full((n_cols,), float("nan"), dtype=dx.dtype, device="cuda:0")

    def run():
        dz.fill_(float("nan"))
        torch.cuda.synchronize()
        capi.hellspmv[letter](gpu, _p(dz), _p(dz), capi.scalar(letter, 1.0), dev["cM"].ptr, dev["rP"].ptr, 32, dev["hack_offsets"].ptr,
                              dev["rS"].ptr, None, got["longest"], n_cols, _p(dx), capi.scalar(letter, 0.0), 0)
        torch.cuda.synchronize()
        return dz.cpu().numpy()

    assert (run() + 0.0).tobytes() == (want + 0.0).tobytes()
    uses = capi.spgpuSpmvAdoptedUses(gpu)
    assert capi.spgpuHellSpmvAdopt(gpu, capi.TYPE_CODE[letter], dev["cM"].ptr, dev["rP"].ptr, 32, dev["hack_offsets"].ptr, dev["rS"].ptr,
                                   n_cols, 0) == capi.SPGPU_SUCCESS
    try:
        adopted = run()
        assert capi.spgpuSpmvAdoptedUses(gpu) > uses      # the call ran on the library's ordered copy
    finally:
        assert capi.spgpuSpmvThaw(gpu, dev["rP"].ptr) == capi.SPGPU_SUCCESS
    assert (adopted + 0.0).tobytes() == (want + 0.0).tobytes()


# ---- 12. the plain-C tool -------------------------------------------------------------------------------------------------------
def test_the_c_harness_transposes_twice():
    exe = os.path.join(ROOT, "tools", "transpose_amd.bin")
    assert os.path.exists(exe), f"{exe} missing: run `make tools`"
    out = subprocess.run([exe, "20000", "15000", "9"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "double transpose: rS, hackOffsets, rP and cM identical to A's (memcmp)" in out.stdout and "PASSED" in out.stdout
    assert "w'(A x)    = " in out.stdout and "(A^T w)' x = " in out.stdout
