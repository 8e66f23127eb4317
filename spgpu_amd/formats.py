"""Host pipeline of the reference's harness, driven through the C ABI.

``hellPerf.cpp:127-317`` does: COO -> ``computeEllRowLenghts`` / ``cooToEll`` ->
``computeHellAllocSize`` / ``ellToHell`` on the CPU, ``cudaMemcpy`` to the GPU,
then ``spgpu?hellspmv``.  The functions below run the same calls of *this*
library (host converters in ``spgpu_amd/csrc/conv_*.c``) on numpy arrays and
move the result into HBM with torch (plumbing only: torch never computes).
"""
import ctypes as C

import numpy as np

from . import capi

NP_DTYPE = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}
LETTER_OF = {np.dtype(v): k for k, v in NP_DTYPE.items()}


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---- host conversions (C ABI: ell_conv.h, hell_conv.h, hdia_conv.h) ---------------

def coo_to_ell(n_rows, coo_rows, coo_cols, coo_vals, coo_base=0, ell_base=0, pitch=None):
    """COO -> ELL exactly as hellPerf.cpp:136-152 drives it (arrays zeroed first)."""
    coo_rows, coo_cols = _i32(coo_rows), _i32(coo_cols)
    coo_vals = np.ascontiguousarray(coo_vals)
    letter = LETTER_OF[coo_vals.dtype]
    nnz = int(coo_rows.size)
    row_len = np.zeros(max(n_rows, 1), dtype=np.int32)
    max_row = C.c_int(0)
    capi.computeEllRowLenghts(_p(row_len), C.byref(max_row), n_rows, nnz, _p(coo_rows), coo_base)
    if pitch is None:
        pitch = capi.computeEllAllocPitch(n_rows)
    values = np.zeros(max(max_row.value * pitch, 1), dtype=coo_vals.dtype)
    indices = np.zeros(max(max_row.value * pitch, 1), dtype=np.int32)
    capi.cooToEll(_p(values), _p(indices), pitch, pitch, max_row.value, ell_base, n_rows, nnz,
                  _p(coo_rows), _p(coo_cols), _p(coo_vals), coo_base, capi.TYPE_CODE[letter])
    return dict(letter=letter, rows=n_rows, values=values[:max_row.value * pitch],
                indices=indices[:max_row.value * pitch], pitch=pitch, max_row=max_row.value,
                row_lengths=row_len[:n_rows], base=ell_base)


def ell_to_hell(ell, hack_size=32):
    """ELL -> HELL exactly as hellPerf.cpp:254-264 drives it (but arrays zeroed, not malloc'd)."""
    n_rows = ell["rows"]
    row_len = np.ascontiguousarray(ell["row_lengths"], dtype=np.int32)
    height = C.c_int(0)
    capi.computeHellAllocSize(C.byref(height), hack_size, n_rows, _p(row_len))
    slots = hack_size * height.value
    hacks = (n_rows + hack_size - 1) // hack_size
    values = np.zeros(max(slots, 1), dtype=ell["values"].dtype)
    indices = np.zeros(max(slots, 1), dtype=np.int32)
    hack_offsets = np.zeros(max(hacks, 1), dtype=np.int32)
    ev = ell["values"] if ell["values"].size else np.zeros(1, dtype=ell["values"].dtype)
    ei = ell["indices"] if ell["indices"].size else np.zeros(1, dtype=np.int32)
    capi.ellToHell(_p(values), _p(indices), _p(hack_offsets), hack_size, _p(ev), _p(ei),
                   ell["pitch"], ell["pitch"], _p(row_len), n_rows, capi.TYPE_CODE[ell["letter"]])
    return dict(letter=ell["letter"], rows=n_rows, values=values[:slots], indices=indices[:slots],
                hack_offsets=hack_offsets[:hacks], hack_size=hack_size, height=height.value,
                row_lengths=row_len, base=ell["base"])


def coo_to_hdia(n_rows, n_cols, coo_rows, coo_cols, coo_vals, hack_size=32, coo_base=0):
    """COO -> HDIA as diaPerf.cpp:254-293 drives it, but hdiaValues zeroed first."""
    coo_rows, coo_cols = _i32(coo_rows), _i32(coo_cols)
    coo_vals = np.ascontiguousarray(coo_vals)
    letter = LETTER_OF[coo_vals.dtype]
    nnz = int(coo_rows.size)
    hacks = capi.getHdiaHacksCount(hack_size, n_rows)
    hack_offsets = np.zeros(hacks + 1, dtype=np.int32)
    height = C.c_int(0)
    capi.computeHdiaHackOffsetsFromCoo(C.byref(height), _p(hack_offsets), hack_size, n_rows, n_cols, nnz,
                                       _p(coo_rows), _p(coo_cols), coo_base)
    values = np.zeros(max(hack_size * height.value, 1), dtype=coo_vals.dtype)
    offsets = np.zeros(max(height.value, 1), dtype=np.int32)
    capi.cooToHdia(_p(values), _p(offsets), _p(hack_offsets), hack_size, n_rows, n_cols, nnz,
                   _p(coo_rows), _p(coo_cols), _p(coo_vals), coo_base, capi.TYPE_CODE[letter])
    return dict(letter=letter, rows=n_rows, cols=n_cols, values=values[:hack_size * height.value],
                offsets=offsets[:height.value], hack_offsets=hack_offsets, hack_size=hack_size,
                height=height.value)


def coo_to_dia(n_rows, n_cols, coo_rows, coo_cols, coo_vals, coo_base=0):
    """COO -> DIA as diaPerf.cpp:127-160 drives it (values zeroed first)."""
    coo_rows, coo_cols = _i32(coo_rows), _i32(coo_cols)
    coo_vals = np.ascontiguousarray(coo_vals)
    letter = LETTER_OF[coo_vals.dtype]
    nnz = int(coo_rows.size)
    diags = capi.computeDiaDiagonalsCount(n_rows, n_cols, nnz, _p(coo_rows), _p(coo_cols))
    pitch = capi.computeDiaAllocPitch(n_rows)
    values = np.zeros(max(diags * pitch, 1), dtype=coo_vals.dtype)
    offsets = np.zeros(max(diags, 1), dtype=np.int32)
    capi.coo2dia(_p(values), _p(offsets), pitch, diags, n_rows, n_cols, nnz, _p(coo_rows), _p(coo_cols), _p(coo_vals),
                 coo_base, capi.TYPE_CODE[letter])
    return dict(letter=letter, rows=n_rows, cols=n_cols, values=values[:diags * pitch], offsets=offsets[:diags],
                pitch=pitch, diags=diags)


def dia_to_hdia(dia, hack_size=32):
    """DIA -> HDIA as diaPerf.cpp:254-275 drives it, with hdiaValues zeroed first."""
    n_rows = dia["rows"]
    hacks = capi.getHdiaHacksCount(hack_size, n_rows)
    hack_offsets = np.zeros(hacks + 1, dtype=np.int32)
    height = C.c_int(0)
    dv = dia["values"] if dia["values"].size else np.zeros(1, dia["values"].dtype)
    do = dia["offsets"] if dia["offsets"].size else np.zeros(1, np.int32)
    code = capi.TYPE_CODE[dia["letter"]]
    capi.computeHdiaHackOffsets(C.byref(height), _p(hack_offsets), hack_size, _p(dv), dia["pitch"], dia["diags"], n_rows, code)
    values = np.zeros(max(hack_size * height.value, 1), dtype=dia["values"].dtype)
    offsets = np.zeros(max(height.value, 1), dtype=np.int32)
    capi.diaToHdia(_p(values), _p(offsets), _p(hack_offsets), hack_size, _p(dv), _p(do), dia["pitch"], dia["diags"], n_rows, code)
    return dict(letter=dia["letter"], rows=n_rows, cols=dia["cols"], values=values[:hack_size * height.value],
                offsets=offsets[:height.value], hack_offsets=hack_offsets, hack_size=hack_size, height=height.value)


def ell_to_oell(ell):
    """ELL -> ordered ELL (rows by descending length) as hellPerf.cpp:319-332 drives it; returns (oell, rIdx)."""
    n_rows = ell["rows"]
    r_idx = np.zeros(max(n_rows, 1), dtype=np.int32)
    dst_rs = np.zeros(max(n_rows, 1), dtype=np.int32)
    values, indices = np.zeros_like(ell["values"]), np.zeros_like(ell["indices"])
    ev = ell["values"] if ell["values"].size else np.zeros(1, ell["values"].dtype)
    ei = ell["indices"] if ell["indices"].size else np.zeros(1, np.int32)
    vv = values if values.size else np.zeros(1, ell["values"].dtype)
    ii = indices if indices.size else np.zeros(1, np.int32)
    rs = np.ascontiguousarray(ell["row_lengths"], dtype=np.int32)
    capi.ellToOell(_p(r_idx), _p(vv), _p(ii), _p(dst_rs), _p(ev), _p(ei), _p(rs), ell["pitch"], ell["pitch"], n_rows,
                   capi.TYPE_CODE[ell["letter"]])
    out = dict(ell, values=values, indices=indices, row_lengths=dst_rs[:n_rows])
    return out, r_idx[:n_rows]


def oell_order(row_lengths, window=0, long_rows=0, aligned=False):
    """The host order call (ell_conv.h oellOrder, or oellOrderAligned): returns (rIdx, sorted lengths)."""
    rs = _i32(row_lengths)
    n = int(rs.size)
    r_idx, dst = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    (capi.oellOrderAligned if aligned else capi.oellOrder)(_p(r_idx), _p(dst), _p(rs if n else np.zeros(1, np.int32)), n, window, long_rows)
    return r_idx[:n], dst[:n]


def _transposed_coo(indices, values, row_lengths, first, step, value_first, value_step, r_idx, base):
    lengths = np.asarray(row_lengths, np.int64)
    n, total = int(lengths.size), int(lengths.sum())
    r = np.repeat(np.arange(n, dtype=np.int64), lengths)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    i = r if r_idx is None else np.asarray(r_idx, np.int64)[r]
    j = np.asarray(indices)[first[r] + k * step].astype(np.int64) - base
    order = np.argsort(i, kind="stable")              # ascending matrix row; the slots of a row keep their order
    order = order[np.argsort(j[order], kind="stable")]  # then by column: entry k of row j of A^T = k-th entry of column j of A
    taken = np.asarray(values)[(value_first[r] + k * value_step)[order]]
    return j[order].astype(np.int32), i[order].astype(np.int32), np.ascontiguousarray(taken)


def hell_transposed_coo(hell, r_idx=None):
    """The COO listing of A^T in the order include/spgpu/ext/transpose_device.h defines, from host HELL arrays (a dict of
    ell_to_hell): zero-based (rows of A^T = columns of A, columns of A^T = matrix rows i of A, values), the entries of A taken
    by ascending i = r_idx[r] (r without r_idx) and within a row by ascending slot.  Padding slots are never looked at."""
    hs = hell["hack_size"]
    r = np.arange(hell["rows"], dtype=np.int64)
    first = np.asarray(hell["hack_offsets"], np.int64)[r // hs] + r % hs if r.size else r
    return _transposed_coo(hell["indices"], hell["values"], hell["row_lengths"][:hell["rows"]], first, hs, first, hs, r_idx, hell["base"])


def ell_transposed_coo(ell, r_idx=None, values_pitch=None):
    """hell_transposed_coo for host ELL arrays (a dict of coo_to_ell; values_pitch if it differs from the indices' pitch)."""
    r = np.arange(ell["rows"], dtype=np.int64)
    return _transposed_coo(ell["indices"], ell["values"], ell["row_lengths"][:ell["rows"]], r, ell["pitch"], r,
                           values_pitch or ell["pitch"], r_idx, ell["base"])


def slabs_to_csr(values, indices, row_lengths, n_rows, hack_offsets=None, hack_size=None, pitch=None, values_pitch=None, r_idx=None,
                 src_base=0, csr_base=0):
    """The CSR arrays include/spgpu/ext/to_csr_device.h defines, from host HELL arrays (hack_offsets and hack_size given) or host
    ELL arrays (pitch of the indices given; values_pitch if it differs), restated in numpy: (row_ptr int32 of n_rows + 1 entries
    starting at csr_base, cols int32, vals).  Storage row r is matrix row r_idx[r] (r without r_idx); the k-th entry of a matrix
    row is slot k of its storage row; a column becomes index - src_base + csr_base.  Padding slots are never looked at."""
    lengths = np.asarray(row_lengths, np.int64)[:n_rows]
    r = np.arange(n_rows, dtype=np.int64)
    if hack_offsets is not None:
        first = np.asarray(hack_offsets, np.int64)[r // hack_size] + r % hack_size if n_rows else r
        step = value_step = hack_size
    else:
        first, step, value_step = r, pitch, values_pitch or pitch
    i = r if r_idx is None else np.asarray(r_idx, np.int64)[:n_rows]
    by_matrix_row = np.zeros(n_rows, np.int64)
    by_matrix_row[i] = lengths
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(by_matrix_row, out=row_ptr[1:])
    total = int(lengths.sum())
    rr = np.repeat(r, lengths)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    at = row_ptr[i[rr]] + k
    cols = np.zeros(total, np.int32)
    vals = np.zeros(total, np.asarray(values).dtype)
    cols[at] = (np.asarray(indices)[first[rr] + k * step].astype(np.int64) - src_base + csr_base).astype(np.int32)
    vals[at] = np.asarray(values)[first[rr] + k * value_step]
    return (row_ptr + csr_base).astype(np.int32), cols, vals


def coo_assemble(n_rows, n_cols, coo_rows, coo_cols, coo_vals, coo_base=0, csr_base=0):
    """The arrays include/spgpu/ext/assemble_device.h defines, restated in numpy: (row_ptr, perm, seg_ptr, cols, vals) of a COO list
    of contributions in which a matrix entry may appear several times.  perm is a stable sort of the list by (row, column); seg_ptr
    has one more element than there are distinct (row, column) pairs; row_ptr int32 of n_rows + 1 elements starting at csr_base;
    a column becomes index - coo_base + csr_base; vals[u] is the sum of entry u's contributions in perm order, left to right, each
    addition rounded in the dtype of coo_vals.  The sums are accumulated by depth -- step k adds the k-th contribution of every
    entry that has one -- and start from the first contribution, which is copied as it is."""
    rows = np.asarray(coo_rows, np.int64) - coo_base
    cols = np.asarray(coo_cols, np.int64) - coo_base
    vals = np.asarray(coo_vals)
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows or cols.min() < 0 or cols.max() >= n_cols):
        raise ValueError("an entry lies outside the matrix")
    perm = np.lexsort((cols, rows)).astype(np.int32)              # lexsort is stable: equal pairs keep their COO order
    sorted_rows, sorted_cols = rows[perm], cols[perm]
    head = np.ones(perm.size, bool)
    head[1:] = (sorted_rows[1:] != sorted_rows[:-1]) | (sorted_cols[1:] != sorted_cols[:-1])
    first = np.flatnonzero(head)
    seg_ptr = np.concatenate((first, [perm.size])).astype(np.int32)
    row_ptr = (np.searchsorted(sorted_rows[first], np.arange(n_rows + 1), side="left") + csr_base).astype(np.int32)
    out_cols = (sorted_cols[first] + csr_base).astype(np.int32)
    out_vals = vals[perm[first]].copy()
    lengths = np.diff(seg_ptr.astype(np.int64))
    for k in range(1, int(lengths.max()) if lengths.size else 0):
        more = np.flatnonzero(lengths > k)
        out_vals[more] = out_vals[more] + vals[perm[first[more] + k]]
    return row_ptr, perm, seg_ptr, out_cols, out_vals


def csr_spgemm(a_ptr, a_cols, a_vals, b_ptr, b_cols, b_vals, n_b_cols, base=0):
    """The arrays include/spgpu/ext/spgemm_device.h defines, restated in numpy: (products, c_ptr, c_cols, c_vals) of C = A * B, all
    three CSR in `base`.  A's rows in any order, duplicates allowed; B's rows strictly ascending.  The pattern is symbolic (an entry
    whose terms cancel stays); c_vals[u] = ((0 + p0) + p1) + ..., the products taken over A's row in storage order, each product
    rounded in the dtype of the values and each addition rounded again.  A complex product is computed on the real views -- re =
    ar*br - ai*bi, im = ar*bi + ai*br, six separately rounded operations -- so that no library fuses anything.  One Python step per
    stored entry of A: a restatement for tests, not a tool."""
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64) - base, np.asarray(b_ptr, np.int64) - base
    a_cols, b_cols = np.asarray(a_cols, np.int64) - base, np.asarray(b_cols, np.int64) - base
    a_vals, b_vals = np.asarray(a_vals), np.asarray(b_vals)
    dtype = a_vals.dtype
    if b_vals.dtype != dtype:
        raise ValueError("A and B hold different types")
    n_rows, n_inner = a_ptr.size - 1, b_ptr.size - 1
    if a_cols.size and (a_cols.min() < 0 or a_cols.max() >= n_inner):
        raise ValueError("a column of A names no row of B")
    if b_cols.size and (b_cols.min() < 0 or b_cols.max() >= n_b_cols):
        raise ValueError("a column of B lies outside the matrix")
    inside_a_row = np.ones(max(b_cols.size - 1, 0), bool)
    inside_a_row[b_ptr[1:-1][(b_ptr[1:-1] > 0) & (b_ptr[1:-1] < b_cols.size)] - 1] = False
    if np.any((np.diff(b_cols) <= 0) & inside_a_row):
        raise ValueError("a row of B does not ascend strictly")
    real = dtype.kind != "c"
    part = dtype if real else np.dtype("f%d" % (dtype.itemsize // 2))
    b_len = np.diff(b_ptr)
    products = 0
    c_ptr = np.zeros(n_rows + 1, np.int64)
    all_cols, all_vals = [], []
    for i in range(n_rows):
        entries = range(a_ptr[i], a_ptr[i + 1])
        products += int(b_len[a_cols[a_ptr[i]:a_ptr[i + 1]]].sum())
        named = [b_cols[b_ptr[a_cols[e]]:b_ptr[a_cols[e] + 1]] for e in entries]
        cols = np.unique(np.concatenate(named)) if named else np.zeros(0, np.int64)
        if real:
            acc = np.zeros(cols.size, dtype)
        else:
            acc_re, acc_im = np.zeros(cols.size, part), np.zeros(cols.size, part)
        for e, js in zip(entries, named):
            at = np.searchsorted(cols, js)                    # distinct slots: B's row has no duplicate column
            b = b_vals[b_ptr[a_cols[e]]:b_ptr[a_cols[e] + 1]]
            if real:
                acc[at] = acc[at] + a_vals[e] * b             # the product array is rounded before the addition reads it
            else:
                ar, ai = part.type(a_vals[e].real), part.type(a_vals[e].imag)
                br, bi = np.ascontiguousarray(b.real), np.ascontiguousarray(b.imag)
                rr, ii, ri, ir = ar * br, ai * bi, ar * bi, ai * br
                re, im = rr - ii, ri + ir
                acc_re[at] = acc_re[at] + re
                acc_im[at] = acc_im[at] + im
        if not real:
            acc = np.empty(cols.size, dtype)
            acc.real, acc.imag = acc_re, acc_im
        c_ptr[i + 1] = c_ptr[i] + cols.size
        all_cols.append(cols)
        all_vals.append(acc)
    c_cols = np.concatenate(all_cols) if all_cols else np.zeros(0, np.int64)
    c_vals = np.concatenate(all_vals) if all_vals else np.zeros(0, dtype)
    return products, (c_ptr + base).astype(np.int32), (c_cols + base).astype(np.int32), np.ascontiguousarray(c_vals.astype(dtype, copy=False))


def _scaled(scalar, vals):
    """scalar * vals as include/spgpu/ext/add_device.h defines it: rounded once in the dtype of vals; a complex product computed on the
    real views -- re = sr*vr - si*vi, im = sr*vi + si*vr, six separately rounded operations -- so that no library fuses anything."""
    dtype = vals.dtype
    if dtype.kind != "c":
        return dtype.type(scalar) * vals
    part = np.dtype("f%d" % (dtype.itemsize // 2))
    s = np.asarray(scalar, dtype)[()]
    sr, si = part.type(s.real), part.type(s.imag)
    vr, vi = np.ascontiguousarray(vals.real), np.ascontiguousarray(vals.imag)
    rr, ii, ri, ir = sr * vr, si * vi, sr * vi, si * vr
    out = np.empty(vals.size, dtype)
    out.real, out.imag = rr - ii, ri + ir
    return out


def csr_add(a_ptr, a_cols, a_vals, b_ptr, b_cols, b_vals, n_cols, alpha, beta, base=0):
    """The arrays include/spgpu/ext/add_device.h defines, restated in numpy: (c_ptr, c_cols, c_vals) of C = alpha * A + beta * B, all
    three CSR in `base`, A and B both of n_cols columns with strictly ascending rows.  The pattern is the union (an entry whose terms
    cancel stays).  Where both store the entry c = (alpha * a) + (beta * b), each product rounded in the dtype of the values (_scaled)
    and the sum rounded again (complex: componentwise); where one stores it, its product alone.  alpha and beta are rounded to that
    dtype first.  ValueError on what spgpuCsrAddPlanDevice refuses."""
    a_ptr, b_ptr = np.asarray(a_ptr, np.int64) - base, np.asarray(b_ptr, np.int64) - base
    a_cols, b_cols = np.asarray(a_cols, np.int64) - base, np.asarray(b_cols, np.int64) - base
    a_vals, b_vals = np.asarray(a_vals), np.asarray(b_vals)
    dtype = a_vals.dtype
    if b_vals.dtype != dtype:
        raise ValueError("A and B hold different types")
    if a_ptr.size != b_ptr.size:
        raise ValueError("A and B have different numbers of rows")
    n_rows = a_ptr.size - 1
    keys = []
    for name, ptr, cols in (("A", a_ptr, a_cols), ("B", b_ptr, b_cols)):
        cols = cols[:ptr[-1]]
        if cols.size and (cols.min() < 0 or cols.max() >= n_cols):
            raise ValueError(f"a column of {name} lies outside the matrix")
        key = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr)) * max(int(n_cols), 1) + cols
        if np.any(np.diff(key) <= 0):                          # rows never descend, so only a row's own order can fail
            raise ValueError(f"a row of {name} does not ascend strictly")
        keys.append(key)
    union = np.union1d(keys[0], keys[1])
    if union.size > 2 ** 31 - 1:
        raise ValueError("more than INT_MAX entries in the union")
    at_a, at_b = np.searchsorted(union, keys[0]), np.searchsorted(union, keys[1])
    from_a, from_b = _scaled(alpha, a_vals[:keys[0].size]), _scaled(beta, b_vals[:keys[1].size])
    in_a, in_b = np.zeros(union.size, bool), np.zeros(union.size, bool)
    in_a[at_a], in_b[at_b] = True, True
    c_vals = np.zeros(union.size, dtype)
    c_vals[at_a] = from_a                                      # the product alone where the other matrix has nothing
    c_vals[at_b] = from_b
    both_a, both_b = in_b[at_a], in_a[at_b]                    # the same entries of C in the same (ascending) order
    c_vals[at_a[both_a]] = from_a[both_a] + from_b[both_b]
    c_ptr = np.searchsorted(union // max(int(n_cols), 1), np.arange(n_rows + 1), side="left")
    c_cols = union % max(int(n_cols), 1)
    return (c_ptr + base).astype(np.int32), (c_cols + base).astype(np.int32), np.ascontiguousarray(c_vals)


def _trsv_rows(row_ptr, col, base, side, diag):
    """The checks of spgpuCsrTrsvPlanDevice; (n_rows, 0-based row_ptr, 0-based col) as int64.  ValueError on each refusal."""
    if side not in (capi.TRSV_LOWER, capi.TRSV_UPPER) or diag not in (capi.TRSV_DIAG_STORED, capi.TRSV_DIAG_UNIT):
        raise ValueError("side is TRSV_LOWER or TRSV_UPPER, diag TRSV_DIAG_STORED or TRSV_DIAG_UNIT")
    ptr = np.asarray(row_ptr, np.int64) - base
    n_rows = ptr.size - 1
    col = np.asarray(col, np.int64)[:ptr[-1]] - base
    if col.size and (col.min() < 0 or col.max() >= n_rows):
        raise ValueError("a column lies outside the matrix")
    if diag == capi.TRSV_DIAG_STORED:
        row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr))
        diagonals = np.bincount(row_of[col == row_of], minlength=n_rows)
        if np.any(diagonals == 0):
            raise ValueError("a row stores no diagonal")
        if np.any(diagonals > 1):
            raise ValueError("a row stores its diagonal twice")
    return n_rows, ptr, col


def csr_trsv_plan(row_ptr, col, base=0, side=capi.TRSV_LOWER, diag=capi.TRSV_DIAG_STORED):
    """The arrays include/spgpu/ext/trsv_device.h defines, restated: (levels, row_order, level_ptr) of the square CSR matrix in
    `base`.  level(i) = 0 if row i stores no off-diagonal entry on `side`, else 1 + the largest level over those entries (symbolic: a
    stored zero counts); row_order lists the 0-based rows by (level, row) ascending; level_ptr[l] = the number of rows in levels
    < l, levels + 1 ints.  ValueError on what spgpuCsrTrsvPlanDevice refuses.  One Python step per row: a restatement for tests."""
    n_rows, ptr, col = _trsv_rows(row_ptr, col, base, side, diag)
    level = np.zeros(n_rows, np.int64)
    lower = side == capi.TRSV_LOWER
    for i in (range(n_rows) if lower else range(n_rows - 1, -1, -1)):
        js = col[ptr[i]:ptr[i + 1]]
        js = js[js < i] if lower else js[js > i]
        level[i] = 1 + level[js].max() if js.size else 0
    levels = int(level.max()) + 1 if n_rows > 0 else 0
    row_order = np.lexsort((np.arange(n_rows), level)).astype(np.int32)
    level_ptr = np.searchsorted(level[row_order], np.arange(levels + 1), side="left").astype(np.int32)
    return levels, row_order, level_ptr


def csr_trsv(row_ptr, col, vals, b, base=0, side=capi.TRSV_LOWER, diag=capi.TRSV_DIAG_STORED):
    """x = T^-1 * b as include/spgpu/ext/trsv_device.h defines it, restated with the element type's own scalar arithmetic, one
    operation at a time: acc = b_i; for each stored off-diagonal entry on `side` in storage order acc = acc - (a_ij * x_j), the
    product rounded and then the difference; x_i = acc / a_ii, or acc under TRSV_DIAG_UNIT.  Complex goes through its real parts:
    the product is re = ar*xr - ai*xi, im = ar*xi + ai*xr; the quotient den = dr*dr + di*di, re = (nr*dr + ni*di) / den,
    im = (ni*dr - nr*di) / den.  Entries on the other side, and a diagonal under TRSV_DIAG_UNIT, are never read.  ValueError on what
    spgpuCsrTrsvPlanDevice refuses.  One Python step per stored entry: a restatement for tests, not a tool."""
    n_rows, ptr, col = _trsv_rows(row_ptr, col, base, side, diag)
    vals, b = np.asarray(vals), np.asarray(b)
    dtype = vals.dtype
    if b.dtype != dtype:
        raise ValueError("the matrix and b hold different types")
    real = dtype.kind != "c"
    part = dtype if real else np.dtype("f%d" % (dtype.itemsize // 2))
    parts = 1 if real else 2
    v = np.ascontiguousarray(vals).view(part).reshape(-1, parts)
    x = np.ascontiguousarray(b[:n_rows]).copy().view(part).reshape(-1, parts)          # in place: b_i is read before x_i is written
    lower, stored = side == capi.TRSV_LOWER, diag == capi.TRSV_DIAG_STORED
    with np.errstate(all="ignore"):
        for i in (range(n_rows) if lower else range(n_rows - 1, -1, -1)):
            acc = [x[i, p] for p in range(parts)]
            pivot = None
            for e in range(ptr[i], ptr[i + 1]):
                j = col[e]
                if j == i:
                    if stored:
                        pivot = [v[e, p] for p in range(parts)]
                elif (j < i) if lower else (j > i):
                    if real:
                        product = v[e, 0] * x[j, 0]
                        acc = [acc[0] - product]
                    else:
                        ar, ai, xr, xi = v[e, 0], v[e, 1], x[j, 0], x[j, 1]
                        rr, ii, ri, ir = ar * xr, ai * xi, ar * xi, ai * xr
                        re, im = rr - ii, ri + ir
                        acc = [acc[0] - re, acc[1] - im]
            if stored and real:
                acc = [acc[0] / pivot[0]]
            elif stored:
                (nr, ni), (dr, di) = acc, pivot
                rr, ii = dr * dr, di * di
                den = rr + ii
                a, bb, c, d = nr * dr, ni * di, ni * dr, nr * di
                top, bottom = a + bb, c - d
                acc = [top / den, bottom / den]
            for p in range(parts):
                x[i, p] = acc[p]
    return x.reshape(-1).view(dtype)


def _ilu0_rows(row_ptr, col, base):
    """The checks of spgpuCsrIlu0PlanDevice; (n_rows, 0-based row_ptr, 0-based col, diag_pos) as int64.  ValueError on each refusal."""
    ptr = np.asarray(row_ptr, np.int64) - base
    n_rows = ptr.size - 1
    col = np.asarray(col, np.int64)[:ptr[-1]] - base
    if col.size and (col.min() < 0 or col.max() >= n_rows):
        raise ValueError("a column lies outside the matrix")
    row_of = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr))
    if np.any(np.diff(row_of * max(n_rows, 1) + col) <= 0):      # rows never descend, so only a row's own order can fail
        raise ValueError("a row does not ascend strictly")
    at = np.flatnonzero(col == row_of)
    if at.size != n_rows:                                         # ascending strictly: at most one per row
        raise ValueError("a row stores no diagonal")
    return n_rows, ptr, col, at


def csr_ilu0_plan(row_ptr, col, base=0):
    """The arrays include/spgpu/ext/ilu0_device.h defines, restated: (levels, row_order, level_ptr, diag_pos) of the square CSR
    matrix in `base` -- csr_trsv_plan's for the lower triangle with a stored diagonal, and diag_pos[i], the 0-based position of entry
    (i, i) in col.  ValueError on what spgpuCsrIlu0PlanDevice refuses: a column outside the matrix, a row that does not ascend
    strictly, a missing diagonal."""
    _, _, _, at = _ilu0_rows(row_ptr, col, base)
    return csr_trsv_plan(row_ptr, col, base, capi.TRSV_LOWER, capi.TRSV_DIAG_STORED) + (at.astype(np.int32),)


def csr_ilu0(row_ptr, col, vals, base=0):
    """lu = ILU(0) of a as include/spgpu/ext/ilu0_device.h defines it, restated with the element type's own scalar arithmetic, one
    operation at a time: lu starts as a copy of vals; row by row, for each stored (i, k) with k < i in ascending k first
    lu_ik = lu_ik / lu_kk, then for each stored (k, j) with j > k in ascending j, where row i stores (i, j),
    lu_ij = lu_ij - (lu_ik * lu_kj), the product rounded and then the difference; where it does not, the term is dropped.  Complex
    goes through its real parts: the product is re = ar*xr - ai*xi, im = ar*xi + ai*xr; the quotient den = dr*dr + di*di,
    re = (nr*dr + ni*di) / den, im = (ni*dr - nr*di) / den.  ValueError on what spgpuCsrIlu0PlanDevice refuses.  One Python step per
    update: a restatement for tests, not a tool."""
    n_rows, ptr, col, diag = _ilu0_rows(row_ptr, col, base)
    vals = np.asarray(vals)
    dtype = vals.dtype
    real = dtype.kind != "c"
    part = dtype if real else np.dtype("f%d" % (dtype.itemsize // 2))
    parts = 1 if real else 2
    lu = np.ascontiguousarray(vals[:ptr[-1]]).copy().view(part).reshape(-1, parts)
    with np.errstate(all="ignore"):
        for i in range(n_rows):
            where = {int(col[q]): q for q in range(ptr[i], ptr[i + 1])}
            for e in range(ptr[i], diag[i]):
                k = col[e]
                if real:
                    m = [lu[e, 0] / lu[diag[k], 0]]
                else:
                    (nr, ni), (dr, di) = lu[e], lu[diag[k]]
                    rr, ii = dr * dr, di * di
                    den = rr + ii
                    a, b, c, d = nr * dr, ni * di, ni * dr, nr * di
                    top, bottom = a + b, c - d
                    m = [top / den, bottom / den]
                for p in range(parts):
                    lu[e, p] = m[p]
                for at in range(diag[k] + 1, ptr[k + 1]):
                    q = where.get(int(col[at]))
                    if q is None:
                        continue                                   # no fill
                    if real:
                        product = m[0] * lu[at, 0]
                        lu[q, 0] = lu[q, 0] - product
                    else:
                        (ar, ai), (xr, xi) = m, lu[at]
                        rr, ii, ri, ir = ar * xr, ai * xi, ar * xi, ai * xr
                        re, im = rr - ii, ri + ir
                        lu[q, 0], lu[q, 1] = lu[q, 0] - re, lu[q, 1] - im
    return lu.reshape(-1).view(dtype)


def _square_csr(row_ptr, col, base):
    """(n_rows, 0-based row_ptr, 0-based col, the row of every entry) of a square CSR matrix in `base`, as int64."""
    ptr = np.asarray(row_ptr, np.int64) - base
    n_rows = ptr.size - 1
    col = np.asarray(col, np.int64)[:ptr[-1]] - base
    return n_rows, ptr, col, np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(ptr))


def csr_strength(row_ptr, col, vals, base, theta):
    """(strong, diag_abs) as include/spgpu/ext/aggregate_device.h defines them, restated in the element type's own arithmetic, one
    operation at a time: d_i = |a_ii| of the first stored (i, i), +0 without one; t = T(theta*theta), the product in double and one
    conversion; strong[p] = (j != i) and a_ij*a_ij >= (t*d_i)*d_j.  A NaN on either side gives 0; a column outside the matrix gives 0
    and d_j is not read.  Real types only (ValueError otherwise)."""
    n_rows, ptr, col, row_of = _square_csr(row_ptr, col, base)
    vals = np.ascontiguousarray(np.asarray(vals)[:ptr[-1]])
    if vals.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("the strength of connection is defined for real types only")
    T = vals.dtype.type
    diag_abs = np.zeros(n_rows, vals.dtype)
    at = np.flatnonzero(col == row_of)
    rows_with, first = np.unique(row_of[at], return_index=True)       # the first stored diagonal of every row that has one
    diag_abs[rows_with] = np.abs(vals[at[first]])
    t = T(float(theta) * float(theta))
    inside = (col >= 0) & (col < n_rows)
    other = np.where(inside, col, 0)
    with np.errstate(all="ignore"):
        lhs = vals * vals
        rhs = (t * diag_abs[row_of]) * diag_abs[other]
        strong = inside & (col != row_of) & (lhs >= rhs)
    return strong.astype(np.uint8), diag_abs


def _lowbias32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def aggregate_priority(n_rows):
    """hash(i) = lowbias32(i) >> 1 for i < n_rows (uint64, 31 bits)."""
    return (_lowbias32(np.arange(n_rows, dtype=np.uint32)) >> np.uint32(1)).astype(np.uint64)


def csr_aggregate(row_ptr, col, strong, base, priority=None):
    """(count, rounds, aggregate_of, sizes) as include/spgpu/ext/aggregate_device.h defines them, restated round by round.  S(i) is
    the columns j != i of row i's entries with strong[p] != 0 (strong None: every stored j != i).  Every node starts UNDECIDED with
    the tuple (state, hash(i), i) in one 64-bit word, OUT = 0 < UNDECIDED = 1 < ROOT = 2.  A round: t1[i] = max(t0[i], max of t0 over
    S(i)), t2[i] = max(t1[i], max of t1 over S(i)); an undecided i with t2[i] == t0[i] becomes ROOT, otherwise under a ROOT's tuple
    OUT.  Rounds repeat until nobody is undecided; roots are numbered by ascending row; two joining passes, each reading the array of
    the pass before, give an unassigned node the smallest aggregate number among the assigned nodes of S(i).  ValueError on what
    spgpuCsrAggregateDevice refuses: a neighbour outside the matrix.  `priority` replaces hash(i) (uint64 below 2**31): for tests
    that compare priorities, not a parameter of the device call."""
    n_rows, ptr, col, row_of = _square_csr(row_ptr, col, base)
    keep = np.ones(col.size, bool) if strong is None else np.asarray(strong)[:col.size] != 0
    if np.any(keep & ((col < 0) | (col >= n_rows))):
        raise ValueError("a neighbour lies outside the matrix")
    keep &= col != row_of
    src, dst = row_of[keep], col[keep]
    OUT, UNDECIDED, ROOT = np.uint64(0), np.uint64(1), np.uint64(2)
    shift = np.uint64(62)
    low = ((aggregate_priority(n_rows) if priority is None else np.asarray(priority, np.uint64)) << np.uint64(31)) \
        | np.arange(n_rows, dtype=np.uint64)
    state = np.full(n_rows, UNDECIDED, np.uint64)

    def sweep(t):
        out = t.copy()
        np.maximum.at(out, src, t[dst])
        return out

    rounds = 0
    while np.any(state == UNDECIDED):
        t0 = (state << shift) | low
        t2 = sweep(sweep(t0))
        undecided = state == UNDECIDED
        roots = undecided & (t2 == t0)
        outs = undecided & ~roots & ((t2 >> shift) == ROOT)
        state[roots], state[outs] = ROOT, OUT
        rounds += 1
    is_root = state == ROOT
    count = int(is_root.sum())
    number = np.cumsum(is_root) - is_root                             # the exclusive scan
    assigned = np.where(is_root, number, -1).astype(np.int64)
    for _ in range(2):                                                # the joining passes, each from the array of the pass before
        theirs = assigned[dst]
        best = np.full(n_rows, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(best, src[theirs >= 0], theirs[theirs >= 0])
        assigned = np.where((assigned < 0) & (best < np.iinfo(np.int64).max), best, assigned)
    assert n_rows == 0 or assigned.min() >= 0, "a node without an aggregate after pass 2"
    return count, rounds, assigned.astype(np.int32), np.bincount(assigned, minlength=count).astype(np.int32)


def csr_tentative(aggregate_of, candidate, base, dtype):
    """(t_ptr, t_cols, t_vals) of the tentative prolongator of include/spgpu/ext/aggregate_device.h: one entry per row, in column
    aggregate_of[i] + base, holding the bits of candidate[i], or 1 of `dtype` when candidate is None."""
    aggregate_of = np.asarray(aggregate_of, np.int32)
    n_rows = aggregate_of.size
    vals = np.ones(n_rows, dtype) if candidate is None else np.ascontiguousarray(np.asarray(candidate)[:n_rows]).copy()
    assert vals.dtype == np.dtype(dtype)
    return (np.arange(n_rows + 1, dtype=np.int32) + np.int32(base)), aggregate_of + np.int32(base), vals


def csr_colour(row_ptr, col, base, priority=None):
    """(colours, rounds, colour_of) as include/spgpu/ext/colour_device.h defines them, restated round by round.  N(i) is the columns
    j != i of row i's stored entries; the tuple of node i is (hash(i), i) in one 64-bit word; every node starts with colour -1.  A
    round reads c0 and writes c1: an uncoloured i is ready if every j in N(i) has c0[j] >= 0 or a smaller tuple, and a ready i takes
    the smallest c >= 0 that is no c0[j], j in N(i); every other node keeps c0[i].  Rounds repeat until nobody is uncoloured.
    ValueError on what spgpuCsrColourDevice refuses: a column outside the matrix.  `priority` replaces hash(i) (uint64 below 2**31):
    for tests that compare priorities, not a parameter of the device call."""
    n_rows, ptr, col, row_of = _square_csr(row_ptr, col, base)
    if np.any((col < 0) | (col >= n_rows)):
        raise ValueError("a column lies outside the matrix")
    keep = col != row_of
    src, dst = row_of[keep], col[keep]
    tuples = ((aggregate_priority(n_rows) if priority is None else np.asarray(priority, np.uint64)) << np.uint64(32)) \
        | np.arange(n_rows, dtype=np.uint64)
    colour = np.full(n_rows, -1, np.int64)
    rounds = 0
    while np.any(colour < 0):
        c0 = colour
        waits = np.zeros(n_rows, bool)                                # an uncoloured neighbour with a larger tuple
        waits[src[(c0[dst] < 0) & (tuples[dst] > tuples[src])]] = True
        ready = (c0 < 0) & ~waits
        taken = ready[src] & (c0[dst] >= 0)                           # (node, a colour one of its neighbours holds), each pair once
        pairs = np.unique(src[taken] * np.int64(n_rows + 1) + c0[dst[taken]])
        node, held = pairs // (n_rows + 1), pairs % (n_rows + 1)
        first = np.searchsorted(node, node, side="left")
        rank = np.arange(pairs.size) - first                          # the held colours of a node ascend: the first gap is free
        free = np.bincount(node, minlength=n_rows).astype(np.int64)   # no gap: the number of colours held
        np.minimum.at(free, node[held != rank], rank[held != rank])
        colour = np.where(ready, free, c0)
        rounds += 1
    return (int(colour.max()) + 1 if n_rows > 0 else 0), rounds, colour.astype(np.int32)


def csr_colour_order(colour_of, colours):
    """(order, inverse, colour_ptr) of include/spgpu/ext/colour_device.h: the 0-based rows by (colour, row) ascending,
    inverse[order[k]] = k, and colour_ptr[c] = the number of rows of colours < c for c <= colours."""
    colour_of = np.asarray(colour_of, np.int64)
    n_rows = colour_of.size
    order = np.lexsort((np.arange(n_rows), colour_of))
    inverse = np.empty(n_rows, np.int64)
    inverse[order] = np.arange(n_rows)
    colour_ptr = np.searchsorted(colour_of[order], np.arange(colours + 1), side="left")
    return order.astype(np.int32), inverse.astype(np.int32), colour_ptr.astype(np.int32)


def csr_permute(order, inverse, a_ptr, a_cols, a_vals, base):
    """(b_ptr, b_cols, b_vals) of B = A(order, order) as include/spgpu/ext/colour_device.h defines it: row k of B is row order[k] of
    A, a stored column j becomes inverse[j - base] + base, a row's entries ascend by new column, equal columns in A's storage
    order; the values are moved, not computed."""
    n_rows, ptr, col, row_of = _square_csr(a_ptr, a_cols, base)
    order, inverse = np.asarray(order, np.int64), np.asarray(inverse, np.int64)
    vals = np.ascontiguousarray(np.asarray(a_vals)[:ptr[-1]])
    b_ptr = np.zeros(n_rows + 1, np.int64)
    b_ptr[1:] = np.cumsum(np.diff(ptr)[order])
    new_row, new_col = inverse[row_of], inverse[col]
    at = np.lexsort((np.arange(col.size), new_col, new_row))
    return (b_ptr + base).astype(np.int32), (new_col[at] + base).astype(np.int32), vals[at].copy()


def csr_sweep_plan(row_ptr, col, base, colours, colour_ptr, colour_of=None, order=None):
    """(diag_pos, colour_ptr_host, entries) as include/spgpu/ext/sweep_device.h defines them: diag_pos[i] the 0-based position of
    entry (i, i), the colours + 1 ints of colour_ptr, and row_ptr[rows] - base.  With `order` the colour of node k is colour_of[k];
    without one it is the c with colour_ptr[c] <= k < colour_ptr[c + 1] and colour_of is not read.  ValueError on what
    spgpuCsrSweepPlanDevice refuses: a column outside the matrix, a row without its diagonal or with two, a colour_of outside
    [0, colours) under an order, a stored off-diagonal entry between two nodes of one colour, a colour_ptr that does not start at 0,
    descends or does not end at the number of rows."""
    n_rows, ptr, col, row_of = _square_csr(row_ptr, col, base)
    colour_ptr = np.asarray(colour_ptr, np.int64)[:colours + 1]
    if n_rows > 0 and (colours < 1 or colour_ptr.size != colours + 1 or colour_ptr[0] != 0 or colour_ptr[-1] != n_rows
                       or np.any(np.diff(colour_ptr) < 0)):
        raise ValueError("colour_ptr does not describe the rows")
    if col.size and (col.min() < 0 or col.max() >= n_rows):
        raise ValueError("a column lies outside the matrix")
    diagonal = col == row_of
    counts = np.bincount(row_of[diagonal], minlength=n_rows)
    if np.any(counts == 0):
        raise ValueError("a row stores no diagonal")
    if np.any(counts > 1):
        raise ValueError("a row stores its diagonal twice")
    if order is not None:
        colour = np.asarray(colour_of, np.int64)[:n_rows]
        if np.any(colour < 0) or np.any(colour >= colours):
            raise ValueError("a colour lies outside [0, colours)")
    else:
        colour = np.searchsorted(colour_ptr, np.arange(n_rows), side="right") - 1
    if np.any(colour[row_of[~diagonal]] == colour[col[~diagonal]]):
        raise ValueError("a stored entry joins two nodes of one colour")
    return np.flatnonzero(diagonal).astype(np.int32), colour_ptr.astype(np.int32), int(ptr[-1])


def _parts_of(a, dtype):
    """A contiguous copy of `a` as rows of its real parts (one part for a real type, two for a complex one) and the part type."""
    part = dtype if dtype.kind != "c" else np.dtype("f%d" % (dtype.itemsize // 2))
    return np.ascontiguousarray(a).copy().view(part).reshape(-1, 1 if dtype.kind != "c" else 2), part


def _sub_products(acc, v, x, ptr, col, i, skip):
    """acc - the sum of a_e * x[col_e] over row i in storage order, position `skip` left out: every product rounded (six operations
    for complex), then the difference, in the part type's own scalar arithmetic."""
    real = len(acc) == 1
    for e in range(ptr[i], ptr[i + 1]):
        if e == skip:
            continue
        j = col[e]
        if real:
            product = v[e, 0] * x[j, 0]
            acc = [acc[0] - product]
        else:
            ar, ai, xr, xi = v[e, 0], v[e, 1], x[j, 0], x[j, 1]
            rr, ii, ri, ir = ar * xr, ai * xi, ar * xi, ai * xr
            re, im = rr - ii, ri + ir
            acc = [acc[0] - re, acc[1] - im]
    return acc


def csr_sweep(row_ptr, col, vals, b, x, base, colours, colour_ptr_host, diag_pos, order=None, direction=capi.SWEEP_FORWARD, omega=None):
    """x after one spgpuCsrSweepDevice as include/spgpu/ext/sweep_device.h defines it (a new array), restated with the element type's
    own scalar arithmetic, one operation at a time.  For every colour of the direction and every row i of it: acc = b_i; for each
    stored entry but the one at diag_pos[i], in storage order, acc = acc - (a_e * x[col_e]); g = acc / a_ii; x_i = g without omega,
    else d = g - x_i and x_i = x_i + (omega * d).  Complex goes through its real parts as in csr_trsv.  SYMMETRIC is the forward
    list and then the backward list.  One Python step per stored entry: a restatement for tests, not a tool."""
    n_rows, ptr, col, _ = _square_csr(row_ptr, col, base)
    vals, b, x = np.asarray(vals), np.asarray(b), np.asarray(x)
    dtype = vals.dtype
    if b.dtype != dtype or x.dtype != dtype:
        raise ValueError("the matrix, b and x hold different types")
    real = dtype.kind != "c"
    v, part = _parts_of(vals, dtype)
    rhs, _ = _parts_of(b[:n_rows], dtype)
    out, _ = _parts_of(x[:n_rows], dtype)
    w = None if omega is None else _parts_of(np.array([omega], dtype), dtype)[0][0]
    cp = np.asarray(colour_ptr_host, np.int64)
    passes = {capi.SWEEP_FORWARD: list(range(colours)), capi.SWEEP_BACKWARD: list(range(colours - 1, -1, -1)),
              capi.SWEEP_SYMMETRIC: list(range(colours)) + list(range(colours - 1, -1, -1))}[direction]
    with np.errstate(all="ignore"):
        for c in (passes if n_rows > 0 else []):
            for t in range(cp[c], cp[c + 1]):
                i = int(order[t]) if order is not None else t
                d = int(diag_pos[i])
                acc = _sub_products([rhs[i, p] for p in range(len(rhs[i]))], v, out, ptr, col, i, d)
                if real:
                    g = [acc[0] / v[d, 0]]
                else:
                    (nr, ni), (dr, di) = acc, (v[d, 0], v[d, 1])
                    rr, ii = dr * dr, di * di
                    den = rr + ii
                    a, bb, cc, dd = nr * dr, ni * di, ni * dr, nr * di
                    top, bottom = a + bb, cc - dd
                    g = [top / den, bottom / den]
                if w is not None:
                    mine = [out[i, p] for p in range(len(g))]
                    diff = [g[p] - mine[p] for p in range(len(g))]
                    if real:
                        product = w[0] * diff[0]
                        g = [mine[0] + product]
                    else:
                        rr, ii, ri, ir = w[0] * diff[0], w[1] * diff[1], w[0] * diff[1], w[1] * diff[0]
                        re, im = rr - ii, ri + ir
                        g = [mine[0] + re, mine[1] + im]
                for p in range(len(g)):
                    out[i, p] = g[p]
    return out.reshape(-1).view(dtype)


def csr_residual(row_ptr, col, vals, b, x, base):
    """r = b - A * x as include/spgpu/ext/sweep_device.h defines it: r_i starts as b_i and every stored entry of row i, the diagonal
    included, is subtracted in storage order, the product rounded and then the difference.  An empty row moves b_i's bits."""
    n_rows, ptr, col, _ = _square_csr(row_ptr, col, base)
    vals, b, x = np.asarray(vals), np.asarray(b), np.asarray(x)
    dtype = vals.dtype
    if b.dtype != dtype or x.dtype != dtype:
        raise ValueError("the matrix, b and x hold different types")
    v, _ = _parts_of(vals, dtype)
    r, _ = _parts_of(b[:n_rows], dtype)
    xs, _ = _parts_of(x, dtype)
    with np.errstate(all="ignore"):
        for i in range(n_rows):
            acc = _sub_products([r[i, p] for p in range(r.shape[1])], v, xs, ptr, col, i, -1)
            for p in range(len(acc)):
                r[i, p] = acc[p]
    return r.reshape(-1).view(dtype)


def hell_transpose_device(handle, cM, rP, hack_offsets, rS, r_idx, n_rows, n_cols, hack_size, base, slots, letter, t_hack_size=32,
                          t_base=0, ell_pitches=None):
    """HELL (or, with ell_pitches = (values pitch, indices pitch), ELL) arrays in HBM -> the HELL arrays of A^T in HBM, through
    the C ABI: spgpu{Hell,Ell}TransposeLengthsDevice -> spgpuHellPlanDevice -> spgpu{Hell,Ell}TransposeDevice.
    Returns a dict of torch tensors (cM, rP, hack_offsets, rS) plus sizes; rows = n_cols."""
    import torch
    dev = rP.device
    torch.cuda.synchronize()
    work = torch.empty(capi.spgpuHellTransposeWorkBytes(n_rows, n_cols, slots), dtype=torch.uint8, device=dev)
    lengths = torch.empty(max(n_cols, 1), dtype=torch.int32, device=dev)
    longest, nnz, height = C.c_int(0), C.c_int(0), C.c_int(0)
    ok = lambda status: status == capi.SPGPU_SUCCESS or (_ for _ in ()).throw(RuntimeError(f"status {status}"))
    if ell_pitches is None:
        ok(capi.spgpuHellTransposeLengthsDevice(handle, _dp(lengths), C.byref(longest), C.byref(nnz), _dp(rP), hack_size,
                                                _dp(hack_offsets), _dp(rS), _dp(r_idx), n_rows, n_cols, base, slots, _dp(work)))
    else:
        ok(capi.spgpuEllTransposeLengthsDevice(handle, _dp(lengths), C.byref(longest), C.byref(nnz), _dp(rP), ell_pitches[1],
                                               _dp(rS), _dp(r_idx), n_rows, n_cols, base, slots, _dp(work)))
    hacks = (n_cols + t_hack_size - 1) // t_hack_size
    t_offsets = torch.empty(max(hacks, 1), dtype=torch.int32, device=dev)
    ok(capi.spgpuHellPlanDevice(handle, C.byref(height), _dp(t_offsets), t_hack_size, n_cols, _dp(lengths), _dp(work)))
    t_slots = t_hack_size * height.value
    t_values = torch.zeros(max(t_slots, 1), dtype=cM.dtype, device=dev)
    t_indices = torch.zeros(max(t_slots, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    code = capi.TYPE_CODE[letter]
    if ell_pitches is None:
        ok(capi.spgpuHellTransposeDevice(handle, _dp(t_values), _dp(t_indices), _dp(t_offsets), t_hack_size, t_base, _dp(cM), _dp(rP),
                                         hack_size, _dp(hack_offsets), _dp(rS), _dp(r_idx), n_rows, n_cols, base, slots, code,
                                         _dp(lengths), _dp(work)))
    else:
        ok(capi.spgpuEllTransposeDevice(handle, _dp(t_values), _dp(t_indices), _dp(t_offsets), t_hack_size, t_base, _dp(cM), _dp(rP),
                                        ell_pitches[0], ell_pitches[1], _dp(rS), _dp(r_idx), n_rows, n_cols, base, slots, code,
                                        _dp(lengths), _dp(work)))
    torch.cuda.synchronize()
    return dict(letter=letter, rows=n_cols, cols=n_rows, hack_size=t_hack_size, nnz=nnz.value, slots=t_slots, cM=t_values,
                rP=t_indices, hack_offsets=t_offsets, rS=lengths, rIdx=None, base=t_base, longest=longest.value)


def coo_to_ordered_hell_device(handle, n_rows, coo_rows, coo_cols, coo_vals, letter, hack_size=32, window=0, long_rows=0,
                               coo_base=0, hell_base=0, order=True, r_idx_given=None, aligned=False):
    """COO arrays in HBM (torch tensors) -> HELL in HBM with its rows ordered by length, all through the C ABI:
    spgpuCooRowLengthsDevice -> spgpuOellOrderDevice -> spgpuCooPermuteRowsDevice -> spgpuCooRowLengthsDevice ->
    spgpuHellPlanDevice -> spgpuCooToHellDevice.  order=False skips the ordering (plain HELL, rIdx None).
    Returns a dict of torch tensors (cM, rP, hack_offsets, rS, rIdx) plus sizes."""
    import torch
    dev = coo_rows.device
    nnz = int(coo_rows.numel())
    torch.cuda.synchronize()   # the COO arrays were filled on torch's stream; the library works on the handle's
    work = torch.empty(capi.spgpuCooConvertWorkBytes(n_rows, nnz), dtype=torch.uint8, device=dev)
    lengths = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    longest = C.c_int(0)
    ok = lambda status: status == capi.SPGPU_SUCCESS or (_ for _ in ()).throw(RuntimeError(f"status {status}"))
    ok(capi.spgpuCooRowLengthsDevice(handle, _dp(lengths), C.byref(longest), n_rows, nnz, _dp(coo_rows), coo_base, _dp(work)))
    r_idx = None
    rows_in = coo_rows
    if order:
        order_work = torch.empty(capi.spgpuOellOrderWorkBytes(n_rows), dtype=torch.uint8, device=dev)
        r_idx = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
        sorted_lengths = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
        if r_idx_given is not None:      # experiments: an order computed elsewhere (any permutation of the rows)
            r_idx.copy_(r_idx_given)
        else:
            order_call = capi.spgpuOellOrderAlignedDevice if aligned else capi.spgpuOellOrderDevice
            ok(order_call(handle, _dp(r_idx), _dp(sorted_lengths), _dp(lengths), n_rows, window, long_rows, _dp(order_work)))
        inverse = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
        rows_in = torch.empty_like(coo_rows)
        ok(capi.spgpuCooPermuteRowsDevice(handle, _dp(rows_in), _dp(coo_rows), nnz, _dp(r_idx), n_rows, coo_base, _dp(inverse)))
        # returns a host scalar, i.e. synchronises the stream: the order scratch can go afterwards
        ok(capi.spgpuCooRowLengthsDevice(handle, _dp(lengths), C.byref(longest), n_rows, nnz, _dp(rows_in), coo_base, _dp(work)))
        del order_work, inverse
    hacks = (n_rows + hack_size - 1) // hack_size
    hack_offsets = torch.empty(max(hacks, 1), dtype=torch.int32, device=dev)
    height = C.c_int(0)
    ok(capi.spgpuHellPlanDevice(handle, C.byref(height), _dp(hack_offsets), hack_size, n_rows, _dp(lengths), _dp(work)))
    slots = hack_size * height.value
    cM = torch.zeros(max(slots, 1), dtype=coo_vals.dtype, device=dev)
    rP = torch.zeros(max(slots, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ok(capi.spgpuCooToHellDevice(handle, _dp(cM), _dp(rP), _dp(hack_offsets), hack_size, hell_base, n_rows, nnz,
                                 _dp(rows_in), _dp(coo_cols), _dp(coo_vals), coo_base, capi.TYPE_CODE[letter], _dp(lengths),
                                 _dp(work)))
    torch.cuda.synchronize()
    return dict(letter=letter, rows=n_rows, hack_size=hack_size, nnz=nnz, slots=slots, cM=cM, rP=rP, hack_offsets=hack_offsets,
                rS=lengths, rIdx=r_idx, base=hell_base, longest=longest.value)


# ---- device residency + SpMV calls -------------------------------------------------

def to_device(a, device="cuda:0"):
    """numpy array -> torch tensor in HBM (the reference's cudaMalloc + cudaMemcpy)."""
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class DeviceHell:
    """A HELL matrix resident in HBM; ``spmv`` is one spgpu?hellspmv call."""

    def __init__(self, hell, device="cuda:0", r_idx=None):
        self.letter, self.rows = hell["letter"], hell["rows"]
        self.hack_size, self.base = hell["hack_size"], hell["base"]
        self.cM, self.rP = to_device(hell["values"], device), to_device(hell["indices"], device)
        self.hack_offsets = to_device(hell["hack_offsets"], device)
        self.rS = to_device(hell["row_lengths"], device)
        self.rIdx = to_device(r_idx, device)
        self.nnz = int(np.sum(hell["row_lengths"], dtype=np.int64))

    def spmv(self, handle, z, y, alpha, x, beta, avg_nnz=0):
        L = self.letter
        capi.hellspmv[L](handle, _dp(z), _dp(y), capi.scalar(L, alpha), _dp(self.cM), _dp(self.rP),
                         self.hack_size, _dp(self.hack_offsets), _dp(self.rS), _dp(self.rIdx), avg_nnz,
                         self.rows, _dp(x), capi.scalar(L, beta), self.base)


class DeviceEll:
    """An ELL matrix resident in HBM; ``spmv`` is one spgpu?ellspmv call."""

    def __init__(self, ell, device="cuda:0", r_idx=None, with_row_sizes=True):
        self.letter, self.rows = ell["letter"], ell["rows"]
        self.pitch, self.max_row, self.base = ell["pitch"], ell["max_row"], ell["base"]
        self.cM, self.rP = to_device(ell["values"], device), to_device(ell["indices"], device)
        self.rS = to_device(ell["row_lengths"], device) if with_row_sizes else None
        self.rIdx = to_device(r_idx, device)
        self.nnz = int(np.sum(ell["row_lengths"], dtype=np.int64))

    def spmv(self, handle, z, y, alpha, x, beta, avg_nnz=0):
        L = self.letter
        capi.ellspmv[L](handle, _dp(z), _dp(y), capi.scalar(L, alpha), _dp(self.cM), _dp(self.rP),
                        self.pitch, self.pitch, _dp(self.rS), _dp(self.rIdx), avg_nnz, self.max_row,
                        self.rows, _dp(x), capi.scalar(L, beta), self.base)


class DeviceHdia:
    """An HDIA matrix resident in HBM; ``spmv`` is one spgpu?hdiaspmv call."""

    def __init__(self, hdia, device="cuda:0"):
        self.letter, self.rows, self.cols = hdia["letter"], hdia["rows"], hdia["cols"]
        self.hack_size = hdia["hack_size"]
        self.dM, self.offsets = to_device(hdia["values"], device), to_device(hdia["offsets"], device)
        self.hack_offsets = to_device(hdia["hack_offsets"], device)

    def spmv(self, handle, z, y, alpha, x, beta):
        L = self.letter
        capi.hdiaspmv[L](handle, _dp(z), _dp(y), capi.scalar(L, alpha), _dp(self.dM), _dp(self.offsets),
                         self.hack_size, _dp(self.hack_offsets), self.rows, self.cols, _dp(x),
                         capi.scalar(L, beta))


class DeviceDia:
    """A DIA matrix resident in HBM; ``spmv`` is one spgpu?diaspmv call."""

    def __init__(self, dia, device="cuda:0"):
        self.letter, self.rows, self.cols = dia["letter"], dia["rows"], dia["cols"]
        self.pitch, self.diags = dia["pitch"], dia["diags"]
        self.dM, self.offsets = to_device(dia["values"], device), to_device(dia["offsets"], device)

    def spmv(self, handle, z, y, alpha, x, beta):
        L = self.letter
        capi.diaspmv[L](handle, _dp(z), _dp(y), capi.scalar(L, alpha), _dp(self.dM), _dp(self.offsets), self.pitch,
                        self.rows, self.cols, self.diags, _dp(x), capi.scalar(L, beta))
