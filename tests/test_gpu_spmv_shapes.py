"""GPU: spgpu{S,D,C,Z}hellspmv / spgpu{S,D,C,Z}ellspmv with rIdx == NULL on every kernel shape and branch the dispatch for rows as
they come can choose (spgpu_amd/csrc/ellpack_spmv.hip launchSlabFamily -> launchRowsAsTheyCome; slabSpmvKernel, sweepSpmvKernel,
formProbeKernel).  The case table, the dispatch restated, the kernel walk and the builders are tests/spmv_launch_shapes.py;
tests/test_spmv_launch_shapes.py checks on the CPU that the table reaches every instantiation and branch.

Each case
  * places its operands as it says (elements past a 16-byte boundary), sentinels on both sides of z;
  * asserts the route from the REAL device addresses through the restated dispatch, and spgpuGetLastSpmvForm after the call (the
    AUTO cases without a lean hint are called twice: STRIPS on the new matrix, then the form its samples settle);
  * compares z with the extended-precision product (exact_ref.spmv, tolerance 1e-6 fp64 / 1e-4 fp32 of the row's magnitude) and,
    byte for byte, with the oracle adding in the order of the kernel the route names (oracle_api.spmv_tail; the CPU module ties
    that to default_spmv / hell_spmv(phases=) where those apply).
The matrices' padding slots, the rows past the last one and the entries below the index base hold NaN: a product that uses one
shows in both comparisons."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O
import spmv_launch_shapes as M
from test_gpu_fused_shapes import SENTINEL, _assert_margins, _guard, _place, _same_bytes, _start

pytestmark = pytest.mark.gpu

TABLE = {L: M.cases(L) for L in M.LETTERS}
# (letter, case id) -> the matrix on the device, kept for the session: AUTO keys what it learnt about a matrix by (rP, rows), and a
# freed rP whose address the next case's gets would hand that case the answers of this one.  About 830 small matrices, 33 MiB of
# coefficients and indices in all (the sum over the table, counted on the host); vectors are not kept.
_DEVICE = {}


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _device_matrix(letter, cid, m, off):
    import torch
    key = (letter, cid)
    if key not in _DEVICE:
        d = dict(cM=_place(m["values"], off["cM"])[1], rP=_place(m["indices"], off["rP"])[1],
                 rS=None if m["rs_null"] else torch.from_numpy(np.ascontiguousarray(m["row_lengths"])).to("cuda:0"))
        if m["fmt"] == "hell":
            d["hackOffsets"] = torch.from_numpy(np.ascontiguousarray(m["hack_offsets"])).to("cuda:0")
        _DEVICE[key] = d
    return _DEVICE[key]


def _call(gpu, cid, letter, m, dev, dz, dy, alpha, dx, beta, avg):
    from spgpu_amd import capi
    if m["fmt"] == "hell":
        _guard(cid, capi.hellspmv[letter], gpu, _p(dz), _p(dy), capi.scalar(letter, alpha), _p(dev["cM"]), _p(dev["rP"]), m["hack_size"],
               _p(dev["hackOffsets"]), _p(dev["rS"]), None, avg, m["rows"], _p(dx), capi.scalar(letter, beta), m["base"])
    else:
        _guard(cid, capi.ellspmv[letter], gpu, _p(dz), _p(dy), capi.scalar(letter, alpha), _p(dev["cM"]), _p(dev["rP"]), m["val_pitch"],
               m["pitch"], _p(dev["rS"]), None, avg, m["max_row"], m["rows"], _p(dx), capi.scalar(letter, beta), m["base"])


def _oracle(m, x, y, alpha, beta, kernel):
    return O.spmv_tail(M.oracle_view(m), x, y if beta != 0 else None, alpha, beta, with_row_sizes=not m["rs_null"], **M.oracle_shape(kernel))


def _nan_vector(letter, n):
    return np.full(n, complex(np.nan, np.nan) if letter in "CZ" else np.nan, M.DTYPE[letter])


@pytest.mark.parametrize("letter,cid", [pytest.param(L, cid, id=f"{L}-{cid}") for L in M.LETTERS for cid in TABLE[L]])
def test_spmv_case(gpu, letter, cid):
    from spgpu_amd import capi
    _start()
    case = TABLE[letter][cid]
    m = M.matrix_of(case)
    n, off = m["rows"], case["off"]
    x, y = M.operands(letter, m)
    alpha, beta = M.scalars_of(case)
    dev = _device_matrix(letter, cid, m, off)
    _, dx = _place(x, off["x"])
    y_dev = y if beta != 0 else _nan_vector(letter, n)                # beta == 0: y is full of NaN and must not be read
    if case["y_mode"] == "z":
        z_buf, dz = _place(y_dev, off["z"])
        dy = dz
    else:
        z_buf, dz = _place(np.full(n, SENTINEL, M.DTYPE[letter]), off["z"])
        dy = _place(y_dev, off["y"])[1]
    # the route, from the addresses the call is made with
    addr = dict(cM=dev["cM"].data_ptr(), rP=dev["rP"].data_ptr(), z=dz.data_ptr(), y=dy.data_ptr())
    route = M.case_dispatch(case, addr=addr)
    planned = M.case_dispatch(case)
    assert (route["kernel"], route["wide_io"]) == (planned["kernel"], planned["wide_io"]), f"{cid}: the allocator moved an operand"
    assert route["kernel"] == M.route_kernel(letter, case["route"], m["fmt"] == "hell", beta != 0), M.kernel_name(route["kernel"])
    capi.spgpuSetSpmvForm(gpu, case["form"])
    try:
        _call(gpu, cid, letter, m, dev, dz, dy, alpha, dx, beta, case["avg"])
        noted = capi.spgpuGetLastSpmvForm(gpu)
        assert noted == route["noted"], (noted, route["noted"])
        if case["route"] == "auto-first":
            # AUTO without a lean hint: the strip-capable kernel on a matrix it has not seen (above); its sample wavefronts see rows of
            # one stage and say "scattered", so the second call -- _call has synchronised -- runs the gather kernel, with the probe
            # in front of it.  Same order of additions: the same bytes.
            settled = M.case_dispatch(case, addr=addr, vote=M.vote_form(letter, n, [1, 1, 1], 1))
            assert (settled["noted"], settled["probe"]) == (M.GATHER, M.form_probe(letter, m["fmt"] == "hell", True))
            first = _assert_margins(z_buf, off["z"], n, f"{cid}: z of the first call")
            if case["y_mode"] == "z":
                z_buf, dz = _place(y_dev, off["z"])
                dy = dz
            else:
                z_buf, dz = _place(np.full(n, SENTINEL, M.DTYPE[letter]), off["z"])
            _call(gpu, cid, letter, m, dev, dz, dy, alpha, dx, beta, case["avg"])
            assert capi.spgpuGetLastSpmvForm(gpu) == settled["noted"], capi.spgpuGetLastSpmvForm(gpu)
            _same_bytes(_assert_margins(z_buf, off["z"], n, f"{cid}: z of the second call"), first, f"{cid}: second call against the first")
    finally:
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
    got = _assert_margins(z_buf, off["z"], n, f"{cid}: z")
    r, c, v = m["coo"]
    want, scale = X.spmv(n, r, c, v, x, y if beta != 0 else None, alpha, beta)
    X.assert_within(got, want, scale, letter, case=cid)
    _same_bytes(got, _oracle(m, x, y, alpha, beta, route["kernel"]), f"{cid}: z against the oracle in the order of {M.kernel_name(route['kernel'])}")


def _forms_matrix(letter, fmt, narrow):
    """Ragged rows: a band in front, scattered columns behind it, empty rows, rows long enough for the whole-wave tail."""
    g, w = M.group_rows(letter), M.WIDE[letter]
    rows = 3 * g + w + 1
    rng = np.random.default_rng(91)
    lens = rng.integers(0, 3 * M.wide_step(letter), rows)
    lens[::13] = 0
    lens[[5, g + 7, rows - 1]] = [300, 70, 41]
    rc = M.band(np.minimum(lens, M.wide_step(letter)))
    far = M.scattered(np.maximum(lens - M.wide_step(letter), 0), 3000, 92)
    rc = [a + [rows + 40 + e for e in b] for a, b in zip(rc, far)]
    kw = {}
    if narrow and w > 1:
        kw = dict(hack=3) if fmt == "hell" else dict(idx_pitch=rows, val_pitch=rows)       # 3 * g + w + 1 rows: no multiple of WIDE
    return M.build(letter, fmt, rc, rows + 3100, 1, seed=93, **kw)


@pytest.mark.parametrize("fmt", ["hell", "ell"])
@pytest.mark.parametrize("letter", M.LETTERS)
def test_same_bytes_through_every_form(gpu, letter, fmt):
    """include/spgpu/tuning.h: AUTO, GATHER, STRIPS and XTILE give the same bits (the order in which a row's products are added does
    not depend on the form), the caller's avgNnzPerRow changes none, and SWEEP gives them too for the 8-byte types; for fp32 and
    complex fp64 SWEEP is the one-phase order.  On a layout the wide kernels can read and on one they cannot."""
    from spgpu_amd import capi
    _start()
    for narrow in (False, True):
        m = _forms_matrix(letter, fmt, narrow)
        n = m["rows"]
        x, y = M.operands(letter, m)
        alpha, beta = (-0.75, 0.5) if letter in "SD" else (complex(-0.75, 0.5), complex(0.5, -0.25))
        dev = _device_matrix(letter, f"forms-{fmt}-{narrow}", m, M.NO_OFF)
        dx, dy = _place(x, 0)[1], _place(y, 0)[1]
        hack, vs, is_, mx = M.strides(m)
        addr = dict(cM=dev["cM"].data_ptr(), rP=dev["rP"].data_ptr(), z=0, y=0)
        outs = {}
        try:
            for name, form, avg in (("gather", M.GATHER, 0), ("strips", M.STRIPS, 0), ("xtile", M.XTILE, 0), ("auto", M.AUTO, 0),
                                    ("auto-hint", M.AUTO, 4), ("sweep", M.SWEEP, 0)):
                z_buf, dz = _place(np.full(n, SENTINEL, M.DTYPE[letter]), 0)
                capi.spgpuSetSpmvForm(gpu, form)
                _call(gpu, f"forms-{letter}-{fmt}-{name}", letter, m, dev, dz, dy, alpha, dx, beta, avg)
                outs[name] = _assert_margins(z_buf, 0, n, name)
        finally:
            capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
        first = M.dispatch(letter, fmt == "hell", M.GATHER, n, hack, vs, is_, mx, 0, addr, True)
        assert (first["kernel"][2] == 1) == (narrow or M.WIDE[letter] == 1)
        want = _oracle(m, x, y, alpha, beta, first["kernel"])
        for name in ("gather", "strips", "xtile", "auto", "auto-hint"):
            _same_bytes(outs[name], want, f"{letter} {fmt} narrow={narrow}: {name} against the gather kernel's order")
        swept = M.dispatch(letter, fmt == "hell", M.SWEEP, n, hack, vs, is_, mx, 0, addr, True)
        _same_bytes(outs["sweep"], _oracle(m, x, y, alpha, beta, swept["kernel"]), f"{letter} {fmt} narrow={narrow}: sweep")
        if letter in "DC" and swept["kernel"][0] == "sweep":
            _same_bytes(outs["sweep"], outs["gather"], f"{letter} {fmt}: SWEEP against GATHER")
        r, c, v = m["coo"]
        ref, scale = X.spmv(n, r, c, v, x, y, alpha, beta)
        for name, got in outs.items():
            X.assert_within(got, ref, scale, letter, case=f"{letter} {fmt} narrow={narrow} {name}")


@pytest.mark.parametrize("pattern", ["band", "window", "scattered"])
@pytest.mark.parametrize("letter", M.LETTERS)
def test_auto_first_call_and_later_call(gpu, letter, pattern):
    """AUTO on a matrix it has not seen runs the strip-capable kernel, whose sample wavefronts report; after a synchronisation the
    next call takes what they said: band -> STRIPS, window -> XTILE, scattered -> GATHER (complex fp64 has the narrow kernel only:
    GATHER at once).  The same bits on every call."""
    from spgpu_amd import capi
    _start()
    m, later = M.auto_patterns(letter)[pattern]
    n = m["rows"]
    x, y = M.operands(letter, m)
    dev = _device_matrix(letter, f"auto-{pattern}", m, M.NO_OFF)
    dx, dy = _place(x, 0)[1], _place(y, 0)[1]
    kernel = M.dispatch(letter, True, M.GATHER, n, 32, 32, 32, 0, 0, dict(cM=0, rP=0, z=0, y=0), True)["kernel"]
    want = _oracle(m, x, y, 1.5, -0.5, kernel)
    capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
    try:
        forms = []
        for call in range(3):
            z_buf, dz = _place(np.full(n, SENTINEL, M.DTYPE[letter]), 0)
            _call(gpu, f"auto-{letter}-{pattern}-{call}", letter, m, dev, dz, dy, 1.5, dx, -0.5, 0)       # (_guard synchronises)
            forms.append(capi.spgpuGetLastSpmvForm(gpu))
            _same_bytes(_assert_margins(z_buf, 0, n, "z"), want, f"{letter} {pattern}: call {call} in form {forms[-1]}")
    finally:
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
    first = M.STRIPS if M.WIDE[letter] > 1 else M.GATHER
    assert forms == [first, later, later], forms
