"""GPU: spgpu{S,D,C,Z}hellspmv / spgpu{S,D,C,Z}ellspmv on the path for rows ordered by length (rIdx given, or SPGPU_DEEP_SPLIT=1), on every
queue-kernel shape and branch of tests/ordered_launch_shapes.py's table (tests/test_ordered_launch_shapes.py proves on the CPU that the
table reaches all 56 raggedSpmvKernel instantiations and every listed branch).  Collected after every other test_gpu_* module, on a handle
of its own: the session handle's plans, AUTO words and deep lists are not touched.

Each case places its operands at the offsets it states with sentinels round z, runs with SPGPU_POISON_SCRATCH=1 under its own SPGPU_DEEP_CAP
/ SPGPU_DEEP_KEEP / SPGPU_RAGGED_SPLIT, and reaches its routes by public calls only: without a plan (SPGPU_PLAN=0: deep list, deep kernels
behind), from a plan (spgpu?SpmvPrepare) and from a frozen plan (spgpu?SpmvFreeze).  Per route it asserts what the handle reports
(spgpuGetLastSpmvForm, spgpuGetLastOrderedLaunch, the plan counters, spgpuSpmvFrozenBytes, no deep-list overflow or fallback), z within
exact_ref's bound of the extended-precision product, and z byte for byte the oracle's in the queue kernel's order of additions -- so the
three routes give the same bytes."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import ordered_launch_shapes as L
import spmv_launch_shapes as M
from test_gpu_fused_shapes import SENTINEL, _assert_margins, _guard, _place, _same_bytes, _start

pytestmark = pytest.mark.gpu

TABLE = {letter: L.cases(letter) for letter in L.LETTERS}
_DEVICE = {}        # the device matrices, kept for the module: plans and AUTO's words are keyed by the arrays' addresses


@pytest.fixture(scope="module")
def own():
    import torch
    from spgpu_amd import capi
    handle = capi.create_handle(0)
    yield handle
    torch.cuda.synchronize()
    capi.spgpuDestroy(handle)
    _DEVICE.clear()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _device_matrix(key, m, slots=None):
    import torch
    if key not in _DEVICE:
        pad = lambda a, fill: np.concatenate((a, np.full(max((slots or a.size) - a.size, 0), fill, a.dtype)))
        d = dict(cM=_place(pad(m["values"], M._nan(m["letter"])), 0)[1], rP=_place(pad(m["indices"], m["base"]), 0)[1],
                 rS=None if m["rs_null"] else torch.from_numpy(np.ascontiguousarray(m["row_lengths"])).to("cuda:0"),
                 rIdx=torch.from_numpy(np.ascontiguousarray(m["r_idx"])).to("cuda:0"))
        if m["fmt"] == "hell":
            d["hackOffsets"] = torch.from_numpy(np.ascontiguousarray(m["hack_offsets"])).to("cuda:0")
        _DEVICE[key] = d
    return _DEVICE[key]


def _matrix_args(m, dev, row_order):
    """The matrix part of Prepare's / Freeze's argument list behind (handle, type)."""
    r_idx = _p(dev["rIdx"]) if row_order else None
    if m["fmt"] == "hell":
        return (_p(dev["cM"]), _p(dev["rP"]), m["hack_size"], _p(dev["hackOffsets"]), _p(dev["rS"]), r_idx, m["rows"], m["base"])
    return (_p(dev["cM"]), _p(dev["rP"]), m["val_pitch"], m["pitch"], _p(dev["rS"]), r_idx, m["max_row"], m["rows"], m["base"])


def _spmv(handle, what, letter, m, dev, dz, dy, alpha, dx, beta, row_order):
    from spgpu_amd import capi
    r_idx = _p(dev["rIdx"]) if row_order else None
    if m["fmt"] == "hell":
        _guard(what, capi.hellspmv[letter], handle, _p(dz), _p(dy), capi.scalar(letter, alpha), _p(dev["cM"]), _p(dev["rP"]), m["hack_size"],
               _p(dev["hackOffsets"]), _p(dev["rS"]), r_idx, 0, m["rows"], _p(dx), capi.scalar(letter, beta), m["base"])
    else:
        _guard(what, capi.ellspmv[letter], handle, _p(dz), _p(dy), capi.scalar(letter, alpha), _p(dev["cM"]), _p(dev["rP"]), m["val_pitch"],
               m["pitch"], _p(dev["rS"]), r_idx, 0, m["max_row"], m["rows"], _p(dx), capi.scalar(letter, beta), m["base"])


def _knobs(tuning, case, plan):
    t = case["tune"]
    tuning(SPGPU_POISON_SCRATCH=1, SPGPU_DEEP_CAP=t["cap"], SPGPU_DEEP_KEEP=t["keep"], SPGPU_RAGGED_SPLIT=t["split"], SPGPU_RAGGED_SHAPE=case["knob"],
           SPGPU_PLAN=1 if plan else 0, SPGPU_FREEZE_MAX_ESCAPES_PCT=100, SPGPU_DEEP_SPLIT=-1 if case["row_order"] else 1)


def _nan_vector(letter, n):
    return np.full(n, complex(np.nan, np.nan) if letter in "CZ" else np.nan, M.DTYPE[letter])


def _run(handle, what, case, m, dev, x, y, row_order=True):
    """One SpMV of the case with fresh output buffers: z as the device left it (margins checked)."""
    letter, n, off = case["letter"], m["rows"], case["off"]
    alpha, beta = L.scalars_of(case)
    _, dx = _place(x, off["x"])
    y_dev = y if beta != 0 else _nan_vector(letter, n)                 # beta == 0: y is full of NaN and must not be read
    if case["y_mode"] == "z":
        z_buf, dz = _place(y_dev, off["z"])
        dy = dz
    else:
        z_buf, dz = _place(np.full(n, SENTINEL, M.DTYPE[letter]), off["z"])
        dy = _place(y_dev, off["y"])[1]
    _spmv(handle, what, letter, m, dev, dz, dy, alpha, dx, beta, row_order)
    return _assert_margins(z_buf, off["z"], n, f"{what}: z")


def _reference(case, m, x, y):
    alpha, beta = L.scalars_of(case)
    r, c, v = m["coo"]
    want, scale = X.spmv(m["rows"], r, c, v, x, y if beta != 0 else None, alpha, beta, r_idx=m["r_idx"] if case["row_order"] else None)
    return want, scale, L.oracle(m, x, y, alpha, beta, case["tune"], with_order=case["row_order"])


def _check_health(handle, before, what):
    from spgpu_amd import capi
    assert (capi.spgpuDeepListOverflows(handle), capi.spgpuDeepListFallbacks(handle)) == before, f"{what}: a deep list overflowed or was missing"


@pytest.mark.parametrize("letter,cid", [pytest.param(letter, cid, id=f"{letter}-{cid}") for letter in L.LETTERS for cid in TABLE[letter]])
def test_ordered_case(own, tuning, letter, cid):
    import torch
    from spgpu_amd import capi
    _start()
    case = TABLE[letter][cid]
    m = L.matrix_of(case)
    x, y = L.operands(letter, m)
    dev = _device_matrix((letter, cid), m)
    assert M.wide_layout(letter, m["fmt"] == "hell", m["rows"], m.get("hack_size", 0), m.get("val_pitch", 0), m.get("pitch", 0),
                         dev["cM"].data_ptr(), dev["rP"].data_ptr())[0], "the layout would take the narrow kernels"
    want, scale, bits = _reference(case, m, x, y)
    code = capi.TYPE_CODE[letter]
    prepare, freeze = (capi.spgpuHellSpmvPrepare, capi.spgpuHellSpmvFreeze) if m["fmt"] == "hell" else (capi.spgpuEllSpmvPrepare, capi.spgpuEllSpmvFreeze)
    health = (capi.spgpuDeepListOverflows(own), capi.spgpuDeepListFallbacks(own))
    capi.spgpuSetSpmvForm(own, case["form"])
    outs = {}
    try:
        for mode in case["modes"]:
            what = f"{letter}-{cid}-{mode}"
            route = L.case_route(case, mode, m)
            assert route["shape"] == case["shape"]
            _knobs(tuning, case, plan=mode != "list")
            counts, frozen = capi.plan_counts(own), capi.spgpuSpmvFrozenBytes(own)
            if mode == "plan":
                assert prepare(own, code, *_matrix_args(m, dev, True)) == capi.SPGPU_SUCCESS, what
            elif mode == "packed":
                assert freeze(own, code, *_matrix_args(m, dev, True)) == capi.SPGPU_SUCCESS, what
                assert capi.spgpuSpmvFrozenBytes(own) >= frozen + 2 * m["indices"].size, what
            torch.cuda.synchronize()
            uses = capi.plan_counts(own)[0]
            outs[mode] = _run(own, what, case, m, dev, x, y, case["row_order"])
            assert capi.spgpuGetLastSpmvForm(own) == route["noted"], what
            assert capi.spgpuGetLastOrderedLaunch(own) == route["word"], (what, hex(capi.spgpuGetLastOrderedLaunch(own)), hex(route["word"]))
            after = capi.plan_counts(own)
            assert after[0] == uses + (1 if route["plan"] else 0), (what, counts, after)
            assert after[2] == counts[2], f"{what}: a plan of the matrix itself was found stale"
            if mode == "list":
                assert after == counts, (what, counts, after)
            X.assert_within(outs[mode], want, scale, letter, case=what)
            _same_bytes(outs[mode], bits, f"{what}: z against the oracle in the queue kernel's order")
            _check_health(own, health, what)
        for mode in case["modes"][1:]:
            _same_bytes(outs[mode], outs[case["modes"][0]], f"{letter}-{cid}: {mode} against {case['modes'][0]}")
    finally:
        if "packed" in outs or "packed" in case["modes"]:
            capi.spgpuSpmvThaw(own, _p(dev["rP"]))
        capi.spgpuSetSpmvForm(own, capi.FORM_AUTO)


@pytest.mark.parametrize("letter,cid", [pytest.param(letter, cid, id=f"{letter}-{cid}") for letter in L.LETTERS for cid in L.stale_pairs(letter)])
def test_stale_plan_case(own, tuning, letter, cid):
    """Matrix A is planned; B is copied over the same arrays.  The next call runs from A's plan: B's deep sub-groups are worked off behind
    their blocks' streams (nine in one block: two batches), the one A's plan lists is shallow now.  B's product in the oracle's bits, the
    report, and a new analysis with the call after."""
    import torch
    from spgpu_amd import capi
    _start()
    case, a_depths, b_depths = L.stale_case(letter, cid)
    a, b = L.matrix_of(case, a_depths, "A"), L.matrix_of(case, b_depths, "B")
    slots = max(a["values"].size, b["values"].size)
    dev = _device_matrix((letter, cid), a, slots)
    other = _device_matrix((letter, cid, "B"), b, slots)
    x, y = L.operands(letter, a if a["cols"] > b["cols"] else b)                     # x long enough for both
    assert a["rows"] == b["rows"]
    _knobs(tuning, case, plan=True)
    capi.spgpuSetSpmvForm(own, case["form"])
    try:
        code = capi.TYPE_CODE[letter]
        assert capi.spgpuHellSpmvPrepare(own, code, *_matrix_args(a, dev, True)) == capi.SPGPU_SUCCESS
        want_a = _reference(case, a, x, y)
        got = _run(own, f"{letter}-{cid}-A", case, a, dev, x, y)
        _same_bytes(got, want_a[2], f"{letter}-{cid}: A from its plan")
        uses, builds, stales = capi.plan_counts(own)
        for name in ("cM", "rP", "hackOffsets", "rS", "rIdx"):
            dev[name].copy_(other[name])
        torch.cuda.synchronize()
        route = L.case_route(case, "plan", b, plan_of=a)
        names = L.walk(b, route, case["tune"], plan_of=a)
        assert {"stale_listed_but_shallow", "stale_deep_but_unlisted", "behind_more_than_8", "behind_1_to_8"} <= names
        want, scale, bits = _reference(case, b, x, y)
        got = _run(own, f"{letter}-{cid}-B-stale", case, b, dev, x, y)
        assert capi.plan_counts(own)[0] == uses + 1 and capi.spgpuGetLastOrderedLaunch(own) == route["word"]
        X.assert_within(got, want, scale, letter, case=f"{letter}-{cid} stale")
        _same_bytes(got, bits, f"{letter}-{cid}: B from A's plan")
        got = _run(own, f"{letter}-{cid}-B-noticed", case, b, dev, x, y)             # the host has read the kernels' report
        _same_bytes(got, bits, f"{letter}-{cid}: B while its own analysis runs")
        after = capi.plan_counts(own)
        assert after[2] == stales + 1 and after[1] == builds + 1, (after, (uses, builds, stales))
        assert capi.spgpuHellSpmvPrepare(own, code, *_matrix_args(b, dev, True)) == capi.SPGPU_SUCCESS
        got = _run(own, f"{letter}-{cid}-B-planned", case, b, dev, x, y)
        _same_bytes(got, bits, f"{letter}-{cid}: B from its own plan")
        assert capi.plan_counts(own)[2] == stales + 1
    finally:
        capi.spgpuSetSpmvForm(own, capi.FORM_AUTO)


def test_last_ordered_launch_is_zero_for_rows_as_they_come(own):
    """spgpuGetLastOrderedLaunch after a call without a row order (default knobs): that call took the dispatch for rows as they come."""
    from spgpu_amd import capi
    _start()
    case = TABLE["D"]["queue-hell-gather"]
    m = L.matrix_of(case)
    x, y = L.operands("D", m)
    dev = _device_matrix(("D", "queue-hell-gather"), m)
    _run(own, "rows-as-they-come", case, m, dev, x, y, row_order=False)
    assert capi.spgpuGetLastOrderedLaunch(own) == 0
