"""GPU: FROZEN ELL / HELL matrices without a row order (spgpu?SpmvFreeze with rIdx == NULL) on every kernel shape and branch: freezeSlab,
slabPackKernel, slabSlotsKernel and findFrozenSlab (spgpu_amd/csrc/frozen_slab.hip.h) and the twelve slabSpmvKernel<..., PACKED = true>
instantiations (slab_spmv.hip.h).  The case table, the freeze restated on the host and the walk of the packed kernels are
tests/frozen_launch_shapes.py; tests/test_frozen_launch_shapes.py checks on the CPU that the table reaches every instantiation and branch.

Every test runs with SPGPU_POISON_SCRATCH=1 (the words of the copy slabPackKernel does not write read 0xA5A5) and
SPGPU_FREEZE_MAX_ESCAPES_PCT=100 (every matrix of the table freezes; the share rule at its default is test_gpu_packed_edges.py's).

Each case
  * places its operands as it says, sentinels on both sides of z, and is called unfrozen: the bytes of the oracle adding in the order of the
    route's kernel (oracle_api.spmv_tail), within exact_ref's bound of the extended-precision product;
  * is frozen: SPGPU_SUCCESS (SPGPU_UNSUPPORTED for exactly the cases the CPU module lists), spgpuSpmvFrozenBytes grows by the restated slot
    count's bytes (the handle counts the copy, rounded to 256 bytes; the groups' bases are not counted), a second Freeze makes no second copy;
  * is called frozen twice: the use counter advances by one per call, the form reported stays, z has the bytes of the unfrozen call;
  * is thawed: the bytes are back, one more call leaves the counter alone.
The matrices' padding slots, the rows past the last one and the entries below the index base hold NaN.  The plan table has 8 records: no
case stays frozen.

Collected after every other test_gpu_* module (hence the name): the cases freeze and thaw on the session's handle, whose plan table has 8
records with the least recently used evicted, so every module in front of this one finds the handle's records, counters and AUTO words
as it did before this module existed; and the device matrices of the inherited cases are those tests/test_gpu_spmv_shapes.py has already
placed (its _DEVICE), not a second copy."""

import numpy as np
import pytest

import exact_ref as X
import frozen_launch_shapes as F
import spmv_launch_shapes as M
from test_gpu_fused_shapes import _RAISED, SENTINEL, _assert_margins, _place, _same_bytes, _start
from test_gpu_spmv_shapes import _call, _device_matrix, _nan_vector, _oracle, _p

pytestmark = pytest.mark.gpu

TABLE = {L: F.cases(L) for L in F.LETTERS}
KNOBS = dict(SPGPU_POISON_SCRATCH=1, SPGPU_FREEZE_MAX_ESCAPES_PCT=100)
REFUSED = F.REFUSED


def _said(cid, fn, *args):
    """One library call that answers, then a synchronisation; whatever either raises stops every later case."""
    import torch
    try:
        out = fn(*args)
        torch.cuda.synchronize()
        return out
    except BaseException:
        _RAISED.append(cid)
        raise


def _freeze(gpu, cid, letter, m, dev, cM=None, **other):
    """spgpu?SpmvFreeze on the matrix' arrays; `other`: arguments that differ from the matrix' own."""
    from spgpu_amd import capi
    a = dict(cM=_p(cM if cM is not None else dev["cM"]), rP=_p(dev["rP"]), rS=_p(dev["rS"]), rows=m["rows"], base=m["base"])
    if m["fmt"] == "hell":
        a.update(hack=m["hack_size"], offsets=_p(dev["hackOffsets"]))
        a.update(other)
        return _said(cid, capi.spgpuHellSpmvFreeze, gpu, capi.TYPE_CODE[letter], a["cM"], a["rP"], a["hack"], a["offsets"], a["rS"], None, a["rows"], a["base"])
    a.update(val_pitch=m["val_pitch"], pitch=m["pitch"], max_row=m["max_row"])
    a.update(other)
    return _said(cid, capi.spgpuEllSpmvFreeze, gpu, capi.TYPE_CODE[letter], a["cM"], a["rP"], a["val_pitch"], a["pitch"], a["rS"], None, a["max_row"],
                 a["rows"], a["base"])


def _thaw(gpu, dev):
    from spgpu_amd import capi
    return capi.spgpuSpmvThaw(gpu, _p(dev["rP"]))


class _Operands:
    """x, y and a fresh z per call, placed as a case says."""

    def __init__(self, letter, m, off, y_mode, beta):
        self.letter, self.n, self.off, self.y_mode = letter, m["rows"], off, y_mode
        self.x, self.y = M.operands(letter, m)
        self.dx = _place(self.x, off["x"])[1]
        self.y_dev = self.y if beta != 0 else _nan_vector(letter, self.n)          # beta == 0: y is full of NaN and must not be read
        self.dy = None if y_mode == "z" else _place(self.y_dev, off["y"])[1]
        self.fresh()

    def fresh(self):
        if self.y_mode == "z":
            self.z_buf, self.dz = _place(self.y_dev, self.off["z"])
            self.dy = self.dz
        else:
            self.z_buf, self.dz = _place(np.full(self.n, SENTINEL, M.DTYPE[self.letter]), self.off["z"])

    def z(self, what):
        return _assert_margins(self.z_buf, self.off["z"], self.n, what)


def _run(gpu, cid, letter, m, dev, ops, alpha, beta, avg=0):
    """One SpMV into a fresh z: (z, by how much the use counter advanced, the form reported)."""
    from spgpu_amd import capi
    ops.fresh()
    uses = capi.plan_counts(gpu)[0]
    _call(gpu, cid, letter, m, dev, ops.dz, ops.dy, alpha, ops.dx, beta, avg)
    return ops.z(f"{cid}: z"), capi.plan_counts(gpu)[0] - uses, capi.spgpuGetLastSpmvForm(gpu)


@pytest.mark.parametrize("letter,cid", [pytest.param(L, cid, id=f"{L}-{cid}") for L in F.LETTERS for cid in TABLE[L]])
def test_frozen_case(gpu, tuning, letter, cid):
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    case = TABLE[letter][cid]
    m = M.matrix_of(case)
    n, off = m["rows"], case["off"]
    alpha, beta = M.scalars_of(case)
    dev = _device_matrix(letter, cid, m, off)
    ops = _Operands(letter, m, off, case["y_mode"], beta)
    # the route, from the addresses the call is made with
    addr = dict(cM=dev["cM"].data_ptr(), rP=dev["rP"].data_ptr(), z=ops.dz.data_ptr(), y=ops.dy.data_ptr())
    route, planned = M.case_dispatch(case, addr=addr), M.case_dispatch(case)
    assert (route["kernel"], route["wide_io"]) == (planned["kernel"], planned["wide_io"]), f"{cid}: the allocator moved an operand"
    assert route["kernel"] == M.route_kernel(letter, case["route"], m["fmt"] == "hell") and F.is_wide(route["kernel"])
    _, _, entries, escapes, slots = F.pack_of(case)
    hack, vs, is_, _ = M.strides(m)
    expected = F.can_freeze(letter, m["fmt"] == "hell", case["form"], n, hack, vs, is_, addr, slots, entries, escapes, pct=100)
    assert expected == ((False, "slots") if cid in REFUSED else (True, None)), (cid, expected)
    r, c, v = m["coo"]
    want, scale = X.spmv(n, r, c, v, ops.x, ops.y if beta != 0 else None, alpha, beta)
    oracle = _oracle(m, ops.x, ops.y, alpha, beta, route["kernel"])
    before = capi.spgpuSpmvFrozenBytes(gpu)
    capi.spgpuSetSpmvForm(gpu, case["form"])
    try:
        unfrozen, used, noted = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
        assert (used, noted) == (0, route["noted"]), (used, noted)
        X.assert_within(unfrozen, want, scale, letter, case=f"{cid} unfrozen")
        _same_bytes(unfrozen, oracle, f"{cid}: unfrozen against the oracle in the order of {M.kernel_name(route['kernel'])}")
        said = _freeze(gpu, cid, letter, m, dev)
        if cid in REFUSED:
            assert said == capi.SPGPU_UNSUPPORTED and capi.spgpuSpmvFrozenBytes(gpu) == before
        else:
            assert said == capi.SPGPU_SUCCESS, said
            assert capi.spgpuSpmvFrozenBytes(gpu) - before == F.packed_bytes(slots), (capi.spgpuSpmvFrozenBytes(gpu) - before, slots)
            assert _freeze(gpu, cid, letter, m, dev) == capi.SPGPU_SUCCESS                 # frozen already: no second copy
            assert capi.spgpuSpmvFrozenBytes(gpu) - before == F.packed_bytes(slots)
        for call in range(2):
            got, used, noted = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
            assert (used, noted) == (0 if cid in REFUSED else 1, route["noted"]), (call, used, noted)
            _same_bytes(got, unfrozen, f"{cid}: frozen call {call} against the unfrozen call")
            _same_bytes(got, oracle, f"{cid}: frozen call {call} against the oracle")
            X.assert_within(got, want, scale, letter, case=f"{cid} frozen call {call}")
        assert _thaw(gpu, dev) == (capi.SPGPU_UNSUPPORTED if cid in REFUSED else capi.SPGPU_SUCCESS)
        assert capi.spgpuSpmvFrozenBytes(gpu) == before
        got, used, noted = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
        assert (used, noted) == (0, route["noted"]), (used, noted)
        _same_bytes(got, unfrozen, f"{cid}: thawed against the unfrozen call")
    finally:
        _thaw(gpu, dev)
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


# ---- the copy is what is read -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["gather", "strips"])
@pytest.mark.parametrize("fmt", ["hell", "ell"])
@pytest.mark.parametrize("letter", F.LETTERS)
def test_the_copy_is_what_is_read(gpu, tuning, letter, fmt, route):
    """After the Freeze the caller's rP is overwritten on the device, at exactly the slots the walk says the packed kernel takes from its
    copy, with the NEXT column of x (wrapped): the frozen call's bytes do not change.  This deliberately breaks the caller's promise that
    the index arrays stay as they are, in the one way the kernel's own comment (slab_spmv.hip.h, PACKED) says is harmless: the stage loads
    read the copy, and only the rare paths -- whole-wave tail rows, an escape, the sample wavefronts' span under AUTO -- read rP.  Every
    replacement column is a valid column of x, so a kernel that does read rP there gives other numbers and never a bad address.  First a
    matrix without a tail row and without an escape (rows a multiple of the group; GATHER on scattered columns, STRIPS on a band; a fixed
    form, so no wavefront samples a span): nothing of rP is read.  Then one with a tail row and an escape: everything but those slots is
    overwritten.  Thawed with the overwritten rP still in place, the unfrozen call gives other bytes (the overwrite is no no-op); then
    rP is restored."""
    import torch
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    form = M.GATHER if route == "gather" else M.STRIPS
    for both in (False, True):
        cid = f"copy-is-read-{letter}-{fmt}-{route}-{both}"
        m = F.copy_is_read_matrix(letter, fmt, route, both)
        kernel = M.route_kernel(letter, route, fmt == "hell")
        n = F.walk(m, F.packed(kernel), 1)
        rows, cols, slots = F.all_entries(m)
        from_copy = sorted(n["word_slots"] - n["rp_reads"])
        assert (set(from_copy) == set(slots.tolist())) == (not both) and len(from_copy) >= slots.size - 41
        dev = _device_matrix(letter, cid, m, M.NO_OFF)
        ops = _Operands(letter, m, M.NO_OFF, "y", 0.5)
        alpha, beta = (-0.75, 0.5) if letter in "SD" else (complex(-0.75, 0.5), complex(0.5, -0.25))
        oracle = _oracle(m, ops.x, ops.y, alpha, beta, kernel)
        at = torch.from_numpy(np.asarray(from_copy, np.int64)).to("cuda:0")
        kept = dev["rP"].clone()
        moved = m["indices"].copy()
        moved[from_copy] = (moved[from_copy] - m["base"] + 1) % m["cols"] + m["base"]
        capi.spgpuSetSpmvForm(gpu, form)
        try:
            assert _freeze(gpu, cid, letter, m, dev) == capi.SPGPU_SUCCESS
            got, used, _ = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
            assert used == 1
            _same_bytes(got, oracle, f"{cid}: frozen")
            dev["rP"][at] = torch.from_numpy(moved[from_copy]).to("cuda:0")
            torch.cuda.synchronize()
            got, used, _ = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
            assert used == 1
            _same_bytes(got, oracle, f"{cid}: frozen, rP overwritten where the copy is read")
            assert _thaw(gpu, dev) == capi.SPGPU_SUCCESS
            got, used, _ = _run(gpu, cid, letter, m, dev, ops, alpha, beta)
            assert used == 0
            _same_bytes(got, _oracle(dict(m, indices=moved), ops.x, ops.y, alpha, beta, kernel), f"{cid}: thawed, on the overwritten rP")
            assert got.tobytes() != oracle.tobytes()
        finally:
            dev["rP"].copy_(kept)
            torch.cuda.synchronize()
            _thaw(gpu, dev)
            capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


# ---- a record that is there and not used ---------------------------------------------------------------------------------------------------
def _key_matrix(fmt):
    """fp64, index base 1, no entry below it, rows of 11 scattered columns (more than a stage)."""
    G = M.group_rows("D")
    lens = M._lens_fill(2 * G + 3, 11)
    return M.build("D", fmt, M.scattered(lens, 3000, 51), 3000, 1, seed=51)


def test_a_record_is_not_used_by_another_route(gpu, tuning):
    """A frozen fp64 matrix called with avgNnzPerRow = 4 under AUTO (the lean kernel), under XTILE and under SWEEP: launchRowsAsTheyCome
    looks the record up in front of the Wide kernel only.  The use counter stays; the bytes are the oracle's in the order of the route's kernel."""
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    m = _key_matrix("hell")
    dev = _device_matrix("D", "key-hell", m, M.NO_OFF)
    ops = _Operands("D", m, M.NO_OFF, "y", 0.5)
    capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
    try:
        assert _freeze(gpu, "key-hell", "D", m, dev) == capi.SPGPU_SUCCESS
        frozen, used, _ = _run(gpu, "key-hell", "D", m, dev, ops, -0.75, 0.5)
        assert used == 1
        _same_bytes(frozen, _oracle(m, ops.x, ops.y, -0.75, 0.5, M.route_kernel("D", "gather", True)), "frozen")
        for route, form, avg in (("lean", M.AUTO, 4), ("tiled", M.XTILE, 0), ("sweep", M.SWEEP, 0)):
            kernel = M.route_kernel("D", route, True)
            assert not F.record_used(kernel, {}, {})
            capi.spgpuSetSpmvForm(gpu, form)
            got, used, noted = _run(gpu, f"key-hell-{route}", "D", m, dev, ops, -0.75, 0.5, avg=avg)
            assert (used, noted) == (0, {"lean": M.GATHER, "tiled": M.XTILE, "sweep": M.SWEEP}[route]), (route, used, noted)
            _same_bytes(got, _oracle(m, ops.x, ops.y, -0.75, 0.5, kernel), f"frozen matrix through {route}")
        capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
        assert _run(gpu, "key-hell", "D", m, dev, ops, -0.75, 0.5)[1] == 1         # ... and is still there for the call it was made for
    finally:
        _thaw(gpu, dev)
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


def _host_call(m, **other):
    """The host matrix a call with other arguments multiplies by (fewer rows, another index base)."""
    out = dict(m, **other)
    n = out["rows"]
    r, c, v = m["coo"]
    keep = r < n
    out.update(row_lengths=m["row_lengths"][:n], coo=(r[keep], c[keep] + (m["base"] - out["base"]), v[keep]), cols=m["cols"] + (m["base"] - out["base"]))
    return out


@pytest.mark.parametrize("fmt", ["hell", "ell"])
def test_a_record_is_found_by_its_key_alone(gpu, tuning, fmt):
    """planKey (slab_args.hip.h) as frozen_launch_shapes.KEY_FIELDS restates it: a call with one of rP, rS, hackOffsets, rows, baseIndex
    (HELL; hackSize and idxStride below) or maxNnz (ELL) changed is another matrix on the same arrays -- the record is not used, the bytes
    are the unpacked gather kernel's for that call.  cM is not in the key: the same indices under other coefficients read the copy."""
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    hell = fmt == "hell"
    m = _key_matrix(fmt)
    cid = f"key-{fmt}"
    dev = _device_matrix("D", cid, m, M.NO_OFF)
    kernel = M.route_kernel("D", "gather", hell)
    n = m["rows"]
    hack, _, is_, mx = M.strides(m)
    frozen_key = F.lookup_key("D", hell, dev["rP"].data_ptr(), dev["rS"].data_ptr(), dev["hackOffsets"].data_ptr() if hell else None, hack, is_, mx, n, 1)
    others = {
        "rP": (dict(rP=dev["rP"].clone()), {}),
        "rS": (dict(rS=dev["rS"].clone()), {}),
        "rows": ({}, dict(rows=n - 1)),
        "baseIndex": ({}, dict(base=0)),
    }
    if hell:
        others["hackOffsets"] = (dict(hackOffsets=dev["hackOffsets"].clone()), {})
    else:
        others["maxNnz"] = ({}, dict(max_row=mx + 1))          # (with rS given no kernel reads maxNnz: the same product)
    capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
    try:
        assert _freeze(gpu, cid, "D", m, dev) == capi.SPGPU_SUCCESS
        ops = _Operands("D", m, M.NO_OFF, "y", 0.5)
        frozen, used, _ = _run(gpu, cid, "D", m, dev, ops, -0.75, 0.5)
        assert used == 1
        _same_bytes(frozen, _oracle(m, ops.x, ops.y, -0.75, 0.5, kernel), "frozen")
        for field, (arrays, numbers) in others.items():
            host = _host_call(m, **numbers)
            dev2 = dict(dev, **arrays)
            key = F.lookup_key("D", hell, dev2["rP"].data_ptr(), dev2["rS"].data_ptr(), dev2["hackOffsets"].data_ptr() if hell else None, hack, is_,
                               host.get("max_row", 0), host["rows"], host["base"])
            assert [f for f in F.KEY_FIELDS if key[f] != frozen_key[f]] == [field] and not F.record_used(kernel, key, frozen_key)
            ops2 = _Operands("D", host, M.NO_OFF, "y", 0.5)
            got, used, _ = _run(gpu, f"{cid}-{field}", "D", host, dev2, ops2, -0.75, 0.5)
            assert used == 0, field
            _same_bytes(got, _oracle(host, ops2.x, ops2.y, -0.75, 0.5, kernel), f"{cid}: {field} changed")
            r, c, v = host["coo"]
            want, scale = X.spmv(host["rows"], r, c, v, ops2.x, ops2.y, -0.75, 0.5)
            X.assert_within(got, want, scale, "D", case=f"{cid} {field}")
        # other coefficients under the same indices: the key is the same, the copy is read
        twice = dict(m, values=m["values"] * 2, coo=(m["coo"][0], m["coo"][1], m["coo"][2] * 2))
        dev2 = dict(dev, cM=_place(twice["values"], 0)[1])
        got, used, _ = _run(gpu, f"{cid}-cM", "D", twice, dev2, ops, -0.75, 0.5)
        assert used == 1 and F.record_used(kernel, dict(frozen_key), frozen_key)
        _same_bytes(got, _oracle(twice, ops.x, ops.y, -0.75, 0.5, kernel), f"{cid}: other coefficients")
    finally:
        _thaw(gpu, dev)
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


def test_a_record_is_keyed_by_the_pitch_and_the_hack_size(gpu, tuning):
    """idxStride (ELL) and hackSize (HELL, where it is the stride too): a matrix of one column per row reads the same slots under any pitch,
    and one of a single hack under any hack size that holds its rows -- the same product, another key, no use of the record."""
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    rc = [[(7 * i) % 50] for i in range(20)]
    for fmt, frozen_as, called_as in (("ell", dict(idx_pitch=24, val_pitch=24), dict(pitch=20)), ("hell", dict(hack=64), dict(hack_size=32))):
        m = M.build("D", fmt, rc, 50, 0, seed=61, **frozen_as)
        cid = f"key-stride-{fmt}"
        dev = _device_matrix("D", cid, m, M.NO_OFF)
        kernel = M.route_kernel("D", "gather", fmt == "hell")
        ops = _Operands("D", m, M.NO_OFF, "y", 0.5)
        other = dict(m, **called_as)
        assert M.wide_layout("D", fmt == "hell", 20, *M.strides(other)[:3], 0, 0)[0]
        capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
        try:
            assert _freeze(gpu, cid, "D", m, dev) == capi.SPGPU_SUCCESS
            want = _oracle(m, ops.x, ops.y, -0.75, 0.5, kernel)
            got, used, _ = _run(gpu, cid, "D", m, dev, ops, -0.75, 0.5)
            assert used == 1
            _same_bytes(got, want, f"{cid}: frozen")
            got, used, _ = _run(gpu, cid + "-other", "D", other, dev, ops, -0.75, 0.5)
            assert used == 0
            _same_bytes(got, want, f"{cid}: the other stride")
        finally:
            _thaw(gpu, dev)
            capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


# ---- Freeze refused -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["hell", "ell"])
@pytest.mark.parametrize("letter", F.LETTERS)
def test_freeze_refused(gpu, tuning, letter, fmt):
    """SPGPU_UNSUPPORTED, nothing kept, and the next call runs unfrozen: a Freeze while the handle's form is XTILE or SWEEP (those forms never
    read a copy), and a layout the wide kernels cannot read -- cM 8 bytes off its boundary, a HELL hack size that is no multiple of WIDE.
    (Complex fp64: test_gpu_freeze.py::test_calls_without_a_packed_form_say_so.)"""
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    G, w = M.group_rows(letter), M.WIDE[letter]
    lens = M._lens_fill(G + w + 1, M.wide_step(letter) + 2)
    plain = M.build(letter, fmt, M.scattered(lens, 2000, 71), 2000, 0, seed=71)
    layouts = [("xtile", plain, M.NO_OFF, M.XTILE), ("sweep", plain, M.NO_OFF, M.SWEEP), ("cM-off", plain, dict(M.NO_OFF, cM=8 // M.SIZEOF[letter]), M.GATHER)]
    if fmt == "hell":
        layouts.append(("hack-odd", M.build(letter, fmt, M.scattered(lens, 2000, 72), 2000, 0, seed=72, hack=w + 1), M.NO_OFF, M.GATHER))
    before = capi.spgpuSpmvFrozenBytes(gpu)
    for name, m, off, form in layouts:
        cid = f"refused-{fmt}-{name}"
        dev = _device_matrix(letter, cid if off is not M.NO_OFF or m is not plain else f"refused-{fmt}-plain", m, off)
        hack, vs, is_, _ = M.strides(m)
        addr = dict(cM=dev["cM"].data_ptr(), rP=dev["rP"].data_ptr())
        _, _, entries, escapes, slots = F.pack(m, letter)
        ok, why = F.can_freeze(letter, fmt == "hell", form, m["rows"], hack, vs, is_, addr, slots, entries, escapes, pct=100)
        assert not ok and why == {"xtile": "form", "sweep": "form", "cM-off": "layout:cM", "hack-odd": "layout:hack"}[name]
        assert F.can_freeze(letter, fmt == "hell", M.GATHER, m["rows"], hack, vs, is_, addr, slots, entries, escapes, pct=100)[0] == (form != M.GATHER)
        ops = _Operands(letter, m, M.NO_OFF, "y", 0.5)
        capi.spgpuSetSpmvForm(gpu, form)
        try:
            assert _freeze(gpu, cid, letter, m, dev) == capi.SPGPU_UNSUPPORTED, name
            assert capi.spgpuSpmvFrozenBytes(gpu) == before
            capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
            got, used, _ = _run(gpu, cid, letter, m, dev, ops, 1.5, -0.5)
            assert used == 0, name
            route = M.dispatch(letter, fmt == "hell", M.GATHER, m["rows"], hack, vs, is_, m.get("max_row", 0), 0, dict(addr, z=0, y=0), True)
            _same_bytes(got, _oracle(m, ops.x, ops.y, 1.5, -0.5, route["kernel"]), cid)
        finally:
            _thaw(gpu, dev)
            capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)


# ---- AUTO on a frozen matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["band", "window", "scattered"])
@pytest.mark.parametrize("letter", F.LETTERS)
def test_auto_on_a_frozen_matrix(gpu, tuning, letter, pattern):
    """Frozen before its first call, a matrix goes through the forms test_auto_first_call_and_later_call expects of an unfrozen one -- STRIPS
    on the new matrix (the packed strip kernel's sample wavefronts report), then band -> STRIPS, window -> XTILE, scattered -> GATHER -- with
    the same bytes on every call; the record is used by the calls that run STRIPS or GATHER and not by those that run XTILE."""
    from spgpu_amd import capi
    _start()
    tuning(**KNOBS)
    m, later = M.auto_patterns(letter)[pattern]
    cid = f"frozen-auto-{pattern}"
    dev = _device_matrix(letter, cid, m, M.NO_OFF)                 # (its own arrays: AUTO keeps what it learnt by rP and rows)
    ops = _Operands(letter, m, M.NO_OFF, "y", -0.5)
    want = _oracle(m, ops.x, ops.y, 1.5, -0.5, M.route_kernel(letter, "gather", True))
    capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
    try:
        assert _freeze(gpu, cid, letter, m, dev) == capi.SPGPU_SUCCESS
        forms, uses = [], []
        for call in range(3):
            got, used, noted = _run(gpu, f"{cid}-{call}", letter, m, dev, ops, 1.5, -0.5)          # (_call synchronises: the samples have landed)
            forms.append(noted)
            uses.append(used)
            _same_bytes(got, want, f"{letter} {pattern}: frozen call {call} in form {noted}")
        assert forms == [M.STRIPS, later, later], forms
        assert uses == [0 if form == M.XTILE else 1 for form in forms], (forms, uses)
    finally:
        _thaw(gpu, dev)
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
