"""GPU: HOLDS (include/spgpu/ext/graph.h spgpuSpmvHold / spgpuSpmvRelease / spgpuSpmvHolds).

A launch captured into a HIP graph keeps the device addresses it was captured with, so by default it uses none of a matrix'
records (plan, frozen copy, adopted copy): a graph outlives a Thaw.  Under a hold the records are never freed while the caller
says a graph may replay, and captured launches use them.  Pinned here: a held capture runs on the record -- counted once, at
capture -- and every replay has the bits of the eager call on the same record and stays within the bound of exact sums; without
a hold nothing changes; Thaw is refused under a hold and works after the last Release; held records are never evicted; a CG
captured on an adopted ragged matrix repeats the eager run bit for bit; the plain-C tool does the same.  Every test releases and
thaws what it held (in a finally): a record left held would change the eviction tests of other files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _adopted_uses(gpu):
    from spgpu_amd import capi
    return capi.spgpuSpmvAdoptedUses(gpu)


def _plan_uses(gpu):
    from spgpu_amd import capi
    return capi.plan_counts(gpu)[0]


def _ragged_coo(n, letter, pattern, near, longest, mean, seed):
    import torch
    from spgpu_amd import synth
    real = {"S": "S", "D": "D", "C": "S", "Z": "D"}[letter]
    lengths = np.minimum(synth.power_law_lengths(n, mean, longest, seed + 2), longest)
    rows_t, cols_t, vals_t = synth.ragged_coo_on_device(lengths, n, pattern, near, real, seed=seed)
    if letter in "CZ":
        vals_t = torch.complex(vals_t, torch.flip(vals_t, [0]))
    return rows_t, cols_t, vals_t


def _hell_host(h, letter, n, hack):
    return dict(letter=letter, rows=n, values=h["cM"][:h["slots"]].cpu().numpy(), indices=h["rP"][:h["slots"]].cpu().numpy(),
                hack_offsets=h["hack_offsets"].cpu().numpy(), hack_size=hack, row_lengths=h["rS"][:n].cpu().numpy(), base=0)


class Case:
    """One matrix with a record: `spmv(dz, dy, dx, alpha, beta)` is the SpMV call on the caller's arrays, `key` the rP a hold
    names, `uses` the counter a launch on the record raises, `exact(x, y, alpha, beta)` the sums of tests/exact_ref.py and
    `unheld(x, y, alpha, beta)` the bits a capture without a hold gives (tests/oracle_api.py)."""


def _case(gpu, kind):
    import torch
    from spgpu_amd import capi, formats, synth
    c = Case()
    c.letter = kind.split("_")[-1] if kind.startswith("adopted") else "D"
    letter = c.letter
    code = capi.TYPE_CODE[letter]
    if kind in ("planned", "frozen"):
        n, hack = 9 * 2048 + 77, 32
        c.n = n
        coo = _ragged_coo(n, letter, "near", 500, 900, 12.0, 7)
        h = formats.coo_to_ordered_hell_device(gpu, n, *coo, letter, hack, 2048, 60, aligned=True)
        sub, r_idx = _hell_host(h, letter, n, hack), h["rIdx"].cpu().numpy()
        c.mat = h
        c.key = h["rP"]
        c.uses = _plan_uses

        def spmv(dz, dy, dx, alpha, beta):
            capi.hellspmv[letter](gpu, _dp(dz), _dp(dy) if beta != 0 else None, capi.scalar(letter, alpha), _dp(h["cM"]), _dp(h["rP"]), hack,
                                  _dp(h["hack_offsets"]), _dp(h["rS"]), _dp(h["rIdx"]), 12, n, _dp(dx), capi.scalar(letter, beta), 0)
        c.spmv = spmv
        args = (gpu, code, _dp(h["cM"]), _dp(h["rP"]), hack, _dp(h["hack_offsets"]), _dp(h["rS"]), _dp(h["rIdx"]), n, 0)
        c.setup = (lambda: capi.spgpuHellSpmvPrepare(*args)) if kind == "planned" else (lambda: capi.spgpuHellSpmvFreeze(*args))
        c.exact = lambda x, y, a, b: X.spmv(n, *X.hell_coo(sub), x, y, a, b, r_idx=r_idx, base=0)
        c.unheld = lambda x, y, a, b: O.spmv_tail(sub, x, y, a, b, r_idx=r_idx, **O.slab_shape(letter, "ragged", deep_cap=O.DEEP_CAP))
    elif kind == "frozen_natural":
        n = 40 * 128 + 50
        c.n = n
        _, _, r, cc, v = synth.banded_coo(n, 16, letter, seed=3)
        hell = formats.ell_to_hell(formats.coo_to_ell(n, r, cc, v), 32)
        dev = formats.DeviceHell(hell)
        c.mat = dev
        c.key = dev.rP
        c.uses = _plan_uses
        c.spmv = lambda dz, dy, dx, a, b: dev.spmv(gpu, dz, dy if b != 0 else None, a, dx, b)
        c.setup = lambda: capi.spgpuHellSpmvFreeze(gpu, code, _dp(dev.cM), _dp(dev.rP), 32, _dp(dev.hack_offsets), _dp(dev.rS), None, n, 0)
        c.exact = lambda x, y, a, b: X.spmv(n, *X.hell_coo(hell), x, y, a, b, base=0)
        c.unheld = lambda x, y, a, b: O.default_spmv(hell, x, y, a, b)
    elif kind.startswith("adopted_hell"):
        hack = int(kind.split("_")[2])
        n = 9 * 2048 + 77
        c.n = n
        coo = _ragged_coo(n, letter, "near", 500, 900, 12.0, 7)
        plain = formats.coo_to_ordered_hell_device(gpu, n, *coo, letter, hack, 0, 0, order=False)
        host = _hell_host(plain, letter, n, hack)
        c.mat = plain
        c.key = plain["rP"]
        c.uses = _adopted_uses

        def spmv(dz, dy, dx, alpha, beta):
            capi.hellspmv[letter](gpu, _dp(dz), _dp(dy) if beta != 0 else None, capi.scalar(letter, alpha), _dp(plain["cM"]), _dp(plain["rP"]), hack,
                                  _dp(plain["hack_offsets"]), _dp(plain["rS"]), None, 12, n, _dp(dx), capi.scalar(letter, beta), 0)
        c.spmv = spmv
        c.setup = lambda: capi.spgpuHellSpmvAdopt(gpu, code, _dp(plain["cM"]), _dp(plain["rP"]), hack, _dp(plain["hack_offsets"]), _dp(plain["rS"]), n, 0)
        c.exact = lambda x, y, a, b: X.spmv(n, *X.hell_coo(host), x, y, a, b, base=0)
        c.unheld = lambda x, y, a, b: O.default_spmv(host, x, y, a, b)
    elif kind.startswith("adopted_ell"):
        n = 5 * 2048 + 100
        c.n = n
        coo = _ragged_coo(n, letter, "near", 400, 600, 10.0, 9)
        rows_h, cols_h, vals_h = (t.cpu().numpy() for t in coo)
        ell = formats.coo_to_ell(n, rows_h, cols_h, vals_h)
        dev = formats.DeviceEll(ell)
        c.mat = dev
        c.key = dev.rP
        c.uses = _adopted_uses
        c.spmv = lambda dz, dy, dx, a, b: dev.spmv(gpu, dz, dy if b != 0 else None, a, dx, b)
        c.setup = lambda: capi.spgpuEllSpmvAdopt(gpu, code, _dp(dev.cM), _dp(dev.rP), dev.pitch, dev.pitch, _dp(dev.rS), dev.max_row, n, 0)
        c.exact = lambda x, y, a, b: X.spmv(n, rows_h.astype(np.int64), cols_h.astype(np.int64), vals_h, x, y, a, b, base=0)
        c.unheld = lambda x, y, a, b: O.default_spmv(ell, x, y, a, b)
    else:
        raise ValueError(kind)
    return c


def _release_all(gpu, key):
    from spgpu_amd import capi
    while capi.spgpuSpmvHolds(gpu, _dp(key)) > 0:
        assert capi.spgpuSpmvRelease(gpu, _dp(key)) == capi.SPGPU_SUCCESS
    capi.spgpuSpmvThaw(gpu, _dp(key))


class SideStream:
    """The handle on a side stream for the test's duration (captures go there, as in test_gpu_fused_solver.py)."""

    def __init__(self, gpu):
        import torch
        from spgpu_amd import capi
        self.gpu, self.stream = gpu, torch.cuda.Stream()
        capi.spgpuSetStream(gpu, C.c_void_p(self.stream.cuda_stream))
        torch.cuda.synchronize()

    def eager(self, fn, *args):
        import torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            fn(*args)
        self.stream.synchronize()

    def capture(self, fn, *args):
        import torch
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream):
            fn(*args)
        torch.cuda.synchronize()
        return graph

    def close(self):
        from spgpu_amd import capi
        capi.spgpuSetStream(self.gpu, None)


def _vectors(c, seed):
    from spgpu_amd import synth
    return synth.values_for(c.letter, seed, c.n)


KINDS = ["planned", "frozen", "frozen_natural", "adopted_hell_32_D", "adopted_hell_32_S", "adopted_hell_32_C", "adopted_hell_64_D",
         "adopted_ell_D", "adopted_ell_S"]


@pytest.mark.parametrize("kind", KINDS)
def test_a_held_capture_runs_on_the_record(gpu, kind):
    import torch
    from spgpu_amd import capi, formats
    c = _case(gpu, kind)
    alpha, beta = -0.5, 2.0
    x, y = _vectors(c, 31), _vectors(c, 32)
    dx, dy = formats.to_device(x), formats.to_device(y)
    dz = torch.full((c.n,), float("nan"), dtype=dx.dtype, device="cuda")
    dz_eager = torch.full_like(dz, float("nan"))
    side = SideStream(gpu)
    graph = None
    try:
        assert c.setup() == capi.SPGPU_SUCCESS
        for _ in range(2):
            side.eager(c.spmv, dz_eager, dy, dx, alpha, beta)       # (the default kernels' AUTO settles on its form)
        assert capi.spgpuSpmvHold(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == 1
        before = c.uses(gpu)
        graph = side.capture(c.spmv, dz, dy, dx, alpha, beta)
        assert c.uses(gpu) - before == 1                            # the captured launch found the held record
        for rep in range(3):
            x = _vectors(c, 50 + rep)
            dx.copy_(formats.to_device(x))
            dz.fill_(float("nan"))
            torch.cuda.synchronize()
            uses = c.uses(gpu)
            graph.replay()
            torch.cuda.synchronize()
            assert c.uses(gpu) == uses                              # replays are not counted
            got = dz.cpu().numpy()
            dz_eager.fill_(float("nan"))
            side.eager(c.spmv, dz_eager, dy, dx, alpha, beta)
            assert c.uses(gpu) == uses + 1                          # the eager call ran on the record too
            assert got.tobytes() == dz_eager.cpu().numpy().tobytes(), (kind, rep)
            exact, scale = c.exact(x, y, alpha, beta)
            X.assert_within(got, exact, scale, c.letter, ("held capture", kind, rep))
    finally:
        if graph is not None:
            graph.reset()
        side.close()
        _release_all(gpu, c.key)


@pytest.mark.parametrize("kind", ["frozen", "frozen_natural", "adopted_hell_32_D", "adopted_ell_D"])
def test_no_hold_no_change(gpu, kind):
    """Without a hold a captured launch looks no record up and replays with the bits captures have always had: the unplanned
    ordered kernel, the unfrozen default kernel, the plain kernel on the caller's arrays of an adopted matrix."""
    import torch
    from spgpu_amd import capi, formats
    c = _case(gpu, kind)
    alpha, beta = 1.5, -0.25
    x, y = _vectors(c, 41), _vectors(c, 42)
    dx, dy = formats.to_device(x), formats.to_device(y)
    dz = torch.full((c.n,), float("nan"), dtype=dx.dtype, device="cuda")
    side = SideStream(gpu)
    graph = None
    try:
        assert c.setup() == capi.SPGPU_SUCCESS
        side.eager(c.spmv, dz, dy, dx, alpha, beta)
        plan_uses, adopted_uses = _plan_uses(gpu), _adopted_uses(gpu)
        graph = side.capture(c.spmv, dz, dy, dx, alpha, beta)
        assert (_plan_uses(gpu), _adopted_uses(gpu)) == (plan_uses, adopted_uses)
        for rep in range(2):
            x = _vectors(c, 60 + rep)
            dx.copy_(formats.to_device(x))
            dz.fill_(float("nan"))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert dz.cpu().numpy().tobytes() == c.unheld(x, y, alpha, beta).tobytes(), (kind, rep)
    finally:
        if graph is not None:
            graph.reset()
        side.close()
        _release_all(gpu, c.key)


@pytest.mark.parametrize("kind", ["frozen", "adopted_hell_32_D"])
def test_thaw_is_refused_under_a_hold(gpu, kind):
    import torch
    from spgpu_amd import capi, formats
    c = _case(gpu, kind)
    x, y = _vectors(c, 71), _vectors(c, 72)
    dx, dy = formats.to_device(x), formats.to_device(y)
    dz = torch.full((c.n,), float("nan"), dtype=dx.dtype, device="cuda")
    dz_eager = torch.full_like(dz, float("nan"))
    side = SideStream(gpu)
    graph = None
    try:
        assert c.setup() == capi.SPGPU_SUCCESS
        side.eager(c.spmv, dz_eager, dy, dx, 1.0, 0.5)
        want = dz_eager.cpu().numpy()
        assert capi.spgpuSpmvHold(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvHold(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == 2
        graph = side.capture(c.spmv, dz, dy, dx, 1.0, 0.5)
        frozen = capi.spgpuSpmvFrozenBytes(gpu)
        assert frozen > 0
        assert capi.spgpuSpmvThaw(gpu, _dp(c.key)) == capi.SPGPU_IN_USE
        assert capi.spgpuSpmvFrozenBytes(gpu) == frozen             # nothing was freed
        graph.replay()
        torch.cuda.synchronize()
        assert dz.cpu().numpy().tobytes() == want.tobytes()
        assert capi.spgpuSpmvRelease(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvThaw(gpu, _dp(c.key)) == capi.SPGPU_IN_USE
        assert capi.spgpuSpmvFrozenBytes(gpu) == frozen
        dz.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert dz.cpu().numpy().tobytes() == want.tobytes()
        graph.reset()                                               # the last graph on the matrix is gone: release, thaw
        graph = None
        assert capi.spgpuSpmvRelease(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == 0
        assert capi.spgpuSpmvThaw(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvFrozenBytes(gpu) < frozen
    finally:
        if graph is not None:
            graph.reset()
        side.close()
        _release_all(gpu, c.key)


def test_held_records_are_not_evicted(gpu):
    """8 records per handle: with all 8 held, a ninth matrix gets none -- Freeze says SPGPU_UNSUPPORTED, its calls run unfrozen
    with the oracle's bits -- and the 8 captured graphs still replay on their records."""
    import torch
    from spgpu_amd import capi, formats, synth
    n = 16 * 128
    mats = []
    for i in range(9):
        _, _, r, cc, v = synth.banded_coo(n, 8 + i, "D", seed=20 + i)
        hell = formats.ell_to_hell(formats.coo_to_ell(n, r, cc, v), 32)
        mats.append((formats.DeviceHell(hell), hell))

    def freeze(dev):
        return capi.spgpuHellSpmvFreeze(gpu, capi.TYPE_DOUBLE, _dp(dev.cM), _dp(dev.rP), 32, _dp(dev.hack_offsets), _dp(dev.rS), None, n, 0)

    x = synth.values_for("D", 77, n)
    dx = formats.to_device(x)
    outs = [torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(8)]
    side = SideStream(gpu)
    graphs = []
    try:
        stales = capi.plan_counts(gpu)[2]
        for (dev, hell), dz in zip(mats[:8], outs):
            assert freeze(dev) == capi.SPGPU_SUCCESS
            side.eager(dev.spmv, gpu, dz, None, 1.0, dx, 0.0)
            assert dz.cpu().numpy().tobytes() == O.default_spmv(hell, x, None, 1.0, 0.0).tobytes()
            assert capi.spgpuSpmvHold(gpu, _dp(dev.rP)) == capi.SPGPU_SUCCESS
            uses = _plan_uses(gpu)
            graphs.append(side.capture(dev.spmv, gpu, dz, None, 1.0, dx, 0.0))
            assert _plan_uses(gpu) == uses + 1
        dev8, hell8 = mats[8]
        assert freeze(dev8) == capi.SPGPU_UNSUPPORTED
        z8 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        uses = _plan_uses(gpu)
        side.eager(dev8.spmv, gpu, z8, None, 1.0, dx, 0.0)
        assert z8.cpu().numpy().tobytes() == O.default_spmv(hell8, x, None, 1.0, 0.0).tobytes()
        assert _plan_uses(gpu) == uses
        x = synth.values_for("D", 78, n)
        dx.copy_(formats.to_device(x))
        for dz in outs:
            dz.fill_(float("nan"))
        torch.cuda.synchronize()
        for g in graphs:
            g.replay()
        torch.cuda.synchronize()
        for (dev, hell), dz in zip(mats[:8], outs):
            assert dz.cpu().numpy().tobytes() == O.default_spmv(hell, x, None, 1.0, 0.0).tobytes()
        assert capi.plan_counts(gpu)[2] == stales
    finally:
        for g in graphs:
            g.reset()
        side.close()
        for dev, _ in mats:
            _release_all(gpu, dev.rP)
    assert capi.spgpuSpmvFrozenBytes(gpu) == 0


def test_edge_cases(gpu):
    import torch
    from spgpu_amd import capi
    c = _case(gpu, "frozen_natural")
    stranger = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert capi.spgpuSpmvHold(gpu, _dp(stranger)) == capi.SPGPU_UNSUPPORTED      # no record under this rP
    assert capi.spgpuSpmvHolds(gpu, _dp(stranger)) == 0
    assert capi.spgpuSpmvRelease(gpu, _dp(stranger)) == capi.SPGPU_UNSUPPORTED
    from spgpu_amd import formats
    x = _vectors(c, 81)
    dx = formats.to_device(x)
    dz = torch.full((c.n,), float("nan"), dtype=dx.dtype, device="cuda")
    side = SideStream(gpu)
    graph = None
    said = []
    try:
        assert c.setup() == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvRelease(gpu, _dp(c.key)) == capi.SPGPU_UNSUPPORTED  # a record, but no hold on it
        uses = _plan_uses(gpu)

        def hold_inside_the_capture():
            said.append(capi.spgpuSpmvHold(gpu, _dp(c.key)))
            c.spmv(dz, None, dx, 1.0, 0.0)

        graph = side.capture(hold_inside_the_capture)
        assert said == [capi.SPGPU_UNSUPPORTED]
        assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == 0
        assert _plan_uses(gpu) == uses                              # not held: the capture ran unfrozen, as ever
        graph.replay()
        torch.cuda.synchronize()
        assert dz.cpu().numpy().tobytes() == c.unheld(x, None, 1.0, 0.0).tobytes()
        for count in (1, 2, 3):
            assert capi.spgpuSpmvHold(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
            assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == count
        for count in (2, 1, 0):
            assert capi.spgpuSpmvRelease(gpu, _dp(c.key)) == capi.SPGPU_SUCCESS
            assert capi.spgpuSpmvHolds(gpu, _dp(c.key)) == count
        assert capi.spgpuSpmvRelease(gpu, _dp(c.key)) == capi.SPGPU_UNSUPPORTED
    finally:
        if graph is not None:
            graph.reset()
        side.close()
        _release_all(gpu, c.key)


def _symmetric_ragged(n, seed, longest=900, mean=12.0):
    """Host COO of a symmetric, diagonally dominant matrix with power-law row lengths: B + B^T (no diagonal) + D, D_ii = 1 +
    sum_j |(B + B^T)_ij|."""
    from spgpu_amd import synth
    lengths = np.minimum(synth.power_law_lengths(n, mean, longest, seed), longest)
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n, dtype=np.int64), lengths)
    cols = (rows + rng.integers(-500, 501, size=rows.size)) % n
    keep = cols != rows
    rows, cols = rows[keep], cols[keep]
    vals = rng.uniform(-1.0, 1.0, size=rows.size)
    r = np.concatenate([rows, cols])
    c = np.concatenate([cols, rows])
    v = np.concatenate([vals, vals])
    key = r * n + c
    key, inv = np.unique(key, return_inverse=True)
    v = np.bincount(inv, weights=v, minlength=key.size)
    r, c = key // n, key % n
    diag = 1.0 + np.bincount(r, weights=np.abs(v), minlength=n)
    r = np.concatenate([r, np.arange(n)])
    c = np.concatenate([c, np.arange(n)])
    v = np.concatenate([v, diag])
    order = np.lexsort((c, r))
    return r[order].astype(np.int32), c[order].astype(np.int32), v[order]


def test_graph_cg_on_an_adopted_ragged_matrix(gpu):
    """20 CG iterations with the scalars on the device, eager and replayed from two held graphs (one per parity of the |r|^2 cell):
    x and |r|^2 bit for bit the same; the two captures ran on the adopted copy."""
    import torch
    from spgpu_amd import capi, formats
    n = 20000
    r, c, v = _symmetric_ragged(n, 5)
    coo = (torch.from_numpy(r).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(v).cuda())
    plain = formats.coo_to_ordered_hell_device(gpu, n, *coo, "D", 32, 0, 0, order=False)
    b = formats.to_device(np.random.default_rng(3).uniform(-1.0, 1.0, n))
    iters = 20
    P = _dp

    def spmv(z, p):
        capi.hellspmv["D"](gpu, P(z), None, capi.scalar("D", 1.0), P(plain["cM"]), P(plain["rP"]), 32, P(plain["hack_offsets"]), P(plain["rS"]),
                           None, 12, n, P(p), capi.scalar("D", 0.0), 0)

    x, rvec, p, ap = torch.zeros_like(b), b.clone(), b.clone(), torch.empty_like(b)
    s = torch.zeros(3, dtype=torch.float64, device="cuda")

    def iteration(rr_old, rr_new):
        spmv(ap, p)
        capi.dot_device["D"](gpu, P(s[2:]), n, P(p), P(ap))
        capi.axpby_quot_device["D"](gpu, P(x), n, None, None, P(x), P(rr_old), P(s[2:]), 0, P(p))
        capi.axpby_quot_device["D"](gpu, P(rvec), n, None, None, P(rvec), P(rr_old), P(s[2:]), 1, P(ap))
        capi.dot_device["D"](gpu, P(rr_new), n, P(rvec), P(rvec))
        capi.axpby_quot_device["D"](gpu, P(p), n, P(rr_new), P(rr_old), P(p), None, None, 0, P(rvec))

    def restart():
        x.zero_(), rvec.copy_(b), p.copy_(b)
        torch.cuda.synchronize()
        side.eager(capi.dot_device["D"], gpu, P(s), n, P(rvec), P(rvec))

    key = plain["rP"]
    side = SideStream(gpu)
    graphs = []
    try:
        assert capi.spgpuHellSpmvAdopt(gpu, capi.TYPE_DOUBLE, P(plain["cM"]), P(key), 32, P(plain["hack_offsets"]), P(plain["rS"]), n, 0) == capi.SPGPU_SUCCESS
        restart()
        rr0 = s[0].item()
        uses = _adopted_uses(gpu)
        for i in range(iters):
            side.eager(iteration, s[(i & 1):], s[1 - (i & 1):])
        assert _adopted_uses(gpu) == uses + iters
        x_eager, rr_eager = x.clone(), s[iters & 1].item()
        assert rr_eager < rr0
        restart()
        assert capi.spgpuSpmvHold(gpu, P(key)) == capi.SPGPU_SUCCESS
        uses = _adopted_uses(gpu)
        for parity in range(2):
            graphs.append(side.capture(iteration, s[parity:], s[1 - parity:]))
        assert _adopted_uses(gpu) == uses + 2
        for i in range(iters):
            graphs[i & 1].replay()
        torch.cuda.synchronize()
        assert _adopted_uses(gpu) == uses + 2
        assert torch.equal(x, x_eager)
        assert s[iters & 1].item() == rr_eager
    finally:
        for g in graphs:
            g.reset()
        side.close()
        _release_all(gpu, key)


def test_c_tool_cg_on_an_adopted_matrix_market_file(tmp_path):
    """tools/cg_ragged_amd: a symmetric ragged .mtx (lower triangle stored), adopted from plain C; the held graph repeats the eager
    run bit for bit, its captures ran on the copy, Thaw is refused under the hold."""
    exe = os.path.join(ROOT, "tools", "cg_ragged_amd.bin")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", ROOT, "tools/cg_ragged_amd.bin"], check=False)
    assert os.path.exists(exe), f"{exe} missing: run `make tools`"
    n = 6000
    r, c, v = _symmetric_ragged(n, 11, longest=500, mean=8.0)
    lower = r >= c
    path = tmp_path / "sym_ragged.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{n} {n} {int(lower.sum())}\n")
        f.writelines(f"{i + 1} {j + 1} {w:.17g}\n" for i, j, w in zip(r[lower], c[lower], v[lower]))
    out = subprocess.run([exe, str(path), "30"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout
    held = [line for line in out.stdout.splitlines() if line.startswith("graph, held:")]
    assert held and "bit-identical to the eager run" in held[0], out.stdout
