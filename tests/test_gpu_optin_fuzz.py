"""GPU: seeded random matrices through every opt-in call of include/spgpu/tuning.h -- Prepare, Freeze (default share of escapes and
SPGPU_FREEZE_MAX_ESCAPES_PCT=100), Adopt (HELL and ELL) and Optimize -- against EXTENDED PRECISION (tests/exact_ref.py), not only
against the kernel-shaped oracle.  Every type, hack sizes that do and do not divide 32, both index bases, empty / uniform /
power-law rows and a few rows of thousands of entries, band / near / scattered columns (some beyond 16 bits of reach), rows as they
come, ordered by length, or ordered in windows.

Per call: the return code the header documents, predicted on the host where the rule is cheap (complex fp64 has no packed form;
Adopt wants a hack size that is a multiple of 32 and 1.25 x the slots of its ordered copy; the unordered copy's share of escapes);
then three SpMV calls (complex alpha and beta for C and Z, one with z == y) that must be within the north_star bound of the
extended-precision product AND have the bits of the call they stand for: the unfrozen call (Freeze, Prepare, a matrix left as it
is), the call on the matrix ordered with the same device calls (Adopt).  Thaw gives the first bits back.  The handle lives for the
whole session: everything frozen or adopted here is thawed in a finally."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X

pytestmark = pytest.mark.gpu

WIDE = {"S": 4, "D": 2, "C": 2, "Z": 1}      # rows per 16-byte load of the slab kernels: a HELL hack must hold whole strips


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _case(seed):
    rng = np.random.default_rng(7000 + seed)
    letter = "SDCZ"[seed % 4]
    n = int(rng.choice([33, 300, 2053, 5003, 9000]))
    hack = int(rng.choice([32, 64, 96, 16, 30, 48]))
    base = int(rng.integers(0, 2))
    kind = str(rng.choice(["uniform", "powerlaw", "huge", "empty_mix"]))
    pattern = str(rng.choice(["band", "near", "scattered"]))
    cols_n = n + (int(rng.choice([0, 140_000])) if pattern != "band" else 0)    # scattered over > 65 535 columns: escapes
    if kind == "uniform":
        lengths = np.full(n, int(rng.integers(1, 30)))
    elif kind == "powerlaw":
        lengths = np.minimum((2.0 * rng.random(n) ** -0.6).astype(np.int64), 600)
    elif kind == "huge":
        lengths = rng.integers(0, 8, n)
        lengths[rng.integers(0, n, max(1, n // 1000))] = int(rng.integers(2000, 5000))
    else:
        lengths = rng.integers(0, 3, n) * rng.integers(0, 9, n)
    lengths = np.minimum(lengths, cols_n).astype(np.int64)
    lengths[int(rng.integers(0, n))] = max(1, int(lengths.max()))    # never an empty matrix
    rows = np.repeat(np.arange(n, dtype=np.int64), lengths)
    k = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    L = np.repeat(lengths, lengths)
    if pattern == "band":
        cols = (rows - L // 2 + k) % cols_n
    elif pattern == "near":       # ascending, distinct, within +- max(600, 2L) of the row
        span = np.maximum(1200, 2 * L)
        cols = (rows - span // 2 + (k * span) // L) % cols_n
    else:                         # ascending, distinct, over all of x
        cols = np.minimum(((k + rng.random(rows.size)) * cols_n / L).astype(np.int64), cols_n - 1)
    real = X.REAL_OF[letter]
    vals = rng.standard_normal(rows.size).astype(real)
    if letter in "CZ":
        vals = (vals + 1j * rng.standard_normal(rows.size).astype(real)).astype(X.DTYPE_OF[letter])
    order = str(rng.choice(["none", "none", "by_length", "windowed"]))
    return dict(seed=seed, letter=letter, n=n, cols_n=cols_n, hack=hack, base=base, kind=kind, pattern=pattern, order=order,
                rows=rows, cols=cols, vals=vals, lengths=lengths, rng=rng)


def _vector(rng, letter, n):
    v = rng.standard_normal(n).astype(X.REAL_OF[letter])
    if letter in "CZ":
        v = (v + 1j * rng.standard_normal(n).astype(X.REAL_OF[letter])).astype(X.DTYPE_OF[letter])
    return v


def _scalars(letter):
    """(alpha, beta, z == y): three calls; complex scalars with non-zero imaginary parts for C and Z."""
    if letter in "CZ":
        return [(0.75 - 1.25j, -0.5 + 2.0j, False), (-1.5 + 0.25j, 0.0, False), (0.5 + 1.0j, 1.0 - 0.75j, True)]
    return [(-0.75, 1.5, False), (1.25, 0.0, False), (2.0, -0.5, True)]


def _ordered_slots(lengths, hack):
    """Slots of the copy Adopt would keep: the rows in oellOrderAligned's order (windows of 2 048, rows longer than 256 set
    aside), each hack as deep as its longest row."""
    from spgpu_amd import formats
    _, sorted_lengths = formats.oell_order(lengths, window=2048, long_rows=256, aligned=True)
    n = len(sorted_lengths)
    pad = np.zeros((n + hack - 1) // hack * hack, np.int64)
    pad[:n] = sorted_lengths
    return int(pad.reshape(-1, hack).max(axis=1).sum()) * hack


class _Run:
    """The matrix of a case in HELL and ELL, on the device, and the SpMV calls on it."""

    def __init__(self, gpu, case):
        from spgpu_amd import formats
        self.gpu, self.case = gpu, case
        c = case
        self.letter, self.n, self.base, self.hack = c["letter"], c["n"], c["base"], c["hack"]
        self.r_idx = None
        rows = c["rows"]
        if c["order"] != "none":
            if c["order"] == "by_length":
                self.r_idx, _ = formats.oell_order(c["lengths"])
            else:
                rng = c["rng"]
                self.r_idx, _ = formats.oell_order(c["lengths"], window=int(rng.choice([64, 512, 2048])), long_rows=int(rng.choice([0, 40])),
                                                   aligned=bool(rng.integers(0, 2)))
            inverse = np.empty(self.n, np.int64)
            inverse[self.r_idx] = np.arange(self.n)
            rows = inverse[rows]            # row i of the stored matrix is row r_idx[i] of the case
            keep = np.argsort(rows, kind="stable")
            self.stored = (rows[keep], c["cols"][keep], c["vals"][keep])
        else:
            self.stored = (rows, c["cols"], c["vals"])
        r, cc, v = self.stored
        self.ell = formats.coo_to_ell(self.n, r + self.base, cc + self.base, v, coo_base=self.base, ell_base=self.base)
        self.hell = formats.ell_to_hell(self.ell, self.hack)
        self.dhell = formats.DeviceHell(self.hell, r_idx=self.r_idx)
        self.dell = formats.DeviceEll(self.ell, r_idx=self.r_idx)
        rng = c["rng"]
        self.x, self.y = _vector(rng, self.letter, c["cols_n"]), _vector(rng, self.letter, self.n)
        self.dx, self.dy = formats.to_device(self.x), formats.to_device(self.y)
        self.want = [X.spmv(self.n, c["rows"], c["cols"], c["vals"], self.x, self.y if b != 0 else None, a, b) for a, b, _ in _scalars(self.letter)]

    def calls(self, mat, what):
        """The three SpMV calls on `mat` (a DeviceHell / DeviceEll, or a dict of ordered device arrays); each within the bound."""
        import torch
        out = []
        for (alpha, beta, in_place), (want, scale) in zip(_scalars(self.letter), self.want):
            dz = self.dy.clone() if in_place else torch.full((self.n,), float("nan"), dtype=self.dx.dtype, device="cuda")
            yy = dz if in_place else (self.dy if beta != 0 else None)
            torch.cuda.synchronize()
            if isinstance(mat, dict):
                from spgpu_amd import capi
                L = self.letter
                capi.hellspmv[L](self.gpu, _p(dz), _p(yy), capi.scalar(L, alpha), _p(mat["cM"]), _p(mat["rP"]), mat["hack_size"],
                                 _p(mat["hack_offsets"]), _p(mat["rS"]), _p(mat["rIdx"]), 0, self.n, _p(self.dx), capi.scalar(L, beta), self.base)
            else:
                mat.spmv(self.gpu, dz, yy, alpha, self.dx, beta)
            torch.cuda.synchronize()
            got = dz.cpu().numpy()
            X.assert_within(got, want, scale, self.letter, (what, self.describe(), alpha, beta, in_place))
            out.append(got)
        return out

    def describe(self):
        c = self.case
        return (f"seed {c['seed']} {self.letter} n={self.n} cols={c['cols_n']} hack={self.hack} base={self.base} {c['kind']} "
                f"{c['pattern']} order={c['order']}")

    # ---- what tuning.h says the calls return -------------------------------------------------------------------------

    def wide_ok(self, fmt):
        return fmt == "ell" or self.hack % WIDE[self.letter] == 0

    def freeze_expected(self, fmt, pct):
        """SPGPU_SUCCESS / SPGPU_UNSUPPORTED, or None where the header leaves it to the device's analysis (the ordered copy's
        blocks count from where the plan's probe put them)."""
        from spgpu_amd import capi
        if self.letter == "Z" or not self.wide_ok(fmt):
            return capi.SPGPU_UNSUPPORTED
        if self.r_idx is not None:
            return capi.SPGPU_SUCCESS if pct >= 100 else None
        r, cc, _ = self.stored
        entries, escapes = X.unordered_escapes(self.n, r, cc, self.letter)
        return capi.SPGPU_SUCCESS if X.freeze_keeps(entries, escapes, pct) else capi.SPGPU_UNSUPPORTED

    def adopt_expected(self, fmt):
        from spgpu_amd import capi
        hack = self.hack if fmt == "hell" else 32
        if hack % 32 != 0:
            return capi.SPGPU_UNSUPPORTED
        caller = self.hell["values"].size if fmt == "hell" else self.n * self.ell["max_row"]
        return capi.SPGPU_SUCCESS if caller * 4 >= _ordered_slots(self.ell["row_lengths"], hack) * 5 else capi.SPGPU_UNSUPPORTED

    def ordered_copy(self, hack):
        """The caller's own ordering with the device calls Adopt makes (spgpuOellOrderAlignedDevice, windows 2 048 / 256)."""
        import torch
        from spgpu_amd import formats
        r, cc, v = self.stored
        rows_t = torch.from_numpy(np.ascontiguousarray(r + self.base, np.int32)).cuda()
        cols_t = torch.from_numpy(np.ascontiguousarray(cc + self.base, np.int32)).cuda()
        vals_t = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        return formats.coo_to_ordered_hell_device(self.gpu, self.n, rows_t, cols_t, vals_t, self.letter, hack, 2048, 256, coo_base=self.base,
                                                  hell_base=self.base, aligned=True)


def _freeze(gpu, run, fmt):
    from spgpu_amd import capi
    code = capi.TYPE_CODE[run.letter]
    if fmt == "hell":
        d = run.dhell
        return capi.spgpuHellSpmvFreeze(gpu, code, _p(d.cM), _p(d.rP), d.hack_size, _p(d.hack_offsets), _p(d.rS), _p(d.rIdx), run.n, run.base)
    d = run.dell
    return capi.spgpuEllSpmvFreeze(gpu, code, _p(d.cM), _p(d.rP), d.pitch, d.pitch, _p(d.rS), _p(d.rIdx), d.max_row, run.n, run.base)


def _same_bits(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), (what, k, int(np.flatnonzero(g.view(np.uint8) != w.view(np.uint8))[0]) // g.itemsize)


@pytest.mark.parametrize("seed", range(48))
def test_opt_in_calls_on_a_random_matrix(gpu, tuning, seed):
    from spgpu_amd import capi
    run = _Run(gpu, _case(seed))
    what = run.describe()
    code = capi.TYPE_CODE[run.letter]
    mats = {"hell": run.dhell, "ell": run.dell}
    before = {fmt: run.calls(m, (fmt, "before")) for fmt, m in mats.items()}
    live = {}              # rP of everything frozen or adopted (by address), thawed in the finally
    try:
        # Prepare: a plan for a call with a row order, nothing to prepare without one
        d = run.dhell
        said = capi.spgpuHellSpmvPrepare(gpu, code, _p(d.cM), _p(d.rP), d.hack_size, _p(d.hack_offsets), _p(d.rS), _p(d.rIdx), run.n, run.base)
        prepared = capi.SPGPU_SUCCESS if run.r_idx is not None and run.wide_ok("hell") else capi.SPGPU_UNSUPPORTED
        assert said == prepared, (what, said)
        _same_bits(run.calls(d, "prepared"), before["hell"], ("prepared", what))

        # Freeze, HELL and ELL, under the default share of escapes and with any share allowed
        frozen_default = {}
        for pct in (1, 100):
            tuning(SPGPU_FREEZE_MAX_ESCAPES_PCT=pct)
            for fmt, m in mats.items():
                assert capi.spgpuSpmvFrozenBytes(gpu) == 0, what
                said = _freeze(gpu, run, fmt)
                if said == capi.SPGPU_SUCCESS:
                    live[m.rP.data_ptr()] = m.rP
                expected = run.freeze_expected(fmt, pct)
                assert said in (capi.SPGPU_SUCCESS, capi.SPGPU_UNSUPPORTED), (what, fmt, pct, said)
                assert expected is None or said == expected, (what, fmt, pct, said, expected)
                assert (capi.spgpuSpmvFrozenBytes(gpu) > 0) == (said == capi.SPGPU_SUCCESS), (what, fmt, pct)
                if pct == 1:
                    frozen_default[fmt] = said
                _same_bits(run.calls(m, (fmt, "frozen", pct, said)), before[fmt], (fmt, "frozen", pct, what))
                thawed = capi.spgpuSpmvThaw(gpu, _p(m.rP))
                if live.pop(m.rP.data_ptr(), None) is not None:
                    assert thawed == capi.SPGPU_SUCCESS, (what, fmt)
                assert capi.spgpuSpmvFrozenBytes(gpu) == 0, (what, fmt)
                _same_bits(run.calls(m, (fmt, "thawed", pct)), before[fmt], (fmt, "thawed", pct, what))
        tuning(SPGPU_FREEZE_MAX_ESCAPES_PCT=1)

        # Adopt (matrices as they come: Adopt keys the caller's arrays without rIdx)
        adopted_bits = {}
        if run.r_idx is None:
            for fmt, m in mats.items():
                if fmt == "hell":
                    said = capi.spgpuHellSpmvAdopt(gpu, code, _p(m.cM), _p(m.rP), m.hack_size, _p(m.hack_offsets), _p(m.rS), run.n, run.base)
                else:
                    said = capi.spgpuEllSpmvAdopt(gpu, code, _p(m.cM), _p(m.rP), m.pitch, m.pitch, _p(m.rS), m.max_row, run.n, run.base)
                if said == capi.SPGPU_SUCCESS:
                    live[m.rP.data_ptr()] = m.rP
                assert said == run.adopt_expected(fmt), (what, fmt, said)
                if said == capi.SPGPU_SUCCESS:
                    uses = capi.spgpuSpmvAdoptedUses(gpu)
                    got = run.calls(m, (fmt, "adopted"))
                    assert capi.spgpuSpmvAdoptedUses(gpu) == uses + 3, (what, fmt)
                    own = run.ordered_copy(m.hack_size if fmt == "hell" else 32)
                    _same_bits(got, run.calls(own, (fmt, "ordered by the caller")), (fmt, "adopted", what))
                    adopted_bits[fmt] = got
                    del own
                    assert capi.spgpuSpmvThaw(gpu, _p(m.rP)) == capi.SPGPU_SUCCESS
                    del live[m.rP.data_ptr()]
                else:
                    assert capi.spgpuSpmvFrozenBytes(gpu) == 0, (what, fmt)
                    _same_bits(run.calls(m, (fmt, "not adopted")), before[fmt], (fmt, "not adopted", what))
                assert capi.spgpuSpmvFrozenBytes(gpu) == 0, (what, fmt)
                _same_bits(run.calls(m, (fmt, "after adopt thawed")), before[fmt], (fmt, "after adopt thawed", what))

        # Optimize: adopt a ragged matrix without an order, else freeze, else nothing -- the same answers as the calls above
        d = run.dhell
        said = capi.spgpuHellSpmvOptimize(gpu, code, _p(d.cM), _p(d.rP), d.hack_size, _p(d.hack_offsets), _p(d.rS), _p(d.rIdx), run.n, run.base)
        if said != capi.SPMV_AS_IS:
            live[d.rP.data_ptr()] = d.rP
        if run.r_idx is None and "hell" in adopted_bits:
            expected = capi.SPMV_ADOPTED
        else:
            expected = capi.SPMV_FROZEN if frozen_default["hell"] == capi.SPGPU_SUCCESS else capi.SPMV_AS_IS
        assert said == expected, (what, said, expected)
        got = run.calls(d, ("optimized", said))
        _same_bits(got, adopted_bits["hell"] if said == capi.SPMV_ADOPTED else before["hell"], ("optimized", said, what))
        if said != capi.SPMV_AS_IS:
            assert capi.spgpuSpmvThaw(gpu, _p(d.rP)) == capi.SPGPU_SUCCESS
            del live[d.rP.data_ptr()]
        assert capi.spgpuSpmvFrozenBytes(gpu) == 0, what
        _same_bits(run.calls(d, "after optimize thawed"), before["hell"], ("after optimize thawed", what))
    finally:
        for rP in live.values():
            capi.spgpuSpmvThaw(gpu, _p(rP))
