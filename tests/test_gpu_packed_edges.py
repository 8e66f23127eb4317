"""GPU: the 16-bit copies of frozen matrices AT THEIR LIMITS (include/spgpu/tuning.h Freeze; frozen_slab.hip.h slabPackKernel,
planned_spmv.hip planPackKernel, ragged_spmv.hip.h lens).

A word of the copy is a column's offset from where its group (no row order: the group of rows one wavefront owns, 32 rows for fp32,
128 for the 8-byte types, from the group's lowest column) or its block of ordered rows (from the block's base: its lowest first / last
column when those lie within 16 bits of each other) counts: 65 534 is the last offset stored, 65 535 (0xFFFF) and beyond are escapes
read from rP, as are negative columns.  The matrices here place columns at exactly those offsets, keep the share of escapes on
either side of the documented 1 %, and give rows of 65 534 .. ~70 000 entries (the ragged kernel's 16-bit row lengths).  Every
result has the bits of the unfrozen call / the oracle, and is within the bound of the extended-precision product (tests/exact_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import exact_ref as X
import oracle_api as O

pytestmark = pytest.mark.gpu

EDGE = [65533, 65534, 65535, 65536]      # offsets from the group's / block's base: two stored, two escapes


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _values(letter, count, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(count).astype(X.REAL_OF[letter])
    if letter in "CZ":
        v = (v + 1j * rng.standard_normal(count).astype(X.REAL_OF[letter])).astype(X.DTYPE_OF[letter])
    return v


def _scalars(letter):
    return (0.75 - 1.5j, -0.5 + 0.25j) if letter in "CZ" else (-1.25, 0.5)


def _call(gpu, dev, x, y, alpha, beta):
    import torch
    from spgpu_amd import formats
    dx, dy = formats.to_device(x), formats.to_device(y)
    dz = torch.full((dev.rows,), float("nan"), dtype=dx.dtype, device="cuda")
    torch.cuda.synchronize()
    dev.spmv(gpu, dz, dy, alpha, dx, beta)
    torch.cuda.synchronize()
    return dz.cpu().numpy()


def _freeze(gpu, dev):
    from spgpu_amd import capi
    return capi.spgpuHellSpmvFreeze(gpu, capi.TYPE_CODE[dev.letter], _p(dev.cM), _p(dev.rP), dev.hack_size, _p(dev.hack_offsets), _p(dev.rS),
                                    _p(dev.rIdx), dev.rows, dev.base)


# ---- without a row order: offsets from the group's lowest column ----------------------------------------------------------

def _band_with_edges(letter, n, base, planted, extra_escapes=0):
    """Band rows col(r, k) = r + k, 8 per row (strips of consecutive columns), x of 150 000 entries.  In each of `planted` groups
    one row has six of its slots replaced: lowest + 65 533 .. 65 536, a far column, and a hole (column -1, base 1) or a second far
    column (base 0).  `extra_escapes` more rows get one slot at lowest + 65 535.  Returns COO (0-based rows / cols) and the group
    rows."""
    G = X.group_rows_of(letter)
    rows = np.repeat(np.arange(n, dtype=np.int64), 8)
    cols = rows + np.tile(np.arange(8, dtype=np.int64), n)
    groups = np.linspace(1, n // G - 1, planted).astype(np.int64) if planted else np.array([], np.int64)
    for g in groups:
        lowest = g * G
        r = lowest + 5
        cols[r * 8 + 1: r * 8 + 7] = [lowest + e for e in EDGE] + [lowest + 120_000, -1 if base else lowest + 140_000]
    others = [r for r in range(0, n, 7) if (r // G) not in set(groups.tolist())][:extra_escapes]
    for r in others:
        cols[r * 8 + 3] = (r // G) * G + 65535
    assert cols.max() < 150_000                     # the length of x in the tests below
    return rows, cols


@pytest.mark.parametrize("letter", ["S", "D", "C"])
@pytest.mark.parametrize("base", [0, 1])
def test_unordered_frozen_at_the_16_bit_limit(gpu, letter, base):
    from spgpu_amd import capi, formats
    n = 4096
    rows, cols = _band_with_edges(letter, n, base, planted=5)
    vals = _values(letter, rows.size, 3)
    entries, escapes = X.unordered_escapes(n, rows, cols, letter)
    assert escapes == 5 * 4 and X.freeze_keeps(entries, escapes), (entries, escapes)     # 65 535, 65 536, far, hole / far per group
    ell = formats.coo_to_ell(n, rows + base, cols + base, vals, coo_base=base, ell_base=base)
    hell = formats.ell_to_hell(ell, 32)
    dev = formats.DeviceHell(hell)
    x, y = _values(letter, 150_000, 4), _values(letter, n, 5)
    alpha, beta = _scalars(letter)
    want_bits = O.default_spmv(hell, x, y, alpha, beta)
    want, scale = X.spmv(n, rows, cols, vals, x, y, alpha, beta)
    try:
        unfrozen = {}
        for form in (capi.FORM_GATHER, capi.FORM_STRIPS, capi.FORM_AUTO):
            capi.spgpuSetSpmvForm(gpu, form)
            unfrozen[form] = _call(gpu, dev, x, y, alpha, beta)
            assert unfrozen[form].tobytes() == want_bits.tobytes(), form
        X.assert_within(want_bits, want, scale, letter, "oracle")
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
        assert _freeze(gpu, dev) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvFrozenBytes(gpu) > 0
        for form in (capi.FORM_GATHER, capi.FORM_STRIPS, capi.FORM_AUTO):
            capi.spgpuSetSpmvForm(gpu, form)
            for call in range(3):
                uses = capi.plan_counts(gpu)[0]
                got = _call(gpu, dev, x, y, alpha, beta)
                if form != capi.FORM_AUTO:
                    assert capi.plan_counts(gpu)[0] == uses + 1, (form, call)        # the packed kernel ran
                assert got.tobytes() == unfrozen[form].tobytes(), (form, call)
                X.assert_within(got, want, scale, letter, ("frozen", form, call, base))
    finally:
        capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
        capi.spgpuSpmvThaw(gpu, _p(dev.rP))
    assert capi.spgpuSpmvFrozenBytes(gpu) == 0


@pytest.mark.parametrize("letter", ["D", "S"])
def test_unordered_escape_share_rule(gpu, tuning, letter):
    """Exactly one escape in a hundred entries is kept, one more is not (escapes * 100 <= entries * SPGPU_FREEZE_MAX_ESCAPES_PCT)."""
    from spgpu_amd import capi, formats
    tuning(SPGPU_FREEZE_MAX_ESCAPES_PCT=1)
    n = 2500                                  # 20 000 entries: 200 escapes allowed
    for extra, expected in ((200, capi.SPGPU_SUCCESS), (201, capi.SPGPU_UNSUPPORTED)):
        rows, cols = _band_with_edges(letter, n, 0, planted=0, extra_escapes=extra)
        entries, escapes = X.unordered_escapes(n, rows, cols, letter)
        assert (entries, escapes) == (20_000, extra)
        vals = _values(letter, rows.size, 6)
        hell = formats.ell_to_hell(formats.coo_to_ell(n, rows, cols, vals), 32)
        dev = formats.DeviceHell(hell)
        x = _values(letter, 150_000, 7)
        try:
            assert _freeze(gpu, dev) == expected, (entries, escapes)
            assert (capi.spgpuSpmvFrozenBytes(gpu) > 0) == (expected == capi.SPGPU_SUCCESS)
            capi.spgpuSetSpmvForm(gpu, capi.FORM_GATHER)
            got = _call(gpu, dev, x, None, 1.0, 0.0)
            assert got.tobytes() == O.default_spmv(hell, x, None, 1.0, 0.0).tobytes()
            want, scale = X.spmv(n, rows, cols, vals, x, None, 1.0, 0.0)
            X.assert_within(got, want, scale, letter, ("share", extra))
        finally:
            capi.spgpuSetSpmvForm(gpu, capi.FORM_AUTO)
            capi.spgpuSpmvThaw(gpu, _p(dev.rP))
        assert capi.spgpuSpmvFrozenBytes(gpu) == 0


# ---- with a row order: offsets from the block's base ------------------------------------------------------------------------

def _ordered_with_edges(letter, window, aligned, base, escapes=None, planted_every=97, seed=11):
    """An ordered matrix whose stored row i (original row r_idx[i]) starts at column c0 = 20 000 * (i // 2048) and ends within
    c0 + 41 200: every 1 024- or 2 048-row block then counts its words from c0 exactly.  Middle entries of every `planted_every`-th
    row are replaced by c0 + 65 533 .. 65 536, a far column and (base 1) a hole; or, with `escapes`, exactly that many rows get
    one middle entry at c0 + 65 535 and the total number of entries is a multiple of 100."""
    from spgpu_amd import formats
    n = 8 * 1024 + 77
    rng = np.random.default_rng(seed)
    lengths = np.minimum(8 + (3.0 * rng.random(n) ** -0.7).astype(np.int64), 200)      # no sub-group deeper than the cap
    if escapes is not None:
        lengths[-1] += (-int(lengths.sum())) % 100
    r_idx, sorted_lengths = formats.oell_order(lengths, window=window, long_rows=0, aligned=aligned)
    rows = np.repeat(np.arange(n, dtype=np.int64), sorted_lengths)
    start = np.repeat(np.cumsum(sorted_lengths) - sorted_lengths, sorted_lengths)
    k = np.arange(rows.size, dtype=np.int64) - start
    c0 = 20_000 * (rows // 2048)
    cols = c0 + (rows % 2048) * 20 + k
    cols[k == 0] = c0[k == 0]
    first = np.cumsum(sorted_lengths) - sorted_lengths
    if escapes is None:
        for i in range(3, n, planted_every):
            at = first[i] + 1
            base_col = 20_000 * (i // 2048)
            cols[at: at + 6] = [base_col + e for e in EDGE] + [base_col + 130_000, -1 if base else base_col + 140_000]
    else:
        for i in np.linspace(0, n - 1, escapes).astype(np.int64) if escapes else []:
            cols[first[i] + 1] = 20_000 * (i // 2048) + 65535
    vals = _values(letter, rows.size, seed + 1)
    assert cols.max() < 230_000                     # the length of x in the tests below
    return n, rows, cols, vals, r_idx


def _ordered_escapes(rows, cols):
    c0 = 20_000 * (rows // 2048)
    off = cols - c0
    return int(rows.size), int(np.count_nonzero((cols < 0) | (off < 0) | (off >= 0xFFFF)))


@pytest.mark.parametrize("letter", ["D", "S", "C"])
@pytest.mark.parametrize("window,aligned", [(2048, True), (512, False)])     # the 2 048-row staged shape / the 1 024-row shape
@pytest.mark.parametrize("base", [0, 1])
def test_ordered_frozen_at_the_16_bit_limit(gpu, letter, window, aligned, base):
    from spgpu_amd import capi, formats
    n, rows, cols, vals, r_idx = _ordered_with_edges(letter, window, aligned, base)
    entries, escapes = _ordered_escapes(rows, cols)
    assert 0 < escapes and X.freeze_keeps(entries, escapes), (entries, escapes)
    ell = formats.coo_to_ell(n, rows + base, cols + base, vals, coo_base=base, ell_base=base)
    hell = formats.ell_to_hell(ell, 32)
    dev = formats.DeviceHell(hell, r_idx=r_idx)
    x, y = _values(letter, 230_000, 8), _values(letter, n, 9)
    alpha, beta = _scalars(letter)
    want_bits = O.spmv_tail(hell, x, y, alpha, beta, r_idx=r_idx, **O.slab_shape(letter, "ragged", deep_cap=O.DEEP_CAP))
    want, scale = X.spmv(n, rows, cols, vals, x, y, alpha, beta, r_idx=r_idx)
    X.assert_within(want_bits, want, scale, letter, "oracle")
    assert _call(gpu, dev, x, y, alpha, beta).tobytes() == want_bits.tobytes()
    try:
        assert _freeze(gpu, dev) == capi.SPGPU_SUCCESS
        assert capi.spgpuSpmvFrozenBytes(gpu) > 0
        for call in range(3):
            uses = capi.plan_counts(gpu)[0]
            got = _call(gpu, dev, x, y, alpha, beta)
            assert capi.plan_counts(gpu)[0] == uses + 1
            assert got.tobytes() == want_bits.tobytes(), call
            X.assert_within(got, want, scale, letter, ("frozen", window, call, base))
    finally:
        capi.spgpuSpmvThaw(gpu, _p(dev.rP))
    assert capi.spgpuSpmvFrozenBytes(gpu) == 0


def test_ordered_escape_share_rule(gpu, tuning):
    """The same rule with a row order: at 1 % the copy is kept; one escape more and Freeze says SPGPU_UNSUPPORTED, holds no memory,
    and the matrix keeps its plan (the next call runs from it)."""
    from spgpu_amd import capi, formats
    tuning(SPGPU_FREEZE_MAX_ESCAPES_PCT=1)
    letter = "D"
    for extra in (0, 1):
        n, rows, cols, vals, r_idx = _ordered_with_edges(letter, 2048, True, 0, escapes=1)     # (the count fixes the entries)
        allowed = rows.size // 100
        n, rows, cols, vals, r_idx = _ordered_with_edges(letter, 2048, True, 0, escapes=allowed + extra)
        entries, escapes = _ordered_escapes(rows, cols)
        assert entries % 100 == 0 and escapes == entries // 100 + extra, (entries, escapes)
        hell = formats.ell_to_hell(formats.coo_to_ell(n, rows, cols, vals), 32)
        dev = formats.DeviceHell(hell, r_idx=r_idx)
        x = _values(letter, 230_000, 12)
        want_bits = O.spmv_tail(hell, x, None, 1.0, 0.0, r_idx=r_idx, **O.slab_shape(letter, "ragged", deep_cap=O.DEEP_CAP))
        try:
            said = _freeze(gpu, dev)
            assert said == (capi.SPGPU_SUCCESS if extra == 0 else capi.SPGPU_UNSUPPORTED), (entries, escapes, said)
            assert (capi.spgpuSpmvFrozenBytes(gpu) > 0) == (extra == 0)
            uses = capi.plan_counts(gpu)[0]
            got = _call(gpu, dev, x, None, 1.0, 0.0)
            assert capi.plan_counts(gpu)[0] == uses + 1               # frozen or not, the call ran from the plan
            assert got.tobytes() == want_bits.tobytes()
        finally:
            capi.spgpuSpmvThaw(gpu, _p(dev.rP))
        assert capi.spgpuSpmvFrozenBytes(gpu) == 0


# ---- rows of 65 534 entries and more ---------------------------------------------------------------------------------------

class _OnDevice:
    """A HELL matrix built on the device (formats.coo_to_ordered_hell_device) behind the DeviceHell call interface."""

    def __init__(self, h, letter, n):
        self.letter, self.rows, self.hack_size, self.base = letter, n, h["hack_size"], h["base"]
        self.cM, self.rP, self.hack_offsets, self.rS, self.rIdx = h["cM"], h["rP"], h["hack_offsets"], h["rS"], h["rIdx"]
        self.host = dict(letter=letter, rows=n, values=h["cM"][:h["slots"]].cpu().numpy(), indices=h["rP"][:h["slots"]].cpu().numpy(),
                         hack_offsets=h["hack_offsets"].cpu().numpy(), hack_size=h["hack_size"], row_lengths=h["rS"][:n].cpu().numpy(),
                         base=h["base"])
        self.r_idx = None if h["rIdx"] is None else h["rIdx"][:n].cpu().numpy()

    def spmv(self, handle, z, y, alpha, x, beta):
        from spgpu_amd import capi
        L = self.letter
        capi.hellspmv[L](handle, _p(z), _p(y), capi.scalar(L, alpha), _p(self.cM), _p(self.rP), self.hack_size, _p(self.hack_offsets),
                         _p(self.rS), _p(self.rIdx), 0, self.rows, _p(x), capi.scalar(L, beta), self.base)


@pytest.mark.parametrize("letter", ["D", "S"])
def test_rows_around_65535_entries(gpu, tuning, letter):
    """Rows of 65 534, 65 535, 65 536 and 70 001 entries among short ones: unplanned, planned, frozen (ordered), adopted (as they
    come) -- the oracle's bits where the order of additions is pinned, and the bound everywhere."""
    import torch
    from spgpu_amd import capi, formats
    n, cols_n = 4096, 72_000
    rng = np.random.default_rng(21)
    lengths = rng.integers(1, 12, n).astype(np.int64)
    for r, length in {5: 65534, 700: 65535, 2100: 65536, 3999: 70001}.items():
        lengths[r] = length
    rows = np.repeat(np.arange(n, dtype=np.int64), lengths)
    k = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    cols = (rows * 17 + k) % cols_n                          # a long row walks nearly all of x, consecutively (wrapping)
    vals = _values(letter, rows.size, 22)
    x, y = _values(letter, cols_n, 23), _values(letter, n, 24)
    alpha, beta = 0.5, -2.0
    want, scale = X.spmv(n, rows, cols, vals, x, y, alpha, beta)
    coo = (torch.from_numpy(rows.astype(np.int32)).cuda(), torch.from_numpy(cols.astype(np.int32)).cuda(), torch.from_numpy(vals).cuda())
    # ordered by length in one sort (the long rows go first: deep sub-groups)
    dev = _OnDevice(formats.coo_to_ordered_hell_device(gpu, n, *coo, letter, 32, 0, 0), letter, n)
    assert sorted(dev.host["row_lengths"][:4].tolist()) == [65534, 65535, 65536, 70001]
    want_bits = O.spmv_tail(dev.host, x, y, alpha, beta, r_idx=dev.r_idx, **O.slab_shape(letter, "ragged", deep_cap=O.DEEP_CAP))
    X.assert_within(want_bits, want, scale, letter, "oracle")
    tuning(SPGPU_PLAN=0)
    got = _call(gpu, dev, x, y, alpha, beta)
    assert got.tobytes() == want_bits.tobytes(), "unplanned"
    tuning(SPGPU_PLAN=1, SPGPU_FREEZE_MAX_ESCAPES_PCT=100)
    for call in range(2):                                    # the first call analyses, the second runs from the plan
        got = _call(gpu, dev, x, y, alpha, beta)
        assert got.tobytes() == want_bits.tobytes(), ("planned", call)
    X.assert_within(got, want, scale, letter, "planned")
    try:
        assert _freeze(gpu, dev) == capi.SPGPU_SUCCESS
        got = _call(gpu, dev, x, y, alpha, beta)
        assert got.tobytes() == want_bits.tobytes(), "frozen"
    finally:
        capi.spgpuSpmvThaw(gpu, _p(dev.rP))
    # as they come, adopted: the bits of the same rows ordered with the device calls Adopt makes, and the bound
    plain = _OnDevice(formats.coo_to_ordered_hell_device(gpu, n, *coo, letter, 32, 0, 0, order=False), letter, n)
    own = _OnDevice(formats.coo_to_ordered_hell_device(gpu, n, *coo, letter, 32, 2048, 256, aligned=True), letter, n)
    mine = _call(gpu, own, x, y, alpha, beta)
    X.assert_within(mine, want, scale, letter, "ordered by the caller")
    try:
        assert capi.spgpuHellSpmvAdopt(gpu, capi.TYPE_CODE[letter], _p(plain.cM), _p(plain.rP), 32, _p(plain.hack_offsets), _p(plain.rS), n,
                                       0) == capi.SPGPU_SUCCESS
        uses = capi.spgpuSpmvAdoptedUses(gpu)
        got = _call(gpu, plain, x, y, alpha, beta)
        assert capi.spgpuSpmvAdoptedUses(gpu) == uses + 1
        assert got.tobytes() == mine.tobytes(), "adopted"
        X.assert_within(got, want, scale, letter, "adopted")
    finally:
        capi.spgpuSpmvThaw(gpu, _p(plain.rP))
    assert capi.spgpuSpmvFrozenBytes(gpu) == 0
