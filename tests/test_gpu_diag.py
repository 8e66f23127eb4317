"""GPU: diagonal extraction (include/spgpu/ext/precond.h, spgpu_amd/csrc/diag_extract.hip: spgpu{S,D}hellDiag, spgpu{S,D}ellDiag,
spgpu{S,D}hdiaDiag).

ELL and HELL matrices are built by hand in numpy, so that the test owns every slot: rows of 0 ... 9 entries, among them rows
without a diagonal entry, rows whose diagonal is the last live slot, rows that store the diagonal twice and one row whose diagonal
value is 0; every padding slot (beyond rS[i]) holds NaN under the column of its own row, and must never count.  The expected
diagonal is summed slot by slot in ascending k in the matrix' dtype, then inverted as dtype(1) / d; at most one addition per row
rounds (the diagonal is stored at most twice), so numpy gives the kernel's bits and the comparison is byte for byte.  HDIA matrices
come from the library's own cooToHdia.  Around d the elements before d[0] and after d[rows - 1] keep a sentinel."""
import numpy as np
import pytest

import exact_ref as X
import test_gpu_fused_shapes as F            # _start / _guard / _place / _assert_margins / _same_bytes: one list of raised calls for both files

pytestmark = pytest.mark.gpu

LETTERS = "SD"
SHAPES = [(1, 32), (33, 32), (70, 32), (70, 64), (70, 6)]       # (rows, hackSize); 6: no 16-byte index loads
ZERO_ROW = 5                                                   # its diagonal is stored, and is 0
_p = F._p


def _rows(rows, dtype, seed):
    """Per row the list of (column, value) in storage order, 0-based columns below rows + 16."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(rows):
        length = (i * 7 + 3) % 10                                # 0 ... 9, mixed; row 0 has 3
        others = [(i + 1 + j) % (rows + 16) for j in range(length)]
        assert i not in others
        cols = list(others)
        kind = i % 5
        if length and kind == 0:
            cols[length - 1] = i                                 # the diagonal is the last live slot
        elif length >= 2 and kind == 1:
            cols[0], cols[length - 1] = i, i                     # stored twice, first and last slot
        elif length and kind == 2:
            cols[length // 2] = i                                # in the middle
        # kinds 3, 4 and the rows of length 0: no diagonal entry
        vals = rng.uniform(0.5, 2.0, length).astype(dtype) * rng.choice(np.array([-1, 1], dtype), length)
        if i == ZERO_ROW and length:
            cols[0] = i
            vals[[k for k, c in enumerate(cols) if c == i]] = 0
        out.append(list(zip(cols, vals)))
    if rows > ZERO_ROW:
        kinds = {"none": any(all(c != i for c, _ in r) for i, r in enumerate(out)),
                 "last": any(r and r[-1][0] == i for i, r in enumerate(out)),
                 "twice": any(sum(c == i for c, _ in r) == 2 for i, r in enumerate(out)),
                 "zero": any(c == ZERO_ROW and v == 0 for c, v in out[ZERO_ROW]),
                 "empty": any(not r for r in out)}
        assert all(kinds.values()), kinds
    assert max(sum(c == i for c, _ in r) for i, r in enumerate(out)) <= 2     # one rounding addition at the most
    return out


def _expected(rows_list, dtype, invert):
    d = np.zeros(len(rows_list), dtype)
    for i, entries in enumerate(rows_list):
        s = dtype(0)
        for c, v in entries:                                     # ascending slot k
            if c == i:
                s = dtype(s + v)
        d[i] = s
    if invert:
        with np.errstate(divide="ignore"):
            d = (dtype(1) / d).astype(dtype)
    return d


def _hell(rows_list, hack, base, dtype):
    rows = len(rows_list)
    hacks = -(-rows // hack)
    depth = [max((len(rows_list[r]) for r in range(h * hack, min(rows, (h + 1) * hack))), default=0) for h in range(hacks)]
    depth = [d + 1 for d in depth]                               # one more slot column: every row has padding
    offsets = np.concatenate(([0], np.cumsum([hack * d for d in depth]))).astype(np.int32)
    cM, rP = np.full(offsets[-1], np.nan, dtype), np.zeros(offsets[-1], np.int32)
    for h in range(hacks):
        for local in range(hack):
            r = h * hack + local
            for k in range(depth[h]):
                slot = offsets[h] + local + k * hack
                rP[slot] = r + base                              # padding: NaN under the row's own column
                if r < rows and k < len(rows_list[r]):
                    rP[slot], cM[slot] = rows_list[r][k][0] + base, rows_list[r][k][1]
    return cM, rP, offsets[:hacks].copy()


def _ell(rows_list, c_pitch, r_pitch, base, dtype, live_padding):
    """live_padding (rS == NULL, every slot counts): the padding is NaN under a column that is NOT the row's."""
    rows, depth = len(rows_list), 10
    cM, rP = np.full(depth * c_pitch, np.nan, dtype), np.zeros(depth * r_pitch, np.int32)
    for r in range(r_pitch):
        for k in range(depth):
            rP[k * r_pitch + r] = r + base + (1 if live_padding else 0)
            if r < rows and k < len(rows_list[r]):
                rP[k * r_pitch + r], cM[k * c_pitch + r] = rows_list[r][k][0] + base, rows_list[r][k][1]
    return cM, rP, depth


def _check(cid, letter, rows, call, expected):
    """call(d): runs the library call on d; d lies one element past a 16-byte boundary."""
    dtype = X.REAL_OF[letter]
    d_buf, d = F._place(np.full(rows, F.SENTINEL, dtype), 1)
    call(d)
    F._same_bytes(F._assert_margins(d_buf, 1, rows, f"{cid}: d"), expected, f"{cid}: d")


@pytest.mark.parametrize("rows,hack", SHAPES, ids=[f"rows{r}-hack{h}" for r, h in SHAPES])
@pytest.mark.parametrize("letter", LETTERS)
def test_hell_diag(gpu, letter, rows, hack):
    import torch
    from spgpu_amd import capi
    F._start()
    dtype = X.REAL_OF[letter]
    rows_list = _rows(rows, dtype, 100 + rows + hack)
    lengths = np.array([len(r) for r in rows_list], np.int32)
    for base in (0, 1):
        cM_h, rP_h, offsets_h = _hell(rows_list, hack, base, dtype)
        cM, rS, offsets = F._place(cM_h, 0)[1], F._place(lengths, 1)[1], torch.from_numpy(offsets_h).to("cuda:0")
        for off in (0, 1):                                       # rP on and off the 16-byte boundary
            rP = F._place(rP_h, off)[1]
            for invert in (0, 1):
                cid = f"{letter}-hell-rows{rows}-hack{hack}-base{base}-off{off}-invert{invert}"
                _check(cid, letter, rows, lambda d: F._guard(cid, capi.hell_diag[letter], gpu, _p(d), _p(cM), _p(rP), hack, _p(offsets),
                                                             _p(rS), rows, base, invert), _expected(rows_list, dtype, invert))


@pytest.mark.parametrize("with_rs", [True, False], ids=["rS", "noRS"])
@pytest.mark.parametrize("rows,hack", SHAPES, ids=[f"rows{r}-hack{h}" for r, h in SHAPES])
@pytest.mark.parametrize("letter", LETTERS)
def test_ell_diag(gpu, letter, rows, hack, with_rs):
    """The index pitch is a multiple of 4 (16-byte index loads possible) for the hackSize 32 / 64 shapes, odd for the hackSize 6 one."""
    from spgpu_amd import capi
    F._start()
    dtype = X.REAL_OF[letter]
    rows_list = _rows(rows, dtype, 200 + rows + hack)
    lengths = np.array([len(r) for r in rows_list], np.int32)
    r_pitch = (rows | 1) if hack == 6 else -(-rows // 4) * 4 + 4
    c_pitch = rows + 3
    for base in (0, 1):
        cM_h, rP_h, depth = _ell(rows_list, c_pitch, r_pitch, base, dtype, live_padding=not with_rs)
        cM = F._place(cM_h, 1)[1]
        rS = F._place(lengths, 1)[1] if with_rs else None
        for off in (0, 1):
            rP = F._place(rP_h, off)[1]
            for invert in (0, 1):
                cid = f"{letter}-ell-rows{rows}-pitch{r_pitch}-{'rS' if with_rs else 'noRS'}-base{base}-off{off}-invert{invert}"
                _check(cid, letter, rows, lambda d: F._guard(cid, capi.ell_diag[letter], gpu, _p(d), _p(cM), _p(rP), c_pitch, r_pitch, _p(rS),
                                                             depth, rows, base, invert), _expected(rows_list, dtype, invert))


def _hdia_coo(kind, rows):
    """(cols, coo rows, coo cols) of a banded matrix: offsets -2, 0, +3."""
    cols = 40 if kind == "tall" else rows
    r, c = [], []
    for i in range(rows):
        for off in (-2, 0, 3):
            j = i + off
            if not 0 <= j < cols:
                continue
            if off == 0 and kind == "gap" and 32 <= i < 64:        # the hack of rows 32 ... 63 stores no main diagonal
                continue
            if off == 0 and i % 7 == 3:                          # the diagonal is stored in the hack, this row has no entry on it
                continue
            r.append(i)
            c.append(j)
    return cols, np.array(r, np.int32), np.array(c, np.int32)


@pytest.mark.parametrize("kind,rows", [("full", 33), ("full", 70), ("gap", 70), ("tall", 70)])
@pytest.mark.parametrize("letter", LETTERS)
def test_hdia_diag(gpu, letter, kind, rows):
    from spgpu_amd import capi, formats
    F._start()
    dtype = X.REAL_OF[letter]
    cols, r, c = _hdia_coo(kind, rows)
    v = np.random.default_rng(300 + rows).uniform(0.5, 2.0, r.size).astype(dtype)
    hdia = formats.coo_to_hdia(rows, cols, r, c, v, 32)
    per_hack = [set(hdia["offsets"][a:b]) for a, b in zip(hdia["hack_offsets"][:-1], hdia["hack_offsets"][1:])]
    assert [0 in s for s in per_hack] == {"full": [True] * len(per_hack), "gap": [True, False, True], "tall": [True, True, False]}[kind]
    want = np.zeros(rows, dtype)
    want[r[r == c]] = v[r == c]
    if kind == "tall":   # a slot whose column offsets[d] + r is not below cols contributes nothing, whatever it holds
        for hack, (a, b) in enumerate(zip(hdia["hack_offsets"][:-1], hdia["hack_offsets"][1:])):
            for diag in range(a, b):
                if hdia["offsets"][diag] == 0:
                    beyond = [i % 32 for i in range(hack * 32, min(rows, hack * 32 + 32)) if i >= cols]
                    hdia["values"][diag * 32 + np.array(beyond, np.int64)] = np.nan
        assert np.isnan(hdia["values"]).sum() == 64 - cols
    dev = formats.DeviceHdia(hdia)
    for invert in (0, 1):
        cid = f"{letter}-hdia-{kind}-rows{rows}-invert{invert}"
        with np.errstate(divide="ignore"):
            expected = (dtype(1) / want).astype(dtype) if invert else want
        _check(cid, letter, rows, lambda d: F._guard(cid, capi.hdia_diag[letter], gpu, _p(d), _p(dev.dM), _p(dev.offsets), 32,
                                                     _p(dev.hack_offsets), rows, cols, invert), expected)
