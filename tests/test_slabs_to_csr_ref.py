"""CPU: formats.slabs_to_csr, the numpy restatement of include/spgpu/ext/to_csr_device.h that the GPU tests may lean on, pinned
independently of the device code: on the ELL / HELL arrays each set of host converters builds (the product's, the oracle's and,
where it was built, the reference's own) it must give synth.coo_to_csr of the COO listing -- without a row order, and with a
random permutation as rIdx on the arrays of the permuted matrix."""
import numpy as np
import pytest

from spgpu_amd import formats, synth
from test_gpu_convert_device import _hosts

N_ROWS, N_COLS = 211, 40          # few columns: duplicates inside the rows


def _matrix(letter, base):
    rng = np.random.default_rng(31 + ord(letter))
    lengths = rng.integers(0, 70, N_ROWS)
    lengths[[0, 1, 2, N_ROWS - 2, N_ROWS - 1]] = 0            # empty rows at both ends
    _, _, r, c, v = synth.random_rows_coo(N_ROWS, N_COLS, lengths, seed=77, letter=letter, base=base, shuffle=True)
    return lengths, r, c, v


def _same_csr(got, want):
    for a, b, name in zip(got, want, ("row_ptr", "cols", "vals")):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("src_base,csr_base", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_restatement_gives_the_csr_of_the_coo_listing(letter, src_base, csr_base):
    lengths, r, c, v = _matrix(letter, src_base)
    assert (np.bincount(r - src_base, minlength=N_ROWS) == lengths).all() and len(set(zip(r.tolist(), c.tolist()))) < r.size
    want_ptr, want_cols, want_vals = synth.coo_to_csr(N_ROWS, r, c, v, src_base)
    want = ((want_ptr - src_base + csr_base).astype(np.int32), (want_cols - src_base + csr_base).astype(np.int32), want_vals)
    perm = np.random.default_rng(5).permutation(N_ROWS).astype(np.int32)      # storage row s holds matrix row perm[s]
    inverse = np.empty(N_ROWS, np.int64)
    inverse[perm] = np.arange(N_ROWS)
    r_stored = (inverse[r - src_base] + src_base).astype(np.int32)
    for name, host in _hosts():
        for r_idx, rows_in in ((None, r), (perm, r_stored)):
            ell = host.coo_to_ell(N_ROWS, rows_in, c, v, coo_base=src_base, ell_base=src_base)
            got = formats.slabs_to_csr(ell["values"], ell["indices"], ell["row_lengths"], N_ROWS, pitch=ell["pitch"], r_idx=r_idx,
                                       src_base=src_base, csr_base=csr_base)
            _same_csr(got, want)
            # the values at a pitch of their own
            wide = ell["pitch"] + 32
            values = np.zeros(ell["max_row"] * wide, ell["values"].dtype)
            values.reshape(ell["max_row"], wide)[:, :ell["pitch"]] = ell["values"].reshape(ell["max_row"], ell["pitch"])
            got = formats.slabs_to_csr(values, ell["indices"], ell["row_lengths"], N_ROWS, pitch=ell["pitch"], values_pitch=wide,
                                       r_idx=r_idx, src_base=src_base, csr_base=csr_base)
            _same_csr(got, want)
            for hs in (32, 24):
                hell = host.ell_to_hell(ell, hs)
                got = formats.slabs_to_csr(hell["values"], hell["indices"], hell["row_lengths"], N_ROWS, hack_offsets=hell["hack_offsets"],
                                           hack_size=hs, r_idx=r_idx, src_base=src_base, csr_base=csr_base)
                _same_csr(got, want)


def test_padding_is_never_looked_at():
    lengths, r, c, v = _matrix("D", 0)
    want = synth.coo_to_csr(N_ROWS, r, c, v, 0)
    hell = formats.ell_to_hell(formats.coo_to_ell(N_ROWS, r, c, v), 32)
    hs, rr = 32, np.arange(N_ROWS)
    stored = np.zeros(hell["values"].size, bool)
    for k in range(int(lengths.max())):
        rows = rr[lengths > k]
        stored[hell["hack_offsets"].astype(np.int64)[rows // hs] + rows % hs + k * hs] = True
    values, indices = hell["values"].copy(), hell["indices"].copy()
    values[~stored], indices[~stored] = np.nan, 0x7FFFFFFF
    _same_csr(formats.slabs_to_csr(values, indices, hell["row_lengths"], N_ROWS, hack_offsets=hell["hack_offsets"], hack_size=hs), want)


def test_no_rows_and_no_entries():
    ptr, cols, vals = formats.slabs_to_csr(np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, pitch=32, csr_base=1)
    assert ptr.tolist() == [1] and cols.size == 0 and vals.size == 0 and vals.dtype == np.float32
    ptr, cols, vals = formats.slabs_to_csr(np.zeros(0), np.zeros(0, np.int32), np.zeros(5, np.int32), 5, hack_offsets=np.zeros(1, np.int32),
                                           hack_size=32)
    assert ptr.tolist() == [0] * 6 and cols.size == 0 and vals.size == 0
