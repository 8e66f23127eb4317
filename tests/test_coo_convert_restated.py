"""CPU: the listings of tests/coo_convert_cases.py, twice over.

(a) Each case reaches what it claims: the length of the scan it drives and its number of 1 024-element tiles (more than 256 where
the scan is meant to carry, the named number at the tile edges), the largest HDIA diagonal key as a Python integer and its low word
(at least 2^31 in the wide cases), the row counts either side of a power of two with the width of their sort key, the number of
writers of the most contended slot.

(b) The host converters -- formats.coo_to_ell, ell_to_hell, coo_to_hdia, coo_to_dia, pinned to the reference's build by
tests/test_oracle_vs_reference.py -- against a restatement written here from the contract in include/spgpu/convert_device.h and
nothing else: one dict keyed by the Python-int pair (row, column) whose lists hold COO positions in encounter order.  ELL and HELL
store the k-th entry of a row in COO order at depth k; HDIA and DIA store the last entry of a pair's list.  No 32-bit arithmetic
takes part, so the wide and the large cases stand on their own.  tests/test_gpu_zz_coo_convert_shapes.py imports the restatements
from here: where they say a slot is occupied the device must have written it, and nowhere else."""
import numpy as np
import pytest

import coo_convert_cases as K
from spgpu_amd import capi, formats


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def book(case):
    """{(row, column): [COO positions, ascending]} with 0-based Python ints."""
    pairs = {}
    for at, (r, c) in enumerate(zip(case.rows.tolist(), case.cols.tolist())):
        pairs.setdefault((r - case.coo_base, c - case.coo_base), []).append(at)
    return pairs


def most_writers(pairs):
    return max(len(v) for v in pairs.values())


def ell_by_the_book(case, out_base, values_pitch=None, indices_pitch=None):
    """dict: row_lengths, max_row, pitches, the ELL slot of every COO position (values and indices) and the column index stored."""
    n = case.n_rows
    depth_of, lengths = [0] * case.rows.size, [0] * n
    for at, r in enumerate(case.rows.tolist()):              # ascending COO position: the k-th entry of a row gets depth k
        depth_of[at] = lengths[r - case.coo_base]
        lengths[r - case.coo_base] += 1
    pitch = (n + 31) // 32 * 32
    values_pitch, indices_pitch = values_pitch or pitch, indices_pitch or pitch
    row = case.rows.astype(np.int64) - case.coo_base
    depth = np.array(depth_of, np.int64)
    stored = case.cols.astype(np.int64) - case.coo_base + out_base
    assert stored.size == 0 or (stored.min() >= 0 and stored.max() <= 2 ** 31 - 1)
    return dict(row_lengths=np.array(lengths, np.int32), max_row=max(lengths, default=0), values_pitch=values_pitch,
                indices_pitch=indices_pitch, row=row, depth=depth, value_slots=row + depth * values_pitch,
                index_slots=row + depth * indices_pitch, stored=stored.astype(np.int32))


def hell_by_the_book(ell, hack_size):
    """dict: hack_offsets (one per hack), height, the HELL slot of every COO position."""
    lengths = ell["row_lengths"].tolist()
    offsets, at = [], 0
    for first in range(0, len(lengths), hack_size):
        offsets.append(at)
        at += hack_size * max(lengths[first:first + hack_size])
    offsets_of = np.array(offsets + [0], np.int64)
    assert at % hack_size == 0 and at <= 2 ** 31 - 1
    slots = offsets_of[ell["row"] // hack_size] + ell["row"] % hack_size + ell["depth"] * hack_size
    return dict(hack_offsets=np.array(offsets, np.int32), height=at // hack_size, slots=slots, slot_count=at)


def hdia_by_the_book(case, pairs, hack_size):
    """dict: hack_offsets (hacks + 1), height, offsets, the slot of every distinct pair with the COO position stored there, the
    largest (hack << 32) | (column - row % hackSize + hackSize) key of the device plan, the diagonals of every hack."""
    hacks = (case.n_rows + hack_size - 1) // hack_size
    diagonals = [set() for _ in range(hacks)]
    for r, c in pairs:
        diagonals[r // hack_size].add(c - r)
    diagonals = [sorted(d) for d in diagonals]
    hack_offsets = [0]
    for d in diagonals:
        hack_offsets.append(hack_offsets[-1] + len(d))
    place = [{d: p for p, d in enumerate(ds)} for ds in diagonals]
    slots = [(hack_offsets[r // hack_size] + place[r // hack_size][c - r]) * hack_size + r % hack_size for r, c in pairs]
    owners = [positions[-1] for positions in pairs.values()]
    keys = [((r // hack_size) << 32) | (c - r % hack_size + hack_size) for r, c in pairs]
    return dict(hack_offsets=np.array(hack_offsets, np.int32), height=hack_offsets[-1], per_hack=[len(d) for d in diagonals],
                offsets=np.array([d for ds in diagonals for d in ds], np.int64).astype(np.int32), slots=np.array(slots, np.int64),
                owners=np.array(owners, np.int64), largest_key=max(keys, default=0), largest_low_word=max((k & 0xFFFFFFFF for k in keys), default=0),
                slot_count=hack_size * hack_offsets[-1])


def dia_by_the_book(case, pairs, pitch=None):
    pitch = pitch or (case.n_rows + 31) // 32 * 32
    offsets = sorted({c - r for r, c in pairs})
    place = {d: p for p, d in enumerate(offsets)}
    slots = [r + place[c - r] * pitch for r, c in pairs]
    owners = [positions[-1] for positions in pairs.values()]
    return dict(diags=len(offsets), pitch=pitch, offsets=np.array(offsets, np.int64).astype(np.int32), slots=np.array(slots, np.int64),
                owners=np.array(owners, np.int64), slot_count=pitch * len(offsets),
                flags=sorted(d + case.n_rows - 1 for d in offsets))


def filled(slot_count, dtype, slots, what, background=0):
    """An array of `slot_count` elements whose every byte is `background`, with what[i] at slots[i]."""
    out = np.full(slot_count * np.dtype(dtype).itemsize, background, np.uint8).view(dtype)
    assert slots.size == 0 or (slots.min() >= 0 and slots.max() < slot_count)
    out[slots] = what
    return out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


# ---- the host converters against it --------------------------------------------------------------------------------------------
def check_ell_and_hell(case, out_base, hack_sizes):
    ell = ell_by_the_book(case, out_base)
    host = formats.coo_to_ell(case.n_rows, case.rows, case.cols, case.vals, coo_base=case.coo_base, ell_base=out_base)
    assert host["max_row"] == ell["max_row"] and host["pitch"] == ell["values_pitch"] == capi.computeEllAllocPitch(case.n_rows)
    _same(host["row_lengths"], ell["row_lengths"], "row lengths")
    _same(host["values"], filled(ell["max_row"] * ell["values_pitch"], case.vals.dtype, ell["value_slots"], case.vals), "ELL values")
    _same(host["indices"], filled(ell["max_row"] * ell["indices_pitch"], np.int32, ell["index_slots"], ell["stored"]), "ELL indices")
    for hack_size in hack_sizes:
        hell = hell_by_the_book(ell, hack_size)
        host_hell = formats.ell_to_hell(host, hack_size)
        assert host_hell["height"] == hell["height"], hack_size
        _same(host_hell["hack_offsets"], hell["hack_offsets"], ("hack offsets", hack_size))
        _same(host_hell["values"], filled(hell["slot_count"], case.vals.dtype, hell["slots"], case.vals), ("HELL values", hack_size))
        _same(host_hell["indices"], filled(hell["slot_count"], np.int32, hell["slots"], ell["stored"]), ("HELL indices", hack_size))
    return ell


def check_hdia(case, hack_size=None):
    hack_size = hack_size or case.info["hack_size"]
    pairs = book(case)
    hdia = hdia_by_the_book(case, pairs, hack_size)
    host = formats.coo_to_hdia(case.n_rows, case.n_cols, case.rows, case.cols, case.vals, hack_size, coo_base=case.coo_base)
    assert host["height"] == hdia["height"]
    _same(host["hack_offsets"], hdia["hack_offsets"], "hack offsets")
    _same(host["offsets"], hdia["offsets"], "offsets")
    _same(host["values"], filled(hdia["slot_count"], case.vals.dtype, hdia["slots"], case.vals[hdia["owners"]]), "HDIA values")
    return pairs, hdia


def check_dia(case):
    pairs = book(case)
    dia = dia_by_the_book(case, pairs)
    host = formats.coo_to_dia(case.n_rows, case.n_cols, case.rows, case.cols, case.vals, coo_base=case.coo_base)
    assert host["diags"] == dia["diags"] and host["pitch"] == dia["pitch"] == capi.computeDiaAllocPitch(case.n_rows)
    _same(host["offsets"], dia["offsets"], "offsets")
    _same(host["values"], filled(dia["slot_count"], case.vals.dtype, dia["slots"], case.vals[dia["owners"]]), "DIA values")
    return pairs, dia


def test_values_name_their_position_and_are_never_zero():
    for letter in "SDCZ":
        v = K.values(100_400, letter)
        assert np.unique(v).size == v.size and (v.real == np.arange(1, v.size + 1)).all() and (v.view(np.uint8).reshape(v.size, -1) != 0).any(1).all()
        if letter in "CZ":
            assert (v.imag == -v.real).all()


# ---- ELL / HELL ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
def test_ell_base_pairs(letter):
    for coo_base, out_base in K.BASE_PAIRS:
        case = K.ell_base_pairs(letter, coo_base)
        ell = check_ell_and_hell(case, out_base, case.info["hack_sizes"])
        lengths = ell["row_lengths"]
        assert case.n_rows == 70 and not lengths[list(case.info["empty_rows"])].any() and lengths[0] and lengths[69]
        assert most_writers(book(case)) >= 2 and (np.diff(case.rows) < 0).any()                  # duplicates; not in row order
        assert int(ell["stored"].min()) == out_base and int(ell["stored"].max()) == 89 + out_base


@pytest.mark.parametrize("n_rows", K.ROW_COUNTS)
def test_ell_row_counts_around_powers_of_two(n_rows):
    assert sorted(K.ROW_COUNTS) == sorted(2 ** k + d for k in (8, 16) for d in (-1, 0, 1))
    bits = K.row_key_bits(n_rows)
    assert (1 << bits) > n_rows >= (1 << (bits - 1)) and bits == {255: 8, 256: 9, 257: 9, 65535: 16, 65536: 17, 65537: 17}[n_rows]
    for coo_base in (0, 1):
        case = K.ell_row_counts(n_rows, coo_base)
        ell = check_ell_and_hell(case, coo_base, (32,))
        assert ell["row_lengths"][0] and ell["row_lengths"][n_rows - 1] and case.info["key_bits"] == bits
        high, low = case.info["row_too_high"], case.info["row_too_low"]
        assert int(high.max()) == coo_base + n_rows and int(low.min()) == coo_base - 1
        assert (high != case.rows).sum() == 1 and (low != case.rows).sum() == 1


@pytest.mark.parametrize("coo_base", [0, 1])
def test_ell_wide_columns(coo_base):
    case = K.ell_wide_columns(coo_base)
    assert case.n_cols == 2 ** 31 - 1 and int(case.cols.max()) == 2 ** 31 - 2 + coo_base and int(case.cols.min()) == coo_base
    for out_base in (0, 1):
        ell = check_ell_and_hell(case, out_base, case.info["hack_sizes"])
        assert int(ell["stored"].max()) == 2 ** 31 - 2 + out_base


@pytest.mark.parametrize("hacks", K.HELL_PLAN_HACKS)
def test_hell_plan_at_the_tile_edge(hacks):
    case = K.hell_plan_hacks(hacks)
    assert case.info["hacks"] == hacks and case.info["scan_tiles"] == {1: 1, 1023: 1, 1024: 1, 1025: 2}[hacks]
    assert case.n_rows % case.info["hack_size"] != 0                                            # a partly filled last hack
    ell = check_ell_and_hell(case, 1 - case.coo_base, (case.info["hack_size"],))
    hs = case.info["hack_size"]
    assert ell["row_lengths"][:hs].any() and ell["row_lengths"][(hacks - 1) * hs:].any()


def test_hell_plan_scan_that_carries():
    case = K.hell_plan_carry()
    assert case.info["hack_size"] == 2 and case.n_rows == 524293 and case.info["hacks"] == 262147
    assert case.info["scan_tiles"] == 257 > K.CARRY_TILES
    ell = check_ell_and_hell(case, 0, (2,))
    assert ell["row_lengths"][:2].any() and ell["row_lengths"][-1] and ell["max_row"] == 3


@pytest.mark.parametrize("kind", ["no entries", "no rows", "one entry"])
def test_ell_degenerate(kind):
    case = K.ell_degenerate(kind)
    ell = check_ell_and_hell(case, 0, (32,))
    assert (case.n_rows, case.rows.size, ell["max_row"]) == {"no entries": (70, 0, 0), "no rows": (0, 0, 0), "one entry": (70, 1, 1)}[kind]


# ---- HDIA ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", "SDCZ")
@pytest.mark.parametrize("hack_size", K.HDIA_HACK_SIZES)
def test_hdia_shapes(letter, hack_size):
    assert [hs % 32 for hs in K.HDIA_HACK_SIZES] == [0, 0, 0, 24]
    for n_rows in K.hdia_row_counts(hack_size):
        for coo_base, wide in ((0, True), (1, False), (1, True), (0, False)):
            case = K.hdia_shape(hack_size, n_rows, letter, coo_base, wide)
            assert (case.n_cols > n_rows) == wide or n_rows == 1
            pairs, hdia = check_hdia(case)
            offsets = set(hdia["offsets"].tolist())
            assert -(n_rows - 1) in offsets and case.n_cols - 1 in offsets and most_writers(pairs) >= 2
            if n_rows == 3 * hack_size + 5:
                assert len(hdia["per_hack"]) == 4 and hdia["per_hack"][1] == 0 and hdia["per_hack"][2] == 1
                assert hdia["per_hack"][0] > 1 and hdia["per_hack"][3] > 1


def test_hdia_single_entry():
    for coo_base in (0, 1):
        pairs, hdia = check_hdia(K.hdia_single_entry(coo_base))
        assert hdia["per_hack"] == [0, 1, 0] and hdia["offsets"].tolist() == [-37] and hdia["slots"].tolist() == [8]


@pytest.mark.parametrize("hack_size", K.HDIA_WIDE_HACK_SIZES)
def test_hdia_wide_keys(hack_size):
    for coo_base in (0, 1):
        case = K.hdia_wide(hack_size, coo_base)
        pairs, hdia = check_hdia(case)
        assert case.n_rows == 70 and case.n_cols == 2 ** 31 - 1 and int(case.cols.max()) == 2 ** 31 - 2 + coo_base
        # the largest key: last hack of 70 rows, the last column seen from the first row of that hack
        last_hack = 69 // hack_size
        assert hdia["largest_key"] == (last_hack << 32) | (2 ** 31 - 2 + hack_size)
        assert hdia["largest_low_word"] == 2 ** 31 - 2 + hack_size >= 2 ** 31
        low_words = [c - r % hack_size + hack_size for r, c in pairs]
        assert sum(w >= 2 ** 31 for w in low_words) > 50 and sum(w < 2 ** 31 for w in low_words) > 50      # both sides of the edge
        assert {r % hack_size for r, c in pairs if c == 2 ** 31 - 2} >= {0, 1, hack_size // 2, hack_size - 1}
        assert int(hdia["offsets"].max()) == 2 ** 31 - 2 and 0 in {c for _, c in pairs}


def test_hdia_contention():
    case = K.hdia_contention()
    pairs, hdia = check_hdia(case)
    slot = case.info["slot"]
    assert most_writers(pairs) == len(pairs[slot]) >= 100_000 and 300 < case.rows.size - 100_000 < 600
    assert np.abs(np.diff(np.array(pairs[slot][:200]))).max() > 1                              # shuffled among the others
    back = K.reversed_listing(case)
    back_pairs, back_hdia = check_hdia(back)
    stored, stored_back = case.vals[pairs[slot][-1]], back.vals[back_pairs[slot][-1]]
    assert stored != stored_back and stored_back == case.vals[pairs[slot][0]]                  # the other end of the list wins
    assert stored.real == pairs[slot][-1] + 1 == max(pairs[slot]) + 1


@pytest.mark.parametrize("coo_base", [0, 1])
def test_hdia_refused_listings(coo_base):
    case = K.hdia_refused(coo_base)
    check_hdia(case)
    for kind in K.OUTSIDE:
        bad = K.spoilt(case, kind)
        r, c = bad.rows.astype(np.int64) - coo_base, bad.cols.astype(np.int64) - coo_base
        outside = (r < 0) | (r >= case.n_rows) | (c < 0) | (c >= case.n_cols)
        assert outside.sum() == 1 and outside[17], kind


# ---- DIA -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", K.DIA_SPANS)
def test_dia_spans_at_the_tile_edge(span):
    for letter, coo_base in (("D", 0), ("C", 1)):
        case = K.dia_span(span, coo_base, letter)
        pairs, dia = check_dia(case)
        assert case.n_rows + case.n_cols - 1 == span and case.info["scan_tiles"] == {1023: 1, 1024: 1, 1025: 2, 1026: 2}[span]
        assert dia["flags"][0] == 0 and dia["flags"][-1] == span - 1 and most_writers(pairs) >= 2
        assert {f for f in (1022, 1023, 1024) if f < span - 1} <= set(dia["flags"])


def test_dia_scan_that_carries():
    case = K.dia_carry()
    pairs, dia = check_dia(case)
    span = case.n_rows + case.n_cols - 1
    assert span == 270_000 and case.info["scan_tiles"] == 264 > K.CARRY_TILES and dia["diags"] == 8
    edge = K.TILE * K.CARRY_TILES
    assert dia["flags"][0] == 0 and dia["flags"][-1] == span - 1 and {edge - 1, edge} <= set(dia["flags"])
    assert 250_000 < case.rows.size < 350_000 and dia["slot_count"] > case.rows.size          # partly filled


def test_dia_contention():
    case = K.dia_contention()
    pairs, dia = check_dia(case)
    slot = case.info["slot"]
    assert most_writers(pairs) == len(pairs[slot]) >= 50_000
    back = K.reversed_listing(case)
    back_pairs, _ = check_dia(back)
    assert case.vals[pairs[slot][-1]] != back.vals[back_pairs[slot][-1]] == case.vals[pairs[slot][0]]


@pytest.mark.parametrize("coo_base", [0, 1])
def test_dia_refused_listings(coo_base):
    case = K.dia_refused(coo_base)
    check_dia(case)
    for kind in K.OUTSIDE:
        bad = K.spoilt(case, kind)
        r, c = bad.rows.astype(np.int64) - coo_base, bad.cols.astype(np.int64) - coo_base
        assert ((r < 0) | (r >= case.n_rows) | (c < 0) | (c >= case.n_cols)).sum() == 1, kind
