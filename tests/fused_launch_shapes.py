"""The constants of the host dispatch of the fused CG steps (spgpu_amd/csrc/fused_solver.hip: hellSpmvDot, axpbyPairDot, and the
wavefront-uniform strip choice of rowSums), that dispatch restated as functions of what a caller passes, and the case table
tests/test_gpu_fused_shapes.py runs -- stated once for that module (which runs the cases on the GPU) and for
tests/test_fused_launch_shapes.py (which checks on the CPU that the table reaches every branch, that each case reaches the branches
it is there for, and that the integer inputs of the exact cases add exactly).  No torch and no library at import: importable
everywhere.  The matrices and vectors of a case are built on demand (numpy; the project's host converters for all but the two
capped matrices)."""
import functools

import numpy as np

# ---- the constants of the dispatch: a change there is a test to revisit here ------------------------------------------------------
kL1Threads = 256                    # level1_grid.h    kL1Threads
kL1Unroll = 4                       # level1_grid.h    kL1Unroll: 16-byte accesses in flight per lane
SPGPU_REDUCE_MAX_BLOCKS = 1024      # spgpu_internal.h SPGPU_REDUCE_MAX_BLOCKS: block partials the handle's scratch holds
kWave = 64                          # numeric.hip.h    kWave: lanes that share one __ballot
TILE = kL1Threads * kL1Unroll       # packs one workgroup takes per trip of the tile-stride loop
LETTERS = "SD"
SIZEOF = {"S": 4, "D": 8}
WIDE = {L: 16 // SIZEOF[L] for L in LETTERS}      # level1_grid.h: wideOf(sizeof(T)): S 4, D 2
PATHS = ("narrow", "wide", "packed")


def _ceil(a, b):
    return -(-a // b)


def _grid(letter, n, wide):
    """blocks() of level1_grid.h with the reduction's cap and the loop of the kernels restated for n elements."""
    vec = WIDE[letter] if wide else 1
    need = _ceil(_ceil(n, WIDE[letter]) if wide else n, TILE)
    blocks = min(need, SPGPU_REDUCE_MAX_BLOCKS)
    packs = n // vec
    return dict(vec=vec, blocks=blocks, cap_binds=need > SPGPU_REDUCE_MAX_BLOCKS, packs=packs,
                trips=_ceil(packs, blocks * TILE),               # of workgroup 0, whose first tile starts at pack 0
                last_trip_partial=packs % TILE != 0,             # the last tile has lanes without a pack
                tail=n - packs * vec)


def spmv_dot_launch(letter, rows, hack, off_w=0, off_z=0, off_cM=0, off_rP=0, off_rS=0, beta=0):
    """hellSpmvDot over reduceGrid / packedRows (level1_grid.h) restated.  off_*: bytes by which an array lies past a 16-byte boundary (w: the array the dot reads, x when the
    caller passes w == NULL).  None where no first stage is launched (rows <= 0), else dict(path, has_beta, blocks, cap_binds, trips
    (of workgroup 0), last_trip_partial, tail (rows the tail code takes), vec, packs)."""
    if rows <= 0:
        return None
    w = WIDE[letter]
    wide = off_w % 16 == 0 and off_z % 16 == 0
    packed = wide and hack % w == 0 and off_cM % 16 == 0 and off_rP % (4 * w) == 0 and off_rS % (4 * w) == 0
    out = _grid(letter, rows, wide)
    out.update(path="packed" if packed else "wide" if wide else "narrow", has_beta=beta != 0)
    return out


def pair_dot_launch(letter, n, off_z2=0):
    """axpbyPairDot restated: the width comes from z2 alone.  None for n <= 0."""
    if n <= 0:
        return None
    wide = off_z2 % 16 == 0
    out = _grid(letter, n, wide)
    out.update(path="wide" if wide else "narrow")
    return out


STRIP_KINDS = ("all-strip", "all-gather", "mixed-k", "one-lane-refuses", "unequal-lengths-in-pack")


def strip_profile(hell, letter, base=None):
    """The ballot of rowSums<T, WIDE, true> restated over the arrays of a host HELL matrix (spgpu_amd.formats.ell_to_hell's keys),
    `base` the baseIndex the call passes (default: the matrix' own).  Pack p = tile base + u * 256 + tid holds rows p * WIDE ...;
    tile bases are multiples of 1024, so a wavefront (tid / 64) is 64 consecutive packs, whatever the grid.  At step k the lanes
    with k < their longest row vote; a lane agrees if every row of its pack has an entry k and the columns are consecutive from a
    column at or above the base.  Returns which of STRIP_KINDS occur:
      all-strip   a wavefront that takes the strip at every k it runs        all-gather  one that takes it at none
      mixed-k     one that takes it at some k and gathers at others          one-lane-refuses  a (wavefront, k) where exactly one
      voting lane refuses       unequal-lengths-in-pack  a strip taken by a wavefront that holds a pack whose rows differ in length."""
    w, hack = WIDE[letter], hell["hack_size"]
    base = hell["base"] if base is None else base
    packs = hell["rows"] // w
    if packs == 0:
        return set()
    r = np.arange(packs * w, dtype=np.int64)
    length = np.asarray(hell["row_lengths"][:packs * w], np.int64).reshape(packs, w)
    slot = (np.asarray(hell["hack_offsets"], np.int64)[r // hack] + r % hack).reshape(packs, w)
    indices = np.asarray(hell["indices"])
    longest = length.max(axis=1)
    waves = _ceil(packs, kWave)
    pad = waves * kWave - packs
    per_wave = lambda a: np.concatenate([a, np.zeros(pad, a.dtype)]).reshape(waves, kWave)
    uneven = per_wave(length.min(axis=1) != longest)
    strips, gathers = np.zeros(waves, np.int64), np.zeros(waves, np.int64)
    found = set()
    for k in range(int(longest.max(initial=0))):
        inside = k < length
        col = np.where(inside, indices[np.where(inside, slot + k * hack, 0)].astype(np.int64) if indices.size else 0, -1)
        mine = (col[:, 0] - base >= 0) & np.all(inside & (col == col[:, :1] + np.arange(w)), axis=1)
        voting = per_wave(k < longest)
        refusing = per_wave((k < longest) & ~mine)
        runs = voting.any(axis=1)
        strip = runs & ~refusing.any(axis=1)
        strips += strip
        gathers += runs & ~strip
        if np.any(refusing.sum(axis=1) == 1):
            found.add("one-lane-refuses")
        if np.any(strip & (uneven & voting).any(axis=1)):
            found.add("unequal-lengths-in-pack")
    if np.any((strips > 0) & (gathers == 0)):
        found.add("all-strip")
    if np.any((strips == 0) & (gathers > 0)):
        found.add("all-gather")
    if np.any((strips > 0) & (gathers > 0)):
        found.add("mixed-k")
    return found


# ---- matrices --------------------------------------------------------------------------------------------------------------------
# Host HELL dicts with the keys of spgpu_amd.formats.ell_to_hell.  All but `uniform2` go COO -> ELL -> HELL through the project's
# converters.  Integer kinds: values in {-2 ... 2}.

def _np_dtype(letter):
    return {"S": np.float32, "D": np.float64}[letter]


def _through_converters(letter, n, rows, cols, vals, hack, base):
    from spgpu_amd import formats
    ell = formats.coo_to_ell(n, rows + base, cols + base, np.asarray(vals, _np_dtype(letter)), coo_base=base, ell_base=base)
    return formats.ell_to_hell(ell, hack)


def _small_ints(rng, count):
    return rng.integers(1, 3, count) * (rng.integers(0, 2, count) * 2 - 1)            # -2, -1, 1, 2


def uniform2_rows(n):
    """(row lengths, columns [n, 2], values [n, 2]) of the capped matrices: two entries per row (columns i and i + 1, wrapped), one
    in every 11th row, none in every 13th; values cycle through -2 ... 2."""
    i = np.arange(n, dtype=np.int64)
    lengths = np.full(n, 2, np.int32)
    lengths[5::11] = 1
    lengths[7::13] = 0
    cols = np.stack([i % n, (i + 1) % n], axis=1)
    vals = np.stack([i % 5 - 2, (i + 3) % 5 - 2], axis=1)
    return lengths, cols, vals


def uniform2_hell(letter, n, hack):
    """The HELL arrays of uniform2_rows(n) written directly (base 0): a hack is as deep as its longest row, slot of row i's k-th
    entry hack_offsets[i / hack] + i % hack + k * hack, unused slots zero -- what the converters produce
    (tests/test_fused_launch_shapes.py compares the two byte for byte at a small size)."""
    lengths, cols, vals = uniform2_rows(n)
    firsts = np.arange(0, n, hack)
    depth = np.maximum.reduceat(lengths, firsts).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(depth * hack)])
    values, indices = np.zeros(int(offsets[-1]), _np_dtype(letter)), np.zeros(int(offsets[-1]), np.int32)
    i = np.arange(n, dtype=np.int64)
    first = offsets[i // hack] + i % hack
    for k in range(2):
        has = lengths > k
        values[first[has] + k * hack] = vals[has, k]
        indices[first[has] + k * hack] = cols[has, k]
    return dict(letter=letter, rows=n, values=values, indices=indices, hack_offsets=offsets[:-1].astype(np.int32), hack_size=hack,
                height=int(depth.sum()), row_lengths=lengths, base=0)


def uniform2_through_converters(letter, n, hack):
    lengths, cols, vals = uniform2_rows(n)
    has = np.arange(2)[None, :] < lengths[:, None]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], has.shape)
    return _through_converters(letter, n, rows[has], cols[has], vals[has], hack, 0)


def _band_rows(n, flavour):
    """Per-row entry lists of a tridiagonal band (columns i - 1, i, i + 1 clipped, in that order), as (rows, cols) in entry order.
      plain      nothing else: every pack but the first (rows 0 ...: columns 0 0 1 2) names consecutive columns at every k
      scatter    two more entries per row, columns 37 i + 11 (k - 3) + 5 mod n: never consecutive from row to row
      holes      rows with i % 5 == 2 lose their last band entry: packs whose rows differ in length
      one-bad    WIDE-independent: the middle entry of row 300 names column 309"""
    i = np.arange(n, dtype=np.int64)
    parts = [(i >= 1, i - 1), (np.ones(n, bool), i.copy()), (i + 1 < n, i + 1)]
    if flavour == "holes":
        parts[2] = (parts[2][0] & (i % 5 != 2), parts[2][1])
    if flavour == "one-bad":
        parts[1][1][300] = 309
    if flavour == "scatter":
        parts += [(np.ones(n, bool), (37 * i + 5) % n), (np.ones(n, bool), (37 * i + 16) % n)]
    mask = np.stack([p[0] for p in parts], axis=1)
    cols = np.stack([p[1] for p in parts], axis=1)
    rows = np.broadcast_to(i[:, None], mask.shape)
    return rows[mask], cols[mask]


@functools.lru_cache(maxsize=4)
def matrix(letter, kind, rows, hack, base, seed=0):
    """The host HELL matrix of a case (square: rows x rows)."""
    if kind == "uniform2":
        assert base == 0
        return uniform2_hell(letter, rows, hack)
    rng = np.random.default_rng(1000 + seed)
    if kind == "ragged":                # power-law lengths with empty rows, real values: tests/test_gpu_fused_solver.py _ragged_hell
        from spgpu_amd import formats, synth
        lengths = np.minimum(synth.power_law_lengths(rows, mean=6.0, max_len=60, seed=seed), rows)
        lengths[3::7] = 0
        _, _, r, c, v = synth.random_rows_coo(rows, rows, lengths, seed=seed, letter=letter, base=base)
        return formats.ell_to_hell(formats.coo_to_ell(rows, r, c, v, coo_base=base, ell_base=base), hack)
    if kind == "empty":                 # every row empty
        none = np.zeros(0, np.int64)
        return _through_converters(letter, rows, none, none, none, hack, base)
    if kind == "ints":                  # 0 ... 4 entries per row, random columns
        lengths = (np.arange(rows) * 7 + seed) % 5
        r = np.repeat(np.arange(rows, dtype=np.int64), lengths)
        return _through_converters(letter, rows, r, rng.integers(0, rows, r.size), _small_ints(rng, r.size), hack, base)
    assert kind.startswith("band-"), kind
    r, c = _band_rows(rows, kind[5:])
    return _through_converters(letter, rows, r, c, _small_ints(rng, r.size), hack, base)


# ---- the case table ---------------------------------------------------------------------------------------------------------------
BRANCHES = tuple(
    [f"spmv-{p}-{b}" for p in PATHS for b in ("beta", "nobeta")] + [f"spmv-second-trip-{p}" for p in PATHS]
    + ["spmv-cap-binds", "spmv-cap-free", "spmv-no-packs", "spmv-one-trip", "spmv-last-trip-partial", "spmv-last-trip-full",
       "spmv-tail", "spmv-no-tail", "spmv-hack-is-pack", "spmv-hack-not-32", "spmv-hack-above-rows", "spmv-rows-off-hack",
       "spmv-off-cM", "spmv-off-rP", "spmv-off-rS", "spmv-off-w", "spmv-off-z", "spmv-off-y-z-on", "spmv-z-is-y", "spmv-w-null",
       "spmv-beta0-nan-y", "spmv-empty", "spmv-all-rows-empty", "spmv-base-1", "spmv-ragged"]
    + [f"strip-{k}" for k in STRIP_KINDS] + ["strip-base-1", "strip-x-off"]
    + ["pair-wide", "pair-narrow", "pair-second-trip-wide", "pair-second-trip-narrow", "pair-cap-binds", "pair-cap-free",
       "pair-no-packs", "pair-one-trip", "pair-last-trip-partial", "pair-last-trip-full", "pair-tail", "pair-no-tail",
       "pair-off-z1", "pair-off-y1", "pair-off-x1", "pair-off-y2", "pair-off-x2", "pair-off-z2", "pair-in-place", "pair-out-of-place",
       "pair-both-given", "pair-num-null", "pair-den-null", "pair-both-null", "pair-empty"])

#: the sixteen kernel instantiations, as branches of one letter's table
INSTANTIATIONS = tuple([f"spmv-{p}-{b}" for p in PATHS for b in ("beta", "nobeta")] + ["pair-wide", "pair-narrow"])

ALPHA, BETA = 2, -3                                   # integer coefficients of the exact SpMV cases
RAGGED_ALPHA, RAGGED_BETA = 1.25, -0.5                # the real-valued ones
#: (alphaNum, alphaDen) of the four forms of the pair-dot's coefficient; every quotient an exact integer
QUOTIENTS = {"both-given": (6.0, -3.0), "num-null": (None, -0.5), "den-null": (3.0, None), "both-null": (None, None)}
PAIR_OPERANDS = ("z1", "y1", "x1", "z2", "y2", "x2")
REAL_PASS_MAX = 200_000          # rows up to which an exact SpMV case repeats the library's bit contract on real-valued vectors


def second_trip_rows(letter, path):
    """packs = 1024 * TILE + TILE + 5: workgroup 0 takes tile 0 and tile 1024, the last tile is ragged; VEC - 1 tail rows."""
    vec = 1 if path == "narrow" else WIDE[letter]
    return (SPGPU_REDUCE_MAX_BLOCKS * TILE + TILE + 5) * vec + (vec - 1)


def cases(letter):
    """id -> case.  Keys of every case: id, letter, call ("spmv" / "pair"), want (the branches it is there for, written out here and
    not computed by the restated dispatch).
    spmv: matrix (kind of matrix()), rows, hack, base, seed, beta (bool), off (elements by which w, z, y, x, cM, rP, rS lie past a
      16-byte boundary), w_null, z_is_y, strip (bool: the strip profile is part of what the case claims), exact (integer inputs).
    pair: n, off (elements, per operand), in_place, form (key of QUOTIENTS)."""
    W = WIDE[letter]
    c = {}

    def spmv(cid, kind, rows, hack, path, beta, want=(), base=0, seed=0, strip=False, w_null=False, z_is_y=False, **off):
        assert cid not in c, cid
        bad = set(off) - {"w", "z", "y", "x", "cM", "rP", "rS"}
        assert not bad, bad
        want = set(want) | ({"spmv-empty"} if rows == 0 else {f"spmv-{path}-{'beta' if beta else 'nobeta'}"})
        if rows > 0 and not beta:
            want.add("spmv-beta0-nan-y")
        c[cid] = dict(id=cid, letter=letter, call="spmv", matrix=kind, rows=rows, hack=hack, base=base, seed=seed, beta=beta,
                      off={k: off.get(k, 0) for k in ("w", "z", "y", "x", "cM", "rP", "rS")}, w_null=w_null, z_is_y=z_is_y,
                      strip=strip, exact=kind != "ragged", want=want)

    def pair(cid, n, path, want=(), in_place=False, form="both-given", **off):
        assert cid not in c, cid
        want = set(want) | ({"pair-empty"} if n == 0 else
                            {f"pair-{path}", "pair-in-place" if in_place else "pair-out-of-place", f"pair-{form}"})
        c[cid] = dict(id=cid, letter=letter, call="pair", n=n, off={k: off.get(k, 0) for k in PAIR_OPERANDS}, in_place=in_place,
                      form=form, want=want)

    one = {"spmv-cap-free", "spmv-one-trip", "spmv-last-trip-partial", "spmv-tail", "spmv-rows-off-hack"}
    R = 1037                                                         # odd, above one tile of rows at VEC = 1, off every hack size used
    # -- the paths, each with and without beta
    for beta in (True, False):
        b = "beta" if beta else "nobeta"
        spmv(f"packed-h32-{b}", "ints", R, 32, "packed", beta, one)
        spmv(f"packed-hW-{b}", "ints", R, W, "packed", beta, one | {"spmv-hack-is-pack", "spmv-hack-not-32"}, seed=1)
        spmv(f"packed-h12-{b}", "ints", R, 12, "packed", beta, one | {"spmv-hack-not-32"}, seed=2)
        spmv(f"wide-h33-{b}", "ints", R, 33, "wide", beta, one | {"spmv-hack-not-32"}, seed=3)
        spmv(f"wide-h1-{b}", "ints", R, 1, "wide", beta, (one | {"spmv-hack-not-32"}) - {"spmv-rows-off-hack"}, seed=4)
        spmv(f"wide-cM-off-{b}", "ints", R, 32, "wide", beta, one | {"spmv-off-cM"}, seed=5, cM=1)
        spmv(f"wide-rP-off-{b}", "ints", R, 32, "wide", beta, one | {"spmv-off-rP"}, seed=6, rP=1)
        spmv(f"wide-rS-off-{b}", "ints", R, 32, "wide", beta, one | {"spmv-off-rS"}, seed=7, rS=1)
        spmv(f"narrow-w-off-{b}", "ints", R, 32, "narrow", beta, (one | {"spmv-off-w", "spmv-no-tail"}) - {"spmv-tail"}, seed=8, w=1)
        spmv(f"narrow-z-off-{b}", "ints", R, 32, "narrow", beta, (one | {"spmv-off-z", "spmv-no-tail"}) - {"spmv-tail"}, seed=9, z=1)
    # -- rows around one pack, one tile and one workgroup: packed (packs of WIDE rows) and narrow (packs of one row)
    small = {"spmv-cap-free", "spmv-hack-above-rows", "spmv-rows-off-hack"}
    spmv("rows-W", "ints", W, 32, "packed", True, small | {"spmv-one-trip", "spmv-last-trip-partial", "spmv-no-tail"}, seed=10)
    spmv("rows-W+1", "ints", W + 1, 32, "packed", False, small | {"spmv-one-trip", "spmv-last-trip-partial", "spmv-tail"}, seed=11)
    spmv("rows-1", "ints", 1, 32, "packed", True, small | {"spmv-no-packs", "spmv-tail"}, seed=12)
    free = {"spmv-cap-free", "spmv-one-trip"}
    spmv("rows-tile-1", "ints", TILE * W - 1, 32, "packed", True,
         free | {"spmv-last-trip-partial", "spmv-tail", "spmv-rows-off-hack"}, seed=13)
    spmv("rows-tile", "ints", TILE * W, 32, "packed", False, free | {"spmv-last-trip-full", "spmv-no-tail"}, seed=14)
    spmv("rows-tile+W+1", "ints", TILE * W + W + 1, 32, "packed", True,
         free | {"spmv-last-trip-partial", "spmv-tail", "spmv-rows-off-hack"}, seed=15)
    spmv("narrow-rows-1", "ints", 1, 32, "narrow", True,
         small | {"spmv-one-trip", "spmv-last-trip-partial", "spmv-no-tail", "spmv-off-w"}, seed=16, w=1)
    spmv("narrow-rows-tile-1", "ints", TILE - 1, 32, "narrow", False,
         free | {"spmv-last-trip-partial", "spmv-no-tail", "spmv-rows-off-hack", "spmv-off-z"}, seed=17, z=1)
    spmv("narrow-rows-tile", "ints", TILE, 32, "narrow", True, free | {"spmv-last-trip-full", "spmv-no-tail", "spmv-off-w"}, seed=18, w=1)
    spmv("narrow-rows-tile+2", "ints", TILE + 2, 32, "narrow", False,
         free | {"spmv-last-trip-partial", "spmv-no-tail", "spmv-rows-off-hack", "spmv-off-z"}, seed=19, z=1)
    # -- past the cap: a second trip on each path
    capped = {"spmv-cap-binds", "spmv-last-trip-partial", "spmv-rows-off-hack"}
    spmv("second-trip-packed", "uniform2", second_trip_rows(letter, "packed"), 32, "packed", True,
         capped | {"spmv-second-trip-packed", "spmv-tail"})
    spmv("second-trip-wide", "uniform2", second_trip_rows(letter, "wide"), 33, "wide", False,
         capped | {"spmv-second-trip-wide", "spmv-tail", "spmv-hack-not-32"})
    spmv("second-trip-narrow", "uniform2", second_trip_rows(letter, "narrow"), 32, "narrow", True,
         capped | {"spmv-second-trip-narrow", "spmv-no-tail", "spmv-off-w"}, w=1)
    # -- the strip choice: 3 wavefronts of packs, one more pack and a tail row
    B = 3 * kWave * W + W + 1
    band = one | {"strip-all-gather", "strip-one-lane-refuses"}          # the first pack refuses at every k: wavefront 0 gathers
    spmv("strip-band", "band-plain", B, 32, "packed", False, band | {"strip-all-strip"}, strip=True, seed=20)
    spmv("strip-band-base1", "band-plain", B, 32, "packed", True, band | {"strip-all-strip", "strip-base-1", "spmv-base-1"},
         strip=True, base=1, seed=21)
    spmv("strip-band-scatter", "band-scatter", B, 32, "packed", True, band | {"strip-mixed-k"}, strip=True, seed=22)
    spmv("strip-band-holes", "band-holes", B, 32, "packed", False,         # the last wavefront's one pack has no hole: all-strip
         band | {"strip-mixed-k", "strip-unequal-lengths-in-pack", "strip-all-strip"}, strip=True, seed=23)
    spmv("strip-band-one-bad", "band-one-bad", B, 32, "packed", True, band | {"strip-all-strip", "strip-mixed-k"}, strip=True, seed=24)
    spmv("strip-band-x-off", "band-plain", B, 32, "packed", True, band | {"strip-all-strip", "strip-x-off"}, strip=True, seed=25, x=1)
    # -- ragged, real-valued rows on each path at base 0 and 1; a matrix without entries
    G = 5001
    for base in (0, 1):
        b1 = {"spmv-base-1"} if base else set()
        spmv(f"ragged-packed-base{base}", "ragged", G, 32, "packed", bool(base), one | b1 | {"spmv-ragged"}, base=base, seed=30 + base)
        spmv(f"ragged-wide-base{base}", "ragged", G, 33, "wide", not base, one | b1 | {"spmv-ragged", "spmv-hack-not-32"}, base=base,
             seed=32 + base)
        spmv(f"ragged-narrow-base{base}", "ragged", G, 32, "narrow", bool(base),
             (one | b1 | {"spmv-ragged", "spmv-off-w", "spmv-no-tail"}) - {"spmv-tail"}, base=base, seed=34 + base, w=1)
    spmv("all-rows-empty", "empty", R, 32, "packed", True, one | {"spmv-all-rows-empty"})
    # -- operands
    spmv("w-null", "ints", R, 32, "packed", True, one | {"spmv-w-null"}, seed=40, w_null=True)
    spmv("y-off-z-on", "ints", R, 32, "packed", True, one | {"spmv-off-y-z-on"}, seed=41, y=1)
    spmv("z-is-y", "ints", R, 32, "packed", True, one | {"spmv-z-is-y"}, seed=42, z_is_y=True)
    spmv("z-is-y-narrow", "ints", R, 32, "narrow", True, (one | {"spmv-z-is-y", "spmv-off-z", "spmv-no-tail"}) - {"spmv-tail"},
         seed=43, z_is_y=True, z=1, y=1)
    spmv("rows-0", "ints", 0, 32, "packed", True)

    # ---- axpbyPairDot
    pfree = {"pair-cap-free", "pair-one-trip"}
    pair("pair-n-W", W, "wide", pfree | {"pair-last-trip-partial", "pair-no-tail"})
    pair("pair-n-W+1", W + 1, "wide", pfree | {"pair-last-trip-partial", "pair-tail"})
    pair("pair-n-1", 1, "wide", {"pair-cap-free", "pair-no-packs", "pair-tail"})
    pair("pair-n-tile-1", TILE * W - 1, "wide", pfree | {"pair-last-trip-partial", "pair-tail"})
    pair("pair-n-tile", TILE * W, "wide", pfree | {"pair-last-trip-full", "pair-no-tail"})
    pair("pair-n-tile+W+1", TILE * W + W + 1, "wide", pfree | {"pair-last-trip-partial", "pair-tail"})
    pair("pair-second-trip-wide", second_trip_rows(letter, "wide"), "wide",
         {"pair-cap-binds", "pair-second-trip-wide", "pair-last-trip-partial", "pair-tail"})
    narrow = {"pair-off-z2", "pair-no-tail"}
    pair("pair-narrow-n-1", 1, "narrow", pfree | narrow | {"pair-last-trip-partial"}, z2=1)
    pair("pair-narrow-n-tile-1", TILE - 1, "narrow", pfree | narrow | {"pair-last-trip-partial"}, z2=1)
    pair("pair-narrow-n-tile", TILE, "narrow", pfree | narrow | {"pair-last-trip-full"}, z2=1)
    pair("pair-narrow-n-tile+2", TILE + 2, "narrow", pfree | narrow | {"pair-last-trip-partial"}, z2=1)
    pair("pair-second-trip-narrow", second_trip_rows(letter, "narrow"), "narrow",
         {"pair-cap-binds", "pair-second-trip-narrow", "pair-last-trip-partial"} | narrow, z2=1)
    N = 2 * TILE * W + W + 1                                           # three workgroups on the wide path, a ragged tile, a tail
    wide = pfree | {"pair-last-trip-partial", "pair-tail"}
    for name in ("z1", "y1", "x1", "y2", "x2"):
        pair(f"pair-{name}-off", N, "wide", wide | {f"pair-off-{name}"}, **{name: 1})
    pair("pair-in-place", N, "wide", wide, in_place=True)
    pair("pair-in-place-narrow", N, "narrow", pfree | narrow | {"pair-last-trip-partial", "pair-off-z1", "pair-off-y1", "pair-off-y2"},
         in_place=True, z1=1, y1=1, z2=1, y2=1)
    for form in ("num-null", "den-null", "both-null"):
        pair(f"pair-{form}", N, "wide", wide, form=form)
    pair("pair-n-0", 0, "wide")
    return c


def reached(case):
    """The branches the restated dispatch takes on what a case passes."""
    L, size = case["letter"], SIZEOF[case["letter"]]
    off = case["off"]
    got = set()
    if case["call"] == "pair":
        launch = pair_dot_launch(L, case["n"], off["z2"] * size)
        if launch is None:
            return {"pair-empty"}
        if case["in_place"]:
            assert off["z1"] == off["y1"] and off["z2"] == off["y2"]
        got |= {f"pair-{launch['path']}", "pair-in-place" if case["in_place"] else "pair-out-of-place", f"pair-{case['form']}"}
        got |= {f"pair-off-{k}" for k, v in off.items() if v * size % 16}
        p = "pair"
    else:
        byte = lambda k: off[k] * (4 if k in ("rP", "rS") else size)
        rows, hack = case["rows"], case["hack"]
        launch = spmv_dot_launch(L, rows, hack, byte("x") if case["w_null"] else byte("w"), byte("z"), byte("cM"), byte("rP"), byte("rS"),
                                 BETA if case["beta"] else 0)
        if launch is None:
            return {"spmv-empty"}
        if case["z_is_y"]:
            assert off["z"] == off["y"] and case["beta"]
        got.add(f"spmv-{launch['path']}-{'beta' if launch['has_beta'] else 'nobeta'}")
        got |= {f"spmv-off-{k}" for k in ("cM", "rP", "rS", "w", "z") if byte(k) % 16 and not (k == "w" and case["w_null"])}
        for flag, name in ((byte("y") % 16 and not byte("z") % 16, "off-y-z-on"), (case["z_is_y"], "z-is-y"), (case["w_null"], "w-null"),
                           (not launch["has_beta"], "beta0-nan-y"), (case["matrix"] == "empty", "all-rows-empty"),
                           (case["base"] == 1, "base-1"), (case["matrix"] == "ragged", "ragged"),
                           (launch["path"] == "packed" and hack == WIDE[L], "hack-is-pack"), (hack != 32, "hack-not-32"),
                           (hack > rows, "hack-above-rows"), (rows % hack != 0, "rows-off-hack")):
            if flag:
                got.add(f"spmv-{name}")
        if case["strip"]:
            assert launch["path"] == "packed"
            kinds = strip_profile(matrix(L, case["matrix"], rows, hack, case["base"], case["seed"]), L, case["base"])
            got |= {f"strip-{k}" for k in kinds}
            if kinds & {"all-strip", "mixed-k", "unequal-lengths-in-pack"}:         # a strip is taken somewhere
                got |= ({"strip-base-1"} if case["base"] == 1 else set()) | ({"strip-x-off"} if byte("x") % 16 else set())
        p = "spmv"
    got.add(f"{p}-cap-binds" if launch["cap_binds"] else f"{p}-cap-free")
    got.add(f"{p}-no-packs" if launch["trips"] == 0 else f"{p}-one-trip" if launch["trips"] == 1 else f"{p}-second-trip-{launch['path']}")
    if launch["trips"] > 0:
        got.add(f"{p}-last-trip-partial" if launch["last_trip_partial"] else f"{p}-last-trip-full")
    got.add(f"{p}-tail" if launch["tail"] else f"{p}-no-tail")
    return got


# ---- inputs and the integers they must give ---------------------------------------------------------------------------------------

def _density(n):
    """Share of nonzero elements of the integer vectors: half of them, 3 % for the capped sizes (whose sums must stay exact)."""
    return 0.5 if n <= 200_000 else 0.03


def spmv_inputs(case):
    """(hell, x, w, y) on the host; w is None for w == NULL, y is None for beta == 0 (the GPU test then passes NaN).  Integer-valued
    for the exact cases (w and y nonzero at the same places, so that the dot has as many terms as w has elements)."""
    import exact_ref as X
    L, rows, seed = case["letter"], case["rows"], 100 + 10 * case["seed"]
    hell = matrix(L, case["matrix"], rows, case["hack"], case["base"], case["seed"])
    if case["exact"]:
        d = _density(rows)
        x = X.integer_vector(L, seed, rows, density=d)
        w = None if case["w_null"] else X.integer_vector(L, seed + 1, rows, support_seed=seed + 2, density=d)
        y = X.integer_vector(L, seed + 3, rows, support_seed=seed + 2, density=d) if case["beta"] else None
    else:
        from spgpu_amd import synth
        x, w = synth.values_for(L, seed, rows), synth.values_for(L, seed + 1, rows)
        y = synth.values_for(L, seed + 3, rows) if case["beta"] else None
    return hell, x, w, y


def coefficients(case):
    if case["exact"]:
        return (ALPHA, BETA) if case["beta"] else (ALPHA, 0)
    return (RAGGED_ALPHA, RAGGED_BETA) if case["beta"] else (RAGGED_ALPHA, 0.0)


def _ints(a):
    out = np.asarray(a).astype(np.int64)
    assert np.array_equal(out, a), "not integer-valued"
    return out


def spmv_exact(case, hell, x, w, y):
    """(z, w . z) in int64 and the sums the exactness condition is about: the largest row's sum of term magnitudes
    (|alpha| sum |a x| + |beta y|, which bounds every partial sum of the row and of the epilogue) and the dot's
    (sum |w_i| times that magnitude of row i, which bounds every partial sum in any order of addition)."""
    import exact_ref as X
    alpha, beta = coefficients(case)
    n = hell["rows"]
    rows, cols, vals = X.hell_coo(hell)                         # entries in row order
    rows, cols = rows - hell["base"], cols - hell["base"]
    assert np.all(cols >= 0)
    xi = _ints(x)
    prod = _ints(vals) * xi[cols]
    lengths = np.asarray(hell["row_lengths"][:n], np.int64)
    ends = np.cumsum(lengths)

    def per_row(terms):
        total = np.concatenate([[0], np.cumsum(terms)])
        return total[ends] - total[ends - lengths]

    z, mag = alpha * per_row(prod), abs(alpha) * per_row(np.abs(prod))
    if beta:
        z, mag = z + beta * _ints(y), mag + abs(beta) * np.abs(_ints(y))
    wi = xi if w is None else _ints(w)
    sums = dict(asum=int(mag.max(initial=0)), dot_terms=int(np.sum(np.abs(wi) * mag)))
    return z, int(np.sum(wi * z)), sums


def quotient(form):
    num, den = QUOTIENTS[form]
    a = (1.0 if num is None else num) / (1.0 if den is None else den)
    assert a == int(a)
    return int(a)


def pair_inputs(case):
    """(x1, y1, x2, y2) on the host: integer vectors, x2 and y2 nonzero at the same places."""
    import exact_ref as X
    L, n = case["letter"], case["n"]
    d = _density(n)
    seed = 500 + n % 97
    return (X.integer_vector(L, seed, n, density=d), X.integer_vector(L, seed + 1, n, density=d),
            X.integer_vector(L, seed + 2, n, support_seed=seed + 4, density=d), X.integer_vector(L, seed + 3, n, support_seed=seed + 4, density=d))


def pair_exact(case, x1, y1, x2, y2):
    """(z1, z2, z2 . z2) in int64 and the sums of term magnitudes: per element |y| + |a x|, and of the dot the squares of those."""
    a = quotient(case["form"])
    z1, z2 = _ints(y1) + a * _ints(x1), _ints(y2) - a * _ints(x2)
    m1, m2 = np.abs(_ints(y1)) + abs(a) * np.abs(_ints(x1)), np.abs(_ints(y2)) + abs(a) * np.abs(_ints(x2))
    sums = dict(asum=int(max(m1.max(initial=0), m2.max(initial=0))), nrm2sq=int(np.sum(m2 * m2)))
    return z1, z2, int(np.sum(z2 * z2)), sums
