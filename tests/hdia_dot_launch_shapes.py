"""The constants of the host dispatch of spgpu?hdiaspmvDotDevice / spgpu?diaspmvDotDevice (spgpu_amd/csrc/fused_hdia.hip: hdiaSpmvDot
over reduceGrid and packedStrips of level1_grid.h), that dispatch and the control flow of hdiaSpmvDotKernel restated as functions of
what a caller passes, and the case table tests/test_gpu_stencil_dot.py runs -- stated once for that module (which runs the cases on the
GPU) and for tests/test_hdia_dot_launch_shapes.py (which checks on the CPU that the table reaches every instantiation and every
branch, that each case reaches the branches it is there for, and that the integer inputs of the exact cases add exactly).  No torch
and no library at import: importable everywhere.

The small matrices are hand-built by hdia_launch_shapes.hdia_matrix / dia_matrix (the number of diagonals of every hack is chosen,
every slot outside the matrix holds NaN); the three matrices past the grid's cap store the same offsets in every hack and are
written directly (uniform_hdia: the same layout, the same NaN rule)."""
import functools

import numpy as np

import hdia_launch_shapes as H

# ---- the constants of the dispatch: a change there is a test to revisit here ------------------------------------------------------
kL1Threads = 256                    # level1_grid.h    kL1Threads
kL1Unroll = 4                       # level1_grid.h    kL1Unroll: packs in flight per lane
SPGPU_REDUCE_MAX_BLOCKS = 1024      # spgpu_internal.h SPGPU_REDUCE_MAX_BLOCKS: block partials the handle's scratch holds
kWave = 64                          # numeric.hip.h    kWave: lanes that share one __ballot
kStage = 4                          # fused_hdia.hip   kStage: diagonals per stage of the packed path
TILE = kL1Threads * kL1Unroll       # packs one workgroup takes per trip of the tile-stride loop
LETTERS = "SD"
SIZEOF = {"S": 4, "D": 8}
WIDE = {L: 16 // SIZEOF[L] for L in LETTERS}      # level1_grid.h: wideOf(sizeof(T)): S 4, D 2
DTYPE = {"S": np.float32, "D": np.float64}
PATHS = ("narrow", "wide", "packed")
OPERANDS = ("w", "z", "y", "x", "dM")


def _ceil(a, b):
    return -(-a // b)


def launch(letter, rows, hack_or_pitch, off_w=0, off_z=0, off_dM=0, beta=0):
    """hdiaSpmvDot restated.  off_*: bytes by which an array lies past a 16-byte boundary (w: the array the dot reads, x when the
    caller passes w == NULL).  None where no first stage is launched (rows <= 0 or hackSize <= 0), else dict(path, has_beta, vec,
    blocks, cap_binds, packs, trips (of workgroup 0), last_trip_partial, tail (rows the tail code takes))."""
    if rows <= 0 or hack_or_pitch <= 0:
        return None
    W = WIDE[letter]
    wide = off_w % 16 == 0 and off_z % 16 == 0                                   # reduceGrid on (w, z)
    packed = wide and hack_or_pitch % W == 0 and off_dM % 16 == 0                # packedStrips
    vec = W if wide else 1
    need = _ceil(_ceil(rows, W) if wide else rows, TILE)                         # blocks() of level1_grid.h
    blocks = min(need, SPGPU_REDUCE_MAX_BLOCKS)
    packs = rows // vec
    return dict(path="packed" if packed else "wide" if wide else "narrow", has_beta=beta != 0, vec=vec, blocks=blocks,
                cap_binds=need > SPGPU_REDUCE_MAX_BLOCKS, packs=packs, trips=_ceil(packs, blocks * TILE),
                last_trip_partial=packs % TILE != 0, tail=rows - packs * vec)


# ---- the kernel's control flow, walked on the CPU -----------------------------------------------------------------------------------
WALK = ("x-strip",             # packed: stages whose x values are one 16-byte load per diagonal
        "x-strip-unaligned",   # ... among them, stages with such a load at an address off a 16-byte boundary
        "x-elements",          # packed: stages with element loads because a strip of the wavefront crosses an edge
        "one-lane-crosses",    # ... among them, stages where exactly one lane's strip does
        "x-small-cols",        # packed: element loads because cols < VEC
        "stage-whole",         # packed: stages whose four offsets are one load
        "stage-guarded",       # packed: stages fetched diagonal by diagonal
        "second-stage",        # packed: wavefronts with more than kStage diagonals: the v / vNext ring turns
        "dead-lanes",          # packed: lanes without a pack in a wavefront that has one
        "pack-in-two-hacks",   # wide, not packed: packs whose rows lie in two hacks
        "hack-no-diags",       # rows of a hack without diagonals: z = alpha * 0 + beta * y
        "last-hack-partial",   # the last hack holds fewer than hackSize rows
        "mask-col-low",        # stored slots of rows of the matrix masked by col < 0
        "mask-col-high")       # ... by col >= cols


def walk(m, letter, path, x_off=0):
    """How often one call takes each branch of WALK on the arrays of a host matrix (hdia_launch_shapes' keys).  A wavefront of the
    first stage is 64 consecutive packs starting at a multiple of 64 (tile bases are multiples of 1024, a wavefront is lanes
    64 k ... 64 k + 63 of one of the four pack slots of a lane), whatever the grid."""
    rows, cols, size = m["rows"], m["cols"], SIZEOF[letter]
    flat = m["fmt"] == "dia"
    hs = m["pitch"] if flat else m["hack_size"]
    ho = np.array([0, m["diags"]], np.int64) if flat else m["hack_offsets"].astype(np.int64)
    hack_of = (lambda r: np.zeros_like(r)) if flat else (lambda r: r // hs)
    offsets = m["offsets"].astype(np.int64)
    n = dict.fromkeys(WALK, 0)
    r = np.arange(rows, dtype=np.int64)
    count = (ho[1:] - ho[:-1])[hack_of(r)] if rows else np.zeros(0, np.int64)
    n["hack-no-diags"] = int((count == 0).sum())
    n["last-hack-partial"] = int(not flat and rows % hs != 0)
    for d in range(int(count.max(initial=0))):
        has = count > d
        col = r[has] + offsets[ho[hack_of(r[has])] + d]
        n["mask-col-low"] += int((col < 0).sum())
        n["mask-col-high"] += int((col >= cols).sum())
    vec = 1 if path == "narrow" else WIDE[letter]
    packs = rows // vec
    if path == "wide" and not flat:
        first = np.arange(packs, dtype=np.int64) * vec
        n["pack-in-two-hacks"] = int((first // hs != (first + vec - 1) // hs).sum())
    if path != "packed" or packs == 0:
        return n
    waves = _ceil(packs, kWave)
    shape = (waves, kWave)
    row0 = (np.arange(waves * kWave, dtype=np.int64) * vec).reshape(shape)
    live = row0 < packs * vec
    hack = np.where(live, hack_of(row0), 0)
    first = ho[hack]
    diags = np.where(live, ho[hack + 1] - first, 0)
    wave_diags = diags.max(axis=1)
    n["dead-lanes"] = int((~live).sum())
    n["second-stage"] = int((wave_diags > kStage).sum())
    for d_base in range(0, int(wave_diags.max(initial=0)), kStage):
        act = wave_diags > d_base
        whole = act & (diags >= d_base + kStage).all(axis=1)
        n["stage-whole"] += int(whole.sum())
        n["stage-guarded"] += int((act & ~whole).sum())
        ragged, unaligned = np.zeros(shape, bool), np.zeros(shape, bool)
        for u in range(kStage):
            d_live = (diags > d_base + u) & act[:, None]
            off = np.where(d_live, offsets[np.where(d_live, first + d_base + u, 0)], 0)
            col0 = row0 + off
            ragged |= d_live & ~((col0 >= 0) & (col0 + vec <= cols))
            unaligned |= d_live & ((x_off + col0 * size) % 16 != 0)
        if cols < vec:
            n["x-small-cols"] += int(act.sum())
            continue
        strip = act & ~ragged.any(axis=1)
        n["x-strip"] += int(strip.sum())
        n["x-strip-unaligned"] += int((strip & unaligned.any(axis=1)).sum())
        n["x-elements"] += int((act & ~strip).sum())
        n["one-lane-crosses"] += int((act & (ragged.sum(axis=1) == 1)).sum())
    return n


# ---- matrices ------------------------------------------------------------------------------------------------------------------------
def as_integers(m):
    """The matrix with every stored value v in [-1, -0.25] u [0.25, 1] replaced by the integer rint(4 v) in {-4 ... -1, 1 ... 4}; NaN
    slots stay NaN."""
    r, c, v = m["coo"]
    return dict(m, values=np.rint(m["values"] * 4), coo=(r, c, np.rint(v * 4)))


def uniform_hdia(letter, rows, cols, hack, offs):
    """Host HDIA whose hacks all store the ascending offsets `offs`; value of (row i, diagonal d) = (3 i + 2 d) % 5 - 2, NaN where the
    row is past the matrix or the column outside [0, cols).  Keys as hdia_launch_shapes.hdia_matrix; coo in row order, a row's
    entries in stored order."""
    assert list(offs) == sorted(set(offs))
    hacks, k = _ceil(rows, hack), len(offs)
    o = np.array(offs, np.int64)
    r = (np.arange(hacks, dtype=np.int64)[:, None, None] * hack + np.arange(hack, dtype=np.int64)[None, None, :])      # [hacks, 1, hack]
    r = np.broadcast_to(r, (hacks, k, hack))
    d = np.broadcast_to(np.arange(k, dtype=np.int64)[None, :, None], r.shape)
    c = r + o[None, :, None]
    ok = (r < rows) & (c >= 0) & (c < cols)
    vals = np.where(ok, (3 * r + 2 * d) % 5 - 2, np.nan).astype(DTYPE[letter])
    rr = np.broadcast_to(np.arange(rows, dtype=np.int64)[:, None], (rows, k))
    cc = rr + o[None, :]
    inside = (cc >= 0) & (cc < cols)
    vv = ((3 * rr + 2 * np.arange(k, dtype=np.int64)[None, :]) % 5 - 2).astype(DTYPE[letter])
    return dict(letter=letter, rows=rows, cols=cols, values=vals.reshape(-1), offsets=np.tile(o, hacks).astype(np.int32),
                hack_offsets=(np.arange(hacks + 1, dtype=np.int64) * k).astype(np.int32), hack_size=hack, height=hacks * k,
                counts=np.full(hacks, k, np.int64), coo=(rr[inside], cc[inside], vv[inside]), fmt="hdia")


@functools.lru_cache(maxsize=2)
def _matrix(fmt, letter, rows, cols, hp, prog, ints):
    if fmt == "uniform":
        return uniform_hdia(letter, rows, cols, hp, prog)
    if fmt == "hdia":
        m = H.hdia_matrix(letter, rows, cols, hp, prog if isinstance(prog, str) else [list(o) for o in prog])
    else:
        m = H.dia_matrix(letter, rows, cols, hp, prog if isinstance(prog[0], str) else list(prog))
    return as_integers(m) if ints else m


def matrix_of(case):
    """The host matrix of a case, built once and left unchanged."""
    return _matrix(case["fmt"], case["letter"], case["rows"], case["cols"], case["hp"], case["prog"], case["exact"])


# ---- the case table ----------------------------------------------------------------------------------------------------------------
BRANCHES = tuple([f"{f}-{p}-{b}" for f in ("hdia", "dia") for p in PATHS for b in ("beta", "nobeta")]
                 + [f"second-trip-{p}" for p in PATHS]
                 + ["cap-binds", "cap-free", "no-packs", "one-trip", "tail", "no-tail", "rows-ne-cols", "w-null", "z-is-y", "beta0-nan-y",
                    "off-w", "off-z", "off-dM", "off-y-z-on", "off-x", "exact", "real", "empty"] + list(WALK))

#: the twelve kernel instantiations of one letter, as branches of its table ({packed, wide, narrow} x {beta, no beta}), each reached
#: through the HDIA and through the DIA entry points
INSTANTIATIONS = tuple(f"{f}-{p}-{b}" for f in ("hdia", "dia") for p in PATHS for b in ("beta", "nobeta"))

ALPHA, BETA = 2, -3                                   # integer coefficients of the exact cases
REAL_ALPHA, REAL_BETA = 1.25, -0.5                    # the real-valued ones
N = 4097                                              # a tile of packs and more at every VEC, one tail row for S and D, off every hack size
BAND = (-1, 0, 1)


def second_trip_rows(letter, path):
    """packs = 1024 * TILE + TILE + 5: workgroup 0 takes tile 0 and tile 1024, the last tile is ragged; VEC - 1 tail rows."""
    vec = 1 if path == "narrow" else WIDE[letter]
    return (SPGPU_REDUCE_MAX_BLOCKS * TILE + TILE + 5) * vec + (vec - 1)


def cases(letter):
    """id -> case.  Keys: id, letter, fmt ("hdia" / "dia" / "uniform": HDIA with the same offsets in every hack), rows, cols, hp (hack
    size or pitch), prog (a programme of hdia_launch_shapes or offset lists), beta (bool), off (elements by which w, z, y, x, dM lie
    past a 16-byte boundary), w_null, z_is_y, exact (integer inputs), path, want (the branches it is there for, written out here and
    not computed by the restated dispatch)."""
    W = WIDE[letter]
    c = {}

    def add(cid, fmt, rows, cols, hp, prog, path, beta, want=(), exact=False, w_null=False, z_is_y=False, **off):
        assert cid not in c and not set(off) - set(OPERANDS), cid
        kind = "dia" if fmt == "dia" else "hdia"
        want = set(want) | {"exact" if exact else "real"}
        want |= {"empty"} if rows <= 0 or hp <= 0 else {f"{kind}-{path}-{'beta' if beta else 'nobeta'}"}
        if rows > 0 and hp > 0 and not beta:
            want.add("beta0-nan-y")
        c[cid] = dict(id=cid, letter=letter, fmt=fmt, rows=rows, cols=cols, hp=hp, prog=prog, beta=beta,
                      off={k: off.get(k, 0) for k in OPERANDS}, w_null=w_null, z_is_y=z_is_y, exact=exact, path=path, want=want)

    one = {"cap-free", "one-trip", "tail"}
    ragged = {"mask-col-low", "mask-col-high", "hack-no-diags", "last-hack-partial"}          # what the `cycle` programme brings
    # N rows are a whole number of wavefronts of packs for both letters (no dead lanes); a wavefront of fp32 packs spans eight hacks
    # of the cycle (counts 0 ... 13), so none of its stages has four diagonals in every lane: stage-whole is fp64's there
    stages = {"x-strip", "x-strip-unaligned", "x-elements", "stage-guarded", "second-stage"} | ({"stage-whole"} if letter == "D" else set())
    alloc = H.dia_alloc_pitch(N)
    edges = {"mask-col-low", "mask-col-high"}
    for beta in (True, False):
        b = "beta" if beta else "nobeta"
        # hack 32: packed for both letters; 30: packed for fp64, unpacked for fp32; 31: unpacked for both
        add(f"hdia-h32-{b}", "hdia", N, N, 32, "cycle", "packed", beta, one | ragged | stages)
        p30 = "packed" if letter == "D" else "wide"
        add(f"hdia-h30-{b}", "hdia", N, N, 30, "cycle", p30, beta,
            one | ragged | (stages if letter == "D" else {"pack-in-two-hacks"}))
        add(f"hdia-h31-{b}", "hdia", N, N, 31, "cycle", "wide", beta, one | ragged | {"pack-in-two-hacks"})
        add(f"hdia-dM-off-{b}", "hdia", N, N, 32, "cycle", "wide", beta, one | ragged | {"off-dM"}, dM=1)
        add(f"hdia-w-off-{b}", "hdia", N, N, 32, "cycle", "narrow", beta, (one | ragged | {"off-w", "no-tail"}) - {"tail"}, w=1)
        add(f"hdia-z-off-{b}", "hdia", N, N, 32, "cycle", "narrow", beta, (one | ragged | {"off-z", "no-tail"}) - {"tail"}, z=1)
        add(f"dia-alloc-{b}", "dia", N, N, alloc, ("edge", 13), "packed", beta,
            one | edges | {"x-strip", "x-strip-unaligned", "x-elements", "stage-whole", "stage-guarded", "second-stage"})
        add(f"dia-rows-{b}", "dia", N, N, N, ("edge", 13), "wide", beta, one | edges)            # the rows themselves: an odd pitch
        add(f"dia-dM-off-{b}", "dia", N, N, alloc, ("edge", 13), "wide", beta, one | edges | {"off-dM"}, dM=1)
        add(f"dia-w-off-{b}", "dia", N, N, alloc, ("edge", 13), "narrow", beta, (one | edges | {"off-w", "no-tail"}) - {"tail"}, w=1)
    # the smallest: one row (no pack: the tail code alone; fewer columns than a strip has rows); 33 rows in hacks of 32
    add("rows-1", "hdia", 1, 1, 32, ((0,),), "packed", True, {"cap-free", "no-packs", "tail", "last-hack-partial"}, exact=True)
    add("rows-33", "hdia", 33, 33, 32, (BAND, (0,)), "packed", False,
        {"cap-free", "one-trip", "tail", "last-hack-partial", "mask-col-low", "x-elements", "one-lane-crosses", "stage-guarded",
         "dead-lanes"}, exact=True)
    add("cols-1", "hdia", 2 * W, 1, 32, ((-1, 0),), "packed", True,
        {"cap-free", "one-trip", "no-tail", "last-hack-partial", "rows-ne-cols", "mask-col-high", "x-small-cols", "stage-guarded",
         "dead-lanes", "mask-col-low"}, exact=True)
    # a band: the first strip alone crosses the low edge (one lane of wavefront 0), every other wavefront takes the strip loads
    band = tuple(BAND for _ in range(_ceil(N, 32)))
    crossing = {"mask-col-low", "mask-col-high", "last-hack-partial", "x-strip", "x-strip-unaligned", "x-elements", "one-lane-crosses",
                "stage-guarded"}                   # the last row's + 1 leaves on the high side: that row is the tail's
    add("band-packed", "hdia", N, N, 32, band, "packed", True, one | crossing, exact=True)
    add("band-wide", "hdia", N, N, 31, tuple(BAND for _ in range(_ceil(N, 31))), "wide", False,
        one | {"mask-col-low", "mask-col-high", "last-hack-partial", "pack-in-two-hacks"}, exact=True)
    add("band-narrow", "hdia", N, N, 32, band, "narrow", True,
        {"cap-free", "one-trip", "no-tail", "mask-col-low", "mask-col-high", "last-hack-partial", "off-z"}, exact=True, z=1)
    add("band-dia", "dia", N, N, alloc, BAND, "packed", False,
        one | {"mask-col-low", "mask-col-high", "x-strip", "x-strip-unaligned", "x-elements", "one-lane-crosses", "stage-guarded"}, exact=True)
    # rows != cols, offsets that leave the matrix on both sides
    add("rect-more-cols", "hdia", N, N + 40, 32, "cycle", "packed", True, one | ragged | stages | {"rows-ne-cols", "w-null"}, w_null=True)
    add("rect-fewer-cols", "hdia", N, N - 97, 32, "cycle", "packed", False, one | ragged | stages | {"rows-ne-cols"})
    add("rect-dia", "dia", N, N - 13, alloc, ("edge", 13), "packed", True,
        one | edges | {"rows-ne-cols", "x-strip", "x-strip-unaligned", "x-elements", "stage-whole", "stage-guarded", "second-stage"})
    # operands
    add("w-null", "hdia", N, N, 32, "cycle", "packed", True, one | ragged | stages | {"w-null"}, w_null=True)
    add("w-null-x-off", "hdia", N, N, 32, "cycle", "narrow", False, (one | ragged | {"w-null", "off-x", "no-tail"}) - {"tail"},
        w_null=True, x=1)
    add("x-off", "hdia", N, N, 32, "interior", "packed", True,
        one | {"off-x", "last-hack-partial", "mask-col-low", "mask-col-high"} | stages, x=1)
    add("y-off-z-on", "hdia", N, N, 32, "cycle", "packed", True, one | ragged | stages | {"off-y-z-on"}, y=1)
    add("z-is-y", "hdia", N, N, 32, "cycle", "packed", True, one | ragged | stages | {"z-is-y"}, z_is_y=True)
    add("z-is-y-narrow", "dia", N, N, alloc, ("edge", 13), "narrow", True, (one | edges | {"z-is-y", "off-z", "no-tail"}) - {"tail"},
        z_is_y=True, z=1, y=1)
    # past the cap: the second trip of the tile-stride loop on each path (three diagonals, integer values)
    capped = {"cap-binds", "mask-col-low", "mask-col-high", "last-hack-partial"}
    add("second-trip-packed", "uniform", second_trip_rows(letter, "packed"), second_trip_rows(letter, "packed"), 32, BAND, "packed", True,
        capped | {"second-trip-packed", "tail", "x-strip", "x-strip-unaligned", "x-elements", "one-lane-crosses", "stage-guarded",
                  "dead-lanes"}, exact=True)
    add("second-trip-wide", "uniform", second_trip_rows(letter, "wide"), second_trip_rows(letter, "wide"), 31, BAND, "wide", False,
        capped | {"second-trip-wide", "tail", "pack-in-two-hacks"}, exact=True)
    add("second-trip-narrow", "uniform", second_trip_rows(letter, "narrow"), second_trip_rows(letter, "narrow"), 32, BAND, "narrow", True,
        capped | {"second-trip-narrow", "no-tail", "off-w"}, exact=True, w=1)
    # no first stage
    add("rows-0", "hdia", 0, 0, 32, (), "packed", True)
    add("hack-0", "hdia", 70, 70, 0, (), "packed", True)
    return c


def reached(case):
    """The branches the restated dispatch and the walked kernel take on what a case passes.  A case's `want` names every branch of the
    dispatch it takes and the branches of WALK it is in the table for; the walk may find more of those (a programme drawn at random
    that happens to leave one strip alone across an edge)."""
    L, size, off = case["letter"], SIZEOF[case["letter"]], case["off"]
    byte = lambda k: off[k] * size
    got = {"exact" if case["exact"] else "real"}
    run = launch(L, case["rows"], case["hp"], byte("x") if case["w_null"] else byte("w"), byte("z"), byte("dM"), BETA if case["beta"] else 0)
    if run is None:
        return got | {"empty"}
    if case["z_is_y"]:
        assert off["z"] == off["y"] and case["beta"]
    if case["w_null"]:
        assert case["cols"] >= case["rows"] and off["w"] == 0
    kind = "dia" if case["fmt"] == "dia" else "hdia"
    got.add(f"{kind}-{run['path']}-{'beta' if run['has_beta'] else 'nobeta'}")
    got |= {f"off-{k}" for k in ("w", "z", "dM", "x") if byte(k) % 16}
    for flag, name in ((byte("y") % 16 and not byte("z") % 16, "off-y-z-on"), (case["z_is_y"], "z-is-y"), (case["w_null"], "w-null"),
                       (not run["has_beta"], "beta0-nan-y"), (case["rows"] != case["cols"], "rows-ne-cols")):
        if flag:
            got.add(name)
    got.add("cap-binds" if run["cap_binds"] else "cap-free")
    if not run["cap_binds"] or run["trips"] < 2:
        got.add("no-packs" if run["trips"] == 0 else "one-trip")
    if run["trips"] >= 2:
        got.add(f"second-trip-{run['path']}")
    got.add("tail" if run["tail"] else "no-tail")
    if case["fmt"] == "uniform":            # too large to walk lane by lane on every CPU run: the same band on one tile of packs, five
        n = (TILE + 5) * run["vec"] + run["vec"] - 1      # packs and VEC - 1 tail rows (the shape of the last trip) stands for it
        counts = walk(uniform_hdia(L, n, n, case["hp"], case["prog"]), L, run["path"], byte("x"))
    else:
        counts = walk(matrix_of(case), L, run["path"], byte("x"))
    return got | {k for k, v in counts.items() if v}


# ---- inputs and the integers they must give -------------------------------------------------------------------------------------------
def inputs(case):
    """(matrix, x [cols], w [rows] or None for w == NULL, y [rows] or None for beta == 0) on the host.  Integer-valued for the exact
    cases (w and y nonzero at the same places)."""
    import exact_ref as X
    L, rows, cols = case["letter"], case["rows"], case["cols"]
    m = matrix_of(case)
    if case["exact"]:
        d = 0.5 if rows <= 200_000 else 0.03
        x = X.integer_vector(L, 11, max(cols, 16), density=d)[:cols]
        w = None if case["w_null"] else X.integer_vector(L, 12, max(rows, 16), support_seed=13, density=d)[:rows]
        y = X.integer_vector(L, 14, max(rows, 16), support_seed=13, density=d)[:rows] if case["beta"] else None
    else:
        x = H.values(L, ("x", cols), cols)
        w = None if case["w_null"] else H.values(L, ("w", rows), rows)
        y = H.values(L, ("y", rows), rows) if case["beta"] else None
    return m, x, w, y


def coefficients(case):
    if case["exact"]:
        return (ALPHA, BETA) if case["beta"] else (ALPHA, 0)
    return (REAL_ALPHA, REAL_BETA) if case["beta"] else (REAL_ALPHA, 0.0)


def _ints(a):
    out = np.asarray(a).astype(np.int64)
    assert np.array_equal(out, a), "not integer-valued"
    return out


def exact(case, m, x, w, y):
    """(z, w . z) in int64 from the matrix' COO triplets (row order) and the sums the exactness condition is about: the largest
    row's sum of term magnitudes and the dot's."""
    alpha, beta = coefficients(case)
    rows = m["rows"]
    r, c, v = m["coo"]
    xi = _ints(x)
    prod = _ints(v) * xi[c]
    lengths = np.bincount(r, minlength=rows).astype(np.int64)
    ends = np.cumsum(lengths)

    def per_row(terms):
        total = np.concatenate([[0], np.cumsum(terms)])
        return total[ends] - total[ends - lengths]

    z, mag = alpha * per_row(prod), abs(alpha) * per_row(np.abs(prod))
    if beta:
        z, mag = z + beta * _ints(y), mag + abs(beta) * np.abs(_ints(y))
    wi = xi[:rows] if w is None else _ints(w)
    return z, int(np.sum(wi * z)), dict(asum=int(mag.max(initial=0)), dot_terms=int(np.sum(np.abs(wi) * mag)))
