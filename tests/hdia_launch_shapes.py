"""The constants of the HDIA / DIA SpMV dispatch (spgpu_amd/csrc/hdia_spmv.hip), the dispatch restated as a function of what a
caller passes, the kernel's control flow restated as a CPU walk that counts every branch a call takes, and the hand-built matrices
and the case table tests/test_gpu_hdia_shapes.py runs, stated once for that module (which runs them on the GPU) and for
tests/test_hdia_launch_shapes.py (which checks on the CPU that every case takes the branches it is there for and that the table
reaches every branch of every instantiation).  No torch, no library: importable everywhere.

The matrices are written slot by slot in numpy, never through cooToHdia / coo2dia / diaToHdia: the number of diagonals of every
hack is chosen, not found.  A stored slot that no product may use (its row is past the matrix, or its column is outside
[0, cols)) holds NaN, and so does the padding behind the rows of a DIA diagonal."""
import zlib

import numpy as np

# ---- the constants of the dispatch, with the line that sets each: a change there is a test to revisit here -------------------
THREADS = 512                 # hdia_spmv.hip:56     kHdiaThreads: lanes (strips) per workgroup
UNROLL = 4                    # hdia_spmv.hip:63     diagonals per stage
WAVE = 64                     # numeric.hip.h:23     kWave
SIZEOF = {"S": 4, "D": 8, "C": 8, "Z": 16}
WIDE = {L: 16 // s for L, s in SIZEOF.items()}     # hdia_spmv.hip:231   rows per lane of the wide kernel: S 4, D 2, C 2, Z 1
CTYPE = {"S": "float", "D": "double", "C": "spgpu::Cx<float>", "Z": "spgpu::Cx<double>"}
DTYPE = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}
ALIGNED = dict(dM=0, z=0, y=0, x=0)


def kernel_name(letter, rpl):
    """The instantiation as the profiler prints it (inside `void spgpu::...(spgpu::HdiaArgs<T>)`)."""
    return f"hdiaSpmvKernel<{CTYPE[letter]}, {rpl}>"


def every_instantiation():
    """The seven: S, D and C wide and narrow; Z, whose elements are 16 bytes, narrow only."""
    return [kernel_name(L, r) for L in "SDCZ" for r in sorted({WIDE[L], 1}, reverse=True)]


def dispatch(letter, hack_or_pitch, off=ALIGNED, has_y=True):
    """hdiaSpmv (hdia_spmv.hip:231-244) restated: (RPL, wideIO).  `off`: bytes by which dM, z, y and x lie past a 16-byte boundary
    (x changes no choice).  Without y (NULL, address 0) nothing of y is off its boundary."""
    wide = WIDE[letter]
    wide_ok = wide > 1 and hack_or_pitch % wide == 0 and off["dM"] % 16 == 0
    if wide_ok:
        return wide, int(off["z"] % 16 == 0 and (not has_y or off["y"] % 16 == 0))
    return 1, 1


def offsets_of(letter, shift):
    """Byte offsets from a 16-byte boundary of the four arrays when those named in `shift` start one element late."""
    off = dict(ALIGNED)
    for name in shift:
        off[name] = SIZEOF[letter] % 16
    return off


def dia_alloc_pitch(rows):
    """computeDiaAllocPitch (conv_dia.c:11)."""
    return (rows + 31) & ~31


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
N = 4503      # S wide: two workgroups of 2 048 rows, one whole 256-row wavefront, a partial one, n % 4 == 3; D, C wide: four
#               workgroups of 1 024 rows and three wavefronts more, n odd; narrow: eight workgroups of 512 rows and more
SMALL_SHAPES = ((1, 1), (5, 700), (70, 70), (300, 3), (300, 1))
RECT_SHAPES = ((N, 4543), (N, 4490))
HACKS = (1, 2, 4, 30, 32, 33, 64, 96, 4512)       # 4512 > N: one hack holds every row
#: the hack sizes of HACKS at which the wide kernel runs (hackSize % WIDE == 0), written out by hand
WIDE_HACKS = {"S": (4, 32, 64, 96, 4512), "D": (2, 4, 30, 32, 64, 96, 4512), "C": (2, 4, 30, 32, 64, 96, 4512), "Z": ()}
CYCLE = (0, 1, 3, 4, 5, 7, 8, 9, 13)              # diagonals per hack of the `cycle` programme, hack after hack
RUN = 640                                         # rows per run of the `runs` programme
RUN_COUNTS = (4, 8, 12, 7, 9, 0)                  # all stages whole / a whole stage then a guarded one / an empty run
INTERIOR = (-40, -37, -6, -3, -2, -1, 0, 1, 2, 3, 5, 8, 41)
INTERIOR_COUNTS = (4, 6, 9)


def dia_pitches(letter, rows):
    """The allocation pitch, that plus 32, the rows themselves, and the rows rounded up to WIDE only."""
    w = WIDE[letter]
    return (dia_alloc_pitch(rows), dia_alloc_pitch(rows) + 32, rows, (rows + w - 1) // w * w)


def candidates(rows, cols):
    """The offsets a programme draws from: 0, +-1, +-2, +-3 (diagonals that enter or leave mid-strip, odd x addresses), mid-range
    odd and even ones, and the last diagonals at either end -- those that cross the matrix."""
    want = [0, 1, -1, 2, -2, 3, -3, 100, 101, -200, -201, 1500, -1501, 2222, -2223, rows // 2, -(cols // 2),
            -(rows - 1), -(rows - 2), cols - 1, cols - 2, cols - 5, -(rows - 6)]
    return sorted({o for o in want if -(rows - 1) <= o <= cols - 1})


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def programme(name, rows, cols, hack):
    """Per hack, the ascending distinct offsets of its diagonals.
      cycle     counts 0, 1, 3, 4, 5, 7, 8, 9, 13 hack after hack (13 where one hack holds every row), offsets drawn from
                candidates()
      runs      640 rows of hacks with 4, then 8, 12, 7, 9 and 0 diagonals (a hack belongs to the run its first row lies in), the
                rest as `cycle`: every run holds a whole wavefront of every kernel shape at every hack size up to 96
      interior  4, 6, 9 diagonals hack after hack, every offset in [-40, 41]: wavefronts away from the first and last rows have
                every strip inside [0, cols)
      all       every hack stores the first 13 candidates (small matrices)"""
    hacks = (rows + hack - 1) // hack
    cand = np.array(candidates(rows, cols))
    inner = np.array([o for o in INTERIOR if -(rows - 1) <= o <= cols - 1])
    rng = _rng(name, rows, cols, hack)

    def draw(pool, count):
        return sorted(int(o) for o in rng.choice(pool, size=min(count, pool.size), replace=False))

    out = []
    for k in range(hacks):
        if name == "cycle":
            out.append(draw(cand, CYCLE[-1] if hacks == 1 else CYCLE[k % len(CYCLE)]))
        elif name == "runs":
            run = k * hack // RUN
            out.append(draw(cand, RUN_COUNTS[run] if run < len(RUN_COUNTS) else CYCLE[k % len(CYCLE)]))
        elif name == "interior":
            out.append(draw(inner, INTERIOR_COUNTS[k % len(INTERIOR_COUNTS)]))
        elif name == "all":
            out.append([int(o) for o in cand[:13]])
        else:
            raise ValueError(name)
    return out


def dia_offsets(name, rows, cols):
    """One ascending offset list: (`edge`, k) k candidates, the two outermost among them; (`interior`, k) k of INTERIOR."""
    kind, k = name
    pool = np.array(candidates(rows, cols) if kind == "edge" else [o for o in INTERIOR if -(rows - 1) <= o <= cols - 1])
    k = min(k, pool.size)
    picked = set(int(o) for o in _rng(kind, k, rows, cols).choice(pool, size=k, replace=False))
    if kind == "edge" and k >= 4:          # whatever the draw: a diagonal of one slot at either end, and the odd neighbours of 0
        for must in (int(pool[0]), int(pool[-1]), 1, -1):
            if must not in picked and must in pool:
                picked.remove(next(o for o in sorted(picked) if o not in (int(pool[0]), int(pool[-1]), 1, -1)))
                picked.add(must)
    return sorted(picked)


def values(letter, seed, n):
    """Values in [-1, -0.25] and [0.25, 1] (both parts of a complex one): nonzero, and no product tiny beside its row's scale."""
    rng = _rng("values", seed)
    part = lambda: rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    v = part() + 1j * part() if letter in "CZ" else part()
    return v.astype(DTYPE[letter])


def _nan(letter):
    return DTYPE[letter](complex(np.nan, np.nan) if letter in "CZ" else np.nan)


def hdia_matrix(letter, rows, cols, hack, prog):
    """Host HDIA of a hack programme (a name of programme() or the per-hack offset lists themselves), keys as oracle_api.hdia_spmv
    reads them, and `coo`: (rows, cols, values) of the slots with row < rows and 0 <= row + offset < cols, a row's in stored order.
    Every other slot holds NaN."""
    lists = programme(prog, rows, cols, hack) if isinstance(prog, str) else [list(o) for o in prog]
    assert len(lists) == (rows + hack - 1) // hack
    assert all(list(o) == sorted(set(o)) for o in lists), "ascending and distinct within a hack"
    counts = np.array([len(o) for o in lists], np.int64)
    hack_offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    height = int(hack_offsets[-1])
    offs = np.array([o for one in lists for o in one], np.int64)
    vals = np.full(max(height * hack, 1), _nan(letter), DTYPE[letter])
    hack_of = np.repeat(np.arange(len(lists), dtype=np.int64), counts)
    r = hack_of[:, None] * hack + np.arange(hack, dtype=np.int64)[None, :]      # [height, hack]
    c = r + offs[:, None]
    ok = (r < rows) & (c >= 0) & (c < cols)
    v = values(letter, ("hdia", rows, cols, hack, str(prog) if isinstance(prog, str) else "lists"), int(ok.sum()))
    vals[:height * hack].reshape(height, hack)[ok] = v
    order = np.lexsort((np.broadcast_to(np.arange(height)[:, None], ok.shape)[ok], r[ok]))    # by row, then stored diagonal
    stored = offs.astype(np.int32) if height else np.zeros(1, np.int32)
    return dict(letter=letter, rows=rows, cols=cols, values=vals, offsets=stored, hack_offsets=hack_offsets, hack_size=hack,
                height=height, counts=counts, coo=(r[ok][order], c[ok][order], v[order]), fmt="hdia")


def dia_matrix(letter, rows, cols, pitch, offs):
    """Host DIA (dM[row + d * pitch]) of one offset list (a name of dia_offsets() or the list), keys as oracle_api.dia_spmv reads
    them, and `coo` as hdia_matrix.  Out-of-range slots and the pitch padding hold NaN."""
    offs = dia_offsets(offs, rows, cols) if isinstance(offs, tuple) else list(offs)
    assert pitch >= rows and offs == sorted(set(offs))
    diags = len(offs)
    o = np.array(offs, np.int64)
    vals = np.full(max(diags * pitch, 1), _nan(letter), DTYPE[letter])
    r = np.broadcast_to(np.arange(pitch, dtype=np.int64)[None, :], (diags, pitch))
    c = r + o[:, None]
    ok = (r < rows) & (c >= 0) & (c < cols)
    v = values(letter, ("dia", rows, cols, tuple(offs)), int(ok.sum()))      # the same values at every pitch
    vals[:diags * pitch].reshape(diags, pitch)[ok] = v
    order = np.lexsort((np.broadcast_to(np.arange(diags)[:, None], ok.shape)[ok], r[ok]))
    return dict(letter=letter, rows=rows, cols=cols, values=vals, offsets=o.astype(np.int32) if diags else np.zeros(1, np.int32),
                pitch=pitch, diags=diags, coo=(r[ok][order], c[ok][order], v[order]), fmt="dia")


def as_one_hack(dia):
    """The DIA arrays read as HDIA with one hack of `pitch` rows: the call the DIA entry points make of themselves."""
    return dict(dia, hack_size=dia["pitch"], hack_offsets=np.array([0, dia["diags"]], np.int32), height=dia["diags"],
                counts=np.array([dia["diags"]], np.int64), fmt="hdia")


# ---- the kernel's control flow, walked on the CPU --------------------------------------------------------------------------------
BRANCHES = (
    "wave_exit",                 # wavefronts that leave at waveRow0 >= rows (:67)
    "dead_lanes",                # lanes with row0 >= rows in a wavefront that stays (:71)
    "wave_no_diags",             # wavefronts with waveDiags == 0: z = beta * y (:87, :130)
    "stage_whole",               # stages whose four offsets are one load (:106-114)
    "stage_guarded",             # stages fetched diagonal by diagonal, the absent ones zeroed (:116-127)
    "wave_three_stages",         # wavefronts with at least three stages: the v / vNext ring turns twice (:131, :168)
    "wave_mixed_counts",         # wavefronts whose live lanes have different diagonal counts (:87 with dead lanes per diagonal)
    "x_wide",                    # stages whose x values are one 16-byte load per diagonal (:150-153)
    "x_wide_unaligned",          # ... among them, stages with such a load at an address off a 16-byte boundary
    "x_elem_edge",               # stages with element loads because a strip of the wavefront crosses an edge (:145, :154)
    "x_elem_small_cols",         # stages with element loads because cols < RPL (:150)
    "store_wide",                # strips stored (and y loaded) as one pack (:178-190)
    "store_elem_no_wideio",      # strips stored by element because z or y is off its boundary (:191)
    "store_elem_partial_strip",  # strips stored by element because the strip ends past the last row (:88, :191)
    "mask_col_low",              # slots of live diagonals masked by col < 0 (:143)
    "mask_col_high",             # ... by col >= cols
    "mask_row",                  # ... by row >= rows
)
#: what the narrow kernels (RPL == 1; Z has no other) cannot reach: `RPL > 1` is false at compile time, a strip is one row, and
#: their only store is the one-element pack.  Stated here so that the coverage test does not skip them silently.
NARROW_HAS_NO = ("x_wide", "x_wide_unaligned", "x_elem_edge", "x_elem_small_cols", "store_wide", "store_elem_no_wideio",
                 "store_elem_partial_strip", "mask_row")
#: DIA: every row sees every stored diagonal
DIA_HAS_NO = ("wave_mixed_counts",)


def reachable(fmt, rpl):
    return [b for b in BRANCHES if not (rpl == 1 and b in NARROW_HAS_NO) and not (fmt == "dia" and b in DIA_HAS_NO)]


def branches(m, letter, rpl, wide_io, has_beta, x_off=0):
    """How often one call takes each branch of BRANCHES (and `stages`, `store_narrow`, `y_read`), from the arrays alone."""
    size, rows, cols = SIZEOF[letter], m["rows"], m["cols"]
    flat = m["fmt"] == "dia"
    hs = m["pitch"] if flat else m["hack_size"]
    strips = (rows + rpl - 1) // rpl
    lanes = (strips + THREADS - 1) // THREADS * THREADS
    shape = (lanes // WAVE, WAVE)
    row0 = (np.arange(lanes, dtype=np.int64) * rpl).reshape(shape)
    stays = row0[:, 0] < rows
    live = row0 < rows
    if flat:
        first = np.zeros(shape, np.int64)
        diags = np.where(live, m["diags"], 0)
    else:
        ho = m["hack_offsets"].astype(np.int64)
        hack = np.where(live, row0 // hs, 0)
        first = ho[hack]
        diags = np.where(live, ho[hack + 1] - first, 0)
    wave_diags = diags.max(axis=1)
    inside = row0 + rpl <= rows
    n = dict.fromkeys(BRANCHES, 0)
    n["wave_exit"] = int((~stays).sum())
    n["dead_lanes"] = int((~live & stays[:, None]).sum())
    n["wave_no_diags"] = int((stays & (wave_diags == 0)).sum())
    n["wave_three_stages"] = int((wave_diags > 2 * UNROLL).sum())
    low = np.where(live, diags, diags.max(initial=0)).min(axis=1)
    n["wave_mixed_counts"] = int((stays & (low != wave_diags)).sum())
    n["stages"] = 0
    offsets = m["offsets"].astype(np.int64)
    for d_base in range(0, int(wave_diags.max(initial=0)), UNROLL):
        act = wave_diags > d_base
        whole = act & (diags >= d_base + UNROLL).all(axis=1)        # dead lanes have no diagonals: their wavefront is never whole
        n["stages"] += int(act.sum())
        n["stage_whole"] += int(whole.sum())
        n["stage_guarded"] += int((act & ~whole).sum())
        ragged = np.zeros(shape, bool)
        unaligned = np.zeros(shape, bool)
        for u in range(UNROLL):
            d_live = (diags > d_base + u) & act[:, None]
            off = np.where(d_live, offsets[np.where(d_live, first + d_base + u, 0)], 0)
            col0 = row0 + off
            ragged |= d_live & ~(inside & (col0 >= 0) & (col0 + rpl <= cols))
            unaligned |= d_live & ((x_off + col0 * size) % 16 != 0)
            for t in range(rpl):
                n["mask_col_low"] += int((d_live & (col0 + t < 0)).sum())
                n["mask_col_high"] += int((d_live & (col0 + t >= cols)).sum())
                n["mask_row"] += int((d_live & (row0 + t >= rows)).sum())
        if rpl > 1:
            if cols < rpl:
                n["x_elem_small_cols"] += int(act.sum())
            else:
                wide_x = act & ~ragged.any(axis=1)
                n["x_wide"] += int(wide_x.sum())
                n["x_wide_unaligned"] += int((wide_x & unaligned.any(axis=1)).sum())
                n["x_elem_edge"] += int((act & ragged.any(axis=1)).sum())
    if rpl > 1:
        n["store_wide"] = int((live & inside).sum()) if wide_io else 0
        n["store_elem_no_wideio"] = 0 if wide_io else int(live.sum())
        n["store_elem_partial_strip"] = int((live & ~inside).sum()) if wide_io else 0
        n["store_narrow"] = 0
    else:
        n["store_narrow"] = int(live.sum())
    n["y_read"] = int(live.sum()) if has_beta else 0
    return n


# ---- the cases of tests/test_gpu_hdia_shapes.py ----------------------------------------------------------------------------------
#: (alpha, beta): plain, with y, and the in-place sum.  C and Z get imaginary parts from test_gpu_fuzz._complex_scalars.
PLAIN, WITH_Y, IN_PLACE = (1.0, 0.0), (-0.75, 0.5), (2.0, 1.0)
#: the eight placements every letter and both formats run: kind -> (shifted arrays, y mode, scalars).  y modes: `y` a vector of its
#: own, `null` y == NULL, `nan` a vector full of NaN that beta == 0 must keep unread, `z` z == y.
PLACEMENTS = {
    "aligned": ((), "y", WITH_Y),
    "dM-shifted": (("dM",), "y", WITH_Y),
    "z-shifted": (("z",), "y", WITH_Y),
    "y-shifted": (("y",), "y", WITH_Y),
    "y-shifted-unread": (("y",), "nan", PLAIN),
    "x-shifted": (("x",), "y", WITH_Y),
    "in-place": ((), "z", IN_PLACE),
    "y-null": ((), "null", PLAIN),
}
ROUTES = ("wide", "wide-elemio", "narrow")


def route_rpl_io(letter, route):
    return {"wide": (WIDE[letter], 1), "wide-elemio": (WIDE[letter], 0), "narrow": (1, 1)}[route]


def _placement_route(letter, kind, wide_matrix):
    """Written out, not computed: the route a placement takes on a matrix whose hack size or pitch allows the wide kernel."""
    if letter == "Z" or not wide_matrix or kind == "dM-shifted":
        return "narrow"
    return "wide-elemio" if kind in ("z-shifted", "y-shifted", "y-shifted-unread") else "wide"


def _claims(fmt, prog, hp, route, kind, rows, cols, letter):
    """The branches a case is in the table for, from how it was made (never from branches() itself)."""
    big = rows == N
    name, count = (prog, None) if isinstance(prog, str) else prog
    one_hack = fmt == "hdia" and hp >= rows
    out = ["wave_exit", "dead_lanes"]     # no shape of the table fills its last workgroup or its last wavefront
    if big:
        if fmt == "hdia" and not one_hack:
            if name in ("cycle", "runs"):
                out += ["stage_guarded", "mask_col_low", "mask_col_high"]
            if name == "cycle":
                out += ["wave_three_stages"]
                if hp % (WAVE * route_rpl_io(letter, route)[0]):     # a wavefront's rows are not all of one hack
                    out += ["wave_mixed_counts"]
            if name == "runs":
                out += ["stage_whole", "wave_three_stages", "wave_no_diags"]
        if fmt == "dia":
            if name == "edge" and count >= 4:
                out += ["stage_guarded", "mask_col_low", "mask_col_high"]   # the partial last wavefront is never `whole`
            if count >= 4 and count % 4 == 0:
                out += ["stage_whole"]
            if count > 8:
                out += ["wave_three_stages"]
            if count == 0:
                out += ["wave_no_diags"]
    if route != "narrow":
        ragged = name in ("cycle", "runs") and not one_hack or name == "edge" and count >= 4
        if big:
            out += ["store_elem_no_wideio"] if route == "wide-elemio" else ["store_wide", "store_elem_partial_strip"]
            if ragged:
                out += ["x_elem_edge"]
            if name == "interior" and (fmt == "hdia" or count >= 2):
                out += ["x_wide", "mask_row"]
                if fmt == "hdia" or count >= 8 or "x" in PLACEMENTS[kind][0]:
                    out += ["x_wide_unaligned"]
        if cols < WIDE[letter] and (fmt == "hdia" or count > 0):
            out += ["x_elem_small_cols"]
    return tuple(out)


def _case(cid, fmt, letter, shape, prog, hp, kind, route):
    shift, y_mode, scalars = PLACEMENTS[kind]
    return dict(id=cid, fmt=fmt, letter=letter, shape=shape, prog=prog, hp=hp, shift=shift, y_mode=y_mode, scalars=scalars,
                kind=kind, route=route, want=route_rpl_io(letter, route),
                claims=_claims(fmt, prog, hp, route, kind, shape[0], shape[1], letter))


def cases(letter):
    """id -> case.  A case: format, letter, shape, programme (HDIA) or offset list name (DIA), hack size or pitch, the arrays that
    start one element late, how y is passed, (alpha, beta), the route (RPL, wideIO) it must take, the branches it is there for."""
    c = {}

    def add(cid, fmt, shape, prog, hp, kind, route):
        assert cid not in c, cid
        c[cid] = _case(cid, fmt, letter, shape, prog, hp, kind, route)

    sq = (N, N)
    # every placement, on a matrix that allows the wide kernel (hack 32 / the allocation pitch), ragged and interior diagonals
    for kind in PLACEMENTS:
        for prog in ("cycle", "interior"):
            add(f"hdia-{prog}-h32-{kind}", "hdia", sq, prog, 32, kind, _placement_route(letter, kind, True))
        for prog in (("edge", 13), ("interior", 8)):
            add(f"dia-{prog[0]}{prog[1]}-alloc-{kind}", "dia", sq, prog, dia_alloc_pitch(N), kind, _placement_route(letter, kind, True))
    # every hack size, every programme
    for hack in HACKS:
        wide = hack in WIDE_HACKS[letter]
        for prog in ("cycle", "runs", "interior"):
            for kind in ("aligned", "y-null", "in-place"):
                if hack == 32 and prog != "runs":
                    continue            # above
                add(f"hdia-{prog}-h{hack}-{kind}", "hdia", sq, prog, hack, kind, _placement_route(letter, kind, wide))
    # hackSize == WIDE with z off its boundary: 64 lanes, 64 hacks, element stores
    if WIDE[letter] > 1:
        add(f"hdia-cycle-h{WIDE[letter]}-z-shifted", "hdia", sq, "cycle", WIDE[letter], "z-shifted", "wide-elemio")
    # every DIA pitch; the rows themselves are odd, so that pitch is the narrow kernel's for every letter
    alloc, alloc32, own, rounded = dia_pitches(letter, N)
    for tag, pitch, wide in (("alloc+32", alloc32, True), ("rows", own, False), ("rounded", rounded, True)):
        for prog in (("edge", 13), ("interior", 8)):
            for kind in ("aligned", "y-null", "in-place"):
                add(f"dia-{prog[0]}{prog[1]}-{tag}-{kind}", "dia", sq, prog, pitch, kind, _placement_route(letter, kind, wide))
    for kind in ("z-shifted", "x-shifted"):
        add(f"dia-edge13-rows-{kind}", "dia", sq, ("edge", 13), own, kind, "narrow")
    # diagonal counts of DIA: none, less than a stage, a stage, one more, two stages, one more
    for k in (0, 1, 3, 4, 5, 9):
        prog = ("interior" if k % 2 else "edge", k)
        add(f"dia-{prog[0]}{k}-alloc-count", "dia", sq, prog, alloc, "aligned", _placement_route(letter, "aligned", True))
        add(f"dia-{prog[0]}{k}-rows-count", "dia", sq, prog, own, "aligned", "narrow")
    # small and rectangular shapes, both kernels: hack 4 and hack 3; the allocation pitch and, narrow by a shifted dM, the same
    for shape in SMALL_SHAPES + RECT_SHAPES:
        rows, cols = shape
        tag = f"{rows}x{cols}"
        progs = ("all",) if rows < N else ("cycle", "interior")
        for prog in progs:
            for kind in ("aligned", "y-null"):
                add(f"hdia-{prog}-{tag}-h4-{kind}", "hdia", shape, prog, 4, kind, _placement_route(letter, kind, True))
                add(f"hdia-{prog}-{tag}-h3-{kind}", "hdia", shape, prog, 3, kind, "narrow")
        for prog in (("edge", 13), ("interior", 8)):
            add(f"dia-{prog[0]}{prog[1]}-{tag}-alloc-aligned", "dia", shape, prog, dia_alloc_pitch(rows), "aligned",
                _placement_route(letter, "aligned", True))
            add(f"dia-{prog[0]}{prog[1]}-{tag}-alloc-dM-shifted", "dia", shape, prog, dia_alloc_pitch(rows), "dM-shifted", "narrow")
            add(f"dia-{prog[0]}{prog[1]}-{tag}-alloc-z-shifted", "dia", shape, prog, dia_alloc_pitch(rows), "z-shifted",
                _placement_route(letter, "z-shifted", True))
    return c


_MATRICES = {}


def matrix_key(case):
    return (case["fmt"], case["letter"], case["shape"], case["prog"], case["hp"])


def matrix_of(case):
    """The host matrix of a case, built once and left unchanged."""
    key = matrix_key(case)
    if key not in _MATRICES:
        rows, cols = case["shape"]
        build = hdia_matrix if case["fmt"] == "hdia" else dia_matrix
        _MATRICES[key] = build(case["letter"], rows, cols, case["hp"], case["prog"])
    return _MATRICES[key]


def operands(letter, rows, cols):
    """x [cols] and y [rows], the same for every case of one letter and shape."""
    return values(letter, ("x", cols), cols), values(letter, ("y", rows), rows)


def case_branches(case):
    rpl, wide_io = case["want"]
    beta = case["scalars"][1]
    return branches(matrix_of(case), case["letter"], rpl, wide_io, beta != 0, offsets_of(case["letter"], case["shift"])["x"])
