"""The constants of the HDIA / DIA SpMM dispatch (spgpu_amd/csrc/hdia_spmm.hip), the dispatch restated as a function of what a
caller passes, and the case table tests/test_gpu_hdia_spmm.py runs, stated once for that module (which runs them on the GPU) and for
tests/test_hdia_spmm_launch_shapes.py (which checks on the CPU that the table reaches every instantiation, with wideIO on and off,
and every composition of passes).  No torch, no library: importable everywhere.

The matrices are those of tests/hdia_launch_shapes.py, imported: hand-built, NaN in every slot that no product may use."""
import hdia_launch_shapes as H

# ---- the constants of the dispatch, with the line that sets each: a change there is a test to revisit here -------------------
THREADS = 512                 # hdia_spmm.hip:49     kHdiaMmThreads: lanes (strips) per workgroup
MAX_V = 8                     # hdia_spmm.hip:50     kHdiaMmMaxV: vectors of a full pass
KERNEL_V = (1, 2, 4, 8)       # hdia_spmm.hip:229-239  launchHdiaMmPass: the smallest of these that holds the vectors of a pass
UNROLL = {"S": {1: 4, 2: 4, 4: 2, 8: 1}, "D": {1: 4, 2: 4, 4: 2, 8: 2}}   # hdia_spmm.hip:55  hdiaMmUnroll: diagonals per stage
LETTERS = "SD"
WIDE = {L: H.WIDE[L] for L in LETTERS}      # hdia_spmm.hip:259   rows per lane of the wide kernel: S 4, D 2
SPMV = "spmv"                 # hdia_spmm.hip:282-332  count == 1: the call is spgpu?hdiaspmv / spgpu?diaspmv itself
ALIGNED = dict(dM=0, z=0, y=0, x=0)


def kernel_name(letter, rpl, v):
    """The instantiation as the profiler prints it (inside `void spgpu::...(spgpu::HdiaMmArgs<T>)`)."""
    return f"hdiaSpmmMvKernel<{H.CTYPE[letter]}, {rpl}, {v}>"


def every_instantiation():
    """The sixteen: S and D, wide and narrow, for 1, 2, 4 and 8 vectors."""
    return [(L, r, v) for L in LETTERS for r in (WIDE[L], 1) for v in KERNEL_V]


def kernel_v(nvec):
    """launchHdiaMmPass (hdia_spmm.hip:229-239) restated."""
    return 1 if nvec <= 1 else 2 if nvec <= 2 else 4 if nvec <= 4 else MAX_V


def dispatch(letter, hack_or_pitch, off, pitch_yz, count, has_y=True):
    """hdiaSpmmMv (hdia_spmm.hip:259-274) and the entry points' first lines restated: the passes of one call, each
    (RPL, V, wideIO, vectors).  `off`: bytes by which dM, z, y and x lie past a 16-byte boundary (x changes no choice); without y
    (NULL, address 0) nothing of y is off its boundary.  No call for count <= 0; count == 1 is the SpMV: [(RPL, SPMV, wideIO, 1)]
    with the SpMV's own choice."""
    if count <= 0 or hack_or_pitch <= 0:
        return []
    if count == 1:
        rpl, wide_io = H.dispatch(letter, hack_or_pitch, off, has_y)
        return [(rpl, SPMV, wide_io, 1)]
    size = H.SIZEOF[letter]
    wide_ok = hack_or_pitch % WIDE[letter] == 0 and off["dM"] % 16 == 0
    wide_io = int(not wide_ok or (off["z"] % 16 == 0 and (not has_y or off["y"] % 16 == 0) and pitch_yz * size % 16 == 0))
    rpl = WIDE[letter] if wide_ok else 1
    out = []
    for first in range(0, count, MAX_V):
        nvec = min(MAX_V, count - first)
        out.append((rpl, kernel_v(nvec), wide_io, nvec))
    return out


# ---- pass compositions, written out by hand ---------------------------------------------------------------------------------------
#: count -> the (V, vectors) of its passes
PASSES = {
    1: ((SPMV, 1),),
    2: ((2, 2),),
    3: ((4, 3),),
    7: ((8, 7),),
    8: ((8, 8),),
    9: ((8, 8), (1, 1)),
    10: ((8, 8), (2, 2)),
    11: ((8, 8), (4, 3)),
    13: ((8, 8), (8, 5)),
    16: ((8, 8), (8, 8)),
    19: ((8, 8), (8, 8), (4, 3)),
}
COUNTS = (1, 2, MAX_V - 1, MAX_V, MAX_V + 1, 2 * MAX_V + 3)       # every case family runs these
MORE_COUNTS = (3, 10, 11, 13, 16)                                 # the remaining compositions, on the hack-32 matrices
#: the compositions the table must reach, by name
COMPOSITIONS = {
    "single partial pass": lambda p: len(p) == 1 and p[0][0] != SPMV and p[0][1] < p[0][0],
    "single partial pass that fills its kernel": lambda p: len(p) == 1 and p[0][0] not in (SPMV, MAX_V) and p[0][1] == p[0][0],
    "exactly one full pass": lambda p: p == ((MAX_V, MAX_V),),
    "full + remainder 1": lambda p: p == ((MAX_V, MAX_V), (1, 1)),
    "full + remainder 2": lambda p: p == ((MAX_V, MAX_V), (2, 2)),
    "full + remainder 4": lambda p: p == ((MAX_V, MAX_V), (4, 3)),
    "full + partial 8": lambda p: len(p) == 2 and p[0] == (MAX_V, MAX_V) and p[1][0] == MAX_V and p[1][1] < MAX_V,
    "two full passes": lambda p: p == ((MAX_V, MAX_V), (MAX_V, MAX_V)),
    "two full passes + remainder": lambda p: len(p) == 3 and p[:2] == ((MAX_V, MAX_V), (MAX_V, MAX_V)),
    "the SpMV itself": lambda p: p == ((SPMV, 1),),
}

# ---- pitches ----------------------------------------------------------------------------------------------------------------------
PITCHES = ("tight", "rounded", "rounded+5")


def pitch_of(letter, kind, n):
    """The element stride of vectors of n elements: n itself; n rounded up to 16 bytes; that plus 5 elements (off 16 bytes again
    for both letters: 20 and 40 bytes)."""
    w = WIDE[letter]
    rounded = (n + w - 1) // w * w
    return {"tight": n, "rounded": rounded, "rounded+5": rounded + 5}[kind]


#: scalars and how Y is passed: kind -> (y mode, (alpha, beta)).  y modes as tests/hdia_launch_shapes.py: `null` Y == NULL, `nan` a
#: multivector full of NaN that beta == 0 must keep unread, `y` a multivector of its own, `z` Z == Y
SCALARS = {
    "y-null": ("null", H.PLAIN),
    "y-unread": ("nan", (-0.75, 0.0)),
    "with-y": ("y", H.WITH_Y),
    "in-place": ("z", H.IN_PLACE),
}
#: the arrays that start one element past a 16-byte boundary, in turn
SHIFTS = {"aligned": (), "dM-shifted": ("dM",), "z-shifted": ("z",), "y-shifted": ("y",), "x-shifted": ("x",)}
HACKS = (1, 2, 30, 32, 33, 64, 4512)
#: the hack sizes of HACKS at which the wide kernel runs (hackSize % WIDE == 0), written out by hand
WIDE_HACKS = {"S": (32, 64, 4512), "D": (2, 30, 32, 64, 4512)}
SMALL_SHAPES = ((1, 1), (5, 700), (300, 3), (300, 1))


def _want(letter, wide_matrix, shift, pitch_kind, scalars, rows, count):
    """Written out, not computed by dispatch(): the passes (RPL, V, wideIO, vectors) a case is there for."""
    y_mode = SCALARS[scalars][0]
    if count == 1:      # the SpMV's own dispatch: one vector, no pitch
        wide = wide_matrix and "dM" not in shift
        late = "z" in shift or ("y" in shift and y_mode in ("y", "nan"))
        return ((WIDE[letter] if wide else 1, SPMV, int(not wide or not late), 1),)
    wide = wide_matrix and "dM" not in shift
    rpl = WIDE[letter] if wide else 1
    pitch_on_16 = pitch_kind == "rounded" or (pitch_kind == "tight" and rows % WIDE[letter] == 0)
    y_late = "y" in shift and y_mode in ("y", "nan")      # Z == Y lies where Z does, whatever the case says of y
    wide_io = int(not wide or (pitch_on_16 and "z" not in shift and not y_late))
    return tuple((rpl, v, wide_io, n) for v, n in PASSES[count])


def _case(cid, fmt, letter, shape, prog, hp, wide_matrix, shift, pitch, scalars, count):
    return dict(id=cid, fmt=fmt, letter=letter, shape=shape, prog=prog, hp=hp, shift=SHIFTS[shift], shift_kind=shift, pitch=pitch,
                y_mode=SCALARS[scalars][0], scalars=SCALARS[scalars][1], scalars_kind=scalars, count=count,
                want=_want(letter, wide_matrix, SHIFTS[shift], pitch, scalars, shape[0], count))


def cases(letter):
    """id -> case.  A case: format, letter, shape, programme (HDIA) or offset list name (DIA), hack size or pitch of dM, the arrays
    that start one element late, the pitch kind of the multivectors, how Y is passed and (alpha, beta), the number of vectors, and the
    passes (RPL, V, wideIO, vectors) the call must be made of."""
    c = {}

    def add(fmt, shape, prog, hp, wide_matrix, shift, pitch, scalars, count, tag=None, again_ok=False):
        name = prog if isinstance(prog, str) else f"{prog[0]}{prog[1]}"
        cid = f"{fmt}-{name}-{tag or f'h{hp}'}-{shift}-{pitch}-{scalars}-n{count}"
        assert again_ok or cid not in c, cid      # again_ok: a sweep may come by a case an earlier family holds already
        c[cid] = _case(cid, fmt, letter, shape, prog, hp, wide_matrix, shift, pitch, scalars, count)

    sq = (H.N, H.N)
    alloc, alloc32, own, rounded = H.dia_pitches(letter, H.N)
    # every count (all compositions of passes) at every pitch, on matrices that allow the wide kernel: ragged and interior diagonals
    for count in COUNTS + MORE_COUNTS:
        for pitch in PITCHES:
            add("hdia", sq, "cycle", 32, True, "aligned", pitch, "with-y", count)
            add("dia", sq, ("edge", 13), alloc, True, "aligned", pitch, "with-y", count, "alloc")
        add("hdia", sq, "interior", 32, True, "aligned", "rounded", "with-y", count)
        add("dia", sq, ("interior", 8), alloc, True, "aligned", "rounded", "with-y", count, "alloc")
        # ... and in the narrow kernels: dM one element late
        add("hdia", sq, "cycle", 32, True, "dM-shifted", "tight", "with-y", count)
    # every placement and every way of passing Y, at the pitch where placement decides wideIO, count V + 1 and 2 V + 3
    for shift in SHIFTS:
        for scalars in SCALARS:
            for count in (MAX_V + 1, 2 * MAX_V + 3):
                if (shift, scalars) != ("aligned", "with-y"):
                    add("hdia", sq, "cycle", 32, True, shift, "rounded", scalars, count)
                if shift != "dM-shifted" and count == MAX_V + 1:
                    add("hdia", sq, "interior", 32, True, shift, "tight", scalars, count)
                    add("dia", sq, ("interior", 8), alloc, True, shift, "rounded+5", scalars, count, "alloc")
    # every hack size, every programme: the counts, pitches and scalars taken in turn, so that each of them meets each kernel shape
    turn = 0
    for hack in HACKS:
        wide = hack in WIDE_HACKS[letter]
        for prog in ("cycle", "runs", "interior"):
            for k in range(2):
                count = COUNTS[1:][(turn + 2 * k) % 5]
                pitch = PITCHES[(turn + k) % 3]
                scalars = tuple(SCALARS)[(turn // 3 + k) % 4]
                add("hdia", sq, prog, hack, wide, "aligned", pitch, scalars, count, again_ok=True)
            turn += 1
    # every DIA pitch, both kinds of offsets; the rows themselves are odd, so that pitch is the narrow kernel's
    for tag, pitch_dm, wide in (("alloc+32", alloc32, True), ("rows", own, False), ("rounded", rounded, True)):
        for prog in (("edge", 13), ("interior", 8)):
            for count, pitch, scalars in ((2, "tight", "y-null"), (MAX_V - 1, "rounded", "with-y"), (MAX_V + 1, "rounded+5", "in-place"),
                                          (2 * MAX_V + 3, "rounded", "y-unread"), (1, "tight", "with-y")):
                add("dia", sq, prog, pitch_dm, wide, "aligned", pitch, scalars, count, tag)
    # small and rectangular shapes, both kernels: hack 4 and hack 3, the allocation pitch and the rows
    for shape in SMALL_SHAPES + H.RECT_SHAPES:
        rows, cols = shape
        tag = f"{rows}x{cols}"
        progs = ("all",) if rows < H.N else ("cycle", "interior")
        for prog in progs:
            for count, pitch, scalars in ((2, "tight", "with-y"), (MAX_V + 1, "rounded", "with-y"), (2 * MAX_V + 3, "rounded+5", "y-null")):
                add("hdia", shape, prog, 4, True, "aligned", pitch, scalars, count, f"{tag}-h4")
                add("hdia", shape, prog, 3, False, "aligned", pitch, scalars, count, f"{tag}-h3")
        for prog in (("edge", 13), ("interior", 8)):
            for count, pitch, scalars in ((MAX_V - 1, "tight", "with-y"), (MAX_V + 1, "rounded", "in-place")):
                add("dia", shape, prog, H.dia_alloc_pitch(rows), True, "aligned", pitch, scalars, count, f"{tag}-alloc")
                add("dia", shape, prog, rows, rows % WIDE[letter] == 0, "aligned", pitch, scalars, count, f"{tag}-rows")
    return c


def matrix_key(case):
    return H.matrix_key(case)


def matrix_of(case):
    """The host matrix of a case (tests/hdia_launch_shapes.py builds it once and leaves it unchanged)."""
    return H.matrix_of(case)


def operands(letter, rows, cols, j):
    """Vector j of X [cols] and of Y [rows]: the same for every case of one letter and shape.  Vector 0 is hdia_launch_shapes.operands."""
    if j == 0:
        return H.operands(letter, rows, cols)
    return H.values(letter, ("x", cols, j), cols), H.values(letter, ("y", rows, j), rows)


def offsets_of(case):
    """Byte offsets from a 16-byte boundary of dM, z, y, x of a case; Z == Y: y lies where z does."""
    off = H.offsets_of(case["letter"], case["shift"])
    if case["y_mode"] == "z":
        off["y"] = off["z"]
    if case["y_mode"] == "null":
        off["y"] = 0
    return off


def case_dispatch(case):
    """dispatch() on what a case passes."""
    rows, _ = case["shape"]
    return tuple(dispatch(case["letter"], case["hp"], offsets_of(case), pitch_of(case["letter"], case["pitch"], rows), case["count"],
                          case["y_mode"] != "null"))
