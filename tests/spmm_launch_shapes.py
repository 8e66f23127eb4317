"""The constants of the SpMM dispatch (spgpu_amd/csrc/hell_spmm.hip; kernels in spmm_rows.hip.h and spmm_strip.hip.h), both
dispatches restated as a function of what a caller passes, and the matrices tests/test_gpu_spmm_shapes.py runs them on, stated once for that module (which runs them on the GPU) and
for tests/test_spmm_launch_shapes.py (which checks on the CPU that the matrices have the windows each kernel branch needs and that
the case table names every instantiation).  No torch, no library: importable everywhere."""
import numpy as np

# ---- the constants of the dispatch, with the name that sets each: a change there is a test to revisit here -------------------
PASS = 16                     # kSpmmPass: right-hand sides of one pass
THREADS = 256                 # kSpmmThreads: 256 rows per workgroup
WAVE = 64                     # rows per wavefront
SPMM_TILE_BYTES = 43 * 1024   # kSpmmTileBytes (the tiled one-row-per-lane kernel)
STRIP_TILE_BYTES = 40 * 1024  # kStripTileBytes (the strip kernel)
SLAB_HEAD = 32                # kStageCols * HEAD (hellSpmmStripKernel): slab columns whose indices the strip kernel keeps in registers
SIZEOF = {"S": 4, "D": 8}
CTYPE = {"S": "float", "D": "double"}


def strip_tile_rows(letter, vec):
    """launchSpmmStrips<T, TRIP, VEC>: a.tileRows"""
    return STRIP_TILE_BYTES // (8 * vec * SIZEOF[letter])


def tiled_tile_rows(letter, kp=8, vec=2):
    """launchSpmm<T, 8, 2, 4, true>: a.tileRows"""
    return SPMM_TILE_BYTES // (kp * vec * SIZEOF[letter])


def mv_strip_tile_rows(letter, vec):
    """launchSpmmStrips<T, TRIP, VEC, true>: the window's low end is rounded down to a 16-byte piece, the rows that costs
    are kept free"""
    return STRIP_TILE_BYTES // (8 * vec * SIZEOF[letter]) - (16 // SIZEOF[letter] - 1)


def all_tile_rows():
    return sorted({f(L, v) for L in "SD" for v in (1, 2) for f in (strip_tile_rows, mv_strip_tile_rows)}
                  | {tiled_tile_rows(L) for L in "SD"})


def strip_name(letter, vec, pitch=False):
    return f"hellSpmmStripKernel<{CTYPE[letter]}, 2, {vec}, {'true' if pitch else 'false'}>"


def plain_name(letter, kp, vec, unroll, tiled=False, pitch=False):
    return f"hellSpmmKernel<{CTYPE[letter]}, {kp}, {vec}, {unroll}, {'true' if tiled else 'false'}, {'true' if pitch else 'false'}>"


ALIGNED = dict(cM=0, rP=0, X=0, Y=0, Z=0)


def interleaved_passes(letter, hack, count, ldx, ldyz, r_idx=False, off=ALIGNED, has_y=True):
    """hellSpmm<T, false> restated: matrixLoads16, spmmShape (enum SpmmShape) and launchSpmmStrips' directFill.  `off`: bytes by
    which cM, rP, X, Y, Z lie past a 16-byte boundary.
    Returns, per pass of 16, (kernel name as the profiler prints it, directFill) -- directFill is None off the strip kernel.
    r_idx changes no choice of this call; it is an argument so that both dispatches take the same ones."""
    size = SIZEOF[letter]
    pair = 2 * size
    pairs_ok = (ldx % 2 == 0 and ldyz % 2 == 0 and off["X"] % pair == 0 and off["Z"] % pair == 0
                and (not has_y or off["Y"] % pair == 0))
    matrix16 = hack % 32 == 0 and off["cM"] % 16 == 0 and off["rP"] % 16 == 0
    out = []
    for first in range(0, count, PASS):
        n = min(PASS, count - first)
        pairs = pairs_ok and n % 2 == 0
        x_off = (off["X"] + first * size) % 16

        def strips(vec):
            direct = n == 8 * vec and (8 * vec * size) % 16 == 0 and x_off == 0 and (ldx * size) % 16 == 0
            return strip_name(letter, vec), bool(direct)

        if n > 8:
            if pairs and matrix16:
                out.append(strips(2))
            elif pairs:
                out.append((plain_name(letter, 8, 2, 4, tiled=True), None))
            else:
                out.append((plain_name(letter, 16, 1, 2), None))
        elif n > 4:
            if matrix16:
                out.append(strips(1))
            elif pairs:
                out.append((plain_name(letter, 4, 2, 4), None))
            else:
                out.append((plain_name(letter, 8, 1, 2), None))
        else:
            if n == 4 and matrix16:
                out.append(strips(1))
            else:
                out.append((plain_name(letter, 4, 1, 4), None))
    return out


def mv_passes(letter, hack, count, pitch_x, pitch_yz, r_idx=False, off=ALIGNED, has_y=True):
    """hellSpmm<T, true> restated (matrixLoads16, spmmMvShape, a.wideRuns): per pass, (kernel name, wideRuns)."""
    size = SIZEOF[letter]
    matrix16 = hack % 32 == 0 and off["cM"] % 16 == 0 and off["rP"] % 16 == 0
    out = []
    for first in range(0, count, PASS):
        n = min(PASS, count - first)
        wide = (not r_idx and (off["X"] + first * pitch_x * size) % 16 == 0 and (off["Z"] + first * pitch_yz * size) % 16 == 0
                and (not has_y or (off["Y"] + first * pitch_yz * size) % 16 == 0)
                and (pitch_x * size) % 16 == 0 and (pitch_yz * size) % 16 == 0)
        if matrix16:
            out.append((strip_name(letter, 2 if n > 8 else 1, pitch=True), bool(wide)))
        else:
            out.append((plain_name(letter, 16, 1, 2, pitch=True), bool(wide)))
    return out


def every_interleaved_instantiation(letter):
    return [strip_name(letter, 2), strip_name(letter, 1), plain_name(letter, 8, 2, 4, tiled=True), plain_name(letter, 16, 1, 2),
            plain_name(letter, 4, 2, 4), plain_name(letter, 8, 1, 2), plain_name(letter, 4, 1, 4)]


def every_mv_instantiation(letter):
    return [strip_name(letter, 2, pitch=True), strip_name(letter, 1, pitch=True), plain_name(letter, 16, 1, 2, pitch=True)]


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
ROWS = 2 * THREADS + WAVE + 37   # 613: two full workgroups, a third with one full and one partial wavefront
COLS = 4000
MAX_LEN = 40                     # > SLAB_HEAD: the strip kernel reads the last columns of such rows a second way
UNIFORM_WAVE = 1                 # rows 64..127: every row 24 long (ALL_PRESENT through all their columns)
UNIFORM_LEN = 24
EMPTY_WAVE = 6                   # rows 384..447: no entries
NARROW_WINDOW = 200              # all columns of a `narrow` workgroup lie inside this many columns
WIDE_SPREAD = 2000               # `wide_*` workgroups span more than this
PROBE_SPREAD = 100               # `wide_after_scan`: first columns within this of each other
ZERO_SCALE_CAP = 0.15            # share of (row, rhs) elements with scale 0 (rows without entries, beta == 0): a condition
PATTERNS = ("narrow", "wide_at_probe", "wide_after_scan", "empty", "band")
MIXED = ("narrow", "wide_after_scan", "wide_at_probe")
NAMED = {"mixed": MIXED, "band": ("band",) * 3, "narrow": ("narrow",) * 3, "empty_group": ("wide_after_scan", "empty", "narrow")}


def workgroups():
    return [(lo, min(lo + THREADS, ROWS)) for lo in range(0, ROWS, THREADS)]


def matrix(patterns="mixed", base=0, seed=0):
    """COO of the test matrix in row order (a row's entries in the order they are stored: slab column k = position in the row).

    patterns: a name of NAMED or one pattern per workgroup.  Returns a dict: rows, cols (both 0-based), lengths [ROWS], hole (bool
    per entry; all False for base 0).  An entry with hole set keeps its place in the row -- it counts in the row's length -- but its
    stored column is 0 in the 1-based arrays, below the base: the caller plants that in the HELL arrays, and every reference drops
    those entries.  Column 0 is named by no entry, so that row 0 of X is read only on behalf of absent entries."""
    patterns = NAMED.get(patterns, patterns) if isinstance(patterns, str) else tuple(patterns)
    assert len(patterns) == len(workgroups()) and all(p in PATTERNS for p in patterns)
    rng = np.random.default_rng([seed, base] + [PATTERNS.index(p) for p in patterns])
    lengths = rng.integers(1, MAX_LEN + 1, size=ROWS)
    lengths[rng.choice(ROWS, size=15, replace=False)] = 0
    lengths[UNIFORM_WAVE * WAVE:(UNIFORM_WAVE + 1) * WAVE] = UNIFORM_LEN
    lengths[EMPTY_WAVE * WAVE:(EMPTY_WAVE + 1) * WAVE] = 0
    for g, (lo, hi) in enumerate(workgroups()):
        if patterns[g] == "empty":
            lengths[lo:hi] = 0
        if patterns[g] == "band":
            # whole wavefronts of equal rows, a multiple of 8 long and at most 32; wavefront 3 of a workgroup stays ragged
            for w0 in range(lo, hi, WAVE):
                w = w0 // WAVE
                if w not in (EMPTY_WAVE, UNIFORM_WAVE) and w % 4 != 3:
                    lengths[w0:min(w0 + WAVE, hi)] = (8, 16, UNIFORM_LEN, 32)[(w + 2) % 4]
    r_parts, c_parts = [], []
    for g, (lo, hi) in enumerate(workgroups()):
        start = 1 + g * 1100                     # column 0 is never named
        kind = patterns[g]
        long_rows = [r for r in range(lo, hi) if lengths[r] > SLAB_HEAD]
        for r in range(lo, hi):
            n = int(lengths[r])
            if n == 0:
                continue
            if kind == "narrow":
                c = np.sort(rng.choice(np.arange(start, start + NARROW_WINDOW), size=n, replace=False))
                if r == lo + 2:                   # the window's ends are named
                    c[0] = start
                if r == lo + 4:
                    c[-1] = start + NARROW_WINDOW - 1
            elif kind == "band":
                c = start + (r - lo) + np.arange(n)   # row r + 1 is row r shifted by one, entries ascending by one
            elif kind == "wide_at_probe":
                c = np.sort(rng.choice(np.arange(1, COLS), size=n, replace=False))
                if r == lo + 1:                   # two first columns more than WIDE_SPREAD apart, whatever the draw
                    c[0] = 1
                if r == lo + 3:
                    c = np.sort(rng.choice(np.arange(COLS - 600, COLS), size=n, replace=False))
            else:
                # wide_after_scan: the first columns within PROBE_SPREAD of each other and the first SLAB_HEAD slab columns inside
                # the narrow window -- what the strip kernel sees before it scans --, the slab columns behind them anywhere
                first = start + int(rng.integers(0, PROBE_SPREAD))
                head = min(n, SLAB_HEAD) - 1
                near = np.sort(rng.choice(np.arange(first + 1, start + NARROW_WINDOW), size=head, replace=False))
                far = np.sort(rng.choice(np.arange(start + NARROW_WINDOW, COLS - 1), size=n - 1 - head, replace=False))
                if r == long_rows[0]:
                    far[-1] = COLS - 1
                if r == long_rows[1]:
                    far[0] = start + NARROW_WINDOW
                c = np.concatenate([[first], near, far])
            assert c.size == n and c.min() >= 1 and c.max() < COLS and np.unique(c).size == n, (kind, r)
            r_parts.append(np.full(n, r, np.int64))
            c_parts.append(np.asarray(c, np.int64))
    rows = np.concatenate(r_parts)
    cols = np.concatenate(c_parts)
    hole = np.zeros(rows.size, bool)
    if base == 1:
        wave_of = rows // WAVE
        band_rows = np.zeros(ROWS, bool)
        for g, (lo, hi) in enumerate(workgroups()):
            band_rows[lo:hi] = patterns[g] == "band"
        k = np.arange(rows.size) - np.repeat(np.cumsum(lengths) - lengths, lengths)
        # one entry in 23, never a row's first (the probes of `wide_after_scan` stay what they are), never in the uniform
        # wavefront, and in band workgroups only in the ragged wavefronts: a band stays a band
        can = (k > 0) & (wave_of != UNIFORM_WAVE) & ~(band_rows[rows] & (wave_of % 4 != 3))
        hole = can & (rng.random(rows.size) < 1.0 / 23)
    return dict(rows=rows, cols=cols, lengths=lengths.astype(np.int32), hole=hole, base=base, patterns=patterns)


def used(m):
    """(rows, cols) of the entries a product uses: the holes dropped."""
    keep = ~m["hole"]
    return m["rows"][keep], m["cols"][keep]


def window_of(m, group, first_only=False):
    """(lo, hi) of the 0-based columns the rows of workgroup `group` use (first_only: their first stored entries, holes included:
    no hole is a row's first), or None if they use none."""
    lo, hi = workgroups()[group]
    sel = (m["rows"] >= lo) & (m["rows"] < hi) & ~m["hole"]
    if first_only:
        starts = np.cumsum(m["lengths"]) - m["lengths"]
        first = np.zeros(m["rows"].size, bool)
        first[starts[m["lengths"] > 0]] = True
        sel &= first
    if not sel.any():
        return None
    return int(m["cols"][sel].min()), int(m["cols"][sel].max())


def values(letter, seed, n):
    """Values in [-1, -0.25] and [0.25, 1]: no product is tiny beside its row's scale by accident of the draw."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    return v.astype(np.float32 if letter == "S" else np.float64)


# ---- the cases of tests/test_gpu_spmm_shapes.py ---------------------------------------------------------------------------------
def case(count, hack=32, ldx=None, ldyz=None, shift=(), want=None):
    """One call of the interleaved API.  shift: names of cM, rP, X, Y, Z moved one element (or `X2`: X by two) off a 16-byte
    boundary.  want: (kernel tag, directFill) of every pass.  betas: 0 stands for Y == NULL; a case that is there for a
    shifted Y has no such call (without Y nothing is off its boundary and another kernel runs)."""
    return dict(count=count, hack=hack, ldx=count if ldx is None else ldx, ldyz=count if ldyz is None else ldyz,
                shift=tuple(shift), want=want, betas=(0.5,) if "Y" in shift else (0.0, 0.5))


def offsets(letter, shift):
    """Byte offsets from a 16-byte boundary of the five arrays for a case's `shift`."""
    off = dict(ALIGNED)
    for name in shift:
        if name == "X2":
            off["X"] = 2 * SIZEOF[letter]
        elif name == "rP":
            off["rP"] = 4
        else:
            off[name] = SIZEOF[letter]
    return off


def interleaved_cases(letter):
    """The table of the issue: id -> case.  `want` is a tuple of (short kernel tag, directFill) per pass; the tags are the members
    of enum SpmmShape: strip2, strip1, tiled, k16, k4x2, k8x1, k4x1."""
    c = {}
    # strip kernel, two per lane, directFill on
    for hack in (32, 64, 96):
        c[f"strip2-direct-h{hack}"] = case(16, hack, want=(("strip2", True),))
    # the same, directFill off
    c["strip2-count12"] = case(12, want=(("strip2", False),))
    # ldX = 18: rows of 72 bytes in fp32; in fp64 every even ldX gives 16-byte rows, so there the fill stays direct
    c["strip2-ldx18"] = case(16, ldx=18, want=(("strip2", letter == "D"),))
    if letter == "S":
        c["strip2-x-shifted-by-two"] = case(16, shift=("X2",), want=(("strip2", False),))
    # strip kernel, one per lane, directFill on
    c["strip1-direct-count8"] = case(8, want=(("strip1", True),))
    # count 4 with ldX = 4: the strip kernel with half of each team idle; directFill needs all 8 right-hand sides
    # (launchSpmmStrips), so it is off here for both types
    c["strip1-count4-ld4"] = case(4, want=(("strip1", False),))
    # the same, directFill off
    c["strip1-count5"] = case(5, ldx=6, want=(("strip1", False),))
    c["strip1-count7"] = case(7, ldx=8, ldyz=8, want=(("strip1", False),))
    c["strip1-odd-ldx"] = case(8, ldx=9, want=(("strip1", False),))
    c["strip1-x-shifted"] = case(8, shift=("X",), want=(("strip1", False),))
    # tiled one-row-per-lane kernel
    c["tiled-count10-h48"] = case(10, 48, want=(("tiled", None),))
    c["tiled-count16-h48"] = case(16, 48, want=(("tiled", None),))
    c["tiled-cM-shifted"] = case(16, 32, shift=("cM",), want=(("tiled", None),))
    c["tiled-rP-shifted"] = case(16, 32, shift=("rP",), want=(("tiled", None),))
    # plain, 16 lanes x 1
    for hack in (32, 48):
        c[f"k16-count11-h{hack}"] = case(11, hack, ldx=12, ldyz=12, want=(("k16", None),))
        c[f"k16-odd-ldx-h{hack}"] = case(16, hack, ldx=17, want=(("k16", None),))
        c[f"k16-odd-ldyz-h{hack}"] = case(16, hack, ldyz=17, want=(("k16", None),))
        for name in "XZY":
            c[f"k16-{name}-shifted-h{hack}"] = case(16, hack, shift=(name,), want=(("k16", None),))
    # plain, 4 lanes x 2
    c["k4x2-count6-h48"] = case(6, 48, want=(("k4x2", None),))
    c["k4x2-count8-h48"] = case(8, 48, want=(("k4x2", None),))
    c["k4x2-cM-shifted"] = case(8, 32, shift=("cM",), want=(("k4x2", None),))
    # plain, 8 lanes x 1
    c["k8x1-count5-h48"] = case(5, 48, want=(("k8x1", None),))
    c["k8x1-count7-h48"] = case(7, 48, ldx=8, want=(("k8x1", None),))
    c["k8x1-count6-odd-ldx-h48"] = case(6, 48, ldx=7, want=(("k8x1", None),))
    # plain, 4 lanes x 1
    c["k4x1-count1"] = case(1, 32, want=(("k4x1", None),))
    c["k4x1-count2-h64"] = case(2, 64, want=(("k4x1", None),))
    c["k4x1-count3-h48"] = case(3, 48, ldx=4, ldyz=5, want=(("k4x1", None),))
    c["k4x1-count4-h48"] = case(4, 48, want=(("k4x1", None),))
    # passes of different kernels
    c["passes-19"] = case(19, want=(("k16", None), ("k4x1", None)))                           # ld 19 is odd: no pairs
    c["passes-19-ld20"] = case(19, ldx=20, ldyz=20, want=(("strip2", True), ("k4x1", None)))
    c["passes-20"] = case(20, want=(("strip2", True), ("strip1", False)))
    c["passes-24"] = case(24, want=(("strip2", True), ("strip1", True)))
    c["passes-27-ld28"] = case(27, ldx=28, ldyz=28, want=(("strip2", True), ("k16", None)))
    c["passes-33"] = case(33, want=(("k16", None), ("k16", None), ("k4x1", None)))            # ld 33 is odd
    c["passes-33-ld36"] = case(33, ldx=36, ldyz=36, want=(("strip2", True), ("strip2", True), ("k4x1", None)))
    c["passes-24-h48"] = case(24, 48, want=(("tiled", None), ("k4x2", None)))
    return c


def tag_name(letter, tag, pitch=False):
    return {"strip2": strip_name(letter, 2, pitch), "strip1": strip_name(letter, 1, pitch),
            "tiled": plain_name(letter, 8, 2, 4, tiled=True), "k16": plain_name(letter, 16, 1, 2, pitch=pitch),
            "k4x2": plain_name(letter, 4, 2, 4), "k8x1": plain_name(letter, 8, 1, 2), "k4x1": plain_name(letter, 4, 1, 4)}[tag]


def expected_passes(letter, c, pitch=False):
    return [(tag_name(letter, tag, pitch), flag) for tag, flag in c["want"]]


#: one case per interleaved instantiation, for the rIdx, in-place and NaN-row tests (ids of interleaved_cases)
ONE_EACH = ("strip2-direct-h32", "strip2-count12", "strip1-direct-count8", "strip1-count7", "tiled-count10-h48", "k16-count11-h48",
            "k4x2-count6-h48", "k8x1-count5-h48", "k4x1-count3-h48")


def mv_case(count, hack=32, extra_x=0, extra_yz=0, shift=(), r_idx=False, want=None):
    """One call of the pitch-layout API: pitches are the vector lengths rounded up to 16 bytes' worth plus `extra` elements."""
    return dict(count=count, hack=hack, extra_x=extra_x, extra_yz=extra_yz, shift=tuple(shift), r_idx=r_idx, want=want,
                betas=(0.5,) if tuple(shift) == ("Y",) else (0.0, 0.5))


def mv_pitches(letter, c):
    per16 = 16 // SIZEOF[letter]
    up = lambda n: (n + per16 - 1) // per16 * per16
    return up(COLS) + c["extra_x"], up(ROWS) + c["extra_yz"]


def mv_cases(letter):
    """id -> case; want: (tag, wideRuns) per pass."""
    odd = 1 if letter == "D" else 2        # fp64: an odd pitch; fp32: a pitch that is no multiple of four
    c = {}
    c["strip2-wide"] = mv_case(16, want=(("strip2", True),))
    c["strip2-wide-h64-count12"] = mv_case(12, 64, extra_x=8, extra_yz=4, want=(("strip2", True),))
    c["strip2-x-shifted"] = mv_case(16, shift=("X",), want=(("strip2", False),))
    c["strip2-z-shifted"] = mv_case(16, shift=("Z",), want=(("strip2", False),))
    c["strip2-y-shifted"] = mv_case(16, shift=("Y",), want=(("strip2", False),))
    c["strip2-pitch-x"] = mv_case(16, extra_x=odd, want=(("strip2", False),))
    c["strip2-pitch-yz"] = mv_case(10, extra_yz=odd, want=(("strip2", False),))
    c["strip2-ridx"] = mv_case(16, r_idx=True, want=(("strip2", False),))
    c["strip1-wide-count8"] = mv_case(8, want=(("strip1", True),))
    c["strip1-wide-count3"] = mv_case(3, 96, want=(("strip1", True),))
    c["strip1-x-shifted"] = mv_case(5, shift=("X",), want=(("strip1", False),))
    c["strip1-pitch-yz"] = mv_case(7, extra_yz=odd, want=(("strip1", False),))
    c["strip1-ridx"] = mv_case(8, r_idx=True, want=(("strip1", False),))
    c["k16-h48"] = mv_case(16, 48, want=(("k16", True),))
    c["k16-h48-count5-shifted"] = mv_case(5, 48, shift=("X", "Z", "Y"), extra_x=odd, want=(("k16", False),))
    c["k16-cM-shifted"] = mv_case(16, 32, shift=("cM",), want=(("k16", True),))
    c["k16-rP-shifted-ridx"] = mv_case(9, 32, shift=("rP",), r_idx=True, want=(("k16", False),))
    c["passes-21"] = mv_case(21, want=(("strip2", True), ("strip1", True)))
    c["passes-21-pitch"] = mv_case(21, extra_x=odd, extra_yz=odd, want=(("strip2", False), ("strip1", False)))
    return c
