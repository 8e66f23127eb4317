"""The ELL / HELL SpMV for rows as they come (spgpu_amd/csrc/ellpack_spmv.hip: launchSlabFamily -> launchRowsAsTheyCome, on the
rules of spgpu_amd/csrc/spmv_rules.h, with slabSpmvKernel, sweepSpmvKernel and formProbeKernel), stated once for
tests/test_gpu_spmv_shapes.py (which runs the cases on the GPU), tests/test_spmv_launch_shapes.py (which checks on the CPU that the table
reaches every instantiation and every named branch) and tests/test_spmv_dispatch.py (which runs the header itself against this
restatement): the constants of the dispatch, the dispatch restated as a function of a call's arguments and addresses (spmv_rules.h:
wideLayout, wideIO, callerForm, autoVote, chooseRoute, slabShape, sweepShape, probeShape, slabGrid, sweepGrid), the control flow
of slabSpmvKernel and sweepSpmvKernel walked wavefront by wavefront, builders that place ELL and HELL matrices slot by slot, and
the case table.  No torch, no library: importable everywhere.

Scope: spgpu{S,D,C,Z}hellspmv / spgpu{S,D,C,Z}ellspmv with rIdx == NULL on matrices that are neither adopted nor frozen.

The matrices are written slot by slot in numpy.  Every padding slot (k >= the row's length) holds NaN under a valid column, the
rows of the last hack (HELL) or of the pitch (ELL) past `rows` are poisoned the same way, and an entry whose column lies below the
index base holds NaN too: no product may use any of them.

Left to tests/test_gpu_oell_device.py, which runs matrices of millions of rows anyway: the cap of 2 048 sweep workgroups and AUTO's
2 Mi-row threshold for the SWEEP form."""
import os
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")

# ---- the constants of the dispatch; header_constants() asks spmv_rules.h for the same and the CPU test compares ----------------------
WAVE = 64                     # spmv_rules.h   kRulesWave (== numeric.hip.h kWave)
BLOCK = 256                   # spmv_rules.h   kBlockThreads
TAIL_LANES = 16               # spmv_rules.h   kTailLanes
TAIL_UNROLL = 4               # spmv_rules.h   kTailUnroll
TILE_BYTES = 32768            # spmv_rules.h   kTileBytes: every x tile
TILED_BLOCK_S = 512           # spmv_rules.h   kTiledBlockFp32: the fp32 wide tile's workgroup
TAIL_EVERY = 8                # spmv_rules.h   kTailEvery: the tiled and lean kernels of the 8-byte types
LEAN_MAX_HINT = 8             # spmv_rules.h   kLeanMaxHint: avgNnzPerRow in 1 .. 8
LEAN_MAX_ELL = 16             # spmv_rules.h   kLeanMaxEll: ELL maxNnz <= 16
SWEEP_LANE_ROWS = 32          # spmv_rules.h   kSweepLaneRows: PACKS = 32 / VEC
SWEEP_PACKS_16 = 16           # spmv_rules.h   kSweepPacks16: PACKS of 16-byte elements
SWEEP_MAX_BLOCKS = 2048       # spmv_rules.h   kSweepMaxBlocks
AUTO_SWEEP_ROWS = 2 * 1024 * 1024   # spmv_rules.h kAutoSweepRows
SIZEOF = {"S": 4, "D": 8, "C": 8, "Z": 16}
WIDE = {L: 16 // s for L, s in SIZEOF.items()}
DTYPE = {"S": np.float32, "D": np.float64, "C": np.complex64, "Z": np.complex128}
CTYPE = {"S": "float", "D": "double", "C": "spgpu::Cx<float>", "Z": "spgpu::Cx<double>"}
LETTERS = "SDCZ"
AUTO, GATHER, STRIPS, XTILE, SWEEP = range(5)
FORM_NAME = {AUTO: "auto", GATHER: "gather", STRIPS: "strips", XTILE: "xtile", SWEEP: "sweep"}


_PROGRAMS = {}


def rules_program(directory, name):
    """tests/<name>.cpp, a stand-alone program around one of the rule headers of spgpu_amd/csrc, built into `directory` with the
    undefined-behaviour sanitizer (once per process): the path of the executable."""
    if name not in _PROGRAMS:
        exe = os.path.join(str(directory), name)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                        os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
        _PROGRAMS[name] = exe
    return _PROGRAMS[name]


def dispatch_program(directory):
    """tests/spmv_dispatch_cases.cpp, the program around spgpu_amd/csrc/spmv_rules.h."""
    return rules_program(directory, "spmv_dispatch_cases")


def header_constants(program):
    """name -> value, as the program's constants mode prints what spmv_rules.h states."""
    done = subprocess.run([program, "constants"], capture_output=True, text=True, check=True)
    return {name: int(value) for name, value in (line.split() for line in done.stdout.splitlines())}


# ---- the dispatch restated -------------------------------------------------------------------------------------------------------
def slab(letter, rpl, ph, hell, unroll, pipe, tail, strips=False, block=BLOCK, tile=0, tail_every=0):
    """slabSpmvKernel's template argument tuple: T, RPL, PH, IS_HELL, NT, UNROLL, PIPE, TAIL, STRIPS, BLOCK, TILE_BYTES, TAIL_EVERY, PACKED."""
    return ("slab", letter, rpl, ph, bool(hell), True, unroll, bool(pipe), bool(tail), bool(strips), block, tile, tail_every, False)


def sweep(letter, vec, hell, has_beta):
    """sweepSpmvKernel's: T, VEC, PACKS, IS_HELL, HAS_BETA, TAIL."""
    packs = SWEEP_PACKS_16 if SIZEOF[letter] == 16 else SWEEP_LANE_ROWS // vec
    return ("sweep", letter, vec, packs, bool(hell), bool(has_beta), SIZEOF[letter] == 8)


def kernel_name(k):
    b = lambda v: "true" if v else "false"
    if k[0] == "probe":
        return f"formProbeKernel<{CTYPE[k[1]]}, {k[2]}, {k[3]}, {b(k[4])}, {k[5]}>"
    if k[0] == "slab":
        _, L, rpl, ph, hell, nt, unroll, pipe, tail, strips, block, tile, every, packed = k
        return (f"slabSpmvKernel<{CTYPE[L]}, {rpl}, {ph}, {b(hell)}, {b(nt)}, {unroll}, {b(pipe)}, {b(tail)}, {b(strips)}, {block}, "
                f"{tile}, {every}, {b(packed)}>")
    _, L, vec, packs, hell, beta, tail = k
    return f"sweepSpmvKernel<{CTYPE[L]}, {vec}, {packs}, {b(hell)}, {b(beta)}, {b(tail)}>"


def wide_layout(letter, hell, rows, hack, val_stride, idx_stride, cM, rP):
    """wideLayout: (ok, the first clause that fails or None).  cM, rP: the addresses (or their residues modulo 16)."""
    w = WIDE[letter]
    strip_rows = (rows + w - 1) // w * w
    if hell:
        if not (hack > 0 and hack % w == 0):
            return False, "hack"
    elif not (val_stride >= strip_rows and idx_stride >= strip_rows):
        return False, "short-stride"
    if cM % 16:
        return False, "cM"
    if rP % (4 * w):
        return False, "rP"
    if val_stride % w or idx_stride % w:
        return False, "stride-multiple"
    return True, None


def tiled_kernel(letter, rpl, hell):
    """slabShape of the Tiled (rpl > 1) and NarrowTiled routes."""
    ph = 2 if SIZEOF[letter] == 16 or rpl == 1 else 1          # narrow: the order of the narrow gather kernel
    if SIZEOF[letter] == 4 and rpl == 4:
        return slab(letter, rpl, 2 * rpl, hell, 2, True, True, False, TILED_BLOCK_S, TILE_BYTES)
    if SIZEOF[letter] == 8 and rpl == 2:
        return slab(letter, rpl, 1, hell, 4, True, True, False, 256, TILE_BYTES, TAIL_EVERY)
    return slab(letter, rpl, ph, hell, 4, True, ph == 1, False, 256, TILE_BYTES)


def slab_grid(k, rows):
    _, _, rpl, ph = k[:4]
    block = k[10]
    group_rows = WAVE // ph * rpl
    groups = (rows + group_rows - 1) // group_rows
    waves = block // WAVE
    return (groups + waves - 1) // waves, block


def wg_rows(k):
    """Rows one workgroup of a kernel owns."""
    if k[0] == "sweep":
        return BLOCK * k[3] * k[2]
    return k[10] // WAVE * (WAVE // k[3] * k[2])


def sweep_grid(k, rows):
    _, _, vec, packs = k[:4]
    n = (rows + vec - 1) // vec
    return min((n + BLOCK * packs - 1) // (BLOCK * packs), SWEEP_MAX_BLOCKS), BLOCK


FIRST_CALL = dict(strips=True, tile=False, sweep=False, probe=False)


def vote_form(letter, rows, said, calls):
    """autoVote (voteForm) under AUTO for an eligible call (wide layout, more than one row per lane, no x tile asked for).  said: what the three
    sample words hold for this matrix (0 nothing yet, 1 scattered, 2 strips, 3 inside a window, 4 a matrix for SWEEP); calls: the
    calls on this (rP, rows) before this one (0: the record is new, its words are zero)."""
    gathers, local, sweeps = said.count(1), said.count(3), said.count(4)
    tile = local >= 2
    strips = gathers + local + sweeps < 2
    return dict(strips=strips, tile=tile, sweep=sweeps >= 2 and not tile and SIZEOF[letter] == 8 and rows >= AUTO_SWEEP_ROWS,
                probe=not strips and (calls % 4 == 0 or calls == 1))


def form_probe(letter, hell, wide_ok):
    """launchFormProbe (probeShape): formProbeKernel's template arguments T, RPL, PH, IS_HELL, STEP; three workgroups of one wavefront."""
    w = WIDE[letter]
    if w > 1 and wide_ok:
        return ("probe", letter, w, 2 * w, bool(hell), 2 * w * 2) if SIZEOF[letter] == 4 else ("probe", letter, w, 1, bool(hell), 8)
    return ("probe", letter, 1, 2, bool(hell), 8)


def every_probe(letter, hell):
    """The probes launchRowsAsTheyCome can put in front of an SpMV: AUTO votes only for wide layouts of 4- and 8-byte elements.
    (spgpu?SpmvForm launches the narrow one too; it is no SpMV call.)"""
    return {form_probe(letter, hell, True)} if WIDE[letter] > 1 else set()


def dispatch(letter, hell, form, rows, hack, val_stride, idx_stride, max_nnz, avg, addr, has_beta, vote=None):
    """launchSlabFamily (callerForm, chooseRoute) for rIdx == NULL, Run, nothing adopted or frozen, SPGPU_X_STRIPS unset.  addr: the addresses of cM, rP, z, y
    (y: None for NULL).  vote: under AUTO what vote_form answers; a first call on a matrix is FIRST_CALL.
    Returns dict(kernel, wide_io, grid, noted: the form spgpuGetLastSpmvForm reports, wide_ok, fails, probe: the formProbeKernel
    launched in front of the kernel, or None)."""
    if rows <= 0:
        return None
    w = WIDE[letter]
    wide_ok, fails = wide_layout(letter, hell, rows, hack, val_stride, idx_stride, addr["cM"], addr["rP"])
    io = int(addr["z"] % 16 == 0 and (addr["y"] or 0) % 16 == 0)
    out = lambda k, wide_io, noted: dict(kernel=k, wide_io=wide_io, noted=noted, wide_ok=wide_ok, fails=fails,
                                         grid=(slab_grid if k[0] == "slab" else sweep_grid)(k, rows),
                                         probe=form_probe(letter, hell, wide_ok) if v["probe"] else None)
    v = dict(strips=False, tile=False, sweep=False, probe=False)
    if form == SWEEP:
        if wide_ok:
            return out(sweep(letter, w, hell, has_beta), io, SWEEP)
        form = AUTO
    tiled = form == XTILE
    eligible = wide_ok and w > 1 and not tiled
    if eligible:
        v = dict(strips=form == STRIPS, tile=False, sweep=False, probe=False) if form != AUTO else dict(FIRST_CALL, **(vote or {}))
    auto_sweep = v["sweep"] and not v["tile"] and SIZEOF[letter] == 8 and rows >= AUTO_SWEEP_ROWS
    noted = XTILE if (tiled or v["tile"]) else (SWEEP if auto_sweep else (STRIPS if v["strips"] else GATHER))
    if auto_sweep and w > 1:
        return out(sweep(letter, w, hell, has_beta), io, SWEEP)
    if wide_ok and w > 1:
        phased = SIZEOF[letter] == 4
        if tiled or v["tile"]:
            return out(tiled_kernel(letter, w, hell), io, noted)
        if not phased and 0 < avg <= LEAN_MAX_HINT and form == AUTO and (hell or max_nnz <= LEAN_MAX_ELL):
            return out(slab(letter, w, 1, hell, 4, False, True, False, BLOCK, 0, TAIL_EVERY), io, GATHER)
        ph, unroll = (2 * w, 2) if phased else (1, 8)
        return out(slab(letter, w, ph, hell, unroll, True, True, v["strips"]), io, noted)
    if tiled:
        return out(tiled_kernel(letter, 1, hell), 1, noted)
    return out(slab(letter, 1, 2, hell, 4, True, False), 1, noted)


def every_instantiation(letter, hell):
    """What the rIdx == NULL dispatch can select for a type and a format (PACKED belongs to frozen matrices)."""
    w = WIDE[letter]
    out = {slab(letter, 1, 2, hell, 4, True, False), tiled_kernel(letter, 1, hell), sweep(letter, w, hell, True), sweep(letter, w, hell, False)}
    if w > 1:
        ph, unroll = (2 * w, 2) if SIZEOF[letter] == 4 else (1, 8)
        out |= {slab(letter, w, ph, hell, unroll, True, True, False), slab(letter, w, ph, hell, unroll, True, True, True),
                tiled_kernel(letter, w, hell)}
        if SIZEOF[letter] == 8:
            out.add(slab(letter, w, 1, hell, 4, False, True, False, BLOCK, 0, TAIL_EVERY))
    return out


def oracle_shape(kernel):
    """oracle_api.spmv_tail's parameters for the order in which a kernel adds a row's products (spmv_tail skips the columns
    below the base, as every kernel does; tail_lanes 0: no row is ever handed to the whole wavefront)."""
    if kernel[0] == "sweep":
        _, L, vec, _, _, _, tail = kernel
        if tail:
            return dict(group_rows=WAVE * vec, rows_per_lane=vec, step=8, tail_lanes=TAIL_LANES, phases=1)
        return dict(group_rows=WAVE, rows_per_lane=1, step=8, tail_lanes=0, phases=1)
    _, L, rpl, ph, _, _, unroll, _, tail, _, _, _, every, _ = kernel
    return dict(group_rows=WAVE // ph * rpl, rows_per_lane=rpl, step=every if every else ph * unroll,
                tail_lanes=TAIL_LANES if tail else 0, phases=ph)


# ---- builders ------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def values(letter, seed, n):
    """Values in [-1, -0.25] and [0.25, 1] (both parts of a complex one)."""
    rng = _rng("values", seed)
    part = lambda: rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    v = part() + 1j * part() if letter in "CZ" else part()
    return v.astype(DTYPE[letter])


def _nan(letter):
    return DTYPE[letter](complex(np.nan, np.nan) if letter in "CZ" else np.nan)


def build(letter, fmt, row_cols, ncols, base, hack=32, val_pitch=None, idx_pitch=None, rs_null=False, seed=0):
    """A host matrix from row_cols[i]: row i's 0-based columns in stored order, -1 for an entry below the index base.
    HELL: keys as oracle_api.hell_spmv reads them.  ELL: `pitch` (the index pitch), `val_pitch`, `max_row`; with rs_null every
    row must be max_row long.  `coo`: (rows, cols, values), 0-based, of the entries a product uses, a row's in stored order."""
    rows = len(row_cols)
    lens = np.array([len(c) for c in row_cols], np.int32)
    rng = _rng("pad", letter, fmt, rows, ncols, seed)
    nan = _nan(letter)
    if fmt == "hell":
        hacks = (rows + hack - 1) // hack
        depth = [int(lens[h * hack:(h + 1) * hack].max(initial=0)) for h in range(hacks)]
        hack_offsets = np.concatenate(([0], np.cumsum([d * hack for d in depth]))).astype(np.int32)
        slots = int(hack_offsets[-1])
        slot0 = lambda i: int(hack_offsets[i // hack]) + i % hack
        vs = is_ = hack
    else:
        max_row = int(lens.max(initial=0))
        idx_pitch = idx_pitch if idx_pitch is not None else (rows + 31) // 32 * 32
        val_pitch = val_pitch if val_pitch is not None else idx_pitch
        assert idx_pitch >= rows and val_pitch >= rows
        assert not rs_null or (lens == max_row).all()
        slots = None
        slot0 = lambda i: i
        vs, is_ = val_pitch, idx_pitch
    n_val = slots if fmt == "hell" else max_row * vs
    n_idx = slots if fmt == "hell" else max_row * is_
    vals = np.full(max(n_val, 1), nan, DTYPE[letter])
    idx = (rng.integers(0, max(ncols, 1), size=max(n_idx, 1)) + base).astype(np.int32)     # valid columns everywhere
    total = int(lens.sum())
    v = values(letter, ("m", fmt, rows, ncols, seed), total)
    r_out, c_out, v_out = [], [], []
    at = 0
    for i, cols in enumerate(row_cols):
        s = slot0(i)
        for k, c in enumerate(cols):
            idx[s + k * is_] = c + base
            if c >= 0:
                vals[s + k * vs] = v[at]
                r_out.append(i)
                c_out.append(c)
                v_out.append(v[at])
            at += 1
    coo = (np.array(r_out, np.int64), np.array(c_out, np.int64), np.array(v_out, DTYPE[letter]))
    m = dict(letter=letter, rows=rows, cols=ncols, values=vals, indices=idx, row_lengths=lens, base=base, coo=coo, fmt=fmt, rs_null=rs_null)
    if fmt == "hell":
        m.update(hack_offsets=hack_offsets, hack_size=hack, height=slots // hack if hack else 0)
    else:
        m.update(pitch=is_, val_pitch=vs, max_row=max_row)
    return m


def oracle_view(m):
    """The dict oracle_api.spmv_tail reads (it takes one pitch for ELL: the value array is re-laid at the index pitch)."""
    if m["fmt"] == "hell" or m["val_pitch"] == m["pitch"]:
        return m
    rows, mx, vp, ip = m["rows"], m["max_row"], m["val_pitch"], m["pitch"]
    vals = np.full(max(mx * ip, 1), _nan(m["letter"]), m["values"].dtype)
    both = min(vp, ip)
    for k in range(mx):
        vals[k * ip:k * ip + both] = m["values"][k * vp:k * vp + both]
    return dict(m, values=vals)


# column patterns: pattern(rows, lens, ...) -> row_cols
def band(lens, shift=0):
    """Row i's k-th column is i + k + shift: neighbouring rows name consecutive columns at every k (strip loads)."""
    return [list(range(i + shift, i + shift + int(n))) for i, n in enumerate(lens)]


def window(lens, spread=3):
    """Row i's k-th column is spread * i + 2 * k: near the diagonal, never consecutive in neighbouring rows."""
    return [[spread * i + 2 * k for k in range(int(n))] for i, n in enumerate(lens)]


def scattered(lens, ncols, seed=0, descend=False):
    rng = _rng("scattered", len(lens), ncols, seed)
    out = []
    for n in lens:
        c = np.sort(rng.choice(ncols, size=int(n), replace=False)) if n <= ncols else rng.integers(0, ncols, int(n))
        out.append([int(x) for x in (c[::-1] if descend else c)])
    return out


# ---- the kernels' control flow, walked on the CPU ------------------------------------------------------------------------------
BRANCHES = (
    "wave_exit",                  # wavefronts that leave at groupRow0 >= rows
    "dead_strips",                # strips with row0 >= rows in a wavefront that stays
    "wave_no_entries",            # wavefronts whose rows are all empty: no stage at all
    "stage_gather",               # stages consumed as gathers (global or LDS)
    "stage_strips",               # stages consumed with one x load per strip
    "strips_refused_ragged",      # the strip loop left because one lane's strip has rows of different length in a slab column
    "strips_refused_below_base",  # ... because a present strip's first column lies below the base
    "strips_refused_scattered",   # ... because the columns of a strip are not consecutive
    "strips_then_gathers",        # wavefronts with strip stages at low k and gather stages behind them
    "strip_absent_load",          # strips past their rows' end inside a strip stage: the load goes to cM
    "strip_x_unaligned",          # strip loads of x at an address off a 16-byte boundary
    "three_stages",               # wavefronts with at least three stages: the cur / nxt ring turns twice
    "col_below_base",             # entries masked because their column lies below the base (stages and tail)
    "tail_switch",                # wavefronts that hand rows to the whole wavefront
    "tail_switch_at_zero",        # ... at kBase 0
    "tail_switch_at_limit",       # ... with exactly tailLanes lanes busy
    "tail_switch_in_strip_loop",  # ... decided by the strip loop's own switchToTail, behind at least one strip stage
    "tail_one_lane_over",         # switch points considered with tailLanes + 1 .. + PH lanes busy: the loop goes on
    "tail_every_deferred",        # stage boundaries that are no multiple of TAIL_EVERY with few enough lanes busy: no switch yet
    "tail_len_1",                 # tail rows of tailFrom + 1 entries
    "tail_len_64",                # ... + 64
    "tail_len_unroll_plus_1",     # ... + kTailUnroll * 64 + 1
    "tail_two_rows_in_strip",     # strips with two tail rows or more
    "tile_fits",                  # workgroups whose columns fit the tile: it starts at the lowest column
    "tile_centred",               # workgroups whose span exceeds the tile
    "tile_count_odd",             # tiles whose element count is no multiple of the 16-byte piece: the tail copy
    "tile_none_empty",            # workgroups whose rows are all empty: tileCount == 0
    "tile_none_below_base",       # workgroups with a sampled column below the base: no tile
    "tile_outside_gather",        # used entries gathered from global memory because they lie outside the tile
    "tile_descending_rows",       # sampled rows whose last column is lower than their first
    "store_wide",                 # strips stored (and y loaded) as one pack
    "store_scalar_no_wideio",     # strips stored by element because z or y is off its boundary
    "store_scalar_partial_strip", # strips stored by element because row0 + RPL > rows
    "store_narrow",               # RPL == 1
)
SWEEP_BRANCHES = ("sweep_pack_whole", "sweep_pack_partial", "sweep_store_wide", "sweep_store_scalar", "sweep_tail_rows",
                  "sweep_lane_idle", "sweep_col_below_base")


def _entry(m, i, k):
    """(0-based column, slot) of row i's k-th slot."""
    if m["fmt"] == "hell":
        hs = m["hack_size"]
        s = int(m["hack_offsets"][i // hs]) + i % hs + k * hs
    else:
        s = i + k * m["pitch"]
    return int(m["indices"][s]) - m["base"], s


def walk(m, kernel, wide_io, x_off_bytes=0):
    """How often one call takes each branch, from the arrays alone.  Also `stages`, `tail_from` (wavefront -> kBase of the switch)."""
    if kernel[0] == "sweep":
        return _walk_sweep(m, kernel, wide_io)
    _, L, rpl, ph, _, _, unroll, pipe, tail, strips, block, tile_bytes, every, _ = kernel
    size, rows = SIZEOF[L], m["rows"]
    lpc = WAVE // ph
    group_rows = lpc * rpl
    waves = block // WAVE
    step = ph * unroll
    tail_stride = every if every > 0 else step
    tile_elems = tile_bytes // size
    piece = 16 // size
    max_nnz = m.get("max_row", 0)
    length = lambda r: (max_nnz if m["rs_null"] else int(m["row_lengths"][r])) if r < rows else 0
    n = dict.fromkeys(BRANCHES, 0)
    n["stages"] = 0
    n["tail_from"] = {}
    grid = slab_grid(kernel, rows)[0]
    for wg in range(grid):
        tile_base, tile_count = 0, 0
        if tile_bytes:
            lo, hi, cnt, mid = None, None, 0, 0
            for r in range(wg * waves * group_rows, min((wg + 1) * waves * group_rows, rows)):
                ln = length(r)
                if ln > 0:
                    f, l = _entry(m, r, 0)[0], _entry(m, r, ln - 1)[0]
                    n["tile_descending_rows"] += l < f
                    lo = min(f, l) if lo is None else min(lo, f, l)
                    hi = max(f, l) if hi is None else max(hi, f, l)
                    mid += (f + l) >> 1
                    cnt += 1
            if cnt == 0:
                n["tile_none_empty"] += 1
            elif lo < 0:
                n["tile_none_below_base"] += 1
            else:
                span = hi - lo + 1
                if span <= tile_elems:
                    tile_base, tile_count = lo, span
                    n["tile_fits"] += 1
                else:
                    start = mid // cnt - tile_elems // 2
                    start = max(start, lo)
                    start = min(start, hi + 1 - tile_elems)
                    tile_base, tile_count = start, tile_elems
                    n["tile_centred"] += 1
                n["tile_count_odd"] += tile_count % piece != 0
        for wave in range(waves):
            group = wg * waves + wave
            g0 = group * group_rows
            if g0 >= rows:
                n["wave_exit"] += 1
                continue
            lens = [[length(g0 + s * rpl + t) for t in range(rpl)] for s in range(lpc)]
            lane_longest = [max(l) for l in lens]
            group_longest = max(lane_longest)
            live = [g0 + s * rpl < rows for s in range(lpc)]
            n["dead_strips"] += live.count(False)
            n["wave_no_entries"] += group_longest == 0
            tail_from = group_longest
            k_base, done, in_strips = 0, False, strips and rpl > 1 and pipe
            stages = strip_stages = gather_stages = 0

            def switch(kb):
                if not tail:
                    return False
                busy = ph * sum(kb < ll for ll in lane_longest)
                if kb % tail_stride:
                    n["tail_every_deferred"] += busy <= TAIL_LANES
                    return False
                n["tail_one_lane_over"] += TAIL_LANES < busy <= TAIL_LANES + ph
                if busy <= TAIL_LANES:
                    n["tail_switch_at_limit"] += busy == TAIL_LANES
                    return True
                return False

            while k_base < group_longest:
                if switch(k_base):
                    tail_from, done = k_base, True
                    n["tail_switch"] += 1
                    n["tail_switch_in_strip_loop"] += in_strips and strip_stages > 0
                    n["tail_switch_at_zero"] += k_base == 0
                    n["tail_from"][group] = k_base
                    break
                if in_strips:
                    why = None
                    for s in range(lpc):
                        for p in range(ph):
                            for u in range(unroll):
                                k = k_base + u * ph + p
                                present = k < lens[s][0]
                                if any((k < lens[s][t]) != present for t in range(rpl)):
                                    why = why or "ragged"
                                elif present:
                                    c0 = _entry(m, g0 + s * rpl, k)[0]
                                    if c0 < 0:
                                        why = why or "below_base"
                                    elif any(_entry(m, g0 + s * rpl + t, k)[0] != c0 + t for t in range(rpl)):
                                        why = why or "scattered"
                    if why:
                        n["strips_refused_" + why] += 1
                        in_strips = False
                    else:
                        for s in range(lpc):
                            for p in range(ph):
                                for u in range(unroll):
                                    k = k_base + u * ph + p
                                    if k < lens[s][0]:
                                        c0 = _entry(m, g0 + s * rpl, k)[0]
                                        n["strip_x_unaligned"] += (x_off_bytes + c0 * size) % 16 != 0
                                    else:
                                        n["strip_absent_load"] += 1
                        strip_stages += 1
                if not in_strips:
                    gather_stages += 1
                    for s in range(lpc):
                        for t in range(rpl):
                            for k in range(k_base, min(k_base + step, lens[s][t])):
                                c = _entry(m, g0 + s * rpl + t, k)[0]
                                if c < 0:
                                    n["col_below_base"] += 1
                                elif tile_bytes and not (0 <= c - tile_base < tile_count):
                                    n["tile_outside_gather"] += 1
                stages += 1
                k_base += step
            n["stages"] += stages
            n["stage_strips"] += strip_stages
            n["stage_gather"] += gather_stages
            n["strips_then_gathers"] += strip_stages > 0 and gather_stages > 0
            n["three_stages"] += stages >= 3
            if tail and done:
                for s in range(lpc):
                    if tail_from < lane_longest[s]:
                        tails = [l for l in lens[s] if l > tail_from]
                        n["tail_two_rows_in_strip"] += len(tails) >= 2
                        for t, l in enumerate(lens[s]):
                            if l > tail_from:
                                n["tail_len_1"] += l - tail_from == 1
                                n["tail_len_64"] += l - tail_from == WAVE
                                n["tail_len_unroll_plus_1"] += l - tail_from == TAIL_UNROLL * WAVE + 1
                                n["col_below_base"] += sum(_entry(m, g0 + s * rpl + t, k)[0] < 0 for k in range(tail_from, l))
            for s in range(lpc):
                if not live[s]:
                    continue
                if rpl == 1:
                    n["store_narrow"] += 1
                elif wide_io and g0 + s * rpl + rpl <= rows:
                    n["store_wide"] += 1
                elif not wide_io:
                    n["store_scalar_no_wideio"] += 1
                else:
                    n["store_scalar_partial_strip"] += 1
    return n


def _walk_sweep(m, kernel, wide_io):
    _, L, vec, packs, _, _, tail = kernel
    rows = m["rows"]
    max_nnz = m.get("max_row", 0)
    length = lambda r: (max_nnz if m["rs_null"] else int(m["row_lengths"][r])) if r < rows else 0
    n = dict.fromkeys(SWEEP_BRANCHES, 0)
    n_packs = (rows + vec - 1) // vec
    grid = sweep_grid(kernel, rows)[0]
    for lane_pack in range(grid * BLOCK * packs):
        row = lane_pack * vec
        if row >= rows:
            n["sweep_lane_idle"] += 1
            continue
        whole = row + vec <= rows
        n["sweep_pack_whole" if whole else "sweep_pack_partial"] += 1
        n["sweep_store_wide" if (wide_io and whole) else "sweep_store_scalar"] += 1
        for t in range(vec):
            n["sweep_col_below_base"] += sum(_entry(m, row + t, k)[0] < 0 for k in range(length(row + t)))
    assert n_packs == n["sweep_pack_whole"] + n["sweep_pack_partial"]
    if tail:
        ref = walk(m, slab(L, vec, 1, kernel[4], 8, True, True), wide_io)
        n["sweep_tail_rows"] = ref["tail_switch"]
    return n


# ---- the case table ----------------------------------------------------------------------------------------------------------
PLAIN, WITH_Y, IN_PLACE = (1.0, 0.0), (-0.75, 0.5), (2.0, 1.0)
NO_OFF = dict(cM=0, rP=0, z=0, y=0, x=0)


def group_rows(letter):
    """Rows of a wavefront of the type's wide gather / strip kernel; Z has the narrow kernel only."""
    return {"S": 32, "D": 128, "C": 128, "Z": 32}[letter]


def wide_step(letter):
    return {"S": 16, "D": 8, "C": 8, "Z": 8}[letter]


def _lens_fill(rows, value):
    return np.full(rows, value, np.int64)


def cases(letter):
    """id -> case.  A case: fmt, form, the matrix recipe (`make`: () -> host matrix), `off`: elements by which cM, rP, z, y, x lie
    past a 16-byte boundary, y mode (`y`, `nan`: beta == 0 and y full of NaN, `z`: z == y), (alpha, beta), avgNnzPerRow, `route`:
    the name of the kernel family it must reach, `claims`: the branches it is in the table for."""
    w, G, STEP = WIDE[letter], group_rows(letter), wide_step(letter)
    wide = w > 1
    c = {}

    def add(cid, fmt, form, make, route, claims=(), off=None, y_mode="y", scalars=WITH_Y, avg=0, fails=None):
        assert cid not in c, cid
        c[cid] = dict(id=cid, letter=letter, fmt=fmt, form=form, make=make, route=route, claims=tuple(claims), off=dict(NO_OFF, **(off or {})),
                      y_mode=y_mode, scalars=scalars, avg=avg, fails=fails)

    def mat(fmt, lens, pattern="band", base=0, hack=32, ncols=None, seed=0, **kw):
        lens = np.asarray(lens, np.int64)

        def make():
            if pattern == "band":
                rc = band(lens)
                nc = len(lens) + int(lens.max(initial=0)) + 4
            elif pattern == "band+1":
                rc = band(lens, shift=1)
                nc = len(lens) + int(lens.max(initial=0)) + 5
            elif pattern == "window":
                rc = window(lens)
                nc = 3 * len(lens) + 2 * int(lens.max(initial=0)) + 4
            elif pattern == "scattered":
                nc = ncols or 4096
                rc = scattered(lens, nc, seed)
            elif pattern == "descending":
                nc = ncols or 4096
                rc = scattered(lens, nc, seed, descend=True)
            else:
                rc, nc = pattern(lens)
            return build(letter, fmt, rc, nc, base, hack=hack, seed=seed, **kw)
        return make

    wide_route = "gather" if wide else "narrow"
    strip_route = "strips" if wide else "narrow"
    tile_route = "tiled" if wide else "narrow-tiled"
    lean_ok = SIZEOF[letter] == 8

    # -- rows: 1, WIDE - 1, WIDE, a wavefront's rows - 1, exactly, + 1, one more than a workgroup's; every form, both formats
    # (a workgroup's rows are those of the kernel the form reaches: 4 wavefronts of G rows for the gather and strip kernels, 8 of 32
    # for the fp32 x tile, 8 192 (complex fp64: 4 096) for the sweep)
    rows_list = sorted({1, max(w - 1, 1), w, G - 1, G, G + 1, 4 * G + 1})
    over = lambda route, hell: wg_rows(route_kernel(letter, route, hell)) + 1
    for fmt in ("hell", "ell"):
        hell = fmt == "hell"
        for route, form, pattern in ((wide_route, GATHER, "scattered"), (strip_route, STRIPS, "band"), (tile_route, XTILE, "window"),
                                     ("sweep", SWEEP, "scattered")):
            rows = over(route, hell)
            if rows in rows_list:
                continue
            tag = f"{fmt}-rows{rows}-{FORM_NAME[form]}"
            lens = _lens_fill(rows, STEP + 1 if route != "sweep" else 3)
            add(tag, fmt, form, mat(fmt, lens, pattern, seed=rows), route, ["tile_fits"] if form == XTILE else [])
            if route == "sweep":
                add(tag + "-unread", fmt, form, mat(fmt, lens, pattern, seed=rows + 1), route, y_mode="nan", scalars=PLAIN)
        if wide:      # ... and of the narrow kernels, on a layout of their own
            rows = over("narrow", hell)
            kw = dict(hack=w + 1 if w > 2 else 3) if hell else dict(idx_pitch=rows, val_pitch=rows)
            add(f"{fmt}-rows{rows}-narrow-gather", fmt, GATHER, mat(fmt, _lens_fill(rows, STEP + 1), "scattered", seed=rows, **kw), "narrow")
            add(f"{fmt}-rows{rows}-narrow-xtile", fmt, XTILE, mat(fmt, _lens_fill(rows, STEP + 1), "window", **kw), "narrow-tiled", ["tile_fits"])
        if lean_ok:
            rows = over("lean", hell)
            add(f"{fmt}-rows{rows}-lean", fmt, AUTO, mat(fmt, _lens_fill(rows, 4), "scattered", seed=rows), "lean", avg=4)
        for rows in rows_list:
            lens = _lens_fill(rows, STEP + 1)
            partial = ["store_scalar_partial_strip"] if wide and rows % w else []
            add(f"{fmt}-rows{rows}-gather", fmt, GATHER, mat(fmt, lens, "scattered", base=rows % 2, seed=rows), wide_route,
                (["stage_gather"] if rows >= G - 1 or not wide else ["tail_switch_at_zero"]) + partial)
            add(f"{fmt}-rows{rows}-strips", fmt, STRIPS, mat(fmt, lens, "band", base=1 - rows % 2), strip_route,
                (["stage_strips"] if wide and rows >= G else []) + partial)
            add(f"{fmt}-rows{rows}-xtile", fmt, XTILE, mat(fmt, lens, "window"), tile_route, ["tile_fits"] + partial)
            add(f"{fmt}-rows{rows}-sweep", fmt, SWEEP, mat(fmt, lens, "scattered", seed=rows + 1), "sweep",
                ["sweep_pack_partial"] if rows % w else ["sweep_pack_whole"], scalars=PLAIN if rows % 2 else WITH_Y,
                y_mode="nan" if rows % 2 else "y")
    # -- row lengths: 0, 1, STEP - 1, STEP, STEP + 1, 2 * STEP + 1, every row alike (no tail: all lanes busy to the end)
    R = 2 * G + w + 1 if wide else 2 * G + 1
    for fmt in ("hell", "ell"):
        for ln in (0, 1, STEP - 1, STEP, STEP + 1, 2 * STEP + 1):
            claims = ["wave_no_entries"] if ln == 0 else (["three_stages"] if ln > 2 * STEP else [])
            add(f"{fmt}-len{ln}-gather", fmt, GATHER, mat(fmt, _lens_fill(R, ln), "scattered", seed=ln), wide_route, claims)
            add(f"{fmt}-len{ln}-strips", fmt, STRIPS, mat(fmt, _lens_fill(R, ln), "band"), strip_route, claims)
            add(f"{fmt}-len{ln}-xtile", fmt, XTILE, mat(fmt, _lens_fill(R, ln), "window"), tile_route,
                ["tile_none_empty"] if ln == 0 else ["tile_fits"])
    add("ell-len-rsnull", "ell", GATHER, mat("ell", _lens_fill(R, STEP + 1), "scattered", seed=77, rs_null=True), wide_route)
    # -- the whole-wave tail: short rows everywhere, long rows in a few lanes
    if letter != "Z":
        ph = 8 if letter == "S" else 1
        strips_at_limit = TAIL_LANES // ph            # strips whose lanes together are exactly tailLanes

        def tail_lens(rows, long_strips, long_len, second=None, short=3, whole_strip=False):
            lens = _lens_fill(rows, short)
            for s in range(long_strips):
                lens[(2 * s + 1) * w] = long_len                     # first row of strip 2s + 1 of the first wavefront
                if whole_strip:
                    lens[(2 * s + 1) * w:(2 * s + 2) * w] = long_len
                if second is not None:
                    lens[(2 * s + 1) * w + 1] = second
            return lens
        T0 = STEP                                        # with rows of 3 entries the first stage runs, then the switch is considered at STEP
        for fmt in ("hell", "ell"):
            for tag, extra, claim in (("+1", 1, "tail_len_1"), ("+64", WAVE, "tail_len_64"),
                                      ("+unroll+1", TAIL_UNROLL * WAVE + 1, "tail_len_unroll_plus_1")):
                for form, pattern, route in ((GATHER, "scattered", wide_route), (XTILE, "window", tile_route), (SWEEP, "scattered", "sweep")):
                    claims = ["tail_switch", claim] if route != "sweep" else (["sweep_tail_rows"] if lean_ok else [])
                    add(f"{fmt}-tail{tag}-{FORM_NAME[form]}", fmt, form, mat(fmt, tail_lens(R, 2, T0 + extra), pattern, seed=extra), route, claims)
            add(f"{fmt}-tail-at-limit", fmt, GATHER, mat(fmt, tail_lens(R, strips_at_limit, T0 + 5), "scattered", seed=5), wide_route,
                ["tail_switch_at_limit"])
            add(f"{fmt}-tail-one-over", fmt, GATHER, mat(fmt, tail_lens(R, strips_at_limit + 1, T0 + 5), "scattered", seed=6), wide_route,
                ["tail_one_lane_over"])
            # the strip loop's own switch: whole strips are long, so that the stage in front of the switch is a strip stage
            add(f"{fmt}-tail-at-limit-strips", fmt, STRIPS, mat(fmt, tail_lens(R, strips_at_limit, T0 + 5, whole_strip=True), "band"), strip_route,
                ["tail_switch_in_strip_loop", "tail_switch_at_limit", "stage_strips"])
            add(f"{fmt}-tail-one-over-strips", fmt, STRIPS, mat(fmt, tail_lens(R, strips_at_limit + 1, T0 + 5, whole_strip=True), "band"),
                strip_route, ["tail_one_lane_over", "stage_strips"])
            add(f"{fmt}-tail-from-zero-strips", fmt, STRIPS, mat(fmt, tail_lens(R, 1, 40, short=0, whole_strip=True), "band"), strip_route,
                ["tail_switch_at_zero"])
            add(f"{fmt}-tail-two-rows-strips", fmt, STRIPS, mat(fmt, tail_lens(R, 2, T0 + 70, second=T0 + 9), "band"), strip_route,
                ["tail_two_rows_in_strip"])
            add(f"{fmt}-tail-from-zero", fmt, GATHER, mat(fmt, tail_lens(R, 1, 40, short=0), "scattered", seed=8), wide_route,
                ["tail_switch_at_zero"])
        if lean_ok:
            # TAIL_EVERY: the 4-column stages of the tiled and lean kernels must switch where the 8-column kernel does
            lens = tail_lens(R, 2, 30, short=3)
            for fmt in ("hell", "ell"):
                add(f"{fmt}-tail-every-xtile", fmt, XTILE, mat(fmt, lens, "window"), tile_route, ["tail_every_deferred", "tail_switch"])
            add("hell-tail-every-lean", "hell", AUTO, mat("hell", lens, "scattered", seed=9), "lean", ["tail_every_deferred", "tail_switch"], avg=4)
    # -- each clause of wideLayout failing alone, and the operands off their boundary one at a time
    lens = _lens_fill(R, STEP + 3)
    if wide:
        rp_fail = 1                               # one int past the boundary: 4 mod 16
        add("hell-cM-off", "hell", GATHER, mat("hell", lens, "scattered", seed=21), "narrow", off=dict(cM=1), fails="cM")
        add("ell-cM-off", "ell", GATHER, mat("ell", lens, "scattered", seed=21), "narrow", off=dict(cM=1), fails="cM")
        add("hell-rP-off", "hell", STRIPS, mat("hell", lens, "band"), "narrow", off=dict(rP=rp_fail), fails="rP")
        add("ell-rP-off", "ell", STRIPS, mat("ell", lens, "band"), "narrow", off=dict(rP=rp_fail), fails="rP")
        if SIZEOF[letter] == 8:
            add("hell-rP-8mod16-stays-wide", "hell", STRIPS, mat("hell", lens, "band"), "strips", ["stage_strips"], off=dict(rP=2))
            add("ell-rP-8mod16-stays-wide", "ell", GATHER, mat("ell", lens, "scattered", seed=22), "gather", off=dict(rP=2))
        add("hell-hack-odd", "hell", GATHER, mat("hell", lens, "scattered", seed=23, hack=w + 1 if w > 2 else 3), "narrow", fails="hack")
        add("hell-hack-odd-xtile", "hell", XTILE, mat("hell", lens, "window", hack=w + 1 if w > 2 else 3), "narrow-tiled", ["tile_fits"], fails="hack")
        add("ell-stride-short", "ell", GATHER, mat("ell", lens, "scattered", seed=24, idx_pitch=R, val_pitch=R), "narrow", fails="short-stride")
        add("ell-stride-no-multiple", "ell", GATHER, mat("ell", lens, "scattered", seed=25, idx_pitch=R + w, val_pitch=R + w),
            "narrow", fails="stride-multiple")
        add("ell-pitches-differ", "ell", GATHER, mat("ell", lens, "scattered", seed=26, idx_pitch=R + w - 1 + 2 * w, val_pitch=R + w - 1),
            wide_route, ["stage_gather"])
        add("ell-pitches-differ-strips", "ell", STRIPS, mat("ell", lens, "band", idx_pitch=R + w - 1, val_pitch=R + w - 1 + 4 * w),
            strip_route, ["stage_strips"])
        add("ell-pitches-differ-sweep", "ell", SWEEP, mat("ell", lens, "scattered", seed=27, idx_pitch=R + w - 1 + 2 * w, val_pitch=R + w - 1), "sweep")
        add("ell-stride-short-sweep-falls-back", "ell", SWEEP, mat("ell", lens, "scattered", seed=28, idx_pitch=R, val_pitch=R), "narrow",
            fails="short-stride")
        for fmt in ("hell", "ell"):
            for which in ("z", "y"):
                for form, pattern, route in ((GATHER, "scattered", wide_route), (STRIPS, "band", strip_route), (XTILE, "window", tile_route)):
                    add(f"{fmt}-{which}-off-{FORM_NAME[form]}", fmt, form, mat(fmt, lens, pattern, seed=31), route, ["store_scalar_no_wideio"],
                        off={which: 1})
                add(f"{fmt}-{which}-off-sweep", fmt, SWEEP, mat(fmt, lens, "scattered", seed=32), "sweep", ["sweep_store_scalar"], off={which: 1})
            add(f"{fmt}-z-off-sweep-unread", fmt, SWEEP, mat(fmt, lens, "scattered", seed=35), "sweep", ["sweep_store_scalar"], off=dict(z=1),
                y_mode="nan", scalars=PLAIN)
            add(f"{fmt}-y-off-unread", fmt, GATHER, mat(fmt, lens, "scattered", seed=33), wide_route, ["store_scalar_no_wideio"], off=dict(y=1),
                y_mode="nan", scalars=PLAIN)
            add(f"{fmt}-x-off-strips", fmt, STRIPS, mat(fmt, lens, "band"), strip_route, ["stage_strips", "strip_x_unaligned"], off=dict(x=1))
            add(f"{fmt}-x-one-past-strips", fmt, STRIPS, mat(fmt, lens, "band+1"), strip_route, ["stage_strips", "strip_x_unaligned"])
            add(f"{fmt}-x-off-xtile", fmt, XTILE, mat(fmt, lens, "window"), tile_route, ["tile_fits"], off=dict(x=1))
            add(f"{fmt}-x-off-gather", fmt, GATHER, mat(fmt, lens, "scattered", seed=34), wide_route, off=dict(x=1))
    else:
        for fmt in ("hell", "ell"):
            add(f"{fmt}-rP-off", fmt, GATHER, mat(fmt, lens, "scattered", seed=21), "narrow", off=dict(rP=1))
            add(f"{fmt}-rP-off-sweep", fmt, SWEEP, mat(fmt, lens, "scattered", seed=22), "sweep", off=dict(rP=3))
        add("ell-pitch-rows-sweep", "ell", SWEEP, mat("ell", lens, "scattered", seed=28, idx_pitch=R, val_pitch=R), "sweep")
    # -- z == y, beta == 0 with y full of NaN, every form
    for fmt in ("hell", "ell"):
        for form, pattern, route in ((GATHER, "scattered", wide_route), (STRIPS, "band", strip_route), (XTILE, "window", tile_route),
                                     (SWEEP, "scattered", "sweep")):
            add(f"{fmt}-in-place-{FORM_NAME[form]}", fmt, form, mat(fmt, lens, pattern, seed=41), route, y_mode="z", scalars=IN_PLACE)
            add(f"{fmt}-y-nan-{FORM_NAME[form]}", fmt, form, mat(fmt, lens, pattern, seed=42), route, y_mode="nan", scalars=PLAIN)
    # -- the x tile, placed
    tile_elems = TILE_BYTES // SIZEOF[letter]
    lens9 = _lens_fill(R, STEP + 1)

    def far_rows(lens_):
        """Window rows, and every 16th row reaches columns far beyond a tile: the tile is centred, those entries are gathered."""
        rc = window(lens_)
        nc = 3 * len(lens_) + 3 * tile_elems
        for i in range(0, len(lens_), 16):
            if rc[i]:
                rc[i][-1] = nc - 1 - i
        return rc, nc

    def odd_span(lens_):
        """Band rows whose span is no multiple of the 16-byte piece."""
        rc = band(lens_)
        span = len(lens_) + int(lens_.max()) - 1
        nc = span + 1
        if nc % (16 // SIZEOF[letter]) == 0 and SIZEOF[letter] < 16:
            nc += 1
        rc[-1][-1] = nc - 1
        return rc, nc

    def below_base(lens_):
        """Scattered rows; the first entry of row 5 and an entry inside row 9 lie below the base."""
        rc = scattered(lens_, 4096, 51)
        rc[5][0] = -1
        rc[9][len(rc[9]) // 2] = -1
        return rc, 4096

    def below_base_band(lens_):
        """A band whose second strip names a column below the base as its first column in slab column 0."""
        rc = band(lens_)
        rc[w if wide else 1][0] = -1
        return rc, len(lens_) + int(lens_.max()) + 4

    def strips_then_scattered(lens_):
        """Two stages of consecutive columns, then scattered ones."""
        rc = band(lens_)
        extra = scattered(_lens_fill(len(lens_), 5), 3000, 52)
        return [a + [5000 + e for e in b] for a, b in zip(rc, extra)], 8000 + len(lens_)

    for fmt in ("hell", "ell"):
        add(f"{fmt}-tile-centred", fmt, XTILE, mat(fmt, lens9, far_rows), tile_route, ["tile_centred", "tile_outside_gather"])
        add(f"{fmt}-tile-odd-count", fmt, XTILE, mat(fmt, lens9, odd_span), tile_route, ["tile_fits", "tile_count_odd"] if SIZEOF[letter] < 16 else ["tile_fits"])
        add(f"{fmt}-tile-below-base", fmt, XTILE, mat(fmt, lens9, below_base, base=1), tile_route, ["tile_none_below_base", "col_below_base", "tile_outside_gather"])
        add(f"{fmt}-tile-descending", fmt, XTILE, mat(fmt, lens9, "descending", ncols=tile_elems // 2, seed=53), tile_route, ["tile_descending_rows", "tile_fits"])
        add(f"{fmt}-gather-below-base", fmt, GATHER, mat(fmt, lens9, below_base, base=1), wide_route, ["col_below_base"])
        add(f"{fmt}-sweep-below-base", fmt, SWEEP, mat(fmt, lens9, below_base, base=1), "sweep", ["sweep_col_below_base"])
        add(f"{fmt}-strips-below-base", fmt, STRIPS, mat(fmt, lens9, below_base_band, base=1), strip_route,
            ["strips_refused_below_base", "col_below_base"] if wide else ["col_below_base"])
        two = _lens_fill(R, 2 * STEP)
        add(f"{fmt}-strips-then-gathers", fmt, STRIPS, mat(fmt, two, strips_then_scattered), strip_route,
            ["strips_then_gathers", "strips_refused_scattered"] if wide else [])
        ragged = _lens_fill(R, STEP + 2)
        ragged[1::2] = STEP - 1 if wide else STEP + 2
        add(f"{fmt}-strips-ragged-strip", fmt, STRIPS, mat(fmt, ragged, "band"), strip_route, ["strips_refused_ragged"] if wide else [])
        absent = _lens_fill(R, 2 * STEP + 2)
        absent[:G // 2] = STEP
        add(f"{fmt}-strips-absent", fmt, STRIPS, mat(fmt, absent, "band"), strip_route, ["stage_strips", "strip_absent_load"] if wide else [])
    # -- the lean kernel (AUTO with the caller's hint; 8-byte types): hints 1 and 8 are members, 0 and 9 are not; ELL maxNnz 16 / 17
    short = _lens_fill(R, 4)
    short[::7] = 0
    short[3::11] = 8
    ell16, ell17 = short.copy(), short.copy()
    ell16[G + 1], ell17[G + 1] = 16, 17
    for hint in (0, 1, 8, 9):
        member = lean_ok and hint in (1, 8)
        add(f"hell-hint{hint}", "hell", AUTO, mat("hell", short, "scattered", seed=61), "lean" if member else ("auto-first" if wide else "narrow"), avg=hint)
        add(f"ell-hint{hint}-max16", "ell", AUTO, mat("ell", ell16, "scattered", seed=62), "lean" if member else ("auto-first" if wide else "narrow"), avg=hint)
    add("ell-hint8-max17", "ell", AUTO, mat("ell", ell17, "scattered", seed=63), "auto-first" if wide else "narrow", avg=8)
    add("ell-hint1-rsnull", "ell", AUTO, mat("ell", _lens_fill(R, 5), "scattered", seed=64, rs_null=True), "lean" if lean_ok else ("auto-first" if wide else "narrow"), avg=1)
    add("ell-xtile-rsnull", "ell", XTILE, mat("ell", _lens_fill(R, STEP + 2), "window", rs_null=True), tile_route, ["tile_fits"])
    add("ell-strips-rsnull", "ell", STRIPS, mat("ell", _lens_fill(R, STEP + 2), "band", rs_null=True), strip_route, ["stage_strips"] if wide else [])
    add("ell-sweep-rsnull", "ell", SWEEP, mat("ell", _lens_fill(R, STEP + 2), "scattered", seed=65, rs_null=True), "sweep")
    # -- the narrow x tile on a layout of its own (every type): two phases, no tail rows, a long row keeps its wavefront going
    nar = _lens_fill(2 * WAVE + 3, 6)
    nar[5], nar[70] = 4 + 4 * 70, 9
    for fmt, kw in (("hell", dict(hack=3)), ("ell", dict(idx_pitch=2 * WAVE + 3, val_pitch=2 * WAVE + 3))):
        if wide:
            add(f"{fmt}-narrow-xtile-long", fmt, XTILE, mat(fmt, nar, "window", **kw), "narrow-tiled", ["tile_fits", "three_stages"])
            add(f"{fmt}-narrow-gather-long", fmt, GATHER, mat(fmt, nar, "scattered", seed=71, **kw), "narrow", ["three_stages"])
        else:
            add(f"{fmt}-narrow-xtile-long", fmt, XTILE, mat(fmt, nar, "window"), "narrow-tiled", ["tile_fits", "three_stages"])
    return c


ROUTES = ("gather", "strips", "tiled", "lean", "narrow", "narrow-tiled", "sweep", "auto-first")


def route_kernel(letter, route, hell, has_beta=True):
    w = WIDE[letter]
    ph, unroll = (2 * w, 2) if SIZEOF[letter] == 4 else (1, 8)
    return {
        "gather": lambda: slab(letter, w, ph, hell, unroll, True, True, False),
        "strips": lambda: slab(letter, w, ph, hell, unroll, True, True, True),
        "auto-first": lambda: slab(letter, w, ph, hell, unroll, True, True, True),      # AUTO on a matrix it has not seen
        "tiled": lambda: tiled_kernel(letter, w, hell),
        "lean": lambda: slab(letter, w, 1, hell, 4, False, True, False, BLOCK, 0, TAIL_EVERY),
        "narrow": lambda: slab(letter, 1, 2, hell, 4, True, False),
        "narrow-tiled": lambda: tiled_kernel(letter, 1, hell),
        "sweep": lambda: sweep(letter, w, hell, has_beta),
    }[route]()


_MATRICES = {}


def matrix_of(case):
    """The host matrix of a case, built once and left unchanged."""
    key = (case["letter"], case["id"])
    if key not in _MATRICES:
        _MATRICES[key] = case["make"]()
    return _MATRICES[key]


def strides(m):
    """(hackSize, valStride, idxStride, maxNnz) as the C ABI passes them on."""
    if m["fmt"] == "hell":
        return m["hack_size"], m["hack_size"], m["hack_size"], 0
    return 0, m["val_pitch"], m["pitch"], m["max_row"]


def byte_offsets(case):
    """Residues modulo 16 of the operands' addresses when they start `off` elements past a boundary."""
    size = SIZEOF[case["letter"]]
    off = case["off"]
    out = dict(cM=off["cM"] * size % 16, rP=off["rP"] * 4 % 16, z=off["z"] * size % 16, x=off["x"] * size % 16)
    out["y"] = out["z"] if case["y_mode"] == "z" else off["y"] * size % 16
    return out


def case_dispatch(case, addr=None, vote=None):
    m = matrix_of(case)
    hack, vs, is_, mx = strides(m)
    return dispatch(case["letter"], m["fmt"] == "hell", case["form"], m["rows"], hack, vs, is_, mx, case["avg"], addr or byte_offsets(case),
                    case["scalars"][1] != 0, vote)


def case_walk(case):
    d = case_dispatch(case)
    return walk(matrix_of(case), d["kernel"], d["wide_io"], byte_offsets(case)["x"])


def operands(letter, m):
    return values(letter, ("x", m["cols"]), m["cols"]), values(letter, ("y", m["rows"]), m["rows"])


def scalars_of(case):
    """(alpha, beta) of a case; C and Z get imaginary parts (beta stays 0 where the case says so)."""
    alpha, beta = case["scalars"]
    if case["letter"] in "CZ":
        alpha = complex(alpha, 0.5)
        beta = complex(beta, -0.25) if beta != 0 else 0.0
    return alpha, beta


# ---- AUTO's first-call / later-call sequence -------------------------------------------------------------------------------------
AUTO_ROWS = 708       # D, C: five whole wavefronts and 34 strips; S: the sample wavefronts 8 and 16 of 23 are whole


def auto_patterns(letter):
    """pattern -> (host HELL matrix, the form the second call runs in): rows longer than two stages, so that the sample
    wavefronts of the strip-capable kernel answer strips / window / scattered.  Z has the narrow kernel only: GATHER."""
    ln = _lens_fill(AUTO_ROWS, 2 * wide_step(letter) + 4)
    far = 4 * (TILE_BYTES // SIZEOF[letter])
    out = {
        "band": (build(letter, "hell", band(ln), AUTO_ROWS + int(ln[0]) + 4, 0, seed=81), STRIPS),
        "window": (build(letter, "hell", window(ln), 3 * AUTO_ROWS + 2 * int(ln[0]) + 4, 0, seed=82), XTILE),
        "scattered": (build(letter, "hell", scattered(ln, far, 83), far, 0, seed=83), GATHER),
    }
    if WIDE[letter] == 1:
        out = {k: (m, GATHER) for k, (m, _) in out.items()}
    return out
