"""TEST INFRASTRUCTURE: the ELL / HELL SpMV for rows ORDERED BY LENGTH (rIdx given, or SPGPU_DEEP_SPLIT=1) -- spgpu_amd/csrc/ellpack_spmv.hip
launchSlabFamily -> attachDeepList -> launchOrdered, ragged_spmv.hip.h (raggedSpmvKernel, launchRagged), planned_spmv.hip (launchPlanned,
planBlocksKernel, planPackKernel), deep_rows.hip.h (wholeSubgroups), deep_items.hip.h (deepItemsKernel, deepFinishKernel) and
form_probe.hip.h (orderedProbeKernel) -- restated: which queue kernel a call launches, over which grid, what spgpuGetLastOrderedLaunch
reports, and a walk of the kernels that names the branches a case takes.  The host rules are spgpu_amd/csrc/ordered_rules.h's;
tests/test_ordered_launch_shapes.py ties this restatement to that header through tests/ordered_dispatch_cases.cpp.

The matrices are written slot by slot (spmv_launch_shapes.build): a list of 32-row sub-groups with chosen depths, per-row lengths,
columns and a chosen rIdx.  Padding slots, rows past the last one and entries below the index base hold NaN values; a padding index
holds a valid column.  No matrix has more than three workgroups of its shape plus a partial one; the deep branches are reached by
lowering SPGPU_DEEP_CAP / SPGPU_DEEP_KEEP / SPGPU_RAGGED_SPLIT (TUNE), not by long rows."""
import numpy as np

import oracle_api as O
import spmv_launch_shapes as M

LETTERS, SIZEOF, WIDE, DTYPE = M.LETTERS, M.SIZEOF, M.WIDE, M.DTYPE
WAVE, SUB_ROWS, PLAN_DEEP_MOST, DEEP_CHUNK, STAGED_KNOB = 64, 32, 8, 64, 4
DEEP_ENTRIES = 8192                      # spgpu_internal.h SPGPU_DEEP_ENTRIES: no case comes near it (asserted in the walk)
GATHER_Q, TILED_Q, STAGED_Q = (4, 0, 16, 0), (8, 65536, 32, 0), (8, 49152, 64, 17408)     # WAVES, TILE_BYTES, SUBS, ZBYTES
SHAPES = {"gather": GATHER_Q, "tiled": TILED_Q, "staged": STAGED_Q}
ORDERED_PLAN, ORDERED_PACKED, ORDERED_DEEP = 0x100, 0x200, 0x400                          # include/spgpu/tuning.h
MODES = ("list", "plan", "packed")       # no plan (deep list, deep kernels behind) / from a plan / from a frozen plan
# the knobs most cases run under (cap 48, keep 12, split asked 12); the same with the split off; and (tune_most) the ones that make a
# sub-group of cap columns the most chunks
TUNE = dict(cap=48, keep=12, split=12)
TUNE_NO_SPLIT = dict(cap=48, keep=12, split=0)


def tune_most(letter):
    return dict(cap=most_chunks(letter) * queue_step(letter), keep=12, split=1)


# ---- ordered_rules.h restated ------------------------------------------------------------------------------------------------------
def unroll(letter):
    return 2 if WIDE[letter] >= 4 else 3


def phases(letter):
    return WAVE // (SUB_ROWS // WIDE[letter])


def queue_step(letter):
    return phases(letter) * unroll(letter)


def most_chunks(letter):
    return STAGED_Q[1] // SIZEOF[letter] // (STAGED_Q[2] * SUB_ROWS)


def staged_shape(letter, tiled, shape):
    return bool(tiled and SIZEOF[letter] <= 8 and shape == STAGED_KNOB)


def queue_shape(letter, tiled, shape):
    return GATHER_Q if not tiled else (STAGED_Q if staged_shape(letter, tiled, shape) else TILED_Q)


def ragged_split(letter, cap, asked):
    return O.ragged_split(letter, queue_step(letter), cap, asked)


def queue_grid(rows, subs):
    return -(-(-(-rows // SUB_ROWS)) // subs)


def plan_grid(main_blocks, deep):
    """(deep workgroups, grid, planDeepStride)."""
    deep_blocks = -(-deep // PLAN_DEEP_MOST)
    grid = main_blocks + deep_blocks
    if deep_blocks == 0:
        return 0, grid, 0
    stride = grid * 60 // 100 // deep_blocks
    return deep_blocks, grid, 1 if stride < 1 else stride | 1


def probe_said(m):
    """orderedProbeKernel's word for the matrix (without the tag): 6, 4 or 5."""
    rows, lens, r_idx = m["rows"], m["row_lengths"], m["r_idx"]
    near = seen = 0
    for q in (1, 2, 3):
        for lane in range(WAVE):
            r = rows * q // 4 + 2 * q + lane
            if r >= rows or (m["max_row"] if m["rs_null"] else lens[r]) <= 0:
                continue
            cols = m["row_cols"][r]
            reach = max(abs(cols[0] - int(r_idx[r])), abs(cols[-1] - int(r_idx[r])))
            seen += 1
            near += reach <= 1024
    windows = blocks = 0
    for q in (1, 2, 3):
        block0 = rows * q // 4 // 2048 * 2048
        if block0 + 2048 > rows:
            continue
        dest = [int(r_idx[block0 + lane * 32 + (lane & 31)]) for lane in range(WAVE)]
        blocks += 1
        windows += max(dest) - min(dest) < 2048 + 512
    return 6 if blocks > 0 and windows == blocks else (4 if seen > 0 and 4 * near >= 3 * seen else 5)


def dispatch(letter, hell, form, knob, row_order, max_nnz, rows, tune, mode, probed=0, no_deep_list=False, deep=0, can_pack=True):
    """launchSlabFamily -> launchOrdered for a layout the wide kernels read (wideLayout; asserted by the cases).  form: M.GATHER or M.AUTO;
    knob: SPGPU_RAGGED_SHAPE; probed: orderedShapeSaid(probe's word) (read only where the shape is the probe's to say); mode: MODES;
    deep: the plan's number of deep sub-groups.  Returns dict(shape name, queue (WAVES, TILE_BYTES, SUBS, ZBYTES), plan, packed, grid, stride,
    deep_follow, word: spgpuGetLastOrderedLaunch, split, kernel: raggedSpmvKernel's template arguments)."""
    tiled = form != M.GATHER
    probes = knob == 0 and tiled and row_order and SIZEOF[letter] <= 8
    shape = probed if probes else knob
    if no_deep_list and shape != STAGED_KNOB:
        shape = 0
    plannable = (not tiled) or shape in (0, STAGED_KNOB)
    q = queue_shape(letter, tiled, shape)
    name = {GATHER_Q: "gather", TILED_Q: "tiled", STAGED_Q: "staged"}[q]
    plan = mode != "list" and plannable and row_order
    packed = plan and mode == "packed" and tiled and SIZEOF[letter] <= 8 and can_pack
    main = queue_grid(rows, q[2])
    if plan:
        _, grid, stride = plan_grid(main, deep)
        follow = False
    else:
        grid, stride = main, 0
        follow = bool(hell or max_nnz > tune["cap"])
    word = q[2] | (ORDERED_PLAN if plan else 0) | (ORDERED_PACKED if packed else 0) | (ORDERED_DEEP if follow else 0)
    rpl = WIDE[letter]
    kernel = (letter, rpl, bool(hell), unroll(letter), q[0], q[1], q[2], True, q[3], bool(plan), bool(packed))
    return dict(shape=name, queue=q, plan=bool(plan), packed=bool(packed), grid=grid, stride=stride, deep_follow=follow, word=word,
                split=ragged_split(letter, tune["cap"], tune["split"]), kernel=kernel, noted=M.XTILE if tiled else M.GATHER, probes=bool(probes),
                knob_shape=shape, plannable=bool(plannable))


def every_instantiation():
    """raggedSpmvKernel<T, RPL, IS_HELL, UNROLL, WAVES, TILE_BYTES, SUBS, DEEP, ZBYTES, PLAN, PACKED> as launchQueue names them."""
    out = set()
    for letter in LETTERS:
        for hell in (False, True):
            for tiled, knob in ((False, 0), (True, 0), (True, STAGED_KNOB)):
                q = queue_shape(letter, tiled, knob)
                for plan, packed in ((False, False), (True, False), (True, True)):
                    if packed and not (tiled and SIZEOF[letter] <= 8):
                        continue
                    out.add((letter, WIDE[letter], hell, unroll(letter), q[0], q[1], q[2], True, q[3], plan, packed))
    return out


# ---- matrices ----------------------------------------------------------------------------------------------------------------------
BIG = 40000        # columns of the matrices whose blocks reach further than any tile (fp32 tiled: 16 384 elements)
REACH = 70000      # ... and further than a 16-bit word


def _lens_of(depths, rows, full):
    lens = np.zeros(rows, np.int32)
    for s, d in enumerate(depths):
        for j in range(SUB_ROWS):
            r = s * SUB_ROWS + j
            if r < rows:
                lens[r] = d if (j == 0 or full) else max(0, d - (j * 7 + s) % (d + 1))
    return lens


def _perm(rows, block_rows, kind):
    """rIdx: "rev" reverses every block of the shape's rows (a block's results lie side by side), "swap" sends a few rows of the first
    block to the highest destinations (beyond any staging buffer: the last rows - 12 > 4 352, fp32's) and brings theirs back."""
    p = np.arange(rows, dtype=np.int64)
    for b0 in range(0, rows, block_rows):
        p[b0:b0 + block_rows] = p[b0:b0 + block_rows][::-1].copy()
    if kind == "swap":
        for a, j in ((3, 0), (40, 5), (block_rows // 2 + 1, 11)):
            b = int(np.flatnonzero(p == rows - 1 - j)[0])
            if 0 <= a < b < rows:
                p[a], p[b] = p[b], p[a]
    return p.astype(np.int32)


def make(letter, fmt, depths, rows, block_rows, cols="near", perm="rev", base=1, hack=32, rs_null=False, pitch_extra=0, seed=0, shift=0):
    """The host matrix (spmv_launch_shapes.build's dict, plus r_idx, row_cols, depths).  shift: every column that far above its row's
    destination (1 500: orderedProbeKernel says "wide", the 1 024-row shape)."""
    assert (len(depths) - 1) * SUB_ROWS < rows <= len(depths) * SUB_ROWS
    lens = _lens_of(depths, rows, rs_null)
    r_idx = _perm(rows, block_rows, perm)
    deepest = int(max(depths))
    shift = 1500 if cols == "far" else shift
    ncols = {"near": rows + 2 * deepest + 8, "far": rows + 2 * deepest + 8, "low": BIG, "high": BIG, "below": rows + 2 * deepest + 8,
             "escape": REACH}[cols] + shift
    row_cols = []
    for r in range(rows):
        n, t = int(lens[r]), int(r_idx[r])
        c = [t + shift + 2 * k for k in range(n)]
        if cols == "high":
            c = [BIG - 1 - (t + 2 * (n - 1 - k)) for k in range(n)]
            if r % block_rows == 0 and n >= 2:
                c[0] = 0                                   # one row reaches down to column 0: the span is all of x
        elif cols == "low":
            c = [v + 1 for v in c]                         # an odd lowest column
            if r % block_rows == 0 and n >= 2:
                c[-1] = ncols - 1
        elif cols == "below":
            c = [-1 if (r + k) % 11 == 5 else v for k, v in enumerate(c)]
            if r == 0 and n >= 1:
                c[0] = -1                                  # the first block's probes see a column below the base: no tile there
        elif cols == "escape":
            if r % 37 == 0 and n >= 3:
                c[1] = ncols - 1                           # out of a 16-bit word's reach
            if r % 41 == 1 and n >= 3:
                c[1] = -1
        if cols in ("low", "high", "near", "far") and n >= 4 and r % 29 == 7:
            c[2] = ncols - 1 - (r % 5)                     # a middle entry the probes do not see
        row_cols.append(c)
    kw = dict(hack=hack) if fmt == "hell" else dict(idx_pitch=(rows + 31) // 32 * 32 + pitch_extra, val_pitch=(rows + 31) // 32 * 32 + 2 * pitch_extra)
    m = M.build(letter, fmt, row_cols, ncols, base, rs_null=rs_null, seed=("ordered", seed), **kw)
    m.update(r_idx=r_idx, row_cols=row_cols, depths=list(depths))
    if fmt == "ell":
        m["max_row"] = int(lens.max(initial=0))
    return m


def operands(letter, m):
    return M.values(letter, ("ox", m["rows"], m["cols"]), m["cols"]), M.values(letter, ("oy", m["rows"]), m["rows"])


def oracle(m, x, y, alpha, beta, tune, with_order=True):
    """The oracle in the queue kernel's order of additions under the case's knobs."""
    shape = O.slab_shape(m["letter"], "ragged", tune["cap"], tune["split"], tune["keep"])
    return O.spmv_tail(M.oracle_view(m), x, y if beta != 0 else None, alpha, beta, r_idx=m["r_idx"] if with_order else None,
                       with_row_sizes=not m["rs_null"], **shape)


# ---- the kernels walked ------------------------------------------------------------------------------------------------------------
BRANCHES = (
    "rows_lt_32", "last_sub_partial", "last_block_partial", "rs_null", "ridx_null",
    "ell_pitch_above_rows", "hell_hack_32", "hell_hack_96", "hell_hack_straddles",
    "who_here", "registered_row_above_keep", "registered_row_below_keep", "who_elsewhere", "behind_1_to_8", "behind_more_than_8",
    "stale_listed_but_shallow", "stale_deep_but_unlisted",
    "plan_no_deep_workgroups", "plan_stride_1", "plan_stride_odd_3_or_more", "plan_last_deep_workgroup_partial",
    "items_fewer_than_waves", "depth_0", "depth_1", "depth_step_minus_1", "depth_step", "depth_step_plus_1", "depth_2_steps_plus_1",
    "split_2_chunks", "split_most_chunks", "split_more_subs_than_2_waves", "split_off",
    "tile_whole_span", "tile_centred_clamped_low", "tile_centred_clamped_high", "tile_empty_block", "tile_column_below_base",
    "tile_count_no_multiple_of_piece", "tile_base_odd", "column_outside_tile",
    "packed_word_in_tile", "packed_word_outside_tile", "packed_escape", "packed_escape_below_base",
    "staged_inside", "staged_beyond", "staged_not_for_registered_or_listed", "staged_writeout_beta_zero", "staged_beyond_beta_zero",
    "deep_item_full", "deep_item_partial_last", "deep_strip_beyond_rows", "deep_straddling_branch",
    "finish_at_most_8_items", "finish_more_than_8_items",
    "whole_one_round", "whole_several_rounds", "whole_expect_deep_contradicted",
    "beta_zero", "beta_nonzero", "y_is_z",
)


def tile_elems(letter, q):
    e = SIZEOF[letter]
    if q[1] > 0:
        return q[1] // e
    chunk_room = q[2] * 32 * most_chunks(letter) if most_chunks(letter) >= 2 else 1
    return max(chunk_room, 16384 // e)


def whole_parks(letter, q):
    """wholeSubgroups: chunk sums one round holds."""
    e = SIZEOF[letter]
    table = PLAN_DEEP_MOST * 32 * e + PLAN_DEEP_MOST * 32 * 4 * 2 + PLAN_DEEP_MOST * 4 * 2
    return (tile_elems(letter, q) * e - table) // (32 * e)


def chunks_of(depth, tune, split):
    deep = depth > tune["cap"]
    walked = tune["keep"] if deep else depth
    main = -(-walked // split) if split > 0 and walked > split else 1
    return main, (-(-(depth - tune["keep"]) // DEEP_CHUNK) if deep else 0)


def sub_depths(m):
    rows, lens = m["rows"], (np.full(m["rows"], m["max_row"]) if m["rs_null"] else m["row_lengths"])
    return [int(lens[s:s + 32].max(initial=0)) for s in range(0, rows, 32)], lens


def walk(m, route, tune, plan_of=None, row_order=True, beta=1.0, y_mode="y"):
    """The names of BRANCHES one call takes.  route: dispatch's answer; plan_of: the matrix the plan was made for (a stale plan), default
    m itself."""
    letter, rows = m["letter"], m["rows"]
    q, e = route["queue"], SIZEOF[letter]
    waves, subs = q[0], q[2]
    step, split, cap, keep = queue_step(letter), route["split"], tune["cap"], tune["keep"]
    depths, lens = sub_depths(m)
    n_sub = len(depths)
    out = set()
    out.add("beta_nonzero" if beta != 0 else "beta_zero")
    if y_mode == "z":
        out.add("y_is_z")
    if rows < 32:
        out.add("rows_lt_32")
    if rows % 32:
        out.add("last_sub_partial")
    if n_sub % subs:
        out.add("last_block_partial")
    if m["rs_null"]:
        out.add("rs_null")
    if not row_order:
        out.add("ridx_null")
    if m["fmt"] == "ell":
        if m["pitch"] > rows and m["val_pitch"] > rows:
            out.add("ell_pitch_above_rows")
    else:
        out.add({32: "hell_hack_32", 96: "hell_hack_96"}.get(m["hack_size"], "hell_hack_straddles" if m["hack_size"] % 32 else "hell_hack_other"))
    if split == 0:
        out.add("split_off")
    deep = [d > cap for d in depths]
    assert sum(deep) < DEEP_ENTRIES
    if route["plan"]:
        listed = [d > cap for d in sub_depths(plan_of or m)[0]]
        who = ["elsewhere" if l else ("behind" if d else "here") for l, d in zip(listed, deep)]
        n_listed = sum(listed)
        deep_blocks, grid, stride = plan_grid(queue_grid(rows, subs), n_listed)
        assert (grid, stride) == (route["grid"], route["stride"])
        out.add("plan_no_deep_workgroups" if deep_blocks == 0 else ("plan_stride_1" if stride == 1 else "plan_stride_odd_3_or_more"))
        assert stride == 0 or (stride % 2 == 1 and (deep_blocks - 1) * stride < grid)
        if n_listed % PLAN_DEEP_MOST:
            out.add("plan_last_deep_workgroup_partial")
        if any(l and not d for l, d in zip(listed, deep)):
            out.update(("stale_listed_but_shallow", "whole_expect_deep_contradicted"))
        if any(d and not l for l, d in zip(listed, deep)):
            out.add("stale_deep_but_unlisted")
        batches = [[s for s in range(n_sub) if listed[s]][i:i + PLAN_DEEP_MOST] for i in range(0, n_listed, PLAN_DEEP_MOST)]
    else:
        who = ["registered" if d else "here" for d in deep]
        batches = []
    registered = [w == "registered" for w in who]
    for s in range(n_sub):
        if who[s] in ("here", "registered"):
            out.add("who_here")
        if who[s] == "elsewhere":
            out.add("who_elsewhere")
        if who[s] == "registered":
            mine = lens[s * 32:s * 32 + 32]
            if (mine > keep).any():
                out.add("registered_row_above_keep")
            if (mine <= keep).any():
                out.add("registered_row_below_keep")
            items = -(-(depths[s] - keep) // DEEP_CHUNK)
            out.add("finish_more_than_8_items" if items > 8 else "finish_at_most_8_items")
            if depths[s] - keep >= DEEP_CHUNK:
                out.add("deep_item_full")
            if (depths[s] - keep) % DEEP_CHUNK:
                out.add("deep_item_partial_last")
            if s * 32 + 32 - WIDE[letter] >= rows:
                out.add("deep_strip_beyond_rows")
            if m["fmt"] == "hell" and m["hack_size"] % 32:
                out.add("deep_straddling_branch")
    here_depth = [keep if who[s] == "registered" else (depths[s] if who[s] == "here" else -1) for s in range(n_sub)]
    room_all = tile_elems(letter, q)
    for b0 in range(0, n_sub, subs):
        block = range(b0, min(b0 + subs, n_sub))
        # (every lane below SUBS counts: a sub-group past the last row has depth 0, is nobody else's and is one item)
        items, parks, splits = subs - len(block), 0, 0
        for s in block:
            d = here_depth[s]
            if d < 0:
                continue
            is_split = split > 0 and d > split and d <= cap
            c = -(-d // split) if is_split else 1
            items += c
            if is_split:
                parks += c
                splits += 1
                if c == 2:
                    out.add("split_2_chunks")
                if c == most_chunks(letter) and c > 2:
                    out.add("split_most_chunks")
                assert c <= most_chunks(letter)
            else:
                for name, v in (("depth_0", 0), ("depth_1", 1), ("depth_step_minus_1", step - 1), ("depth_step", step), ("depth_step_plus_1", step + 1),
                                ("depth_2_steps_plus_1", 2 * step + 1)):
                    if d == v:
                        out.add(name)
        if items < waves:
            out.add("items_fewer_than_waves")
        if splits > 2 * waves:
            out.add("split_more_subs_than_2_waves")
        orphans = sum(1 for s in block if who[s] == "behind")
        if orphans:
            out.add("behind_more_than_8" if orphans > 8 else "behind_1_to_8")
            got = [s for s in block if who[s] == "behind"]
            batches += [got[i:i + PLAN_DEEP_MOST] for i in range(0, len(got), PLAN_DEEP_MOST)]
        block_rows = [r for s in block for r in range(s * 32, min(s * 32 + 32, rows))]
        # ---- the x tile ----
        tile_base = tile_count = 0
        stale = plan_of is not None
        if q[1] > 0 and not stale:
            probed = [r for r in block_rows if lens[r] > 0 and not (route["plan"] and deep[r // 32])]
            room = room_all - parks * 32
            assert room >= 0
            if not probed:
                out.add("tile_empty_block")
            else:
                f = [m["row_cols"][r][0] for r in probed]
                l = [m["row_cols"][r][int(lens[r]) - 1] for r in probed]
                low, high = min(min(f), min(l)), max(max(f), max(l))
                middle = sum((a + b) >> 1 for a, b in zip(f, l)) // len(probed)
                if low < 0:
                    out.add("tile_column_below_base")
                else:
                    span = high - low + 1
                    if span <= room:
                        out.add("tile_whole_span")
                        tile_base, tile_count = low, span
                    elif room > 0:
                        start = middle - room // 2
                        if start < low:
                            out.add("tile_centred_clamped_low")
                            start = low
                        if start + room > high + 1:
                            out.add("tile_centred_clamped_high")
                            start = high + 1 - room
                        tile_base, tile_count = start, room
                    piece = 16 // e
                    if tile_count % piece:
                        out.add("tile_count_no_multiple_of_piece")
                    if tile_base % 2:
                        out.add("tile_base_odd")
                pack_base = 0
                if route["packed"]:
                    if high - low <= 0xFFFE:
                        pack_base = low
                    else:
                        pack_base = min(max(middle - 0x7FFF, low), high - 0xFFFE)
            for r in block_rows:
                d = here_depth[r // 32]
                if d < 0:
                    continue
                for k, col in enumerate(m["row_cols"][r][:min(int(lens[r]), d)]):
                    inside = col >= 0 and tile_base <= col < tile_base + tile_count
                    if route["packed"] and probed:
                        fits = col >= 0 and 0 <= col - pack_base < 0xFFFF
                        out.add(("packed_word_in_tile" if inside else "packed_word_outside_tile") if fits else
                                ("packed_escape" if col >= 0 else "packed_escape_below_base"))
                    if col >= 0 and not inside:
                        out.add("column_outside_tile")
        # ---- staged results ----
        if q[3] > 0:
            zw = q[3] // e
            mine = [r for r in block_rows if who[r // 32] == "here"]
            if mine:
                z_base = min(int(m["r_idx"][r]) if row_order else r for r in mine)
                for r in mine:
                    off = (int(m["r_idx"][r]) if row_order else r) - z_base
                    out.add("staged_inside" if off < zw else "staged_beyond")
                    if beta == 0:
                        out.add("staged_writeout_beta_zero" if off < zw else "staged_beyond_beta_zero")
            if any(who[s] != "here" for s in block):
                out.add("staged_not_for_registered_or_listed")
    parks_room = whole_parks(letter, q)
    assert parks_room >= 2 * waves
    for batch in batches:
        chunks = sum(sum(chunks_of(depths[s], tune, split)) for s in batch)
        out.add("whole_several_rounds" if chunks > parks_room else "whole_one_round")
    assert out <= set(BRANCHES), out - set(BRANCHES)
    return out


# ---- the case table ----------------------------------------------------------------------------------------------------------------
def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


def _queue_depths(letter, subs, tune, blocks=2, extra=3):
    """Every depth the queue treats differently, none above the cap: 0, 1, STEP-1, STEP, STEP+1, 2*STEP+1, two chunks, the cap."""
    step, split = queue_step(letter), ragged_split(letter, tune["cap"], tune["split"])
    kinds = [2 * step + 1, step + 1, step, step - 1, 1, 0, 5]
    if split:
        kinds = [tune["cap"], split + 1] + kinds
    return _cycle(kinds, blocks * subs + extra)


def _deep_depths(letter, subs, tune, many=False, big=True):
    """Sub-groups deeper than the cap among shallow ones: a partial item, whole items, more than eight items; the last sub-group is deep
    and partly beyond the rows."""
    keep = tune["keep"]
    d = _cycle([9, 3, 14, 0, 7], 2 * subs + 3)
    if many:
        for i in range(10):
            d[2 + 3 * i] = keep + DEEP_CHUNK * (1 + i % 2) + (5 if i % 3 else 0)
    else:
        d[1], d[4], d[subs + 2] = keep + 40, keep + 2 * DEEP_CHUNK, keep + (8 * DEEP_CHUNK + 5 if big else DEEP_CHUNK + 20)
    d[-1] = keep + DEEP_CHUNK + 9
    return d


def _rounds_depths(letter, tune):
    """Eight deep sub-groups whose chunks do not fit one round of the gather form's 16 KiB."""
    per = whole_parks(letter, GATHER_Q) // PLAN_DEEP_MOST + 1
    deep = tune["keep"] + DEEP_CHUNK * (per - 2) + 1 + 7            # one walked chunk and per - 1 items
    return [deep] * 8 + _cycle([4, 0, 9], 8 + 2)


def _shallow(n):
    return _cycle([6, 2, 11, 0, 8], n)


def _specs(letter):
    """name -> dict(fmt, shapes, depths(subs), rows_cut, make keywords, tune, modes, ...)."""
    z = letter == "Z"
    tiled_shapes = ("tiled",) if z else ("tiled", "staged")
    all_shapes = ("gather",) + tiled_shapes
    straddle = {"S": 48, "D": 8, "C": 48, "Z": 8}[letter]
    s = {}
    s["queue-hell"] = dict(fmt="hell", shapes=all_shapes, depths=lambda subs: _queue_depths(letter, subs, TUNE), cut=5, beta=0.5)
    s["queue-ell"] = dict(fmt="ell", shapes=all_shapes, depths=lambda subs: _queue_depths(letter, subs, TUNE_NO_SPLIT), cut=5, pitch_extra=64, beta=0.5,
                          tune=TUNE_NO_SPLIT)
    s["queue-ell-norS"] = dict(fmt="ell", shapes=("gather", "tiled"), depths=lambda subs: [queue_step(letter) + 1] * (subs + 2), cut=0, rs_null=True,
                               beta=0.0, pitch_extra=32)
    if not z:
        s["queue-most"] = dict(fmt="hell", shapes=("tiled",) if letter == "D" else (("staged",) if letter == "S" else ("gather",)),
                               depths=lambda subs: [v for v in _queue_depths(letter, subs, tune_most(letter)) if v <= tune_most(letter)["cap"]],
                               cut=9, tune=tune_most(letter), y_mode="z", expects=("split_most_chunks", "y_is_z"))
    s["queue-knob"] = dict(fmt="hell", shapes=("tiled",), depths=lambda subs: _queue_depths(letter, subs, TUNE), cut=1, knob=1, beta=0.0)
    s["queue-near-probe"] = dict(fmt="hell", shapes=tiled_shapes[-1:], depths=lambda subs: _queue_depths(letter, subs, TUNE), cut=1, knob=0,
                                 modes=("plan", "packed"))   # (without a plan a first call runs the 1 024-row shape: the probe's answer is for later calls)
    s["all-split"] = dict(fmt="hell", shapes=("tiled",), depths=lambda subs: [TUNE["cap"]] * (subs + 1), cut=3, hack=96,
                          expects=("hell_hack_96",) + (() if z else ("split_more_subs_than_2_waves",)))
    s["deep-hell32"] = dict(fmt="hell", shapes=tiled_shapes[-1:] + ("gather",), depths=lambda subs: _deep_depths(letter, subs, TUNE), cut=7)
    s["deep-hell96"] = dict(fmt="hell", shapes=("tiled",), depths=lambda subs: _deep_depths(letter, subs, TUNE), cut=7, hack=96, y_mode="z")
    s["deep-straddle"] = dict(fmt="hell", shapes=all_shapes, depths=lambda subs: _deep_depths(letter, subs, TUNE), cut=7, hack=straddle,
                              expects=("hell_hack_straddles", "deep_straddling_branch", "deep_strip_beyond_rows", "finish_more_than_8_items"))
    s["deep-ell"] = dict(fmt="ell", shapes=("tiled",), depths=lambda subs: _deep_depths(letter, subs, TUNE, big=False), cut=7, beta=0.0)
    s["many-deep"] = dict(fmt="hell", shapes=tiled_shapes[-1:], depths=lambda subs: _deep_depths(letter, subs, TUNE, many=True), cut=2, expects=("plan_stride_1", "plan_last_deep_workgroup_partial"))
    s["rounds"] = dict(fmt="hell", shapes=("gather",), depths=lambda subs: _rounds_depths(letter, TUNE), cut=4, modes=("list", "plan"),
                       expects=("whole_several_rounds",))
    for cols in ("low", "high", "below", "escape"):
        s[f"tile-{cols}"] = dict(fmt="ell" if cols == "below" else "hell", shapes=tiled_shapes, depths=lambda subs: _shallow(subs) + [0] * subs + [9, 5], cut=0,
                                 cols=cols, base=0 if cols == "high" else 1,
                                 expects={"low": ("tile_centred_clamped_low", "tile_base_odd"), "high": ("tile_centred_clamped_high",),
                                          "below": ("tile_column_below_base",), "escape": ("column_outside_tile",) if z else ("packed_escape", "packed_escape_below_base")}[cols])
    s["tile-high"]["beta"] = 0.0
    # a planned block most of whose sub-groups are the plan's: fewer items than wavefronts (13 of 16 elsewhere and more)
    s["mostly-deep"] = dict(fmt="hell", shapes=("gather",), depths=lambda subs: [TUNE["keep"] + 40] * 14 + [5, 9] + [TUNE["keep"] + 41] * 15 + [3, 7, 2], cut=3,
                            modes=("list", "plan"), expects=("items_fewer_than_waves", "plan_stride_1"))
    s["tiny"] = dict(fmt="hell", shapes=all_shapes, depths=lambda subs: [7], cut=12)
    if not z:
        s["staged-beyond"] = dict(fmt="hell", shapes=("staged",), depths=lambda subs: _shallow(2 * subs + 9), cut=6, perm="swap", expects=("staged_beyond",))
        s["staged-beyond-b0"] = dict(fmt="hell", shapes=("staged",), depths=lambda subs: _shallow(2 * subs + 9), cut=6, perm="swap", beta=0.0,
                                     expects=("staged_beyond_beta_zero", "staged_writeout_beta_zero"))
    s["no-row-order"] = dict(fmt="hell", shapes=("tiled", "gather"), depths=lambda subs: _deep_depths(letter, subs, TUNE), cut=7, modes=("list",),
                             row_order=False, knob=0)
    return s


def cases(letter):
    """case id -> dict(letter, fmt, shape, form, knob, tune, modes, beta, y_mode, row_order, off, and what make() needs)."""
    out = {}
    for name, spec in _specs(letter).items():
        for shape in spec["shapes"]:
            subs = SHAPES[shape][2]
            # (2 048 rows and more whose blocks of 2 048 are windows of the order: the probe says "staged" whatever the columns do -- the
            # matrices that are to run the 1 024-row shape from a plan stay below that: one whole workgroup and a partial one)
            small = shape == "tiled" and letter != "Z" and spec.get("knob", 0) == 0 and spec.get("row_order", True)
            depths = spec["depths"](30 if small else subs)
            rows = len(depths) * 32 - spec["cut"]
            # the 1 024-row shape has a plan only where the probe chose it (SPGPU_RAGGED_SHAPE 0: columns far from the diagonal, or complex
            # fp64); under the knob (1) it is the same kernel without one
            by_knob = shape == "tiled" and spec.get("knob") == 1
            knob = spec.get("knob", {"gather": 0, "tiled": 0, "staged": STAGED_KNOB}[shape])
            shift = 1500 if shape == "tiled" and knob == 0 and letter != "Z" and spec.get("row_order", True) else 0
            modes = ("list",) if by_knob else spec.get("modes", MODES)
            if SIZEOF[letter] > 8 or shape == "gather":
                modes = tuple(md for md in modes if md != "packed")
            cid = f"{name}-{shape}"
            out[cid] = dict(letter=letter, name=name, fmt=spec["fmt"], shape=shape, form=M.GATHER if shape == "gather" else M.AUTO, knob=knob,
                            tune=spec.get("tune", TUNE), modes=modes, beta=spec.get("beta", -0.5), y_mode=spec.get("y_mode", "y"),
                            row_order=spec.get("row_order", True), depths=depths, rows=rows, block_rows=subs * 32, expects=tuple(spec.get("expects", ())),
                            off=dict(x=(len(out) % 2) * WIDE[letter], z=len(out) % 3, y=(len(out) + 1) % 3),
                            make=dict(cols=spec.get("cols", "near"), perm=spec.get("perm", "rev"), base=spec.get("base", 1), hack=spec.get("hack", 32),
                                      rs_null=spec.get("rs_null", False), pitch_extra=spec.get("pitch_extra", 0), seed=cid, shift=shift))
    return out


def stale_pairs(letter):
    """case id -> (A, B, shape): A is planned, then B -- same rows, other depths -- is copied over the same arrays.  B's deep sub-groups are
    not in A's plan (worked off behind, nine of them in one block: two batches), and one that A's plan lists is shallow in B."""
    out = {}
    for shape in (("gather", "tiled") if letter == "Z" else ("gather", "staged" if letter in "SC" else "tiled")):
        subs = SHAPES[shape][2]
        n = subs + 3
        a, b = _shallow(n), _shallow(n)
        a[0] = a[subs + 1] = TUNE["keep"] + DEEP_CHUNK + 3
        for i in range(9):
            b[1 + i] = TUNE["keep"] + DEEP_CHUNK + i
        b[subs + 2] = TUNE["keep"] + 2 * DEEP_CHUNK
        out[f"stale-{shape}"] = (a, b, shape)
    return out


_MATRICES = {}


def matrix_of(case, depths=None, key=""):
    k = (case["letter"], case["make"]["seed"], key)
    if k not in _MATRICES:
        _MATRICES[k] = make(case["letter"], case["fmt"], depths or case["depths"], case["rows"], case["block_rows"], **case["make"])
    return _MATRICES[k]


def stale_case(letter, cid):
    a, b, shape = stale_pairs(letter)[cid]
    subs = SHAPES[shape][2]
    case = dict(letter=letter, name=cid, fmt="hell", shape=shape, form=M.GATHER if shape == "gather" else M.AUTO,
                knob={"gather": 0, "tiled": 0, "staged": STAGED_KNOB}[shape], tune=TUNE, beta=-0.5, y_mode="y", row_order=True, depths=b,
                rows=len(b) * 32 - 3, block_rows=subs * 32, off=dict(x=0, z=1, y=2),
                make=dict(cols="far" if shape == "tiled" and letter != "Z" else "near", perm="rev", base=1, hack=32, rs_null=False, pitch_extra=0, seed=cid, shift=0))
    return case, a, b


def case_route(case, mode, m, plan_of=None):
    """dispatch for one mode of a case."""
    probed = STAGED_KNOB if probe_said(m) in (4, 6) else 0
    deep = sum(d > case["tune"]["cap"] for d in sub_depths(plan_of or m)[0])
    route = dispatch(case["letter"], case["fmt"] == "hell", case["form"], case["knob"], case["row_order"], m.get("max_row", 0), m["rows"],
                     case["tune"], mode, probed=probed, deep=deep)
    assert route["plan"] or mode == "list", "this call has no plan"
    return route


def case_walk(case):
    """mode -> the branch names of that call."""
    m = matrix_of(case)
    return {mode: walk(m, case_route(case, mode, m), case["tune"], row_order=case["row_order"], beta=case["beta"], y_mode=case["y_mode"])
            for mode in case["modes"]}


def scalars_of(case):
    alpha = 1.5 if case["letter"] in "SD" else complex(1.5, -0.25)
    beta = case["beta"] if case["letter"] in "SD" or case["beta"] == 0 else complex(case["beta"], 0.75)
    return alpha, beta
