"""The FROZEN form of an ELL / HELL matrix without a row order (spgpu?SpmvFreeze with rIdx == NULL: spgpu_amd/csrc/frozen_slab.hip.h
freezeSlab, slabPackKernel, slabSlotsKernel, findFrozenSlab; slab_spmv.hip.h slabSpmvKernel<..., PACKED = true>), stated once for
tests/test_gpu_zz_unordered_frozen_shapes.py (which runs the cases on the GPU) and tests/test_frozen_launch_shapes.py (which checks on the CPU that the
table reaches all twelve PACKED instantiations and every named branch).  Builders, operands, the dispatch of an unfrozen call and the
walk of the unpacked kernels are tests/spmv_launch_shapes.py's; here are

  * the freeze restated on the host (pack: the groups' bases, the 16-bit words, entries, escapes, the copy's slot count),
  * the dispatch at Freeze time (can_freeze) and the lookup at run time (lookup_key, record_used) restated,
  * the PACKED kernels' control flow walked wavefront by wavefront (walk), the freeze side's branches (freeze_walk),
  * the case table: every gather / strips case of spmv_launch_shapes.cases, to be run frozen, plus the packed-only cases.

No torch, no library: importable everywhere.

Scope: S, D and C (complex fp64 has one row per lane and no 16-bit copy), rIdx == NULL, the forms GATHER and STRIPS (AUTO on a frozen
matrix is a test of its own in the GPU module; XTILE, SWEEP and the lean kernel never look the record up)."""
import numpy as np

import spmv_launch_shapes as M

LETTERS = "SDC"
ESCAPE = 0xFFFF               # the word that says "ask rP"
WORD_MAX = 0xFFFE             # the largest offset a word holds
UNWRITTEN = -1                # pack()'s mark for a slot of the copy slabPackKernel never writes
PACK_ROUND = 256              # ordered_rules.h packedBytes: the copy's bytes, rounded up
PLAN_RECORDS = 8              # spgpu_internal.h SPGPU_PLANS: records of the handle's plan table
#: the cases of every type whose Freeze is refused (slots == 0: all rows empty); tests/test_frozen_launch_shapes.py asserts that refused() finds
#: exactly these, tests/test_gpu_zz_unordered_frozen_shapes.py that exactly these answer SPGPU_UNSUPPORTED
REFUSED = ["ell-len0-gather", "ell-len0-strips", "hell-len0-gather", "hell-len0-strips"]


# ---- the freeze restated ------------------------------------------------------------------------------------------------------------
def lengths(m):
    """Row lengths as the kernels take them: rS, or maxNnz for every row where rS is NULL."""
    if m["rs_null"]:
        return np.full(m["rows"], m["max_row"], np.int64)
    return np.asarray(m["row_lengths"], np.int64)


def slot_count(m):
    """Slots of the 16-bit copy.  HELL (slabSlotsKernel): the last hack's offset + hackSize x its longest row; ELL: idxStride * maxNnz.
    0: the Freeze is refused."""
    if m["fmt"] == "hell":
        hack, rows = m["hack_size"], m["rows"]
        last = (rows - 1) // hack
        return int(m["hack_offsets"][last]) + hack * int(lengths(m)[last * hack:rows].max(initial=0))
    return m["pitch"] * m["max_row"]


def packed_bytes(slots):
    return (2 * slots + PACK_ROUND - 1) // PACK_ROUND * PACK_ROUND


def all_entries(m):
    """(rows, 0-based columns, slots) of every stored entry k < len, the ones below the index base (column < 0) included."""
    lens = lengths(m)
    rows = np.repeat(np.arange(m["rows"], dtype=np.int64), lens)
    k = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    if m["fmt"] == "hell":
        hack = m["hack_size"]
        slots = np.asarray(m["hack_offsets"], np.int64)[rows // hack] + rows % hack + k * hack
    else:
        slots = rows + k * m["pitch"]
    return rows, np.asarray(m["indices"], np.int64)[slots] - m["base"], slots


def pack(m, letter=None):
    """slabPackKernel restated: (bases, words, entries, escapes, slots).  bases[g]: the lowest column >= 0 of group g's rows, 0 if it has
    none; words[slot]: the column's offset from its group's base, ESCAPE where the column is negative or the offset is >= 0xFFFF,
    UNWRITTEN at every slot no row owns at a k below its length."""
    letter = letter or m["letter"]
    g_rows = M.group_rows(letter)
    slots = slot_count(m)
    groups = (m["rows"] + g_rows - 1) // g_rows
    rows, cols, at = all_entries(m)
    group = rows // g_rows
    lowest = np.full(groups, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lowest, group[cols >= 0], cols[cols >= 0])
    bases = np.where(lowest == np.iinfo(np.int64).max, 0, lowest)
    off = cols - bases[group]
    fits = (cols >= 0) & (off < ESCAPE)
    words = np.full(max(slots, 0), UNWRITTEN, np.int64)
    if slots > 0:
        assert at.size == 0 or int(at.max()) < slots
        words[at] = np.where(fits, off, ESCAPE)
    return bases, words, int(rows.size), int(np.count_nonzero(~fits)), slots


_PACKS = {}


def pack_of(case):
    key = (case["letter"], case["id"])
    if key not in _PACKS:
        _PACKS[key] = pack(M.matrix_of(case), case["letter"])
    return _PACKS[key]


# ---- Freeze's dispatch and the run-time lookup restated -----------------------------------------------------------------------------------
def can_freeze(letter, hell, form, rows, hack, val_stride, idx_stride, addr, slots, entries, escapes, pct=1, row_order=False):
    """launchSlabFamily(..., SpmvCall::Freeze) down to freezeSlab's verdict: (frozen, the first condition that fails or None).  form: the
    handle's at the time of the call."""
    import exact_ref as X
    if rows <= 0:
        return False, "rows"
    if M.SIZEOF[letter] not in (4, 8):
        return False, "type"                    # wideOf == 1: no wide kernel, no copy
    if row_order:
        return False, "row-order"               # (a row order has a frozen form of its own: planned_spmv.hip)
    ok, fails = M.wide_layout(letter, hell, rows, hack, val_stride, idx_stride, addr["cM"], addr["rP"])
    if not ok:
        return False, "layout:" + fails
    if form in (M.XTILE, M.SWEEP):
        return False, "form"                    # SWEEP on a wide layout returns before the Freeze; XTILE is excluded by name
    if slots <= 0:
        return False, "slots"
    if not X.freeze_keeps(entries, escapes, max(pct, 0)):
        return False, "share"
    return True, None


def case_can_freeze(case, pct=100):
    m = M.matrix_of(case)
    hack, vs, is_, _ = M.strides(m)
    _, _, entries, escapes, slots = pack_of(case)
    return can_freeze(case["letter"], m["fmt"] == "hell", case["form"], m["rows"], hack, vs, is_, M.byte_offsets(case), slots, entries, escapes, pct)


#: what planKey (slab_args.hip.h) puts into a record's key and samePlanKey (spmv_records.c) compares; rIdx is NULL, deepCap 0 and subs
#: -groupRows for every record of this kind.  NOT in the key: cM, valStride, x, y, z, alpha, beta, avgNnzPerRow.
KEY_FIELDS = ("rP", "rS", "hackOffsets", "idxStride", "rows", "hackSize", "baseIndex", "maxNnz", "subs")


def lookup_key(letter, hell, rP, rS, hack_offsets, hack, idx_stride, max_nnz, rows, base):
    """planKey(a, nullptr, 0, -groupRows) of a call, as the C ABI fills SlabArgs (HELL: idxStride = hackSize, maxNnz = 0; ELL: hackSize = 0,
    hackOffsets = NULL).  rP, rS, hack_offsets: addresses (None for NULL)."""
    return dict(rP=rP, rS=rS, hackOffsets=hack_offsets if hell else None, idxStride=hack if hell else idx_stride, rows=rows,
                hackSize=hack if hell else 0, baseIndex=base, maxNnz=0 if hell else max_nnz, subs=-M.group_rows(letter))


def is_wide(kernel):
    """The kernel of the Wide route (spmv_rules.h): the only one in front of which launchRowsAsTheyCome looks the record up."""
    return kernel[0] == "slab" and kernel[2] > 1 and kernel[7] and kernel[11] == 0


def record_used(unfrozen_kernel, call_key, frozen_key):
    """findFrozenSlab: is the record used (and counted) by a call whose unfrozen dispatch names `unfrozen_kernel`?"""
    return is_wide(unfrozen_kernel) and all(call_key[f] == frozen_key[f] for f in KEY_FIELDS)


def packed(kernel):
    """The PACKED twin of a Wide kernel."""
    assert is_wide(kernel)
    return kernel[:13] + (True,)


def every_instantiation():
    """slabSpmvKernel<T, WIDE, PH, IS_HELL, true, UNROLL, true, true, STRIPS, 256, 0, 0, true>: S, D, C x ELL / HELL x gather / strips."""
    return {packed(M.route_kernel(L, route, hell)) for L in LETTERS for hell in (True, False) for route in ("gather", "strips")}


def frozen_dispatch(case, addr=None):
    """The dispatch of a call on the case's matrix once it is frozen: the unfrozen one with PACKED set."""
    d = M.case_dispatch(case, addr=addr)
    return dict(d, kernel=packed(d["kernel"]))


# ---- the PACKED kernels' control flow, walked on the CPU ---------------------------------------------------------------------------------
KERNEL_BRANCHES = (
    "packed_word",                        # a word below 0xFFFF consumed as a column (gather stages; the first word of a strip)
    "packed_word_max",                    # ... 0xFFFE
    "escape_far",                         # 0xFFFF for a column 65 535 or more above the base: columnOf asks rP
    "escape_negative",                    # 0xFFFF for a column below the index base: asks rP, the entry is masked
    "escape_in_first_stage",              # an escape consumed by the stage at kBase 0
    "escape_in_last_partial_stage",       # ... by a stage that reaches beyond the group's longest row
    "escape_in_tail_row_staged_part",     # ... at k < tailFrom in a row the whole wavefront finishes
    "escape_in_tail_row_tail_part",       # 0xFFFF at k >= tailFrom of such a row: the tail reads rP, the word is never loaded
    "pad_word_in_live_strip",             # k < laneLongest, k >= len[t]: an unwritten word is loaded and must not count
    "stage_past_lane_longest",            # k >= laneLongest inside a stage: the 0xFFFF filler, nothing loaded
    "strip_stage_packed",                 # stages consumed as strips: x from packBase + the strip's first word
    "strip_broken_by_escape",             # stageIsStrips says no because a present word is 0xFFFF
    "strip_broken_by_escape_at_t_gt_0",   # ... and the strip's first word is not
    "strip_broken_by_pad",                # ... because a strip's rows end at different k
    "strip_broken_by_columns",            # ... because the words are not consecutive
    "strip_first_word_0xFFFE",            # the strip test on a first word 0xFFFE (its neighbour cannot be 0xFFFF: that is the escape)
    "group_base_zero",                    # a group with entries whose lowest column is 0
    "group_base_above_65535",             # a base no 16-bit word could hold
    "group_empty",                        # all rows empty: base 0, no stage
    "group_all_negative",                 # entries, all below the index base: base 0, every word an escape
    "group_partial_last",                 # the last group has fewer rows than a wavefront owns
    "workgroup_partial_last",             # wavefronts of the last workgroup leave at once
    "wide_store",                         # a strip stored as one pack
    "scalar_store_wide_io_off",           # ... by element because z or y is off its 16-byte boundary
    "scalar_store_last_strip_partial",    # ... because the strip runs past the last row
    "tail_taken",                         # wavefronts that hand rows to the whole wavefront
    "tail_not_taken",                     # wavefronts whose stage loop runs to the end
)
CALL_BRANCHES = ("beta_zero", "beta_nonzero", "y_is_z")
FREEZE_BRANCHES = (
    "hack_holds_several_groups",          # HELL: hackSize a multiple of the group's rows
    "group_spans_several_hacks",          # HELL: hackSize below the group's rows
    "hack_equals_group",
    "last_hack_partial",                  # rows no multiple of hackSize
    "last_hack_depth_0",                  # slabSlotsKernel: the last hack's rows are all empty, behind hacks that are not
    "ell_pitches_differ",                 # the copy is indexed with idxStride, the coefficients with valStride
    "ell_pitch_above_rows",               # idxStride beyond the rows rounded up to whole strips
    "ell_rs_null",                        # every row maxNnz long
    "rows_lt_group",                      # fewer rows than one group
    "pack_lane_two_rows",                 # slabPackKernel's j == 1: a row at lane + 64 of its group with entries (groups of 128 rows)
    "slots_round_up_by_last_hack",        # the last hack's depth decides the copy's bytes after the rounding to 256
)
BRANCHES = KERNEL_BRANCHES + CALL_BRANCHES + FREEZE_BRANCHES

#: what cannot exist: the hack branches on ELL, the pitch and rS == NULL branches on HELL (hell.h: rS is required), and slabPackKernel's
#: second row per lane for fp32, whose groups have 32 rows.
NEVER = {
    ("ell", L): {b for b in FREEZE_BRANCHES if "hack" in b} for L in LETTERS
}
NEVER.update({("hell", L): {b for b in FREEZE_BRANCHES if b.startswith("ell_")} for L in LETTERS})
for _fmt in ("hell", "ell"):
    NEVER[(_fmt, "S")] = NEVER[(_fmt, "S")] | {"pack_lane_two_rows"}


def walk(m, kernel, wide_io, the_pack=None):
    """How often one call of a PACKED kernel takes each branch, from the arrays and the restated copy alone.  Also `stages`, `tail_from`
    (wavefront -> kBase of the switch), `rp_reads`: the slots of rP the kernel reads (escapes its stages consume, and the tail rows'
    entries from tailFrom on), `word_slots`: the slots of the copy it loads."""
    _, L, rpl, ph, _, _, unroll, pipe, tail, strips, block, tile, every, pk = kernel
    assert pk and pipe and tail and tile == 0 and every == 0 and rpl > 1
    bases, words, _, _, _ = the_pack if the_pack is not None else pack(m, L)
    rows = m["rows"]
    lens_all = lengths(m)
    lpc = M.WAVE // ph
    group_rows = lpc * rpl
    waves = block // M.WAVE
    step = ph * unroll
    length = lambda r: int(lens_all[r]) if r < rows else 0
    n = dict.fromkeys(KERNEL_BRANCHES, 0)
    n.update(stages=0, stage_gather=0, tail_from={}, rp_reads=set(), word_slots=set())
    grid = M.slab_grid(kernel, rows)[0]
    for group in range(grid * waves):
        g0 = group * group_rows
        if g0 >= rows:
            n["workgroup_partial_last"] += 1
            continue
        n["group_partial_last"] += g0 + group_rows > rows
        lens = [[length(g0 + s * rpl + t) for t in range(rpl)] for s in range(lpc)]
        lane_longest = [max(l) for l in lens]
        group_longest = max(lane_longest)
        cols = [M._entry(m, g0 + s * rpl + t, k)[0] for s in range(lpc) for t in range(rpl) for k in range(lens[s][t])]
        live_cols = [c for c in cols if c >= 0]
        n["group_empty"] += group_longest == 0
        n["group_all_negative"] += bool(cols) and not live_cols
        n["group_base_zero"] += bool(live_cols) and min(live_cols) == 0
        n["group_base_above_65535"] += int(bases[group]) > 0xFFFF
        assert int(bases[group]) == (min(live_cols) if live_cols else 0)

        def word(s, t, k):
            col, slot = M._entry(m, g0 + s * rpl + t, k)
            w = int(words[slot])
            assert w != UNWRITTEN and (w == ESCAPE or int(bases[group]) + w == col)
            return w, col, slot

        tail_from, done, in_strips = group_longest, False, bool(strips)
        k_base, stages, consumed_escapes = 0, 0, []
        while k_base < group_longest:
            busy = ph * sum(k_base < ll for ll in lane_longest)
            if k_base % step == 0 and busy <= M.TAIL_LANES:
                tail_from, done = k_base, True
                n["tail_from"][group] = k_base
                break
            if in_strips:
                why = set()
                for s in range(lpc):
                    for k in range(k_base, k_base + step):
                        present = k < lens[s][0]
                        if any((k < lens[s][t]) != present for t in range(rpl)):
                            why.add("strip_broken_by_pad")
                        if present:
                            ws = [word(s, t, k)[0] if k < lens[s][t] else None for t in range(rpl)]
                            n["strip_first_word_0xFFFE"] += ws[0] == WORD_MAX
                            esc = [t for t in range(rpl) if ws[t] == ESCAPE]
                            if esc:
                                why.add("strip_broken_by_escape")
                                if esc[0] > 0:
                                    why.add("strip_broken_by_escape_at_t_gt_0")
                            elif any(ws[t] is not None and ws[t] != ws[0] + t for t in range(rpl)):
                                why.add("strip_broken_by_columns")
                if why:
                    for name in why:
                        n[name] += 1
                    in_strips = False
                else:
                    n["strip_stage_packed"] += 1
                    for s in range(lpc):
                        for k in range(k_base, min(k_base + step, lens[s][0])):
                            w, _, slot = word(s, 0, k)
                            n["packed_word"] += 1
                            n["packed_word_max"] += w == WORD_MAX
                            n["word_slots"].update(word(s, t, k)[2] for t in range(rpl))
                        n["stage_past_lane_longest"] += max(0, k_base + step - max(lane_longest[s], k_base))
            if not in_strips:
                n["stage_gather"] += 1
                for s in range(lpc):
                    for k in range(k_base, k_base + step):
                        if k >= lane_longest[s]:
                            n["stage_past_lane_longest"] += 1
                            continue
                        for t in range(rpl):
                            if k >= lens[s][t]:
                                n["pad_word_in_live_strip"] += 1
                                continue
                            w, col, slot = word(s, t, k)
                            n["word_slots"].add(slot)
                            if w != ESCAPE:
                                n["packed_word"] += 1
                                n["packed_word_max"] += w == WORD_MAX
                                continue
                            n["rp_reads"].add(slot)
                            n["escape_negative" if col < 0 else "escape_far"] += 1
                            n["escape_in_first_stage"] += k_base == 0
                            n["escape_in_last_partial_stage"] += k_base + step > group_longest
                            consumed_escapes.append((s, t, k))
            stages += 1
            k_base += step
        n["stages"] += stages
        n["tail_taken" if done else "tail_not_taken"] += 1
        if done:
            for s in range(lpc):
                for t in range(rpl):
                    if lens[s][t] > tail_from:
                        n["escape_in_tail_row_staged_part"] += sum((s, t) == e[:2] for e in consumed_escapes)
                        for k in range(tail_from, lens[s][t]):
                            w, _, slot = word(s, t, k)
                            n["rp_reads"].add(slot)
                            n["escape_in_tail_row_tail_part"] += w == ESCAPE
        for s in range(lpc):
            if g0 + s * rpl >= rows:
                continue
            if wide_io and g0 + s * rpl + rpl <= rows:
                n["wide_store"] += 1
            elif not wide_io:
                n["scalar_store_wide_io_off"] += 1
            else:
                n["scalar_store_last_strip_partial"] += 1
    return n


def freeze_walk(m, letter):
    """The branches of freezeSlab, slabSlotsKernel and slabPackKernel a matrix takes."""
    g, w, rows = M.group_rows(letter), M.WIDE[letter], m["rows"]
    lens = lengths(m)
    n = dict.fromkeys(FREEZE_BRANCHES, 0)
    slots = slot_count(m)
    n["rows_lt_group"] = int(rows < g)
    n["pack_lane_two_rows"] = int(any(lens[r] > 0 for r in range(rows) if r % g >= M.WAVE))
    if m["fmt"] == "hell":
        hack = m["hack_size"]
        last = (rows - 1) // hack
        n["hack_holds_several_groups"] = int(hack > g and hack % g == 0)
        n["group_spans_several_hacks"] = int(hack < g)
        n["hack_equals_group"] = int(hack == g)
        n["last_hack_partial"] = int(rows % hack != 0)
        n["last_hack_depth_0"] = int(slots > 0 and lens[last * hack:rows].max(initial=0) == 0)
        n["slots_round_up_by_last_hack"] = int(packed_bytes(slots) > packed_bytes(int(m["hack_offsets"][last])) > 0)
    else:
        n["ell_pitches_differ"] = int(m["pitch"] != m["val_pitch"])
        n["ell_pitch_above_rows"] = int(m["pitch"] > (rows + w - 1) // w * w)
        n["ell_rs_null"] = int(m["rs_null"])
    return n


_WALKS = {}


def case_walk(case):
    """Every branch of BRANCHES with how often the case's frozen call (and its Freeze) takes it."""
    key = (case["letter"], case["id"])
    if key not in _WALKS:
        m = M.matrix_of(case)
        d = frozen_dispatch(case)
        n = walk(m, d["kernel"], d["wide_io"], pack_of(case))
        n.update(freeze_walk(m, case["letter"]))
        n["beta_zero"] = int(case["scalars"][1] == 0)
        n["beta_nonzero"] = int(case["scalars"][1] != 0)
        n["y_is_z"] = int(case["y_mode"] == "z")
        _WALKS[key] = n
    return _WALKS[key]


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
FAR = 70000                   # columns of neighbouring groups lie this far apart: more than a word holds


def packed_only(letter):
    """id -> case (spmv_launch_shapes' fields): the matrices that put a frozen call on a named branch.  At most three workgroups of 4 G rows
    and a partial one; x of at most 6 * FAR + a few thousand elements."""
    w, G, STEP = M.WIDE[letter], M.group_rows(letter), M.wide_step(letter)
    c = {}

    def add(cid, fmt, route, rc_nc, claims=(), base=0, off=None, y_mode="y", scalars=M.WITH_Y, seed=0, **kw):
        assert cid not in c, cid
        form = M.GATHER if route == "gather" else M.STRIPS

        def make():
            rc, nc = rc_nc()
            return M.build(letter, fmt, rc, nc, base, seed=seed, **kw)
        c[cid] = dict(id=cid, letter=letter, fmt=fmt, form=form, make=make, route=route, claims=tuple(claims), off=dict(M.NO_OFF, **(off or {})),
                      y_mode=y_mode, scalars=scalars, avg=0, fails=None)

    def pattern(route, lens, seed=0, ncols=3000):
        """Band rows for the strip kernel, scattered ones for the gather kernel: (row_cols, ncols)."""
        lens = np.asarray(lens, np.int64)
        if route == "strips":
            return M.band(lens), len(lens) + int(lens.max(initial=0)) + 4
        return M.scattered(lens, ncols, seed), ncols

    def shifted(rc, nc):
        """Group i's columns moved up by i * FAR: a base taken from another group names other elements of x."""
        return [[col + (i // G) * FAR for col in cols] for i, cols in enumerate(rc)], nc + ((len(rc) - 1) // G) * FAR

    R1 = 4 * G + G + w + 1            # two workgroups, the second with one whole group and a partial one
    R2 = 2 * G + w + 1
    fill = M._lens_fill
    for fmt in ("hell", "ell"):
        for route in ("gather", "strips"):
            # -- bases differ: group i's columns start at i * FAR
            for base in (0, 1):
                def bases_differ(route=route):
                    rc, nc = pattern(route, fill(R1, STEP + 1), seed=11)
                    rc[0][0] = 0                                            # group 0 counts from column 0
                    return shifted(rc, nc)
                add(f"{fmt}-pk-bases-differ-base{base}-{route}", fmt, route, bases_differ, ["group_base_above_65535", "group_base_zero", "packed_word",
                    "group_partial_last", "workgroup_partial_last"] + (["strip_stage_packed"] if route == "strips" else []), base=base, seed=11)

                # -- the 16-bit limit: in group 1, offsets 65 533 .. 65 536 from the group's lowest column; row G + w is the first row (t == 0) of
                # a strip, so under STRIPS the word 0xFFFE is the first word of a strip
                def limit(route=route):
                    rc, nc = pattern(route, fill(R2, STEP + 1), seed=12)
                    lowest = min(col for cols in rc[G:2 * G] for col in cols)
                    rc[G + w][1:5] = [lowest + e for e in (65533, 65534, 65535, 65536)]
                    return rc, max(nc, lowest + 65537)
                add(f"{fmt}-pk-limit-base{base}-{route}", fmt, route, limit, ["packed_word_max", "escape_far", "escape_in_first_stage"] +
                    (["strip_first_word_0xFFFE", "strip_broken_by_columns"] if route == "strips" else []), base=base, seed=12)

            # -- negatives (index base 1, index 0): one inside a live group, a group whose only entries are negative, an empty group
            def negatives(route=route):
                lens = fill(3 * G + w + 1, STEP + 1)
                lens[G:2 * G] = 2
                lens[2 * G:3 * G] = 0
                rc, nc = pattern(route, lens, seed=13)
                for i in range(G, 2 * G):
                    rc[i] = [-1, -1]
                rc[w + 1][2] = -1
                rc[3 * G][0] = -1
                return rc, nc
            add(f"{fmt}-pk-negatives-{route}", fmt, route, negatives, ["escape_negative", "group_all_negative", "group_empty", "group_partial_last"],
                base=1, seed=13)

            # -- escapes in the first and in the last, partial stage (rows of two stages and three columns: no tail row)
            def stage_escapes(route=route):
                rc, nc = pattern(route, fill(R2, 2 * STEP + 3), seed=14)
                rc[w][1] = nc + FAR
                rc[G + 2 * w + 1][2 * STEP + 1] = nc + FAR + 5
                return rc, nc + FAR + 6
            add(f"{fmt}-pk-stage-escapes-{route}", fmt, route, stage_escapes, ["escape_in_first_stage", "escape_in_last_partial_stage", "escape_far",
                "tail_not_taken"] + (["strip_broken_by_escape"] if route == "strips" else []), seed=14)

            # -- tail rows with escapes: strip 1 of group 0 and strip 1 of group 1 are long (whole strips, so that the band's first stage is
            # a strip stage); group 0's escape lies behind tailFrom, group 1's in front of it, at t == 1
            def tail_escapes(route=route):
                lens = fill(R2, 3)
                lens[w:2 * w] = STEP + 70
                lens[G + w:G + 2 * w] = STEP + 9
                rc, nc = pattern(route, lens, seed=15)
                rc[w + 1][STEP + 5] = nc + FAR
                rc[G + w + 1][2] = nc + FAR + 3
                return rc, nc + FAR + 4
            add(f"{fmt}-pk-tail-escapes-{route}", fmt, route, tail_escapes, ["tail_taken", "escape_in_tail_row_tail_part", "escape_in_tail_row_staged_part"] +
                (["strip_stage_packed", "strip_broken_by_escape_at_t_gt_0"] if route == "strips" else []), seed=15)

            # -- ragged lengths inside every strip: words never written, loaded by the live lanes
            def pad_words(route=route):
                lens = M._rng("pk-pad", letter, fmt).integers(0, STEP + 4, R2)
                lens[::w] = np.maximum(lens[::w], 1) - 1                     # (every t == 0 row differs from some neighbour)
                return pattern(route, lens, seed=16)
            add(f"{fmt}-pk-pad-words-{route}", fmt, route, pad_words, ["pad_word_in_live_strip", "stage_past_lane_longest"] +
                (["strip_broken_by_pad"] if route == "strips" else []), seed=16, off=dict(z=1) if fmt == "hell" else dict(y=1))

        # -- strips broken in the second stage: by an escape at t == 0, at t == WIDE - 1; by a t == 0 row one entry shorter than its neighbour
        for tag, t in (("t0", 0), ("tlast", w - 1)):
            def strip_escape(t=t):
                rc, nc = pattern("strips", fill(R2, 2 * STEP + 3))
                rc[G + 3 * w + t][STEP + 1] = nc + FAR
                return rc, nc + FAR + 1
            add(f"{fmt}-pk-strip-escape-{tag}-strips", fmt, "strips", strip_escape, ["strip_stage_packed", "strip_broken_by_escape", "escape_far"] +
                (["strip_broken_by_escape_at_t_gt_0"] if t else []), seed=17)

        def strip_short():
            lens = fill(R2, 2 * STEP + 3)
            lens[G + 3 * w] -= 1
            return pattern("strips", lens)
        add(f"{fmt}-pk-strip-short-t0-strips", fmt, "strips", strip_short, ["strip_stage_packed", "strip_broken_by_pad", "pad_word_in_live_strip"], seed=18)

    # -- HELL: hacks of one strip, half a group, a group, three groups; ragged depths, a partial last hack; a last hack of depth 0
    for hack in (w, G // 2, G, 3 * G):
        rows = 3 * G + w + 1
        for route in ("gather", "strips"):
            for empty_last in ((False, True) if route == "gather" or hack == G // 2 else (False,)):
                def hacks(route=route, hack=hack, empty_last=empty_last):
                    h = np.arange(rows) // hack
                    lens = (h * 5 + 3) % (STEP + 4) + 1
                    if hack >= G:
                        lens = lens + (np.arange(rows) // G) % 3             # (ragged inside a hack that holds several groups)
                    if empty_last:
                        lens[(rows - 1) // hack * hack:] = 0
                    return pattern(route, lens, seed=19 + hack)
                claims = [{True: "group_spans_several_hacks", False: "hack_holds_several_groups"}[hack < G] if hack != G else "hack_equals_group",
                          "last_hack_partial"] + (["last_hack_depth_0"] if empty_last else [])
                add(f"hell-pk-hack{hack}{'-empty-last' if empty_last else ''}-{route}", "hell", route, hacks, claims, hack=hack, seed=19)
    # -- ELL: an index pitch that is not the value pitch; pitches far above the rows; rS == NULL with maxNnz on a stage boundary and one above
    Rw = (R2 + w - 1) // w * w
    for route in ("gather", "strips"):
        add(f"ell-pk-pitches-differ-{route}", "ell", route, lambda route=route: pattern(route, fill(R2, STEP + 3), seed=31),
            ["ell_pitches_differ", "ell_pitch_above_rows"], idx_pitch=Rw + 2 * w, val_pitch=Rw + 6 * w, seed=31)
        add(f"ell-pk-index-pitch-smaller-{route}", "ell", route, lambda route=route: pattern(route, fill(R2, STEP + 3), seed=32),
            ["ell_pitches_differ"], idx_pitch=Rw, val_pitch=Rw + 4 * w, seed=32, base=1)
        add(f"ell-pk-pitch-above-rows-{route}", "ell", route, lambda route=route: pattern(route, fill(R2, STEP + 3), seed=33),
            ["ell_pitch_above_rows"], idx_pitch=Rw + G, val_pitch=Rw + G, seed=33)
        for mx in (2 * STEP, 2 * STEP + 1):
            add(f"ell-pk-rsnull-max{mx}-{route}", "ell", route, lambda route=route, mx=mx: pattern(route, fill(R2, mx), seed=34),
                ["ell_rs_null", "tail_not_taken"], rs_null=True, seed=34, y_mode="nan" if mx % 2 else "y",
                scalars=M.PLAIN if mx % 2 else M.WITH_Y)
    return c


_TABLES = {}


def cases(letter):
    """id -> case: (a) every case of spmv_launch_shapes.cases whose route is gather or strips, as it stands, to be run frozen; (b) the
    packed-only cases."""
    if letter not in _TABLES:
        table = {cid: c for cid, c in M.cases(letter).items() if c["route"] in ("gather", "strips")}
        new = packed_only(letter)
        assert not set(table) & set(new)
        table.update(new)
        _TABLES[letter] = table
    return _TABLES[letter]


def refused(letter):
    """The ids of the cases whose Freeze is refused even with every escape allowed (slots == 0)."""
    return sorted(cid for cid, c in cases(letter).items() if not case_can_freeze(c)[0])


# ---- matrices of the tests beside the table -----------------------------------------------------------------------------------------------
def copy_is_read_matrix(letter, fmt, route, with_tail_and_escape):
    """A matrix for "the copy is what is read": rows a multiple of the group.  Plain: no tail row, no escape, so the frozen call reads no
    word of rP.  Otherwise: one tail row and one escape."""
    G, STEP = M.group_rows(letter), M.wide_step(letter)
    lens = M._lens_fill(3 * G if with_tail_and_escape else 2 * G, STEP + 3)
    if with_tail_and_escape:
        lens[:2 * G] = 3                                                # (the third group stays a band of whole stages)
        lens[M.WIDE[letter]] = STEP + 40
    if route == "strips":
        rc, nc = M.band(lens), len(lens) + int(lens.max()) + 4
    else:
        rc, nc = M.scattered(lens, 3000, 41), 3000
    if with_tail_and_escape:
        rc[G + 5][1] = nc + FAR
        nc += FAR + 1
    return M.build(letter, fmt, rc, nc, 0, seed=41)
