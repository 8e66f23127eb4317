"""CPU: the case table of tests/frozen_launch_shapes.py (run on the GPU by tests/test_gpu_zz_unordered_frozen_shapes.py) is what that module needs it
to be.  The restated shapes are spmv_rules.h's (asked through tests/spmv_dispatch_cases.cpp with frozen = 1); the table names all twelve
slabSpmvKernel<..., PACKED = true> instantiations, each with a case of more than one workgroup; every branch of
frozen_launch_shapes.BRANCHES is reached for every type and format where it can exist (NEVER states where it cannot), by two cases
at least, so that no single case can be removed without another one still standing on everything it reaches; a case named for a branch
reaches it; pack() agrees with exact_ref.unordered_escapes on every matrix and with a slot-by-slot brute force on the packed-only ones;
and the cases whose Freeze is refused are the all-empty matrices, by name."""
import numpy as np
import pytest

import exact_ref as X
import frozen_launch_shapes as F
import spmv_launch_shapes as M
import test_spmv_dispatch as D

TABLE = {L: F.cases(L) for L in F.LETTERS}
NEW = {L: F.packed_only(L) for L in F.LETTERS}
#: slots == 0: spgpu?SpmvFreeze answers SPGPU_UNSUPPORTED (every row empty); the GPU module asserts exactly these
REFUSED = F.REFUSED
#: the cases that alone reach something (per type and format): none
SOLE = {}


def _reach():
    """(letter, fmt, case id) -> (kernel, grid, the names of the branches taken) of every case that freezes."""
    out = {}
    for L in F.LETTERS:
        for cid, c in TABLE[L].items():
            if cid in REFUSED:
                continue
            n = F.case_walk(c)
            d = F.frozen_dispatch(c)
            out[(L, c["fmt"], cid)] = (d["kernel"], d["grid"][0], {b for b in F.BRANCHES if n[b] > 0})
    return out


REACH = _reach()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return M.dispatch_program(tmp_path_factory.mktemp("frozen_shapes"))


def test_the_restated_shapes_are_the_headers(program):
    """slabShape(Wide, bytes, strips, packed = true), wideGroupRows and slabGrid, on every case at its own byte offsets."""
    src = M.header_constants(program)
    assert all(src[f"wideGroupRows{M.SIZEOF[L]}"] == M.group_rows(L) == X.group_rows_of(L) for L in F.LETTERS)
    for L in F.LETTERS:
        calls = []
        for c in TABLE[L].values():
            m = M.matrix_of(c)
            hack, vs, is_, mx = M.strides(m)
            calls.append(D.call(L, m["fmt"] == "hell", c["form"], m["rows"], hack, vs, is_, mx, c["avg"], M.byte_offsets(c),
                                has_beta=c["scalars"][1] != 0, frozen=True))
        for c, g in zip(TABLE[L].values(), D.check(program, calls)):
            d = F.frozen_dispatch(c)
            assert g["route"] == "wide" and g["kernel"][13] is True, c["id"]
            assert (g["kernel"], g["grid"], g["wide_io"], g["noted"], g["probe"]) == (d["kernel"], d["grid"], d["wide_io"], d["noted"], None), c["id"]
            assert g["kernel"] == F.packed(M.route_kernel(L, c["route"], c["fmt"] == "hell")), c["id"]


def test_the_twelve_instantiations_by_name():
    names = sorted(M.kernel_name(k) for k in F.every_instantiation())
    assert len(names) == 12
    assert "slabSpmvKernel<double, 2, 1, true, true, 8, true, true, false, 256, 0, 0, true>" in names
    assert "slabSpmvKernel<float, 4, 8, false, true, 2, true, true, true, 256, 0, 0, true>" in names
    assert "slabSpmvKernel<spgpu::Cx<float>, 2, 1, true, true, 8, true, true, true, 256, 0, 0, true>" in names
    assert all(name.endswith("256, 0, 0, true>") for name in names)


def test_every_instantiation_has_a_case_and_one_of_more_than_one_workgroup():
    grids = {}
    for kernel, grid, _ in REACH.values():
        grids[kernel] = max(grids.get(kernel, 0), grid)
    assert set(grids) == F.every_instantiation()
    assert all(g > 1 for g in grids.values()), [M.kernel_name(k) for k, g in grids.items() if g < 2]
    # ... and of both store forms
    for kernel in F.every_instantiation():
        stores = set().union(*(names & {"wide_store", "scalar_store_wide_io_off"} for k, _, names in REACH.values() if k == kernel))
        assert stores == {"wide_store", "scalar_store_wide_io_off"}, M.kernel_name(kernel)


def _missing(reach, letter, fmt):
    """What the coverage assertions would miss for a type and a format on this reach."""
    mine = [v for (L, f, _), v in reach.items() if (L, f) == (letter, fmt)]
    kernels = {k for k in F.every_instantiation() if k[1] == letter and k[4] == (fmt == "hell")}
    taken = set().union(*(names for _, _, names in mine)) if mine else set()
    return (kernels - {k for k, _, _ in mine}) | (set(F.BRANCHES) - F.NEVER[(fmt, letter)] - taken)


@pytest.mark.parametrize("fmt", ["hell", "ell"])
@pytest.mark.parametrize("letter", F.LETTERS)
def test_every_branch_is_reached_where_it_can_exist(letter, fmt):
    assert not _missing(REACH, letter, fmt), sorted(map(str, _missing(REACH, letter, fmt)))
    taken = set().union(*(names for (L, f, _), (_, _, names) in REACH.items() if (L, f) == (letter, fmt)))
    assert not taken & F.NEVER[(fmt, letter)], sorted(taken & F.NEVER[(fmt, letter)])


def test_removing_a_case_leaves_everything_covered():
    """The coverage evaluated again on the table without each case in turn: nothing is lost (SOLE would name the case and what only it
    reaches), and for everything the case reaches another case of its type and format is named."""
    sole, named = {}, 0
    for gone in REACH:
        rest = {key: v for key, v in REACH.items() if key != gone}
        lost = _missing(rest, gone[0], gone[1])
        if lost:
            sole[gone] = lost
            continue
        kernel, _, names = REACH[gone]
        for thing in names | {kernel}:
            other = next((key for key, (k, _, n) in rest.items() if key[:2] == gone[:2] and (thing == k or thing in n)), None)
            assert other is not None, (gone, thing)
            named += 1
    assert sole == SOLE, sole
    assert named > 10 * len(REACH)


def test_a_case_named_for_a_branch_reaches_it():
    claimed = 0
    for L in F.LETTERS:
        for cid, c in NEW[L].items():
            n = F.case_walk(c)
            assert c["claims"] and all(n[b] > 0 for b in c["claims"]), (L, cid, [b for b in c["claims"] if n[b] == 0])
            assert cid.startswith(c["fmt"] + "-pk-") and cid.endswith("-" + c["route"]), cid
            claimed += len(c["claims"])
    assert claimed >= 3 * 150


def test_the_inherited_part_is_every_gather_and_strips_case_as_it_stands():
    for L in F.LETTERS:
        theirs = {cid: c for cid, c in M.cases(L).items() if c["route"] in ("gather", "strips")}
        plain = lambda case: {key: v for key, v in case.items() if key != "make"}         # (the recipe is a closure; its matrix is compared)
        assert len(theirs) >= 100 and all(plain(TABLE[L][cid]) == plain(c) for cid, c in theirs.items())
        assert all(np.array_equal(M.matrix_of(TABLE[L][cid])["indices"], c["make"]()["indices"]) for cid, c in list(theirs.items())[::9])
        assert set(TABLE[L]) == set(theirs) | set(NEW[L]) and not set(theirs) & set(NEW[L])
        assert all(M.case_dispatch(c)["kernel"] == M.route_kernel(L, c["route"], c["fmt"] == "hell") for c in TABLE[L].values())
    assert "Z" not in F.LETTERS and all(c["route"] not in ("gather", "strips") for c in M.cases("Z").values())      # one row per lane: nothing to pack


def test_the_cases_that_cannot_freeze_are_the_all_empty_matrices():
    for L in F.LETTERS:
        assert F.refused(L) == REFUSED == ["ell-len0-gather", "ell-len0-strips", "hell-len0-gather", "hell-len0-strips"]
        for cid, c in TABLE[L].items():
            m = M.matrix_of(c)
            empty = int(F.lengths(m).sum()) == 0
            ok, why = F.case_can_freeze(c)
            assert ok == (not empty) and (cid in REFUSED) == empty, (L, cid)
            assert why == ("slots" if empty else None)
            assert (F.slot_count(m) == 0) == empty


def test_freeze_dispatch_and_lookup_restated_on_hand_worked_calls():
    a = dict(cM=0, rP=0)
    args = dict(slots=640, entries=1000, escapes=10)
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, a, **args) == (True, None)
    assert F.can_freeze("D", True, M.GATHER, 100, 32, 32, 32, a, **args)[0] and F.can_freeze("S", False, M.STRIPS, 100, 0, 128, 104, a, **args)[0]
    assert F.can_freeze("Z", True, M.AUTO, 100, 32, 32, 32, a, **args) == (False, "type")
    assert F.can_freeze("D", True, M.XTILE, 100, 32, 32, 32, a, **args) == (False, "form")
    assert F.can_freeze("D", True, M.SWEEP, 100, 32, 32, 32, a, **args) == (False, "form")
    assert F.can_freeze("D", True, M.SWEEP, 100, 3, 3, 3, a, **args) == (False, "layout:hack")        # (a narrow layout: SWEEP runs as AUTO, no copy either)
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, dict(cM=8, rP=0), **args) == (False, "layout:cM")
    assert F.can_freeze("S", True, M.AUTO, 100, 6, 6, 6, a, **args) == (False, "layout:hack")
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, a, row_order=True, **args) == (False, "row-order")
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, a, slots=0, entries=0, escapes=0) == (False, "slots")
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, a, slots=640, entries=1000, escapes=11) == (False, "share")
    assert F.can_freeze("D", True, M.AUTO, 100, 32, 32, 32, a, slots=640, entries=1000, escapes=1000, pct=100)[0]
    assert X.freeze_keeps(1000, 10) and not X.freeze_keeps(1000, 11)
    # the key: a call finds the record only with every field of KEY_FIELDS as it was frozen, and only in front of the Wide kernel
    frozen = F.lookup_key("D", True, 0x1000, 0x2000, 0x3000, 32, 32, 0, 500, 1)
    assert frozen == dict(rP=0x1000, rS=0x2000, hackOffsets=0x3000, idxStride=32, rows=500, hackSize=32, baseIndex=1, maxNnz=0, subs=-128)
    wide = M.route_kernel("D", "gather", True)
    assert F.record_used(wide, dict(frozen), frozen) and F.record_used(M.route_kernel("D", "strips", True), dict(frozen), frozen)
    for field, other in (("rP", 0x1010), ("rS", 0x2010), ("hackOffsets", 0x3010), ("idxStride", 64), ("rows", 499), ("hackSize", 64), ("baseIndex", 0),
                         ("maxNnz", 9), ("subs", -32)):
        assert not F.record_used(wide, dict(frozen, **{field: other}), frozen), field
    for route in ("tiled", "lean", "narrow", "narrow-tiled", "sweep"):
        assert not F.record_used(M.route_kernel("D", route, True), dict(frozen), frozen), route
    ell = F.lookup_key("S", False, 1, None, 99, 0, 104, 7, 100, 0)
    assert (ell["hackOffsets"], ell["hackSize"], ell["idxStride"], ell["maxNnz"], ell["rS"], ell["subs"]) == (None, 0, 104, 7, None, -32)


def test_pack_and_slots_on_matrices_worked_by_hand():
    """fp32 (groups of 32 rows), hacks of 4: 34 rows; row 0 names columns 5 and 65 539, row 1 a column below the base, row 33 column 70 000."""
    rc = [[5, 65539], [-1]] + [[7]] * 30 + [[], [70000]]
    m = M.build("S", "hell", rc, 70001, 1, hack=4)
    bases, words, entries, escapes, slots = F.pack(m, "S")
    assert bases.tolist() == [5, 70000] and (entries, escapes) == (34, 1)      # 65 539 is 0xFFFE above 5: the last offset a word holds
    assert m["hack_offsets"].tolist() == [0, 8] + [8 + 4 * i for i in range(1, 8)] + [40]
    assert slots == 36 + 4 and F.packed_bytes(slots) == 256                  # the last hack (rows 32, 33) is one slot deep
    assert words[:8].tolist() == [0, F.ESCAPE, 2, 2, 65534, F.UNWRITTEN, F.UNWRITTEN, F.UNWRITTEN]
    assert words[36:].tolist() == [F.UNWRITTEN, 0, F.UNWRITTEN, F.UNWRITTEN]
    n = F.freeze_walk(m, "S")
    assert n["group_spans_several_hacks"] and n["last_hack_partial"] and not n["last_hack_depth_0"] and not n["rows_lt_group"]
    # the last hack empty behind hacks that are not: the slots end with the hack in front of it
    rc[33] = []
    m = M.build("S", "hell", rc, 70001, 1, hack=4)
    assert F.slot_count(m) == 36 and F.freeze_walk(m, "S")["last_hack_depth_0"] == 1 and F.pack(m, "S")[0].tolist() == [5, 0]
    # ELL: the copy is indexed with the index pitch
    e = M.build("D", "ell", [[3], [4, 9], [5]], 10, 0, idx_pitch=4, val_pitch=8)
    bases, words, entries, escapes, slots = F.pack(e, "D")
    assert slots == 8 and words.tolist() == [0, 1, 2, F.UNWRITTEN, F.UNWRITTEN, 6, F.UNWRITTEN, F.UNWRITTEN] and bases.tolist() == [3]


def test_walk_on_calls_worked_by_hand():
    """fp64, the packed strip kernel: a band of 256 rows, 10 columns each; row 130 (t == 0 of strip 1 of wavefront 1) names a far column at k = 9."""
    rc = M.band(np.full(256, 10))
    rc[130][9] = 100000
    m = M.build("D", "hell", rc, 100001, 0)
    k = F.packed(M.route_kernel("D", "strips", True))
    n = F.walk(m, k, 1)
    # wavefront 0: two strip stages; wavefront 1: one, then the escape at t == 0 breaks the second: a gather stage
    assert (n["strip_stage_packed"], n["stage_gather"], n["stages"], n["strip_broken_by_escape"], n["strip_broken_by_escape_at_t_gt_0"]) == (3, 1, 4, 1, 0)
    assert (n["escape_far"], n["escape_in_first_stage"], n["escape_in_last_partial_stage"]) == (1, 0, 1) and len(n["rp_reads"]) == 1
    assert n["packed_word"] == 64 * 10 + 64 * 8 + 128 * 2 - 1              # strips: the first word of each; the gather stage: every word but one
    assert (n["tail_taken"], n["tail_not_taken"], n["workgroup_partial_last"], n["wide_store"]) == (0, 2, 2, 128)
    assert n["stage_past_lane_longest"] == 2 * 64 * 6 and n["pad_word_in_live_strip"] == 0
    rc[130][9] = 139
    rc[131][9] = 100000                                                  # the same at t == 1
    n = F.walk(M.build("D", "hell", rc, 100001, 0), k, 0)
    assert (n["strip_broken_by_escape"], n["strip_broken_by_escape_at_t_gt_0"], n["scalar_store_wide_io_off"], n["wide_store"]) == (1, 1, 128, 0)
    # the gather kernel consumes every word; a tail row reads rP from tailFrom on
    lens = np.full(131, 3)
    lens[2] = 13
    g = M.build("D", "hell", M.scattered(lens, 500, 1), 500, 0)
    n = F.walk(g, F.packed(M.route_kernel("D", "gather", True)), 1)
    assert n["tail_from"] == {0: 8, 1: 0} and n["tail_taken"] == 2 and n["packed_word"] == 127 * 3 + 8
    assert len(n["rp_reads"]) == 5 + 9 and n["pad_word_in_live_strip"] == 5 and n["scalar_store_last_strip_partial"] == 1
    assert n["group_partial_last"] == 1 and n["workgroup_partial_last"] == 2


@pytest.mark.parametrize("letter", F.LETTERS)
def test_the_walk_keeps_the_unpacked_kernels_stages_and_tail(letter):
    """PACKED changes where a column comes from, not the loop: stages and the switch to the tail are spmv_launch_shapes.walk's on every
    case, and without an escape so are the strip stages."""
    compared = 0
    for cid, c in TABLE[letter].items():
        if cid in REFUSED:
            continue
        theirs, mine = M.case_walk(c), F.case_walk(c)
        assert (mine["stages"], mine["tail_from"], mine["tail_taken"]) == (theirs["stages"], theirs["tail_from"], theirs["tail_switch"]), cid
        assert mine["wide_store"] == theirs["store_wide"] and mine["workgroup_partial_last"] == theirs["wave_exit"], cid
        if F.pack_of(c)[3] == 0:
            assert (mine["strip_stage_packed"], mine["stage_gather"]) == (theirs["stage_strips"], theirs["stage_gather"]), cid
            assert not mine["rp_reads"] or mine["tail_taken"], cid
            compared += 1
    assert compared >= 100


@pytest.mark.parametrize("letter", F.LETTERS)
def test_pack_agrees_with_the_documented_rule_on_every_matrix(letter):
    """entries and escapes are exact_ref.unordered_escapes' (include/spgpu/tuning.h as exact_ref states it); with every escape allowed the
    share rule keeps every copy, at the default 1 % it is exact_ref.freeze_keeps that decides."""
    kept = dropped = 0
    for cid, c in TABLE[letter].items():
        m = M.matrix_of(c)
        rows, cols, _ = F.all_entries(m)
        _, _, entries, escapes, slots = F.pack_of(c)
        assert (entries, escapes) == X.unordered_escapes(m["rows"], rows, cols, letter), cid
        if slots > 0:
            assert F.case_can_freeze(c, pct=100)[0], cid
            ok, why = F.case_can_freeze(c, pct=1)
            assert ok == X.freeze_keeps(entries, escapes) and why == (None if ok else "share"), cid
            kept, dropped = kept + ok, dropped + (not ok)
    assert kept > 100 and dropped >= 2                    # (the GPU module runs with every escape allowed; the rule itself: test_gpu_packed_edges.py)


@pytest.mark.parametrize("letter", F.LETTERS)
def test_pack_slot_by_slot_on_the_packed_only_matrices(letter):
    """Every slot of the copy, asked who owns it: row and k from the slot's number, the group's base by a scan of the group's rows."""
    g_rows = M.group_rows(letter)
    for cid, c in NEW[letter].items():
        m = M.matrix_of(c)
        bases, words, entries, escapes, slots = F.pack_of(c)
        lens, idx, base, rows = F.lengths(m), m["indices"], m["base"], m["rows"]
        assert slots == (int(m["hack_offsets"][-1]) if c["fmt"] == "hell" else m["pitch"] * m["max_row"]) > 0, cid
        assert words.size == slots and idx.size >= slots
        lowest = {}
        for r in range(rows):
            for k in range(int(lens[r])):
                col = M._entry(m, r, k)[0]
                if col >= 0:
                    lowest[r // g_rows] = min(lowest.get(r // g_rows, col), col)
        assert bases.tolist() == [lowest.get(g, 0) for g in range((rows + g_rows - 1) // g_rows)], cid
        seen = far = 0
        for s in range(slots):
            if c["fmt"] == "hell":
                hack = m["hack_size"]
                h = int(np.searchsorted(m["hack_offsets"], s, side="right")) - 1
                r, k = h * hack + (s - int(m["hack_offsets"][h])) % hack, (s - int(m["hack_offsets"][h])) // hack
            else:
                r, k = s % m["pitch"], s // m["pitch"]
            if r >= rows or k >= lens[r]:
                assert words[s] == F.UNWRITTEN, (cid, s)
                continue
            col = int(idx[s]) - base
            off = col - lowest.get(r // g_rows, 0)
            want = off if col >= 0 and off < 0xFFFF else F.ESCAPE
            assert words[s] == want, (cid, s, r, k)
            seen += 1
            far += want == F.ESCAPE
        assert (seen, far) == (entries, escapes), cid


def test_the_matrices_stay_small():
    for L in F.LETTERS:
        G = M.group_rows(L)
        for cid, c in NEW[L].items():
            m = M.matrix_of(c)
            assert m["rows"] <= 3 * 4 * G + 4 * G - 1 and m["cols"] <= 6 * F.FAR + 8000 and m["values"].size <= 40000, (L, cid)
            r, cc, v = m["coo"]
            stored = m["values"][:F.slot_count(m) if c["fmt"] == "hell" else m["max_row"] * m["val_pitch"]]
            assert np.count_nonzero(~np.isnan(stored)) == v.size, cid          # every slot no product uses holds NaN
            assert ((m["indices"] - m["base"]) < m["cols"]).all(), cid
    for L in F.LETTERS:
        for fmt in ("hell", "ell"):
            for route in ("gather", "strips"):
                for both in (False, True):
                    m = F.copy_is_read_matrix(L, fmt, route, both)
                    k = F.packed(M.route_kernel(L, route, fmt == "hell"))
                    n = F.walk(m, k, 1)
                    assert m["rows"] % M.group_rows(L) == 0
                    if not both:
                        assert not n["rp_reads"] and n["tail_taken"] == 0 and n["escape_far"] + n["escape_negative"] == 0
                        assert n["strip_stage_packed" if route == "strips" else "stage_gather"] == n["stages"] > 0
                    else:
                        assert n["tail_taken"] == 1 and n["escape_far"] == 1 and len(n["rp_reads"]) == 1 + 40
                        assert (n["strip_stage_packed"] > 0) == (route == "strips")
