"""CPU: the case table of tests/test_gpu_spmv_shapes.py (tests/spmv_launch_shapes.py) is what that module needs it to be -- the
constants equal the sources' (spmv_rules.h, asked through tests/spmv_dispatch_cases.cpp), the table names every instantiation the rIdx == NULL dispatch can select for every type and both
formats, each with a case of more than one workgroup, autoVote and launchFormProbe restated give AUTO's sequence, every case takes the route its name claims and the branches it is in the table for (the kernels' control flow walked on
the CPU), every named branch is reached per type, and on every matrix the oracle, reading the NaN-poisoned arrays in the order of
the case's kernel, returns no NaN and keeps exact_ref's bound of the extended-precision sums: the host half of the GPU module's
assertions, without a GPU.

Deleting a case that is alone on its branch makes test_every_named_branch_is_reached_per_type fail; checked by hand for
  hell- and ell-tail+unroll+1-{gather,xtile,sweep} (tail_len_unroll_plus_1), hell- and ell-strips-below-base
  (strips_refused_below_base) and hell- and ell-tile-centred (tile_centred): with the pair out of the table the branch is reached
  by no case of the type.  SOLO below names them, and the test repeats the deletion on every run."""
import numpy as np
import pytest

import exact_ref as X
import oracle_api as O
import spmv_launch_shapes as M

TABLE = {L: M.cases(L) for L in M.LETTERS}

#: branches only the cases named reach (per type; both formats of the case): the table loses the branch with them
SOLO = {"tail_len_unroll_plus_1": ("tail+unroll+1", "SDC"), "strips_refused_below_base": ("strips-below-base", "SDC"),
        "tile_centred": ("tile-centred", "SDCZ")}
#: what a type's kernels cannot reach: Z has the narrow kernels only (one row per lane, two phases, no whole-wave tail); the fp32
#: kernels consider the tail at every stage
NEVER = {
    "Z": {b for b in M.BRANCHES if b.startswith(("tail_", "strip", "stage_strips")) or b in
          ("tile_count_odd", "store_wide", "store_scalar_no_wideio", "store_scalar_partial_strip")}
         | {"sweep_pack_partial", "sweep_store_scalar"},      # (a pack is one row, and a 16-byte element is never off its boundary)
    "S": {"tail_every_deferred"}, "D": set(), "C": set(),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return M.dispatch_program(tmp_path_factory.mktemp("spmv_dispatch"))


def test_constants_equal_the_sources(program):
    """The sources' side is spmv_rules.h itself, asked through tests/spmv_dispatch_cases.cpp (ellpack_spmv.hip asserts kRulesWave == kWave)."""
    src = M.header_constants(program)
    assert src["kRulesWave"] == M.WAVE and src["kBlockThreads"] == M.BLOCK
    assert src["kTailLanes"] == M.TAIL_LANES and src["kTailUnroll"] == M.TAIL_UNROLL
    assert src["kTileBytes"] == M.TILE_BYTES and src["kTiledBlockFp32"] == M.TILED_BLOCK_S
    assert src["kTailEvery"] == M.TAIL_EVERY
    assert src["kLeanMaxHint"] == M.LEAN_MAX_HINT and src["kLeanMaxEll"] == M.LEAN_MAX_ELL
    assert src["kSweepLaneRows"] == M.SWEEP_LANE_ROWS and src["kSweepPacks16"] == M.SWEEP_PACKS_16
    assert src["kSweepMaxBlocks"] == M.SWEEP_MAX_BLOCKS and src["kAutoSweepRows"] == M.AUTO_SWEEP_ROWS
    assert (src["kTileBytes"], src["kTileSpanNum"], src["kTileSpanDen"]) == (M.TILE_BYTES, 5, 4)
    assert [src[f"tileSpanLimit{s}"] for s in (4, 8, 16)] == [M.TILE_BYTES // s * 5 // 4 for s in (4, 8, 16)]
    assert [src[k] for k in ("kFormAuto", "kFormGather", "kFormStrips", "kFormXtile", "kFormSweep")] == [M.AUTO, M.GATHER, M.STRIPS, M.XTILE, M.SWEEP]
    assert all(src[f"wideGroupRows{M.SIZEOF[L]}"] == M.group_rows(L) for L in "SDC")
    # the oracle's own statement of the default kernels' shapes
    for L in "SDC":
        ph, unroll = (8, 2) if L == "S" else (1, 8)
        assert M.oracle_shape(M.slab(L, M.WIDE[L], ph, True, unroll, True, True)) == O.TAIL_SHAPE[L]
        assert M.group_rows(L) == O.TAIL_SHAPE[L]["group_rows"] and M.wide_step(L) == O.TAIL_SHAPE[L]["step"]


def test_dispatch_restated_on_a_few_hand_worked_calls():
    a = dict(cM=0, rP=0, z=0, y=0)
    d = M.dispatch("D", True, M.GATHER, 1000, 32, 32, 32, 0, 0, a, True)
    assert M.kernel_name(d["kernel"]) == "slabSpmvKernel<double, 2, 1, true, true, 8, true, true, false, 256, 0, 0, false>"
    assert d["grid"] == (2, 256) and d["wide_io"] == 1 and d["noted"] == M.GATHER
    d = M.dispatch("S", False, M.XTILE, 1000, 0, 1024, 1024, 20, 0, dict(a, z=4), False)
    assert M.kernel_name(d["kernel"]) == "slabSpmvKernel<float, 4, 8, false, true, 2, true, true, false, 512, 32768, 0, false>"
    assert d["grid"] == (4, 512) and d["wide_io"] == 0 and d["noted"] == M.XTILE
    assert M.dispatch("D", True, M.STRIPS, 10, 32, 32, 32, 0, 0, dict(a, rP=8), True)["kernel"][9] is True        # 8 mod 16 stays wide
    d = M.dispatch("D", True, M.STRIPS, 10, 32, 32, 32, 0, 0, dict(a, rP=4), True)
    assert (d["kernel"][2:4], d["fails"], d["noted"], d["wide_io"]) == ((1, 2), "rP", M.GATHER, 1)
    assert M.dispatch("S", True, M.GATHER, 10, 32, 32, 32, 0, 0, dict(a, rP=8), True)["fails"] == "rP"
    assert M.dispatch("D", False, M.GATHER, 11, 0, 11, 12, 3, 0, a, True)["fails"] == "short-stride"
    assert M.dispatch("D", False, M.GATHER, 11, 0, 13, 12, 3, 0, a, True)["fails"] == "stride-multiple"
    assert M.dispatch("D", False, M.GATHER, 11, 0, 14, 12, 3, 0, a, True)["fails"] is None
    d = M.dispatch("C", False, M.AUTO, 500, 0, 512, 512, 16, 8, a, True)
    assert M.kernel_name(d["kernel"]) == "slabSpmvKernel<spgpu::Cx<float>, 2, 1, false, true, 4, false, true, false, 256, 0, 8, false>"
    assert M.dispatch("C", False, M.AUTO, 500, 0, 512, 512, 17, 8, a, True)["kernel"][7] is True                   # maxNnz 17: prefetching
    assert M.dispatch("C", True, M.AUTO, 500, 32, 32, 32, 0, 9, a, True)["noted"] == M.STRIPS
    assert M.dispatch("S", True, M.AUTO, 500, 32, 32, 32, 0, 4, a, True)["kernel"][7] is True                      # fp32 has no lean kernel
    d = M.dispatch("Z", True, M.SWEEP, 5000, 32, 32, 32, 0, 0, a, False)
    assert M.kernel_name(d["kernel"]) == "sweepSpmvKernel<spgpu::Cx<double>, 1, 16, true, false, false>" and d["grid"] == (2, 256)
    d = M.dispatch("D", True, M.SWEEP, 5000, 32, 32, 32, 0, 0, dict(a, cM=8), False)
    assert d["kernel"][:4] == ("slab", "D", 1, 2) and d["noted"] == M.GATHER
    assert M.dispatch("D", True, M.XTILE, 5000, 3, 3, 3, 0, 0, a, False)["kernel"][2:4] == (1, 2)
    assert M.dispatch("Z", True, M.XTILE, 5000, 3, 3, 3, 0, 0, a, False)["kernel"][2:4] == (1, 2)
    assert M.dispatch("D", True, M.GATHER, 0, 32, 32, 32, 0, 0, a, False) is None


def test_vote_and_probe_restated_on_the_auto_sequence():
    """autoVote (voteForm) and launchFormProbe: a new record votes strips and launches no probe; two samples of three decide; a form that does
    not report itself gets the three-wavefront probe with its first call and every fourth."""
    assert M.vote_form("D", 708, [0, 0, 0], 0) == M.FIRST_CALL
    assert M.vote_form("D", 708, [2, 2, 3], 1) == dict(strips=True, tile=False, sweep=False, probe=False)
    assert M.vote_form("D", 708, [3, 3, 3], 1) == dict(strips=False, tile=True, sweep=False, probe=True)
    assert M.vote_form("S", 708, [1, 1, 3], 1) == dict(strips=False, tile=False, sweep=False, probe=True)
    assert [M.vote_form("D", 708, [1, 1, 1], c)["probe"] for c in range(1, 9)] == [True, False, False, True, False, False, False, True]
    assert M.vote_form("D", 708, [4, 4, 1], 2)["sweep"] is False and M.vote_form("D", M.AUTO_SWEEP_ROWS, [4, 4, 1], 2)["sweep"] is True
    assert M.vote_form("S", M.AUTO_SWEEP_ROWS, [4, 4, 1], 2)["sweep"] is False
    a = dict(cM=0, rP=0, z=0, y=0)
    names = {L: M.kernel_name(M.form_probe(L, True, True)) for L in "SDCZ"}
    assert names == {"S": "formProbeKernel<float, 4, 8, true, 16>", "D": "formProbeKernel<double, 2, 1, true, 8>",
                     "C": "formProbeKernel<spgpu::Cx<float>, 2, 1, true, 8>", "Z": "formProbeKernel<spgpu::Cx<double>, 1, 2, true, 8>"}
    assert M.kernel_name(M.form_probe("D", False, False)) == "formProbeKernel<double, 1, 2, false, 8>"
    assert M.every_probe("Z", True) == set() and len(M.every_probe("S", False)) == 1
    # the sequence the AUTO tests of the GPU module run: call 0 on a new record, calls 1 and 2 on what the samples said
    for letter in "SDC":
        for said, forms, probes in (([2, 2, 2], [M.STRIPS] * 3, [False] * 3), ([3, 3, 3], [M.STRIPS, M.XTILE, M.XTILE], [False, True, False]),
                                    ([1, 1, 1], [M.STRIPS, M.GATHER, M.GATHER], [False, True, False])):
            got = [M.dispatch(letter, True, M.AUTO, 708, 32, 32, 32, 0, 0, a, True, M.vote_form(letter, 708, said if call else [0, 0, 0], call))
                   for call in range(3)]
            assert [d["noted"] for d in got] == forms and [d["probe"] is not None for d in got] == probes
            assert all(d["probe"] in (None, M.form_probe(letter, True, True)) for d in got)
    # a fixed form, a narrow layout and complex fp64 never vote: no probe
    assert M.dispatch("D", True, M.GATHER, 708, 32, 32, 32, 0, 0, a, True)["probe"] is None
    assert M.dispatch("Z", True, M.AUTO, 708, 32, 32, 32, 0, 0, a, True, dict(probe=True))["probe"] is None


def test_builders_poison_every_slot_no_product_uses():
    m = M.build("D", "hell", [[0, 2], [], [1], [-1, 3, 4], [2]], 6, 1, hack=4)
    assert m["hack_offsets"].tolist() == [0, 12, 16] and m["row_lengths"].tolist() == [2, 0, 1, 3, 1]
    v, i = m["values"].reshape(4, 4), m["indices"].reshape(4, 4)
    assert np.isnan(v).tolist() == [[False, True, False, True], [False, True, True, False], [True, True, True, False], [False, True, True, True]]
    assert i[0].tolist()[0::2] == [1, 2] and i[0, 3] == 0 and i[1, 3] == 4 and i[2, 3] == 5 and i[3, 0] == 3
    assert (i >= 1).sum() == 15 and (i <= 6).all()                          # every padding slot names a valid column
    assert m["coo"][0].tolist() == [0, 0, 2, 3, 3, 4] and m["coo"][1].tolist() == [0, 2, 1, 3, 4, 2]
    e = M.build("C", "ell", [[1], [0, 2], [2]], 3, 0, idx_pitch=4, val_pitch=6)
    assert e["max_row"] == 2 and e["values"].size == 12 and e["indices"].size == 8
    assert np.isnan(e["values"]).tolist() == [False, False, False, True, True, True, True, False, True, True, True, True]
    assert M.oracle_view(e)["values"].size == 8 and M.oracle_view(e)["values"][5] == e["values"][7]


def test_walk_on_calls_worked_by_hand():
    """fp64, wide gather kernel (two rows per lane, 8 columns per stage): 131 rows; rows 2 and 3 (one strip) hold 13 and 10 entries,
    every other row 3."""
    lens = np.full(131, 3)
    lens[2], lens[3] = 13, 10
    m = M.build("D", "hell", M.scattered(lens, 500, 1), 500, 0)
    n = M.walk(m, M.slab("D", 2, 1, True, 8, True, True), 1)
    # wavefront 0: stage at 0, at 8 one lane busy: switch; wavefront 1: rows 128 .. 130, two strips: switch at 0; two wavefronts leave
    assert (n["wave_exit"], n["dead_strips"], n["stages"], n["tail_switch"], n["tail_switch_at_zero"]) == (2, 62, 1, 2, 1)
    assert n["tail_from"] == {0: 8, 1: 0} and n["tail_two_rows_in_strip"] == 2 and n["tail_len_1"] == 0    # rows 2, 3 and rows 128, 129
    assert (n["store_wide"], n["store_scalar_partial_strip"], n["store_scalar_no_wideio"]) == (65, 1, 0)
    assert M.walk(m, M.slab("D", 2, 1, True, 8, True, True), 0)["store_scalar_no_wideio"] == 66
    # the tiled kernel: 4 columns per stage, the switch considered at multiples of 8 only
    n = M.walk(m, M.tiled_kernel("D", 2, True), 1)
    assert n["tail_from"] == {0: 8, 1: 0} and n["tail_every_deferred"] == 1 and n["stages"] == 2 and n["tile_fits"] == 1
    # narrow: 32 rows per wavefront, two phases x 4 columns, no tail: rows 2 and 3 keep wavefront 0 going for 13 columns
    n = M.walk(m, M.slab("D", 1, 2, True, 4, True, False), 1)
    assert (n["stages"], n["tail_switch"], n["store_narrow"], n["three_stages"]) == (2 + 4, 0, 131, 0)
    # strips: a band of 10 columns runs one strip stage, then rows of 10 are past their end: the second stage is strips as well
    b = M.build("D", "hell", M.band(np.full(256, 10)), 300, 0)
    n = M.walk(b, M.slab("D", 2, 1, True, 8, True, True, True), 1)
    assert (n["stage_strips"], n["stage_gather"], n["strip_absent_load"], n["strip_x_unaligned"]) == (4, 0, 2 * 64 * 6, 2 * 64 * 5)
    # (row 2s, slab column k names column 2s + k: the odd k are 8 bytes past a boundary; with x itself 8 bytes past one, the even k)
    assert M.walk(b, M.slab("D", 2, 1, True, 8, True, True, True), 1, x_off_bytes=8)["strip_x_unaligned"] == 2 * 64 * 5
    # the sweep: 131 rows are 65 whole packs and a partial one
    n = M.walk(m, M.sweep("D", 2, True, True), 1)
    assert (n["sweep_pack_whole"], n["sweep_pack_partial"], n["sweep_store_wide"], n["sweep_store_scalar"], n["sweep_tail_rows"]) == (65, 1, 65, 1, 2)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_case_takes_the_route_and_the_branches_it_claims(letter):
    for cid, c in TABLE[letter].items():
        d = M.case_dispatch(c)
        hell = c["fmt"] == "hell"
        assert d["kernel"] == M.route_kernel(letter, c["route"], hell, c["scalars"][1] != 0), (cid, M.kernel_name(d["kernel"]))
        if c["fails"]:
            assert d["fails"] == c["fails"], cid
        if c["route"] in ("gather", "strips", "tiled", "lean", "auto-first") or (c["route"] == "sweep" and M.WIDE[letter] > 1):
            assert d["wide_ok"], cid
        if c["form"] != M.AUTO:
            want = {"gather": M.GATHER, "strips": M.STRIPS, "tiled": M.XTILE, "narrow-tiled": M.XTILE, "narrow": M.GATHER, "sweep": M.SWEEP}
            assert d["noted"] == want[c["route"]], cid
        n = M.case_walk(c)
        for claim in c["claims"]:
            assert n[claim] > 0, (cid, claim)
        # the name says the format and the form
        assert cid.startswith(c["fmt"] + "-"), cid
        m = M.matrix_of(c)
        assert m["fmt"] == c["fmt"] and (c["y_mode"] != "nan" or c["scalars"][1] == 0), cid


@pytest.mark.parametrize("letter", M.LETTERS)
def test_table_names_every_instantiation_for_both_formats_and_both_stores(letter):
    for hell in (True, False):
        seen = {}
        for c in TABLE[letter].values():
            if (c["fmt"] == "hell") == hell:
                d = M.case_dispatch(c)
                seen.setdefault(d["kernel"], set()).add(d["wide_io"])
        assert set(seen) == M.every_instantiation(letter, hell), [M.kernel_name(k) for k in M.every_instantiation(letter, hell) ^ set(seen)]
        # ... each with a case of more than one workgroup (blockIdx.x > 0, a tile placement of its own, a partly filled last one)
        grids = {}
        for c in TABLE[letter].values():
            if (c["fmt"] == "hell") == hell:
                d = M.case_dispatch(c)
                grids[d["kernel"]] = max(grids.get(d["kernel"], 0), d["grid"][0])
        assert all(g > 1 for g in grids.values()), [M.kernel_name(k) for k, g in grids.items() if g < 2]
        for k, io in seen.items():
            if (k[0] == "slab" and k[2] > 1) or (k[0] == "sweep" and k[2] > 1):
                assert io == {0, 1} or (k[0] == "slab" and not k[7]), (M.kernel_name(k), io)     # (the lean kernel: one store form suffices)
    assert len(M.every_instantiation(letter, True)) == {"S": 7, "D": 8, "C": 8, "Z": 4}[letter]


@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_named_branch_is_reached_per_type(letter):
    taken, by_case = set(), {}
    for cid, c in TABLE[letter].items():
        n = M.case_walk(c)
        got = {b for b in M.BRANCHES + M.SWEEP_BRANCHES if n.get(b, 0) > 0}
        by_case[cid] = got
        taken |= got
    want = set(M.BRANCHES + M.SWEEP_BRANCHES) - NEVER[letter]
    if letter in "SZ":
        want -= {"sweep_tail_rows"}             # their sweep adds in one phase: no tail rows
    assert taken >= want, sorted(want - taken)
    assert not (taken & NEVER[letter]), sorted(taken & NEVER[letter])
    for branch, (name, letters) in SOLO.items():
        if letter in letters:
            rest = set().union(*(got for cid, got in by_case.items() if name not in cid))
            assert branch not in rest, (branch, name)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_oracle_on_the_poisoned_arrays_is_finite_and_within_the_bound_of_the_exact_sums(letter):
    for cid, c in TABLE[letter].items():
        m = M.matrix_of(c)
        stored = m["values"][:m["hack_offsets"][-1]] if c["fmt"] == "hell" else m["values"][:m["max_row"] * m["val_pitch"]]
        r, cc, v = m["coo"]
        assert np.count_nonzero(~np.isnan(stored)) == v.size and (v != 0).all(), cid
        x, y = M.operands(letter, m)
        alpha, beta = M.scalars_of(c)
        d = M.case_dispatch(c)
        got = O.spmv_tail(M.oracle_view(m), x, y if beta != 0 else None, alpha, beta, with_row_sizes=not m["rs_null"],
                          **M.oracle_shape(d["kernel"]))
        assert not np.isnan(got).any(), cid
        want, scale = X.spmv(m["rows"], r, cc, v, x, y if beta != 0 else None, alpha, beta)
        X.assert_within(got, want, scale, letter, cid)
        # where the oracle of the reference's own orders applies (no column below the base, one pitch), it says the same
        shape = M.oracle_shape(d["kernel"])
        if shape["tail_lanes"] == 0 and not any("below-base" in s for s in (cid,)) and (c["fmt"] == "hell" or m["val_pitch"] == m["pitch"]):
            fn = O.hell_spmv if c["fmt"] == "hell" else O.ell_spmv
            kw = {} if c["fmt"] == "hell" else dict(with_row_sizes=not m["rs_null"])
            assert fn(m, x, y if beta != 0 else None, alpha, beta, phases=shape["phases"], **kw).tobytes() == got.tobytes(), cid


@pytest.mark.parametrize("letter", M.LETTERS)
def test_auto_patterns_are_what_the_sample_wavefronts_must_see(letter):
    """band: every stage of a whole wavefront is strips; window: no strip, the columns of a wavefront's rows inside the span limit;
    scattered: beyond it."""
    limit = M.TILE_BYTES // M.SIZEOF[letter] * 5 // 4
    for name, (m, form) in M.auto_patterns(letter).items():
        w = M.WIDE[letter]
        if w == 1:
            assert form == M.GATHER
            continue
        ph, unroll = (8, 2) if letter == "S" else (1, 8)
        n = M.walk(m, M.slab(letter, w, ph, True, unroll, True, True, True), 1)
        assert int(m["row_lengths"].max()) > 2 * ph * unroll
        g = M.group_rows(letter)
        cols = m["indices"][:m["hack_offsets"][-1]].reshape(-1, 32)
        first = m["coo"][1][np.searchsorted(m["coo"][0], np.arange(g, 2 * g))]
        last = m["coo"][1][np.searchsorted(m["coo"][0], np.arange(g, 2 * g), side="right") - 1]
        span = int(max(first.max(), last.max()) - min(first.min(), last.min()) + 1)
        if name == "band":
            assert form == M.STRIPS and n["stage_gather"] <= 3 and n["stage_strips"] > 10
        elif name == "window":
            assert form == M.XTILE and n["stage_strips"] == 0 and span <= limit
        else:
            assert form == M.GATHER and n["stage_strips"] == 0 and span > limit
        assert cols.size
