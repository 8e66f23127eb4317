"""CPU: the case table of tests/ordered_launch_shapes.py (run on the GPU by tests/test_gpu_zz_ordered_shapes.py) reaches every
raggedSpmvKernel instantiation the library has and every branch of the ordered path's kernels that the table names; its restated dispatch
is spgpu_amd/csrc/ordered_rules.h's (through tests/ordered_dispatch_cases.cpp); and the oracle in the queue kernel's order of additions
is within exact_ref's bound of the extended-precision product on every matrix, the ones whose 32-row sub-groups straddle hacks included."""
import itertools
import subprocess

import numpy as np
import pytest

import exact_ref as X
import ordered_launch_shapes as L
import spmv_launch_shapes as M

TABLE = {letter: L.cases(letter) for letter in L.LETTERS}
SIZE = {"S": 4, "D": 8, "C": 8, "Z": 16}
CT = {"S": "f", "D": "d", "C": "NS_2CxIfEE", "Z": "NS_2CxIdEE"}

# raggedSpmvKernel<T, RPL, IS_HELL, UNROLL, WAVES, TILE_BYTES, SUBS, DEEP, ZBYTES, PLAN, PACKED>: the 56 the library instantiates, written out
# (launchQueue over launchRagged's and launchWithPlan's constants; complex fp64 has no staged shape and no packed kernels, gather no packed)
G, T, S = (4, 0, 16, 0), (8, 65536, 32, 0), (8, 49152, 64, 17408)
EVERY = {
    (letter, rpl, hell, unroll, q[0], q[1], q[2], True, q[3], plan, packed)
    for letter, rpl, unroll, shapes in (("S", 4, 2, ((G, 0), (T, 1), (S, 1))), ("D", 2, 3, ((G, 0), (T, 1), (S, 1))),
                                        ("C", 2, 3, ((G, 0), (T, 1), (S, 1))), ("Z", 1, 3, ((G, 0), (T, 0))))
    for hell in (False, True) for q, packs in shapes for plan, packed in ((False, False), (True, False)) + (((True, True),) if packs else ())
}


def _reach():
    """(letter, case id, mode) -> (kernel, branch names), the stale pairs under mode "stale"."""
    out = {}
    for letter in L.LETTERS:
        for cid, case in TABLE[letter].items():
            m = L.matrix_of(case)
            names = L.case_walk(case)
            for mode in case["modes"]:
                out[(letter, cid, mode)] = (L.case_route(case, mode, m)["kernel"], names[mode])
        for cid in L.stale_pairs(letter):
            case, a, b = L.stale_case(letter, cid)
            ma, mb = L.matrix_of(case, a, "A"), L.matrix_of(case, b, "B")
            route = L.case_route(case, "plan", mb, plan_of=ma)
            out[(letter, cid, "stale")] = (route["kernel"], L.walk(mb, route, case["tune"], plan_of=ma))
    return out


REACH = _reach()


def test_the_56_instantiations_written_out_are_the_restated_ones():
    assert len(EVERY) == 56
    assert EVERY == L.every_instantiation()
    for letter, size in SIZE.items():
        assert L.queue_shape(letter, False, 0) == L.queue_shape(letter, False, 4) == G
        assert L.queue_shape(letter, True, 0) == L.queue_shape(letter, True, 1) == T
        assert L.queue_shape(letter, True, 4) == (S if size <= 8 else T)


def test_every_instantiation_is_reached():
    got = {kernel for kernel, _ in REACH.values()}
    assert got == EVERY, sorted(EVERY - got)


def test_every_branch_is_reached():
    got = set().union(*(names for _, names in REACH.values()))
    assert got == set(L.BRANCHES), sorted(set(L.BRANCHES) - got)


# the cases that alone reach something, and what: taking one of them out of the table makes a coverage assertion fail.  (None: every
# instantiation and branch has two cases and more.)
SOLE = {}


def _coverage_failures(reach):
    """What test_every_instantiation_is_reached and test_every_branch_is_reached would miss on this table."""
    return (EVERY - {kernel for kernel, _ in reach.values()}) | (set(L.BRANCHES) - set().union(*(names for _, names in reach.values())))


def test_removing_a_case_fails_the_coverage_or_another_case_is_named():
    """The two coverage assertions evaluated again on the table without each case in turn (all its modes): they fail -- then the case and
    what only it reaches are written out in SOLE -- or for everything the case reaches another case is named."""
    assert not _coverage_failures(REACH)
    cases = sorted({key[:2] for key in REACH})
    sole, named = {}, 0
    for gone in cases:
        rest = {key: v for key, v in REACH.items() if key[:2] != gone}
        lost = _coverage_failures(rest)
        if lost:
            sole[gone] = lost
            continue
        for mode_key in (key for key in REACH if key[:2] == gone):
            kernel, names = REACH[mode_key]
            for thing in names | {kernel}:
                other = next((key for key, (k, n) in rest.items() if thing == k or thing in n), None)
                assert other is not None and other[:2] != gone, (gone, thing)
                named += 1
    assert sole == SOLE, sole
    assert named > len(cases)


def test_a_case_named_for_a_branch_reaches_it():
    for letter in L.LETTERS:
        for cid, case in TABLE[letter].items():
            got = set().union(*(REACH[(letter, cid, mode)][1] for mode in case["modes"]))
            assert set(case["expects"]) <= got, (letter, cid, sorted(set(case["expects"]) - got))
    assert sum(bool(c["expects"]) for t in TABLE.values() for c in t.values()) >= 40


def test_items_are_counted_as_the_kernel_counts_them():
    """raggedSpmvKernel: every lane below SUBS has a sub-group -- one past the last row is depth 0, nobody else's, one item -- so a block has
    fewer items than wavefronts only when all but a few of its SUBS sub-groups are the plan's (or worked off behind)."""
    took = {key for key, (_, names) in REACH.items() if "items_fewer_than_waves" in names}
    assert took and all(mode in ("plan", "stale") for _, _, mode in took), sorted(took)
    assert {cid for _, cid, _ in took} == {"mostly-deep-gather"}
    case = TABLE["D"]["tiny-gather"]                                   # 20 rows: 1 real sub-group and 15 of depth 0 -- 16 items
    assert "items_fewer_than_waves" not in set().union(*L.case_walk(case).values())


def test_the_matrices_stay_small():
    for letter in L.LETTERS:
        for cid, case in TABLE[letter].items():
            m = L.matrix_of(case)
            assert m["values"].size <= 320000, (letter, cid, m["values"].size)
            assert m["rows"] <= 3 * case["block_rows"] + case["block_rows"] - 1
            assert all(d <= 1100 for d in case["depths"]), (letter, cid)
            assert np.isnan(m["values"]).sum() >= m["values"].size - m["coo"][2].size      # every slot no product uses holds NaN
            assert ((m["indices"] - m["base"] < m["cols"])).all()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return M.rules_program(tmp_path_factory.mktemp("ordered_shapes"), "ordered_dispatch_cases")


def _ask(program, rule, questions):
    questions = list(questions)
    done = subprocess.run([program], input="".join(f"{rule} " + " ".join(str(int(v)) for v in q) + "\n" for q in questions), capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, done.stderr[-2000:]
    return [[int(v) for v in line.split()] for line in done.stdout.splitlines()]


def test_the_restated_dispatch_is_the_headers(program):
    for letter, size in SIZE.items():
        shapes = list(itertools.product((0, 1), (0, 4, 1)))
        got = _ask(program, "shape", [(size, tiled, knob) for tiled, knob in shapes])
        for (tiled, knob), g in zip(shapes, got):
            assert tuple(g[:4]) == L.queue_shape(letter, tiled, knob) and g[5] == L.staged_shape(letter, tiled, knob)
        tunes = [L.TUNE, L.TUNE_NO_SPLIT] + ([L.tune_most(letter)] if letter != "Z" else [])
        got = _ask(program, "split", [(size, t["cap"], t["split"]) for t in tunes])
        for t, g in zip(tunes, got):
            assert g == [L.ragged_split(letter, t["cap"], t["split"]), L.queue_step(letter), L.most_chunks(letter), L.unroll(letter)]
    asked = list(itertools.product((0, 4, 1), (0, 1), (0, 1), (4, 8, 16), (0, 4), (0, 1)))
    got = _ask(program, "decide", asked)
    letter_of = {4: "S", 8: "D", 16: "Z"}
    packs = {}
    for (knob, tiled, order, size, probed, no_list), g in zip(asked, got):
        for mode in L.MODES:
            d = L.dispatch(letter_of[size], True, M.AUTO if tiled else M.GATHER, knob, bool(order), 0, 4000, L.TUNE, mode, probed=probed,
                           no_deep_list=bool(no_list), deep=9)
            assert (d["probes"], d["knob_shape"], d["plannable"]) == (bool(g[0]), g[1], bool(g[2])), (knob, tiled, order, size, probed, no_list)
            assert d["queue"] == L.queue_shape(letter_of[size], tiled, g[1])
            assert d["plan"] == (mode != "list" and bool(g[2]) and bool(order))          # launchPlanned: a plan only with a row order
            want = d["queue"][2] | (L.ORDERED_PLAN if d["plan"] else L.ORDERED_DEEP) | (L.ORDERED_PACKED if d["packed"] else 0)
            assert d["word"] == want and d["deep_follow"] == (not d["plan"])            # (HELL: the deep kernels follow every call without a plan)
            assert (d["grid"], d["stride"]) == ((L.plan_grid(L.queue_grid(4000, d["queue"][2]), 9)[1:]) if d["plan"] else (L.queue_grid(4000, d["queue"][2]), 0))
            packs[(tiled, size, d["queue"][2], d["plan"] and mode == "packed")] = d["packed"]
    keys = sorted(k for k in packs if k[3])
    for (tiled, size, subs, _), g in zip(keys, _ask(program, "pack", [k[:3] for k in keys])):
        assert packs[(tiled, size, subs, True)] == bool(g[0]) == bool(g[1])             # mayPack, and the kernels that read the copy
    # every grid and stride the table's plans have
    plans = set()
    for (letter, cid, mode), (kernel, _) in REACH.items():
        if kernel[9]:
            case = TABLE[letter].get(cid) or L.stale_case(letter, cid)[0]
            if mode == "stale":
                _, a, b = L.stale_case(letter, cid)
                m, of = L.matrix_of(case, b, "B"), L.matrix_of(case, a, "A")
            else:
                m = of = L.matrix_of(case)
            deep = sum(d > case["tune"]["cap"] for d in L.sub_depths(of)[0])
            plans.add((L.queue_grid(m["rows"], kernel[6]), deep))
    plans = sorted(plans)
    assert _ask(program, "plan", plans) == [list(L.plan_grid(*p)) for p in plans]
    rows = sorted({(L.matrix_of(c)["rows"], L.SHAPES[c["shape"]][2]) for t in TABLE.values() for c in t.values()})
    assert [g[0] for g in _ask(program, "grid", rows)] == [L.queue_grid(*r) for r in rows]
    deeps = [(hell, cap + more, cap) for hell in (0, 1) for cap in (6, 36, 48, 96, 256) for more in (-1, 0, 1)]
    for (hell, mx, cap), g in zip(deeps, _ask(program, "deep", deeps)):
        assert bool(g[0]) == L.dispatch("D", hell, M.GATHER, 0, True, mx, 100, dict(L.TUNE, cap=cap), "list")["deep_follow"]


def test_matrices_on_both_sides_of_the_probe():
    said = {L.probe_said(L.matrix_of(c)) for t in TABLE.values() for c in t.values() if c["row_order"]}
    assert said == {4, 5, 6}, said
    for letter in L.LETTERS:
        for cid, case in TABLE[letter].items():
            for mode in case["modes"]:
                assert L.case_route(case, mode, L.matrix_of(case))["shape"] == case["shape"], (letter, cid, mode)


@pytest.mark.parametrize("letter", L.LETTERS)
def test_the_oracle_in_the_ragged_order_is_within_the_bound(letter):
    straddling = 0
    for cid, case in TABLE[letter].items():
        m = L.matrix_of(case)
        x, y = L.operands(letter, m)
        alpha, beta = L.scalars_of(case)
        r, c, v = m["coo"]
        order = m["r_idx"] if case["row_order"] else None
        want, scale = X.spmv(m["rows"], r, c, v, x, y if beta != 0 else None, alpha, beta, r_idx=order)
        got = L.oracle(m, x, y, alpha, beta, case["tune"], with_order=case["row_order"])
        assert not np.isnan(got).any(), f"{letter}-{cid}: the oracle used a padding slot"
        X.assert_within(got, want, scale, letter, case=f"{letter}-{cid}")
        straddling += m["fmt"] == "hell" and m["hack_size"] % 32 != 0
    assert straddling >= 2
