"""CPU: spgpu_amd/csrc/ordered_rules.h -- the one place where the ELL / HELL SpMV for rows ordered by length (rIdx given; planned, frozen and
adopted matrices) decides the queue kernel's shape, its stage and split, the grids with and without a plan, the layout of a plan's buffer,
when a matrix gets a plan and when a 16-bit index copy -- executed.  tests/ordered_dispatch_cases.cpp is a stand-alone program around that
header (g++, undefined-behaviour sanitizer on: an overflow in the grid arithmetic ends it); its answers are compared with the expressions
ragged_spmv.hip.h, planned_spmv.hip, frozen_slab.hip.h and ellpack_spmv.hip wrote out before the header existed (the before_* functions
keep them as they stood), with a table of the kernel shapes written out from the launch macros of that time, and with the oracle's own
restatement of the split (oracle_api.ragged_split)."""
import itertools
import subprocess

import pytest

import oracle_api as O
import spmv_launch_shapes as M

INT_MAX = 2**31 - 1
TYPES = (("S", 4), ("D", 8), ("C", 8), ("Z", 16))          # letter, sizeof: fp32, fp64, complex fp32, complex fp64
DEEPS = (0, 1, 7, 8, 9, 8192, 37500)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return M.rules_program(tmp_path_factory.mktemp("ordered_dispatch"), "ordered_dispatch_cases")


def ask(program, rule, questions):
    """The header's answers, a list of ints per question (a tuple of ints)."""
    questions = list(questions)
    done = subprocess.run([program], input="".join(f"{rule} " + " ".join(str(int(v)) for v in q) + "\n" for q in questions), capture_output=True,
                          text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])          # the sanitizer's report ends the program
    assert "runtime error" not in done.stderr, done.stderr[-2000:]
    out = [[int(v) for v in text.split()] for text in done.stdout.splitlines()]
    assert len(out) == len(questions)
    return out


# ---- the ordered path as it stood: ragged_spmv.hip.h, planned_spmv.hip, frozen_slab.hip.h, ellpack_spmv.hip ---------------------------
# LAUNCH_RAGGED(4, 0, 16) / LAUNCH_RAGGED_Z(8, 49152, 64, 17408) / LAUNCH_RAGGED(8, 65536, 32) and SPGPU_PLANNED[_PACKED] with the same
# numbers: (WAVES, TILE_BYTES, SUBS, ZBYTES) by (type, tiled, shape), every case written out
GATHER, TILED, STAGED = (4, 0, 16, 0), (8, 65536, 32, 0), (8, 49152, 64, 17408)
SHAPE_TABLE = {
    ("S", 0, 0): GATHER, ("S", 0, 4): GATHER, ("S", 0, 1): GATHER, ("S", 1, 0): TILED, ("S", 1, 4): STAGED, ("S", 1, 1): TILED,
    ("D", 0, 0): GATHER, ("D", 0, 4): GATHER, ("D", 0, 1): GATHER, ("D", 1, 0): TILED, ("D", 1, 4): STAGED, ("D", 1, 1): TILED,
    ("C", 0, 0): GATHER, ("C", 0, 4): GATHER, ("C", 0, 1): GATHER, ("C", 1, 0): TILED, ("C", 1, 4): STAGED, ("C", 1, 1): TILED,
    ("Z", 0, 0): GATHER, ("Z", 0, 4): GATHER, ("Z", 0, 1): GATHER, ("Z", 1, 0): TILED, ("Z", 1, 4): TILED, ("Z", 1, 1): TILED,
}


def before_staged(size, tiled, shape):
    """launchPlanned: const bool staged = tiled && sizeof(T) <= 8 && shape == 4 (launchRagged: the same, as nested ifs)."""
    return bool(tiled and size <= 8 and shape == 4)


def before_plan_subs(size, tiled, shape):
    """launchPlanned: const int subs = !tiled ? 16 : (staged ? 64 : 32)."""
    return 16 if not tiled else (64 if before_staged(size, tiled, shape) else 32)


def before_may_pack(tiled, size, subs):
    """launchPlanned, Freeze: tiled && sizeof(T) <= 8 && (subs == 64 || subs == 32)."""
    return bool(tiled and size <= 8 and (subs == 64 or subs == 32))


def before_shape_for(knob, tiled, row_order, size, probed, no_deep_list):
    """launchOrdered: the knob, the probe where the shape is the probe's to say, and the stream without a deep list."""
    shape = knob
    if shape == 0 and tiled and row_order and size <= 8:
        shape = probed
    if no_deep_list and shape != 4:
        shape = 0
    return shape


def before_plannable(tiled, shape):
    return bool(not tiled or shape == 0 or shape == 4)


def before_shape_said(said):
    """orderedShape: return said == 4 || said == 6 ? 4 : 0."""
    return 4 if said == 4 or said == 6 else 0


def before_reprobe(said, calls):
    """orderedShape: if (said == 0 || calls % 64 == 0) the probe is launched."""
    return bool(said == 0 or calls % 64 == 0)


def before_deep_kernels_follow(is_hell, max_nnz, deep_cap):
    """launchOrdered: const bool deepPossible = IS_HELL || a.maxNnz > a.deepCap (launchRagged's own answer was always true)."""
    return bool(is_hell or max_nnz > deep_cap)


def before_gives_up(uses, stales):
    """launchPlanned: const bool giveUp = plan->uses < 16 && plan->stales >= 3."""
    return bool(uses < 16 and stales >= 3)


def before_queue_grid(rows, subs_per_block):
    """launchRagged: subs = (rows + 31) / 32; dim3((unsigned)((subs + SUBS - 1) / SUBS)).  startPlan's blocks and launchPlanned's
    planMainBlocks: the same expression."""
    subs = (rows + 31) // 32
    return (subs + subs_per_block - 1) // subs_per_block


def before_plan_grid(main_blocks, deep):
    """launchPlanned's launch lambda: (deepBlocks, grid, planDeepStride), kPlanDeepMost = 8."""
    deep_blocks = (deep + 8 - 1) // 8
    grid = main_blocks + deep_blocks
    if deep_blocks == 0:
        return deep_blocks, grid, 0
    reach = grid * 60 // 100
    stride = reach // deep_blocks
    return deep_blocks, grid, 1 if stride < 1 else stride | 1


def before_layout(blocks, sub_groups, record):
    """startPlan / launchPlanned: roundUp16(blocks * sizeof(SpgpuPlanBlock)), roundUp16(blocks * sizeof(int)), the list, and startPlan's
    hipMalloc argument."""
    up16 = lambda v: (v + 15) // 16 * 16
    block_bytes, count_bytes = up16(blocks * record), up16(blocks * 4)
    return [block_bytes, count_bytes, sub_groups * 4, block_bytes + count_bytes + sub_groups * 4]


def before_pack_plan_bytes(slots):
    """packPlan: ((size_t)slots * sizeof(unsigned short) + 255) / 256 * 256 + 256 -- the copy and, behind it, 256 bytes for its counters."""
    return (slots * 2 + 255) // 256 * 256 + 256


def before_freeze_slab_bytes(slots):
    """freezeSlab: ((size_t)slots * sizeof(unsigned short) + 255) / 256 * 256 (its counters live in the other allocation)."""
    return (slots * 2 + 255) // 256 * 256


def before_pack_plan_keeps(entries, escapes, pct):
    """packPlan gave the copy up if said[1] * 100ull > said[0] * (unsigned long long)(pct < 0 ? 0 : pct)."""
    return not escapes * 100 > entries * (0 if pct < 0 else pct)


def before_freeze_slab_keeps(entries, escapes, pct):
    """freezeSlab kept it if said[1] * 100ull <= said[0] * (unsigned long long)mostPct, mostPct = pct < 0 ? 0 : pct."""
    return escapes * 100 <= entries * (0 if pct < 0 else pct)


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
def test_the_constants(program):
    assert ask(program, "constants", [()]) == [[32, 8, 4, 32, 60, 96]]


def test_the_shape_table(program):
    cases = [(letter, size, tiled, shape) for letter, size in TYPES for tiled in (0, 1) for shape in (0, 4, 1)]
    got = ask(program, "shape", [c[1:] for c in cases])
    assert len(cases) == len(SHAPE_TABLE) == 24
    for (letter, size, tiled, shape), g in zip(cases, got):
        want = SHAPE_TABLE[(letter, tiled, shape)]
        assert tuple(g[:4]) == want, (letter, tiled, shape, g)
        assert g[4] == want[2] * 32                                                # rows per workgroup
        assert g[5] == before_staged(size, tiled, shape) == (want == STAGED)
        assert g[6] == before_plan_subs(size, tiled, shape) == want[2]
        assert g[7] == before_may_pack(tiled, size, g[6])
    assert {tuple(g[:4]) for g in got} == {GATHER, TILED, STAGED}
    # the 16-bit copy: by the sub-group count a plan was made for
    packs = [(tiled, size, subs) for tiled in (0, 1) for _, size in TYPES for subs in (16, 32, 64, 8)]
    got = ask(program, "pack", packs)
    assert [g[0] for g in got] == [before_may_pack(*p) for p in packs]
    assert [g[1] for g in got] == [bool(tiled and size <= 8) for tiled, size, _ in packs]  # launchPlanned: if (tiled && sizeof(T) <= 8) a.planPacked = ...


def test_the_decisions(program):
    """Every value of the knob the table speaks of (0, 4, and 1 for "any other"), both forms, with and without a row order, every
    element size, every answer of the probe, with and without a deep list."""
    asked = list(itertools.product((0, 4, 1), (0, 1), (0, 1), (4, 8, 16), (0, 4), (0, 1)))
    got = ask(program, "decide", asked)
    for (knob, tiled, order, size, probed, no_list), g in zip(asked, got):
        shape = before_shape_for(knob, tiled, order, size, probed, no_list)
        assert g[0] == bool(knob == 0 and tiled and order and size <= 8), (knob, tiled, order, size)   # where launchOrdered asked the probe
        assert g[1] == shape, (knob, tiled, order, size, probed, no_list)
        assert g[2] == before_plannable(tiled, shape)
    # a knob other than 0 and 4 on the tiled form: the 1 024-row shape without a plan -- unless the stream has no deep list
    assert ask(program, "decide", [(1, 1, 1, 8, 0, 0), (1, 1, 1, 8, 0, 1), (1, 0, 1, 8, 0, 0)]) == [[0, 1, 0], [0, 0, 1], [0, 1, 1]]
    said = list(itertools.product(range(8), (0, 1, 63, 64, 65, 128)))
    got = ask(program, "said", said)
    assert got == [[before_shape_said(s), before_reprobe(s, calls)] for s, calls in said]
    assert [before_shape_said(s) for s in range(8)] == [0, 0, 0, 0, 4, 0, 4, 0]
    deep = [(hell, cap + more, cap) for hell in (0, 1) for cap in (1, 64, 256) for more in (-1, 0, 1)]
    assert ask(program, "deep", deep) == [[before_deep_kernels_follow(*d)] for d in deep]
    assert ask(program, "deep", [(0, 256, 256), (0, 257, 256), (1, 0, 256)]) == [[0], [1], [1]]
    ups = list(itertools.product((0, 15, 16, 17), (0, 2, 3, 4)))
    assert ask(program, "giveup", ups) == [[before_gives_up(*u)] for u in ups]
    assert ask(program, "giveup", [(15, 2), (15, 3), (16, 3)]) == [[0], [1], [0]]


def test_the_split_is_the_oracles(program):
    asked = [(letter, size, cap, want) for letter, size in TYPES for cap in (0, 1, 2, 95, 96, 97, 256, 257, 4096)
             for want in (-1, 0, 1, 47, 48, 96, 150, 100000)]
    got = ask(program, "split", [a[1:] for a in asked])
    most = {"S": 6, "D": 3, "C": 3, "Z": 1}                                        # 49152 / sizeof / 2048
    for (letter, size, cap, want), (split, step, chunks, unroll) in zip(asked, got):
        shape = O.slab_shape(letter, "ragged")
        assert step == shape["step"] and step == shape["phases"] * unroll
        assert chunks == most[letter] == 49152 // size // 2048
        assert split == O.ragged_split(letter, step, cap, want), (letter, cap, want)
    assert O.ragged_split("D", 12, 256, -1) == 96 and O.ragged_split("S", 16, 4096, -1) == 688 and O.ragged_split("Z", 6, 256, -1) == 0


def test_the_grids(program):
    rows = (1, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, INT_MAX)
    asked = [(r, subs) for r in rows for subs in (16, 32, 64)]
    got = ask(program, "grid", asked)
    assert got == [[before_queue_grid(r, subs), (r + 31) // 32] for r, subs in asked]
    per = {r: g[0] for (r, subs), g in zip(asked, got) if subs == 32}
    assert (per[1], per[1024], per[1025], per[INT_MAX]) == (1, 1, 2, 2**21)
    plans = [(main, deep) for main in (1, 2, 3, 5, 9, 10, 100, 4883, 9766, 65536, 2**21) for deep in DEEPS]
    got = ask(program, "plan", plans)
    assert got == [list(before_plan_grid(main, deep)) for main, deep in plans]


def test_the_deep_workgroups_stride(program):
    plans = [(main, deep) for main in (1, 2, 3, 5, 9, 10, 100, 4883, 9766, 65536) for deep in DEEPS]
    got = ask(program, "plan", plans)
    for (main, deep), (deep_blocks, grid, stride) in zip(plans, got):
        assert (deep_blocks, grid, stride) == before_plan_grid(main, deep)
        assert deep_blocks == (deep + 7) // 8 and grid == main + deep_blocks
        assert (stride == 0) == (deep_blocks == 0)
        if deep_blocks:
            assert stride >= 1 and stride % 2 == 1
            assert (deep_blocks - 1) * stride < grid, (main, deep, stride)         # the last of them has a place in the grid
    assert before_plan_grid(9766, 37500)[2] == 1 and before_plan_grid(9766, 8192)[2] == 7 and before_plan_grid(4883, 8)[2] == 2931


def test_the_plan_layout(program):
    asked = [(blocks, subs * blocks - cut, 32) for blocks in (1, 2, 3, 4, 5, 1000, 2**20) for subs in (16, 32, 64) for cut in (0, subs - 1)]
    got = ask(program, "layout", asked)
    for (blocks, sub_groups, record), g in zip(asked, got):
        assert g == before_layout(blocks, sub_groups, record)
        assert g[0] % 16 == 0 and (g[0] + g[1]) % 16 == 0                          # the counts and the list start on 16-byte boundaries
        assert g[0] >= blocks * record and g[1] >= blocks * 4 and g[3] == g[0] + g[1] + 4 * sub_groups


def test_the_freeze_rules_are_one(program):
    """packPlan's and freezeSlab's: the same bytes for the copy -- packPlan puts 256 bytes for its counters behind it, a named addend there
    -- and the same threshold, one written as "gives up if more", the other as "keeps if at most"."""
    slots = (1, 127, 128, 129, 2**31)
    got = ask(program, "freeze", [(s,) for s in slots])
    assert got == [[before_freeze_slab_bytes(s)] for s in slots]
    assert all(g[0] + 256 == before_pack_plan_bytes(s) and g[0] % 256 == 0 and g[0] >= 2 * s for s, g in zip(slots, got))
    assert [g[0] for g in got[:4]] == [256, 256, 256, 512]
    asked = []
    for pct in (-1, 0, 1, 5):
        for entries in (0, 1, 99, 100, 101, 250, 300, 10**6, 2**40):
            at = entries * max(pct, 0)                                             # escapes * 100 one step below, at, and one step above it
            for escapes in sorted({max(at // 100 - 1, 0), at // 100, at // 100 + 1, -(-at // 100), -(-at // 100) + 1}):
                asked.append((entries, escapes, pct))
    got = ask(program, "keeps", asked)
    assert [g[0] for g in got] == [before_pack_plan_keeps(*a) for a in asked] == [before_freeze_slab_keeps(*a) for a in asked]
    assert ask(program, "keeps", [(300, 2, 1), (300, 3, 1), (300, 4, 1), (300, 0, -1), (300, 1, -1), (300, 1, 0)]) == [[1], [1], [0], [1], [0], [0]]
    assert {g[0] for g in got} == {0, 1}


def test_an_unknown_rule_is_an_error(program):
    assert subprocess.run([program], input="nonsense 1 2\n", capture_output=True, text=True).returncode == 2
