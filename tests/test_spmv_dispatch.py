"""CPU: spgpu_amd/csrc/spmv_rules.h -- the one place where the ELL / HELL SpMV for rows as they come decides the wide layout, wideIO, the
vote, the route, the kernel shape and the grid -- executed.  tests/spmv_dispatch_cases.cpp is a stand-alone program around that header
(g++, undefined-behaviour sanitizer on: an overflow in the grid arithmetic ends it); its answers are compared with the dispatch as
tests/spmv_launch_shapes.py restates it (dispatch, vote_form, form_probe) on every case of the case table at the case's own byte offsets,
on AUTO's call sequences and on the boundary of every rule, and with spgpu?SpmvForm's verdict as ellpack_spmv.hip wrote it out before the
header existed (before_analyse_form keeps that expression as it stood)."""
import itertools
import subprocess

import pytest

import spmv_launch_shapes as M

INT_MAX = 2**31 - 1
ALIGNED = dict(cM=0, rP=0, z=0, y=0)
TRIPLES = list(itertools.product(range(5), repeat=3))
SLAB_ROUTES = {"gather": "wide", "strips": "wide", "tiled": "tiled", "lean": "lean", "narrow": "narrow", "narrow-tiled": "narrow-tiled"}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return M.dispatch_program(tmp_path_factory.mktemp("spmv_dispatch"))


def call(letter, hell, form, rows, hack=None, vs=None, is_=None, max_nnz=0, avg=0, addr=None, y_given=True, has_beta=True, said=(0, 0, 0),
         calls=0, frozen=False, knob=True, row_order=False):
    """One Run call.  HELL: hack size 32 unless given; ELL: both pitches the rows rounded up to 32 unless given."""
    hack = (32 if hell else 0) if hack is None else hack
    pitch = hack if hell else (rows + 31) // 32 * 32
    return dict(letter=letter, hell=hell, form=form, rows=rows, hack=hack, vs=pitch if vs is None else vs, is_=pitch if is_ is None else is_,
                max_nnz=max_nnz, avg=avg, addr=dict(ALIGNED, **(addr or {})), y_given=y_given, has_beta=has_beta, said=tuple(said), calls=calls,
                frozen=frozen, knob=knob, row_order=row_order)


def line(c):
    a = c["addr"]
    return " ".join(str(int(v)) for v in (M.SIZEOF[c["letter"]], c["hell"], c["form"], c["rows"], c["hack"], c["vs"], c["is_"], c["max_nnz"], c["avg"],
                                          a["cM"], a["rP"], a["z"], a["y"], c["y_given"], not c["has_beta"], *c["said"], c["calls"], c["frozen"],
                                          c["knob"], c["row_order"]))


def run(program, calls_):
    """What the header answers per call: None, or dict(kernel, grid, wide_io, noted, wide_ok, probe, route, vote) with the kernels as
    spmv_launch_shapes writes them."""
    done = subprocess.run([program], input="".join(line(c) + "\n" for c in calls_), capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])          # the sanitizer's report ends the program
    assert "runtime error" not in done.stderr, done.stderr[-2000:]
    out = []
    for text in done.stdout.splitlines():
        f = text.split()
        if f[0] == "case":
            assert int(f[1]) == len(out)
            out.append(None)
            continue
        letter = calls_[len(out) - 1]["letter"]
        n = [int(v) for v in f[1:] if v.lstrip("-").isdigit()]
        if f[0] == "call":
            out[-1] = dict(wide_ok=bool(n[0]), route=f[2], wide_io=n[1], noted=n[2],
                           vote=dict(strips=bool(n[3]), tile=bool(n[4]), sweep=bool(n[5]), probe=bool(n[6])))
        elif f[0] == "slab":
            rpl, ph, hell, nt, unroll, pipe, tail, strips, block, tile, every, packed, grid, threads = n
            out[-1].update(kernel=("slab", letter, rpl, ph, bool(hell), bool(nt), unroll, bool(pipe), bool(tail), bool(strips), block, tile, every,
                                   bool(packed)), grid=(grid, threads))
        elif f[0] == "sweep":
            vec, packs, hell, beta, tail, grid, threads = n
            out[-1].update(kernel=("sweep", letter, vec, packs, bool(hell), bool(beta), bool(tail)), grid=(grid, threads))
        elif f[0] == "probe":
            out[-1]["probe"] = None if f[1] == "none" else ("probe", letter, n[0], n[1], bool(n[2]), n[3])
            assert f[1] == "none" or (n[4], n[5]) == (3, M.WAVE)                   # three workgroups of one wavefront
        else:
            assert f == ["none"], text
    assert len(out) == len(calls_)
    return out


def route_of(kernel, hell):
    if kernel[0] == "sweep":
        return "sweep"
    plain = kernel[:9] + (False,) + kernel[10:13] + (False,)                       # strips and packed apart
    for name in ("narrow-tiled", "narrow", "tiled", "lean", "gather"):             # (complex fp64: its "tiled" is the narrow one)
        if plain == M.route_kernel(kernel[1], name, hell):
            return SLAB_ROUTES[name]
    raise AssertionError(M.kernel_name(kernel))


def restated(c):
    """The same call through spmv_launch_shapes.  Its dispatch is written for rIdx == NULL on a matrix that is not frozen and with the
    sweep knob on; the three inputs beyond that are applied here as the header's table states them: a row order or the knob takes SWEEP
    from AUTO's vote, a row order sends a caller's SWEEP to AUTO, and PACKED marks the Wide kernel of a frozen matrix."""
    L, form = c["letter"], c["form"]
    if form == M.SWEEP and c["row_order"]:
        form = M.AUTO
    vote = M.vote_form(L, c["rows"], list(c["said"]), c["calls"])
    vote["sweep"] = vote["sweep"] and c["knob"] and not c["row_order"]
    d = M.dispatch(L, c["hell"], form, c["rows"], c["hack"], c["vs"], c["is_"], c["max_nnz"], c["avg"],
                   dict(c["addr"], y=c["addr"]["y"] if c["y_given"] else None), c["has_beta"], vote)
    if d is None:
        return None
    d = dict(d, route=route_of(d["kernel"], c["hell"]))
    if c["frozen"] and d["route"] == "wide":
        d["kernel"] = d["kernel"][:13] + (True,)
    return d


def check(program, calls_):
    """The header's answers, each equal to the restated dispatch's."""
    got = run(program, calls_)
    for c, g in zip(calls_, got):
        want = restated(c)
        if want is None:
            assert g is None, line(c)
            continue
        for key in ("kernel", "grid", "wide_io", "noted", "wide_ok", "probe", "route"):
            assert g[key] == want[key], (line(c), key, "header", g[key], "restated", want[key])
    return got


def before_analyse_form(size, rows, seen):
    """analyseForm of ellpack_spmv.hip, behind the probe's answer, as it stood."""
    strips = local = sweeps = 0
    for q in range(3):
        strips += seen[q] == 2
        local += seen[q] == 3
        sweeps += seen[q] == 4
    if sweeps >= 2 and size == 8 and rows >= 2 * 1024 * 1024:
        return M.SWEEP
    return M.STRIPS if strips >= 2 else (M.XTILE if local >= 2 else M.GATHER)


# ---- the case table and AUTO's sequences ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", M.LETTERS)
def test_every_case_of_the_table_at_its_own_offsets(program, letter):
    table = M.cases(letter)
    calls_ = []
    for c in table.values():
        m = M.matrix_of(c)
        hack, vs, is_, mx = M.strides(m)
        calls_.append(call(letter, m["fmt"] == "hell", c["form"], m["rows"], hack, vs, is_, mx, c["avg"], M.byte_offsets(c), has_beta=c["scalars"][1] != 0))
    got = check(program, calls_)
    for c, g in zip(table.values(), got):
        d = M.case_dispatch(c)                                                     # what the GPU module expects of the case
        assert (g["kernel"], g["grid"], g["wide_io"], g["noted"], g["probe"]) == (d["kernel"], d["grid"], d["wide_io"], d["noted"], d["probe"]), c["id"]
        assert g["kernel"] == M.route_kernel(letter, c["route"], c["fmt"] == "hell", c["scalars"][1] != 0), c["id"]


def test_the_auto_sequences(program):
    """The sequences of test_vote_and_probe_restated_on_the_auto_sequence: call 0 on a new record, calls 1 and 2 on what the samples said."""
    for letter in "SDC":
        for said, forms, probes in (([2, 2, 2], [M.STRIPS] * 3, [False] * 3), ([3, 3, 3], [M.STRIPS, M.XTILE, M.XTILE], [False, True, False]),
                                    ([1, 1, 1], [M.STRIPS, M.GATHER, M.GATHER], [False, True, False])):
            got = check(program, [call(letter, True, M.AUTO, 708, said=said if n else (0, 0, 0), calls=n) for n in range(3)])
            assert [g["noted"] for g in got] == forms and [g["probe"] is not None for g in got] == probes
            assert all(g["probe"] in (None, M.form_probe(letter, True, True)) for g in got)
    got = check(program, [call("D", True, M.AUTO, 708, said=(1, 1, 1), calls=n) for n in range(1, 9)])
    assert [g["probe"] is not None for g in got] == [True, False, False, True, False, False, False, True]
    # a fixed form, a narrow layout and complex fp64 never vote: no probe, whatever the words say
    got = check(program, [call("D", True, M.GATHER, 708, said=(1, 1, 1), calls=1), call("D", True, M.AUTO, 708, addr=dict(cM=8), said=(1, 1, 1), calls=1),
                          call("Z", True, M.AUTO, 708, said=(1, 1, 1), calls=1)])
    assert [g["probe"] for g in got] == [None] * 3 and [g["vote"]["probe"] for g in got] == [False] * 3


# ---- the boundary of every rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letter", M.LETTERS)
def test_wide_layout_clause_by_clause(program, letter):
    w = M.WIDE[letter]
    calls_ = [call(letter, hell, M.GATHER, 100, addr=dict(cM=off)) for hell in (True, False) for off in (0, 8)]
    calls_ += [call(letter, hell, M.STRIPS, 100, addr=dict(rP=off)) for hell in (True, False) for off in (0, 4, 8, 16)]
    calls_ += [call(letter, True, M.GATHER, 100, hack=h) for h in (0, 1, 2, 3, 4, 32)]
    calls_ += [call(letter, False, M.GATHER, 11, vs=vs, is_=12, max_nnz=3) for vs in (11, 12, 13, 14)]
    got = check(program, calls_)
    wide = w > 1
    assert [g["wide_ok"] for g in got[:4]] == [True, False] * 2                                        # cM: 8 past a boundary is off for every type
    assert [g["wide_ok"] for g in got[4:12]] == [True, w == 1, w <= 2, True] * 2                       # rP: on a boundary of 4 * WIDE bytes
    assert [g["wide_ok"] for g in got[12:18]] == [False, w == 1, w <= 2, w == 1, True, True]           # a hack of whole strips
    assert [g["wide_ok"] for g in got[18:]] == [w == 1, True, w == 1, w <= 2]                          # ELL: 11 rows are 12 (fp32, and fp64's 6 strips)
    assert all((g["kernel"][2] > 1) == (g["wide_ok"] and wide) for g in got)
    want = [None if w == 1 else "short-stride", None, None if w == 1 else "stride-multiple", None if w <= 2 else "stride-multiple"]
    assert [restated(c)["fails"] for c in calls_[18:]] == want


@pytest.mark.parametrize("letter", M.LETTERS)
def test_wide_io_operand_by_operand(program, letter):
    calls_ = []
    for hell in (True, False):
        for form in (M.GATHER, M.STRIPS, M.XTILE, M.SWEEP, M.AUTO):
            calls_ += [call(letter, hell, form, 300, addr=a, y_given=y) for a, y in ((None, True), (dict(z=8), True), (dict(y=8), True), (dict(y=8), False),
                                                                                      (None, False))]
    got = check(program, calls_)
    for g in got:
        assert g["kernel"][0] == "sweep" or (g["kernel"][2] > 1) == (M.WIDE[letter] > 1)
    for k in range(0, len(got), 5):
        narrow = got[k]["kernel"][0] == "slab" and got[k]["kernel"][2] == 1
        assert [g["wide_io"] for g in got[k:k + 5]] == ([1] * 5 if narrow else [1, 0, 0, 1, 1])     # y == NULL lies on every boundary


def _reach(letter, route, hell, rows, **kw):
    """A call that reaches `route` (a name of spmv_launch_shapes.route_kernel, or "packed-gather" / "packed-strips")."""
    off = dict(cM=8) if M.WIDE[letter] > 1 else None                             # a narrow layout for the types that have a wide one
    if route.startswith("packed-"):
        return call(letter, hell, M.STRIPS if route == "packed-strips" else M.GATHER, rows, frozen=True, **kw)
    how = {"gather": dict(form=M.GATHER), "strips": dict(form=M.STRIPS), "tiled": dict(form=M.XTILE), "lean": dict(form=M.AUTO, avg=4),
           "narrow": dict(form=M.GATHER, addr=off), "narrow-tiled": dict(form=M.XTILE, addr=off), "sweep": dict(form=M.SWEEP),
           "auto-first": dict(form=M.AUTO)}[route]
    return call(letter, hell, rows=rows, **dict(how, **kw))


def routes_of(letter):
    if M.WIDE[letter] == 1:
        return ("narrow", "narrow-tiled", "sweep")
    return ("gather", "strips", "auto-first", "tiled", "narrow", "narrow-tiled", "sweep", "packed-gather", "packed-strips") + \
        (("lean",) if M.SIZEOF[letter] == 8 else ())


@pytest.mark.parametrize("letter", M.LETTERS)
def test_grid_of_every_shape(program, letter):
    """One row, one workgroup's rows exactly, one more; the sweep's cap of 2 048 workgroups; INT_MAX rows (the sanitizer watches)."""
    for hell in (True, False):
        for route in routes_of(letter):
            plain = {"packed-gather": "gather", "packed-strips": "strips"}.get(route, route)
            per = M.wg_rows(M.route_kernel(letter, plain, hell))
            rows = [1, per - 1, per, per + 1, INT_MAX]
            if route == "sweep":
                rows += [M.SWEEP_MAX_BLOCKS * per, M.SWEEP_MAX_BLOCKS * per + 1]
            kw = {} if hell else dict(vs=2**31, is_=2**31)                         # ELL: a pitch that holds the strips of every count of rows
            got = check(program, [_reach(letter, route, hell, r, **kw) for r in rows])
            want_route = "sweep" if route == "sweep" else SLAB_ROUTES.get(plain, "wide")
            assert all(g["route"] == want_route for g in got), (route, [g["route"] for g in got])
            assert all(g["kernel"][-1] is route.startswith("packed-") for g in got if g["kernel"][0] == "slab")
            grids = {r: g["grid"][0] for r, g in zip(rows, got)}
            assert (grids[1], grids[per], grids[per + 1]) == (1, 1, 2), (route, grids)
            if route == "sweep":
                assert grids[M.SWEEP_MAX_BLOCKS * per] == grids[M.SWEEP_MAX_BLOCKS * per + 1] == grids[INT_MAX] == M.SWEEP_MAX_BLOCKS
            else:
                assert grids[INT_MAX] == -(-INT_MAX // per)


@pytest.mark.parametrize("letter", M.LETTERS)
def test_lean_takes_short_rows_of_8_byte_types_under_auto_only(program, letter):
    calls_ = [call(letter, False, M.AUTO, 500, max_nnz=mx, avg=hint) for hint in (0, 1, 8, 9) for mx in (16, 17)]
    calls_ += [call(letter, True, M.AUTO, 500, avg=hint) for hint in (0, 1, 8, 9)]
    calls_ += [call(letter, True, form, 500, avg=4) for form in (M.GATHER, M.STRIPS, M.XTILE, M.SWEEP)]
    calls_ += [call(letter, True, M.AUTO, 500, avg=4, said=(3, 3, 3), calls=2), call(letter, True, M.AUTO, 500, avg=4, addr=dict(cM=8))]
    got = check(program, calls_)
    member = M.SIZEOF[letter] == 8
    want = [member and hint in (1, 8) and mx == 16 for hint in (0, 1, 8, 9) for mx in (16, 17)] + [member and hint in (1, 8) for hint in (0, 1, 8, 9)] + [False] * 6
    assert [g["route"] == "lean" for g in got] == want
    assert all(g["noted"] == M.GATHER and g["kernel"] == M.route_kernel(letter, "lean", g["kernel"][4]) for g in got if g["route"] == "lean")


def test_votes_on_every_triple_of_words(program):
    """All 125 triples of the words 0 .. 4, calls 0 .. 8, rows on both sides of kAutoSweepRows, for the 4- and the 8-byte types, with the
    knob off and with a row order: the header's vote is vote_form's, and the launch what dispatch makes of it."""
    for letter in "SD":
        calls_ = [call(letter, True, M.AUTO, rows, said=said, calls=n, knob=knob, row_order=order)
                  for said in TRIPLES for n in range(9) for rows in (M.AUTO_SWEEP_ROWS - 1, M.AUTO_SWEEP_ROWS)
                  for knob, order in ((True, False), (False, False), (True, True))]
        got = check(program, calls_)
        for c, g in zip(calls_, got):
            want = M.vote_form(letter, c["rows"], list(c["said"]), c["calls"])
            want["sweep"] = want["sweep"] and c["knob"] and not c["row_order"]
            assert g["vote"] == want, line(c)
        swept = [c for c, g in zip(calls_, got) if g["route"] == "sweep"]
        assert (len(swept) > 0) == (letter == "D")
        assert all(c["rows"] == M.AUTO_SWEEP_ROWS and c["knob"] and not c["row_order"] and c["said"].count(4) >= 2 for c in swept)
    # SWEEP asked for by the caller: a row order or a narrow layout sends the call to AUTO
    got = check(program, [call("D", True, M.SWEEP, 708), call("D", True, M.SWEEP, 708, row_order=True), call("D", True, M.SWEEP, 708, addr=dict(cM=8)),
                          call("D", True, M.SWEEP, 708, row_order=True, said=(1, 1, 1), calls=1)])
    assert [(g["route"], g["noted"]) for g in got] == [("sweep", M.SWEEP), ("wide", M.STRIPS), ("narrow", M.GATHER), ("wide", M.GATHER)]
    assert got[3]["probe"] == M.form_probe("D", True, True)


def test_the_form_verdict_on_every_triple_of_words(program):
    asked = [(size, rows, said) for size in (4, 8, 16) for rows in (708, M.AUTO_SWEEP_ROWS - 1, M.AUTO_SWEEP_ROWS) for said in TRIPLES]
    done = subprocess.run([program, "verdict"], input="".join(f"{s} {r} {a} {b} {c}\n" for s, r, (a, b, c) in asked), capture_output=True, text=True)
    assert done.returncode == 0 and "runtime error" not in done.stderr, done.stderr[-2000:]
    got = [int(v) for v in done.stdout.split()]
    assert got == [before_analyse_form(size, rows, said) for size, rows, said in asked]
    assert before_analyse_form(8, M.AUTO_SWEEP_ROWS, (4, 4, 2)) == M.SWEEP and before_analyse_form(4, M.AUTO_SWEEP_ROWS, (4, 4, 2)) == M.GATHER
    assert before_analyse_form(8, 708, (2, 3, 2)) == M.STRIPS and before_analyse_form(8, 708, (3, 0, 3)) == M.XTILE


def test_a_frozen_matrix_takes_the_packed_kernels(program):
    """PACKED belongs to the Wide route alone; names in full."""
    got = check(program, [call("D", True, M.GATHER, 1000, frozen=True), call("S", False, M.STRIPS, 1000, frozen=True),
                          call("C", True, M.AUTO, 1000, frozen=True), call("D", True, M.XTILE, 1000, frozen=True),
                          call("D", True, M.AUTO, 1000, avg=4, frozen=True), call("D", True, M.GATHER, 1000, addr=dict(cM=8), frozen=True),
                          call("Z", True, M.GATHER, 1000, frozen=True), call("D", True, M.SWEEP, 1000, frozen=True)])
    names = [M.kernel_name(g["kernel"]) for g in got]
    assert names[0] == "slabSpmvKernel<double, 2, 1, true, true, 8, true, true, false, 256, 0, 0, true>" and got[0]["grid"] == (2, 256)
    assert names[1] == "slabSpmvKernel<float, 4, 8, false, true, 2, true, true, true, 256, 0, 0, true>" and got[1]["grid"] == (8, 256)
    assert names[2] == "slabSpmvKernel<spgpu::Cx<float>, 2, 1, true, true, 8, true, true, true, 256, 0, 0, true>" and got[2]["noted"] == M.STRIPS
    assert names[3] == "slabSpmvKernel<double, 2, 1, true, true, 4, true, true, false, 256, 32768, 8, false>"
    assert names[4] == "slabSpmvKernel<double, 2, 1, true, true, 4, false, true, false, 256, 0, 8, false>"
    assert names[5] == "slabSpmvKernel<double, 1, 2, true, true, 4, true, false, false, 256, 0, 0, false>"
    assert names[6] == "slabSpmvKernel<spgpu::Cx<double>, 1, 2, true, true, 4, true, false, false, 256, 0, 0, false>"
    assert names[7] == "sweepSpmvKernel<double, 2, 16, true, true, true>"


@pytest.mark.parametrize("letter", M.LETTERS)
def test_the_header_can_name_exactly_the_instantiations_of_the_dispatch(program, letter):
    """Every form, layout, vote, hint, beta, frozen or not: the distinct kernels are every_instantiation's plus the packed pair."""
    for hell in (True, False):
        calls_ = [call(letter, hell, form, rows, max_nnz=mx, avg=avg, addr=addr, has_beta=beta, said=said, calls=1, frozen=frozen)
                  for form in range(5) for rows in (708, M.AUTO_SWEEP_ROWS) for mx in (16, 17) for avg in (0, 4) for addr in (None, dict(cM=8))
                  for beta in (True, False) for said in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (4, 4, 4)) for frozen in (False, True)]
        got = check(program, calls_)
        want = M.every_instantiation(letter, hell)
        if M.WIDE[letter] > 1:
            want |= {M.route_kernel(letter, r, hell)[:13] + (True,) for r in ("gather", "strips")}
        assert {g["kernel"] for g in got} == want
        probes = {g["probe"] for g in got} - {None}
        assert probes == M.every_probe(letter, hell)
