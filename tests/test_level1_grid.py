"""CPU: spgpu_amd/csrc/level1_grid.h -- the one place where the Level-1 calls and the fused CG steps choose `wide`, the grid, the passes
and the non-temporal kernel -- executed.  tests/level1_grid_cases.cpp is a stand-alone program around that header (g++, undefined-behaviour
sanitizer on: an overflow in the grid arithmetic ends it); its answers are compared with the dispatch as the test modules restate it
(device_scalars_mv_launch_shapes, fused_launch_shapes, the thresholds of level1_launch_shapes) on every entry of their case tables, and on
the boundaries of every rule with the dispatch as it was written out, call by call, in level1.hip / fused_solver.hip / reduce.hip.h before
the header existed (the `before_*` functions below keep those expressions as they stood)."""
import os
import re
import subprocess

import pytest

import device_scalars_mv_launch_shapes as M
import fused_launch_shapes as F
import level1_launch_shapes as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spgpu_amd", "csrc")
SIZES = (4, 8, 16)
TILE, CAP_REDUCE, CAP_MAP, NT = 1024, 1024, 16384, 256 << 20


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    internal = open(os.path.join(CSRC, "spgpu_internal.h")).read()
    cap = re.search(r"#define SPGPU_REDUCE_MAX_BLOCKS (\d+)\b", internal).group(1)
    exe = str(tmp_path_factory.mktemp("level1_grid") / "level1_grid_cases")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
                    f"-DSPGPU_REDUCE_MAX_BLOCKS={cap}", os.path.join(ROOT, "tests", "level1_grid_cases.cpp"), "-o", exe], check=True)
    return exe


def case(family, eb, n, count=1, pitch=0, has_beta=0, y_given=1, extra=0, offs=()):
    offs = tuple(offs) + (0,) * (5 - len(offs))
    return (family, eb, n, count, pitch, int(has_beta), int(y_given), extra) + offs


def run(program, cases):
    """One list of launches (tuples of ints: first vectors wide blocks nt [packed]) per case."""
    text = "".join(" ".join(str(v) for v in c) + "\n" for c in cases)
    done = subprocess.run([program], input=text, capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])          # the sanitizer's report ends the program
    assert "runtime error" not in done.stderr, done.stderr[-2000:]
    out = []
    for line in done.stdout.splitlines():
        if line.startswith("case "):
            assert int(line.split()[1]) == len(out)
            out.append([])
        else:
            out[-1].append(tuple(int(v) for v in line.split()))
    assert len(out) == len(cases)
    return out


def check(program, pairs):
    got = run(program, [c for c, _ in pairs])
    for (c, want), g in zip(pairs, got):
        assert g == want, (c, "header", g, "expected", want)


# ---- the dispatch as the call sites wrote it out before level1_grid.h (uintptr_t arithmetic on addresses; NULL is address 0) ----
def _addr(off, given=True):
    return (1 << 40) + off if given else 0


def _blocks_before(n, wide, W, cap):
    work = (n + W - 1) // W if wide else n
    return min((work + 256 * 4 - 1) // (256 * 4), cap)


def before_axpby(eb, n, count, pitch, off_z, off_x, off_y, has_beta, y_given):
    """axpbyLaunch."""
    if n <= 0 or count <= 0:
        return []
    W, z, x, y = 16 // eb, _addr(off_z), _addr(off_x), _addr(off_y, y_given)
    wide = W > 1 and z % 16 == 0 and x % 16 == 0 and (not has_beta or y % 16 == 0) and (count == 1 or pitch % W == 0)
    cap = 16384 // (count if count < 16384 else 16384)
    nt = n * eb * count * (2 + (1 if has_beta else 0)) >= (256 << 20)
    return [(0, count, int(wide), _blocks_before(n, wide, W, cap if cap > 1 else 1), int(nt))]


def before_map(eb, n, count, pitch, offs, streams):
    """mapLaunch: streams 2 (scal, abs: out, x), 3 (axy: + y), 4 (axypbz: + z)."""
    if n <= 0 or count <= 0:
        return []
    W = 16 // eb
    out, x, y, z = (_addr(o) for o in offs[:4])
    wide = (W > 1 and out % 16 == 0 and x % 16 == 0 and (streams < 3 or y % 16 == 0) and (streams != 4 or z % 16 == 0)
            and (count == 1 or pitch % W == 0))
    cap = 16384 // (count if count < 16384 else 16384)
    nt = wide and n * eb * count * streams >= (256 << 20)
    return [(0, count, int(wide), _blocks_before(n, wide, W, cap if cap > 1 else 1), int(nt))]


def before_reduce(eb, n, count, pitch, off_a, off_b, streams):
    """reduceVectors / reduceVectorsToDevice over reduceFirstStage, reduceWide, reduceBlocks (b == NULL unless dot: streams 2)."""
    W, out = 16 // eb, []
    for first in range(0, max(count, 0), 1024):
        vectors = min(count - first, 1024)
        if n <= 0:
            out.append((first, vectors, 0, 0, 0))
            continue
        a, b = _addr(off_a) + first * pitch * eb, (_addr(off_b) + first * pitch * eb if streams == 2 else 0)
        wide = W > 1 and a % 16 == 0 and b % 16 == 0 and (vectors == 1 or pitch % W == 0)
        nt = wide and n * eb * vectors * streams >= (256 << 20)
        out.append((first, vectors, int(wide), _blocks_before(n, wide, W, 1024 // vectors), int(nt)))
    return out


def before_reduce_device(eb, n, off_a, off_b, streams):
    """dotToDevice / nrm2ToDevice (S, D): no non-temporal kernel; also dotBlocks + aligned() of fused_solver.hip."""
    if n <= 0:
        return [(0, 1, 0, 0, 0)]
    W = 16 // eb
    wide = W > 1 and _addr(off_a) % 16 == 0 and (streams != 2 or _addr(off_b) % 16 == 0)
    return [(0, 1, int(wide), _blocks_before(n, wide, W, 1024), 0)]


def before_pair_dot_mv(eb, n, count, pitch, off_z2):
    """axpbyPairDotMv: reduceWide / reduceBlocks on (z2, z2) per pass; it has no non-temporal kernel."""
    return [p[:4] + (0,) for p in before_reduce(eb, n, count, pitch, off_z2, off_z2, 2)]


def before_axpby_device(eb, n, count, pitch, off_z, off_x, off_y, has_beta, y_given, mv):
    """axpbyFromDevice (mv False: one vector) / axpbyFromDeviceMv."""
    if n <= 0 or (mv and count <= 0):
        return []
    W, z, x, y = 16 // eb, _addr(off_z), _addr(off_x), _addr(off_y, y_given)
    wide = z % 16 == 0 and x % 16 == 0 and (not has_beta or not y or y % 16 == 0) and (not mv or count == 1 or pitch % W == 0)
    if not mv:
        return [(0, 1, int(wide), _blocks_before(n, wide, W, 16384), 0)]
    return [(first, min(count - first, 16384), int(wide), _blocks_before(n, wide, W, 16384 // min(count - first, 16384)), 0)
            for first in range(0, count, 16384)]


def before_spmv_dot(eb, rows, hack, off_w, off_z, off_cM, off_rP, off_rS):
    """hellSpmvDot."""
    if rows <= 0:
        return [(0, 1, 0, 0, 0, 0)]
    W = 16 // eb
    wide = _addr(off_w) % 16 == 0 and _addr(off_z) % 16 == 0
    packed = wide and hack % W == 0 and _addr(off_cM) % 16 == 0 and _addr(off_rP) % (4 * W) == 0 and _addr(off_rS) % (4 * W) == 0
    return [(0, 1, int(wide), _blocks_before(rows, wide, W, 1024), 0, int(packed))]


# ---- the constants ----------------------------------------------------------------------------------------------------------------
def test_the_header_states_each_constant_once_and_the_restated_dispatch_agrees():
    grid = open(os.path.join(CSRC, "level1_grid.h")).read()
    value = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", grid).group(1))
    assert value("kL1Threads") == M.THREADS == F.kL1Threads == L.THREADS == 256 and value("kL1Unroll") == M.UNROLL == F.kL1Unroll == L.UNROLL == 4
    assert value("kL1MaxBlocks") == M.L1_MAX_BLOCKS == L.MAP_MAX_BLOCKS == CAP_MAP
    assert "constexpr long long kL1StreamedBytes = 256ll << 20;" in grid and L.NT_BYTES == NT
    assert M.REDUCE_MAX_BLOCKS == F.SPGPU_REDUCE_MAX_BLOCKS == L.REDUCE_MAX_BLOCKS == CAP_REDUCE and M.TILE == F.TILE == L.TILE == TILE
    # what section E of the refactor asks of the four files together
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("level1.hip", "fused_solver.hip", "reduce.hip.h", "level1_grid.h"))
    assert len(re.findall(r"16 / \(?(int\))?sizeof|16 / elemBytes", text)) == 1 and len(re.findall(r"256ll? << 20", text)) == 1
    assert len(re.findall(r"% 16 == 0|% bytes [!=]= 0", text)) == 1 and len(re.findall(r"\(a \+ b - 1\) / b", text)) == 1
    assert not re.search(r"- 1\) / \(?kL1|#define SPGPU_\w*_GO", text)
    for kernel in ("axpbyKernel", "reduceKernel", "mapKernel", "axpbyDeviceKernel", "axpbyDeviceMvKernel", "axpbyPairDotKernel",
                   "axpbyPairDotMvKernel", "hellSpmvDotKernel"):
        assert len(re.findall(rf"hipLaunchKernelGGL\(\({kernel}<", text)) == 1, kernel


# ---- the three case tables --------------------------------------------------------------------------------------------------------
def test_the_multivector_case_table(program):
    pairs = []
    for letter in M.LETTERS:
        eb = M.SIZEOF[letter]
        for c in M.cases(letter).values():
            n, count, pitch, off = c["n"], c["count"], c["pitch"], c["off"]
            passes = M.reduce_passes(letter, n, count, pitch, off, off)
            firsts = range(0, count, M.REDUCE_MAX_BLOCKS)
            want = [(f, p["vectors"], int(bool(p["wide"])), p["blocks"], 0) for f, p in zip(firsts, passes)]
            assert want == before_reduce(eb, n, count, pitch, off, off, 2)                     # far below the non-temporal threshold
            pairs.append((case("reduce", eb, n, count, pitch, extra=2, offs=(off, off)), want))
            pairs.append((case("pair-dot-mv", eb, n, count, pitch, offs=(off,)), want))
            nrm2 = M.reduce_passes(letter, n, count, pitch, off, 0)
            pairs.append((case("reduce", eb, n, count, pitch, extra=1, offs=(off, 0)),
                          [(f, p["vectors"], int(bool(p["wide"])), p["blocks"], 0) for f, p in zip(firsts, nrm2)]))
            for beta_given in (True, False):
                for off_y in (off, None):
                    u = M.update_launch(letter, n, count, pitch, off, off, off_y, beta_given)
                    want = [] if u is None else [(0, count, int(u["wide"]), u["blocks"], 0)]
                    assert want == before_axpby_device(eb, n, count, pitch, off, off, off_y or 0, beta_given, off_y is not None, True)
                    pairs.append((case("axpby-device-mv", eb, n, count, pitch, beta_given, off_y is not None, offs=(off, off, off_y or 0)), want))
    check(program, pairs)


def test_the_fused_case_table(program):
    pairs = []
    for letter in F.LETTERS:
        eb = F.SIZEOF[letter]
        for c in F.cases(letter).values():
            off = c["off"]
            if c["call"] == "pair":
                got = F.pair_dot_launch(letter, c["n"], off["z2"] * eb)
                want = [(0, 1, 0, 0, 0)] if got is None else [(0, 1, int(got["path"] == "wide"), got["blocks"], 0)]
                assert want == before_reduce_device(eb, c["n"], off["z2"] * eb, off["z2"] * eb, 2)
                pairs.append((case("pair-dot", eb, c["n"], offs=(off["z2"] * eb,)), want))
                continue
            byte = lambda k: off[k] * (4 if k in ("rP", "rS") else eb)
            offs = (byte("x") if c["w_null"] else byte("w"), byte("z"), byte("cM"), byte("rP"), byte("rS"))
            got = F.spmv_dot_launch(letter, c["rows"], c["hack"], *offs)
            want = [(0, 1, 0, 0, 0, 0)] if got is None else [(0, 1, int(got["path"] != "narrow"), got["blocks"], 0, int(got["path"] == "packed"))]
            assert want == before_spmv_dot(eb, c["rows"], c["hack"], *offs)
            pairs.append((case("spmv-dot", eb, c["rows"], extra=c["hack"], offs=offs), want))
    assert len(pairs) > 100
    check(program, pairs)


def test_the_level1_thresholds(program):
    """The sizes of tests/test_gpu_level1_shapes.py: past the caps the grid is the cap, wide; at n_reduce_nt nrm2 and dot stream."""
    pairs = []
    for letter, eb in L.SIZEOF.items():
        W = L.WIDE[letter]
        n = L.n_past_map_cap(letter)
        nt = lambda streams: int(n * eb * streams >= NT)
        pairs.append((case("axpby", eb, n, has_beta=1), [(0, 1, int(W > 1), CAP_MAP, nt(3))]))
        pairs.append((case("axpby", eb, n, has_beta=0), [(0, 1, int(W > 1), CAP_MAP, nt(2))]))
        for streams in (2, 3, 4):
            pairs.append((case("map", eb, n, extra=streams), [(0, 1, int(W > 1), CAP_MAP, int(W > 1 and nt(streams)))]))
        if letter in "SD":
            pairs.append((case("axpby-device", eb, n, has_beta=1), [(0, 1, 1, CAP_MAP, 0)]))
        n = L.n_past_reduce_cap(letter)
        for streams in (1, 2):
            pairs.append((case("reduce", eb, n, extra=streams), [(0, 1, int(W > 1), CAP_REDUCE, int(W > 1 and n * eb * streams >= NT))]))
        n = L.n_reduce_nt(letter)
        for streams in (1, 2):
            pairs.append((case("reduce", eb, n, extra=streams), [(0, 1, int(W > 1), CAP_REDUCE, int(W > 1))]))
            pairs.append((case("reduce-device", eb, n, extra=streams), [(0, 1, int(W > 1), CAP_REDUCE, 0)]))   # never streams
    check(program, pairs)


# ---- the boundaries of every rule, against the dispatch as it was written out ------------------------------------------------------
COUNTS = (1, 2, 1024, 1025, 8192, 16384, 16400)


def _all_families(eb, n, count, pitch, offs=(0, 0, 0, 0, 0), has_beta=1, y_given=1):
    """(case, expected) of every family on one shape; the device-scalar and fused families for the S and D sizes only."""
    o = tuple(offs) + (0,) * (5 - len(offs))
    pairs = [(case("axpby", eb, n, count, pitch, has_beta, y_given, offs=o), before_axpby(eb, n, count, pitch, o[0], o[1], o[2], has_beta, y_given))]
    for streams in (2, 3, 4):
        pairs.append((case("map", eb, n, count, pitch, extra=streams, offs=o), before_map(eb, n, count, pitch, o, streams)))
    for streams in (1, 2):
        pairs.append((case("reduce", eb, n, count, pitch, extra=streams, offs=o), before_reduce(eb, n, count, pitch, o[0], o[1], streams)))
    if eb < 16:
        for streams in (1, 2):
            pairs.append((case("reduce-device", eb, n, extra=streams, offs=o), before_reduce_device(eb, n, o[0], o[1], streams)))
        pairs.append((case("axpby-device", eb, n, has_beta=has_beta, y_given=y_given, offs=o),
                      before_axpby_device(eb, n, 1, 0, o[0], o[1], o[2], has_beta, y_given, False)))
        pairs.append((case("axpby-device-mv", eb, n, count, pitch, has_beta, y_given, offs=o),
                      before_axpby_device(eb, n, count, pitch, o[0], o[1], o[2], has_beta, y_given, True)))
        pairs.append((case("pair-dot", eb, n, offs=o), before_reduce_device(eb, n, o[0], o[0], 2)))
        pairs.append((case("pair-dot-mv", eb, n, count, pitch, offs=o), before_pair_dot_mv(eb, n, count, pitch, o[0])))
        pairs.append((case("spmv-dot", eb, n, extra=32, offs=o), before_spmv_dot(eb, n, 32, *o)))
    return pairs


@pytest.mark.parametrize("eb", SIZES)
def test_the_tile_and_cap_boundaries(program, eb):
    W = 16 // eb
    ns = [0, 1, TILE * W - 1, TILE * W, TILE * W + 1, TILE - 1, TILE, TILE + 1]
    for cap in (CAP_REDUCE, CAP_MAP):
        ns += [cap * TILE * W, cap * TILE * W + TILE * W, cap * TILE, cap * TILE + TILE]
    pairs = []
    for n in ns:
        for off in (0, eb):                                    # wide (where the type has it) and narrow
            pairs += _all_families(eb, n, 1, 0, (off, 0, 0, 0, 0))
    for count in COUNTS + (0,):
        for n in (5, 3 * TILE * W + 1, 70 * TILE * W):       # below, at and above what a vector's share of the cap allows
            pairs += _all_families(eb, n, count, 70 * TILE * W + 8)
    # the written expectations at the corners, not only the restated expressions
    assert before_reduce(eb, CAP_REDUCE * TILE * W + TILE * W, 1, 0, 0, 0, 1)[0][3] == CAP_REDUCE
    # 1 024 vectors of 70 x 16 KiB are 1 120 MiB: the first pass streams where it is wide; the one vector of the second does not
    assert before_reduce(eb, 70 * TILE * W, 1025, 8, 0, 0, 1) == [(0, 1024, int(W > 1), 1, int(W > 1)), (1024, 1, int(W > 1), 70, 0)]
    assert before_axpby(eb, 70 * TILE * W, 16400, 8, 0, 0, 0, 1, 1)[0][1:4] == (16400, int(W > 1), 1)
    assert before_axpby(eb, 70 * TILE * W, 8192, 8, 0, 0, 0, 1, 1)[0][3] == 2 and before_axpby(eb, 3 * TILE, 1, 0, eb, 0, 0, 1, 1)[0][3] == 3
    if eb < 16:
        assert [p[:2] + p[3:4] for p in before_axpby_device(eb, 70 * TILE * W, 16400, 8, 0, 0, 0, 1, 1, True)] == [(0, 16384, 1), (16384, 16, 70)]
    check(program, pairs)


@pytest.mark.parametrize("eb", SIZES)
def test_the_non_temporal_threshold(program, eb):
    """Streamed bytes exactly at 256 MiB and one element below, per family and number of streams; narrow only for axpby."""
    pairs, seen = [], set()
    for streams in (1, 2, 3, 4):
        for count in (1, 2):
            n = NT // (eb * streams * count)
            if n * eb * streams * count != NT:                 # 3 streams: 256 MiB is no multiple; take the first n past it
                n += 1
            for m in (n, n - 1):
                for off in (0, eb):
                    for pair in _all_families(eb, m, count, n + 8 - n % 8, (off,), has_beta=1) + _all_families(eb, m, count, n + 8 - n % 8, (off,), has_beta=0):
                        pairs.append(pair)
                        seen |= {(pair[0][0], launch[2], launch[4]) for launch in pair[1]}
    wide = int(eb < 16)
    assert {("axpby", wide, 1), ("axpby", 0, 1), ("axpby", wide, 0), ("map", wide, wide), ("reduce", wide, wide), ("map", 0, 0), ("reduce", 0, 0)} <= seen
    assert not {s for s in seen if s[2] and s[0] not in ("axpby", "map", "reduce")} and ("map", 0, 1) not in seen and ("reduce", 0, 1) not in seen
    assert before_axpby(eb, NT // (2 * eb), 1, 0, 0, 0, 0, 0, 1)[0][4] == 1 and before_axpby(eb, NT // (2 * eb) - 1, 1, 0, 0, 0, 0, 0, 1)[0][4] == 0
    assert before_axpby(eb, NT // (2 * eb) - 1, 1, 0, 0, 0, 0, 1, 1)[0][4] == 1                              # with y: three streams
    assert before_reduce(eb, NT // eb, 1, 0, 0, 0, 1)[0][4] == wide and before_reduce(eb, NT // eb - 1, 1, 0, 0, 0, 1)[0][4] == 0
    assert before_reduce(eb, NT // (2 * eb), 1, 0, 0, 0, 2)[0][4] == wide
    check(program, pairs)


@pytest.mark.parametrize("eb", SIZES)
def test_alignment_of_every_operand_and_the_pitch(program, eb):
    W = 16 // eb
    n, pairs = 3 * TILE * W + 1, []
    for count, pitch in ((1, n + 2), (2, n + 2), (2, n + W + 2), (1, n + W + 2), (1025, 9), (1025, 8), (1, 9)):
        pitch |= 1                                              # odd: no multiple of WIDE for S, D and C
        for k in range(5):                                      # each operand off a 16-byte boundary in turn
            for by in (eb, 4, 8):
                offs = tuple(by if j == k else 0 for j in range(5))
                pairs += _all_families(eb, n, count, pitch, offs) + _all_families(eb, n, count, pitch + 1, offs)
        pairs += _all_families(eb, n, count, pitch) + _all_families(eb, n, count, pitch + 1)
    # one vector: the pitch plays no part; two: an odd pitch is the narrow path; a second pass of one vector decides for itself
    assert before_reduce(eb, n, 1, 9, 0, 0, 1)[0][2] == int(W > 1) and before_reduce(eb, n, 2, 9, 0, 0, 1)[0][2] == 0
    assert [p[2] for p in before_reduce(4, n, 1025, 4, 0, 0, 1)] == [1, 1] and [p[2] for p in before_reduce(4, n, 1025, 9, 0, 0, 1)] == [0, 1]
    assert before_spmv_dot(8, 100, 32, 0, 0, 0, 8, 0)[0][5] == 1 and before_spmv_dot(4, 100, 32, 0, 0, 0, 8, 0)[0][5] == 0
    for hack in (1, 2, 4, 12, 33):
        pairs += [(case("spmv-dot", e, n, extra=hack), before_spmv_dot(e, n, hack, 0, 0, 0, 0, 0)) for e in (4, 8)]
    check(program, pairs)


@pytest.mark.parametrize("eb", SIZES)
def test_y_null_or_misaligned(program, eb):
    """y counts where beta says it is read.  The host-scalar rule (`!hasBeta || y % 16 == 0`) and the device-scalar one
    (`!hasBeta || !y || y % 16 == 0`) are written differently and decide alike: NULL lies on every boundary."""
    n, pairs = 3000, []
    for has_beta in (0, 1):
        for y_given in (0, 1):
            for off_y in (0, eb):
                for count, pitch in ((1, 0), (2, 3008)):
                    pairs += _all_families(eb, n, count, pitch, (0, 0, off_y), has_beta, y_given)
                want_wide = int(eb < 16 and not (has_beta and y_given and off_y))
                assert before_axpby(eb, n, 1, 0, 0, 0, off_y, has_beta, y_given)[0][2] == want_wide
                if eb < 16:
                    assert before_axpby_device(eb, n, 1, 0, 0, 0, off_y, has_beta, y_given, False)[0][2] == want_wide
                    assert before_axpby_device(eb, n, 2, 3008, 0, 0, off_y, has_beta, y_given, True)[0][2] == want_wide
    check(program, pairs)


@pytest.mark.parametrize("eb", SIZES)
def test_the_largest_sizes_do_not_overflow(program, eb):
    """n = 2^31 - 1 with 16 400 vectors: 2^51 streamed bytes, byte shifts of passes past 2^49.  The sanitizer reports nothing
    (run() checks) and the launches are those of exact arithmetic."""
    n = 2**31 - 1
    pairs = _all_families(eb, n, 16400, n - n % 4 + 4) + _all_families(eb, n, 16400, n) + _all_families(eb, n, 1, 0)
    pairs += _all_families(eb, 0, 0, 0) + _all_families(eb, 0, 3, 4) + _all_families(eb, 5, 0, 8) + _all_families(eb, -1, -1, 0)
    assert before_reduce(eb, n, 1, 0, 0, 0, 1) == [(0, 1, int(eb < 16), CAP_REDUCE, int(eb < 16))]
    assert len(before_reduce(eb, n, 16400, n + 1, 0, 0, 2)) == 17 and before_reduce(eb, 0, 3, 4, 0, 0, 2) == [(0, 3, 0, 0, 0)]
    check(program, pairs)
