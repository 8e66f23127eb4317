"""The constants of the host dispatch behind include/spgpu/ext/device_scalars_mv.h (spgpu_amd/csrc/level1_grid.h, called from level1.hip
and fused_solver.hip), that dispatch restated as a function of what a caller passes, and the case table tests/test_gpu_device_scalars_mv.py
runs -- stated once for that module (which runs the cases on the GPU) and for tests/test_device_scalars_mv_launch_shapes.py (which
checks on the CPU that the table reaches every branch, and that each case reaches the branches it is there for).  No torch, no library:
importable everywhere."""

# ---- the constants of the dispatch: a change there is a test to revisit here ------------------------------------------------------
THREADS = 256                 # level1_grid.h    kL1Threads
UNROLL = 4                    # level1_grid.h    kL1Unroll: 16-byte accesses in flight per lane
TILE = THREADS * UNROLL       # packs (wide) or elements (narrow) one workgroup takes per trip
REDUCE_MAX_BLOCKS = 1024      # spgpu_internal.h SPGPU_REDUCE_MAX_BLOCKS: partials the scratch holds = vectors of a pass = blocks they share
L1_MAX_BLOCKS = 16384         # level1_grid.h    kL1MaxBlocks: the same two roles for the updates
LETTERS = "SD"
SIZEOF = {"S": 4, "D": 8}
WIDE = {L: 16 // SIZEOF[L] for L in LETTERS}      # elements of a 16-byte access: S 4, D 2


def _ceil(a, b):
    return -(-a // b)


def reduce_passes(letter, n, count, pitch, off_a=0, off_b=0):
    """reduceVectorsToDevice / reduceVectors (level1.hip) over forEachPass / reduceGrid (level1_grid.h) restated: the passes of
    spgpu?mdotDevice, each dict(vectors, wide, blocks, cap_binds).  off_a, off_b: bytes by which the bases lie past a 16-byte
    boundary (nrm2: off_b = 0; the pair-dot: both those of z2).  count <= 0: no pass.  n <= 0: passes without a first stage
    (blocks 0)."""
    size, w = SIZEOF[letter], WIDE[letter]
    out = []
    for first in range(0, max(count, 0), REDUCE_MAX_BLOCKS):
        vectors = min(REDUCE_MAX_BLOCKS, count - first)
        if n <= 0:
            out.append(dict(vectors=vectors, wide=None, blocks=0, cap_binds=False))
            continue
        at = first * pitch * size
        wide = (off_a + at) % 16 == 0 and (off_b + at) % 16 == 0 and (vectors == 1 or pitch % w == 0)
        blocks = _ceil(_ceil(n, w) if wide else n, TILE)
        cap = REDUCE_MAX_BLOCKS // vectors
        out.append(dict(vectors=vectors, wide=wide, blocks=min(blocks, cap), cap_binds=blocks > cap))
    return out


def cap_free(letter, n, count):
    """The header's third condition: ceil(ceil(n / (16 / sizeof(T))) / 1024) * count <= SPGPU_REDUCE_MAX_BLOCKS."""
    return _ceil(_ceil(n, WIDE[letter]), TILE) * count <= REDUCE_MAX_BLOCKS


def repeats_single_vector_call(letter, n, count, pitch, *offs):
    """The header's three conditions under which result[j] has the bits of spgpu?dotDevice / spgpu?nrm2Device on vector j alone."""
    return all(o % 16 == 0 for o in offs) and pitch * SIZEOF[letter] % 16 == 0 and cap_free(letter, n, count)


def update_launch(letter, n, count, pitch, off_z=0, off_x=0, off_y=None, beta_given=True):
    """axpbyFromDeviceMv (level1.hip) over axpbyDeviceGrid (level1_grid.h) restated: None where nothing is launched, else dict(wide, blocks) of the (only, for
    count <= 16384) pass.  off_y None: y == NULL; beta_given False: spgpu?maxpbyDevice with beta == NULL (y is never read)."""
    if n <= 0 or count <= 0:
        return None
    assert count <= L1_MAX_BLOCKS
    w = WIDE[letter]
    y_counts = beta_given and off_y is not None
    wide = off_z % 16 == 0 and off_x % 16 == 0 and (not y_counts or off_y % 16 == 0) and (count == 1 or pitch % w == 0)
    blocks = _ceil(_ceil(n, w) if wide else n, TILE)
    return dict(wide=wide, blocks=min(blocks, L1_MAX_BLOCKS // count))


# ---- per-vector coefficients of the updates ---------------------------------------------------------------------------------------
#: mode -> (call, how beta is given).  `quot`: spgpu?maxpbyQuotDevice, `plain`: spgpu?maxpbyDevice.
#:   quot-mixed   beta_j = betaNum[j] / betaDen[j] with betaNum[j] == 0 for j % 3 == 1; alpha_j = -(alphaNum[j] / alphaDen[j])
#:   quot-ones    betaNum == betaDen == alphaNum == NULL (beta_j = 1, alpha_j = 1 / alphaDen[j])
#:   plain-mixed  beta[j] == 0 for j % 2 == 0; alpha[j]
#:   plain-null   beta == NULL: no vector of y is read; alpha[j]
#:   in-place     quot-mixed with z == y
MODES = ("quot-mixed", "quot-ones", "plain-mixed", "plain-null", "in-place")


def has_beta(mode, j):
    """The body axpbyDeviceMvKernel takes for vector j: True HAS_BETA (y is read), False alpha*x alone."""
    if mode in ("quot-mixed", "in-place"):
        return j % 3 != 1
    if mode == "quot-ones":
        return True
    if mode == "plain-mixed":
        return j % 2 != 0
    assert mode == "plain-null"
    return False


def beta_branches(mode, count):
    """The branches of the per-vector choice a mode reaches with `count` vectors."""
    if mode == "plain-null":
        return {"beta-null"}
    return {"beta-nonzero" if has_beta(mode, j) else "beta-zero" for j in range(count)}


# ---- the case table ---------------------------------------------------------------------------------------------------------------
NS = (1, 3, 255, 1025, 2049, 4099)
COUNTS = (1, 2, 3, 8)
PITCHES = ("rounded", "rounded+6", "odd")
BASES = ("aligned", "shifted")
CAP_N = {"D": 40_001, "S": 70_001}       # 20 resp. 18 workgroups of 16-byte accesses per vector; 64 vectors leave 16 each
CAP_COUNT = 64
TWO_PASS = dict(n=5, count=REDUCE_MAX_BLOCKS + 1, pitch=8)
EMPTY = dict(n=0, count=3)

BRANCHES = ("wide", "narrow", "cap-binds", "cap-free", "one-pass", "two-pass", "empty", "update-16-byte", "update-elementwise",
            "beta-zero", "beta-nonzero", "beta-null")


def pitch_of(letter, kind, n):
    """Element stride of vectors of n elements: n rounded up to 16 bytes; that plus 6 elements (24 bytes for S: off the boundary;
    48 bytes for D: on it); the rounded one plus 1, which is odd."""
    w = WIDE[letter]
    rounded = _ceil(n, w) * w
    return {"rounded": rounded, "rounded+6": rounded + 6, "odd": rounded + 1}[kind]


def _want(letter, pitch_kind, base, n, count, passes=1, cap_binds=False):
    """Written out, not computed by reduce_passes() / update_launch(): the branches a case is there for."""
    if n <= 0:
        return {"empty", "one-pass"}
    pitch_on_16 = pitch_kind == "rounded" or (pitch_kind == "rounded+6" and letter == "D") or pitch_kind == "fixed-on-16"
    wide = base == "aligned" and (pitch_on_16 or count == 1)
    want = {"wide" if wide else "narrow", "cap-binds" if cap_binds else "cap-free", "one-pass" if passes == 1 else "two-pass",
            "update-16-byte" if wide else "update-elementwise"}
    for mode in MODES:
        want |= beta_branches(mode, count)
    return want


def cases(letter):
    """id -> case: dict(id, letter, n, count, pitch, pitch_kind, base, off (bytes of every base past a 16-byte boundary), want)."""
    size = SIZEOF[letter]
    c = {}

    def add(cid, n, count, pitch, pitch_kind, base, **kw):
        assert cid not in c, cid
        c[cid] = dict(id=cid, letter=letter, n=n, count=count, pitch=pitch, pitch_kind=pitch_kind, base=base,
                      off=size if base == "shifted" else 0, want=_want(letter, pitch_kind, base, n, count, **kw))

    for n in NS:
        for count in COUNTS:
            for kind in PITCHES:
                for base in BASES:
                    add(f"n{n}-c{count}-{kind}-{base}", n, count, pitch_of(letter, kind, n), kind, base)
    n = CAP_N[letter]
    add(f"cap-n{n}-c{CAP_COUNT}", n, CAP_COUNT, pitch_of(letter, "rounded", n), "rounded", "aligned", cap_binds=True)
    add("two-pass", TWO_PASS["n"], TWO_PASS["count"], TWO_PASS["pitch"], "fixed-on-16", "aligned", passes=2)
    add("empty", EMPTY["n"], EMPTY["count"], 4, "fixed-on-16", "aligned")
    return c


def reached(case):
    """The branches the restated dispatch takes on what a case passes (every array of a call lies `off` bytes past a boundary)."""
    L, n, count, pitch, off = case["letter"], case["n"], case["count"], case["pitch"], case["off"]
    passes = reduce_passes(L, n, count, pitch, off, off)
    got = {"one-pass" if len(passes) == 1 else "two-pass"}
    if n <= 0:
        assert all(p["blocks"] == 0 for p in passes) and update_launch(L, n, count, pitch, off, off, off) is None
        return got | {"empty"}
    first = passes[0]
    got |= {"wide" if first["wide"] else "narrow", "cap-binds" if any(p["cap_binds"] for p in passes) else "cap-free"}
    if repeats_single_vector_call(L, n, count, pitch, off):      # the header's conditions are sufficient ones
        assert len(passes) == 1 and first["wide"] and not first["cap_binds"]
    for mode in MODES:
        launch = update_launch(L, n, count, pitch, off, off, off, beta_given=mode != "plain-null")
        got.add("update-16-byte" if launch["wide"] else "update-elementwise")
        got |= beta_branches(mode, count)
    return got
