#pragma once
/*
 * Where the ELL / HELL SpMV for rows as they come (ellpack_spmv.hip: no row order, or one without the deep split) chooses its launches:
 * everything the dispatch decides from numbers and addresses, each rule once.  Plain host C++17, no HIP header: the rules compile and run
 * on their own (tests/spmv_dispatch_cases.cpp).  Wavefronts of kRulesWave lanes; WIDE = 16 / sizeof(T) rows share a 16-byte slab access.
 *
 * slabSpmvKernel<T, RPL, PH, IS_HELL, NT, UNROLL, PIPE, TAIL, STRIPS, BLOCK, TILE_BYTES, TAIL_EVERY, PACKED>; NT is true everywhere; grid
 * (slabGrid): a wavefront per 64 / PH * RPL rows, BLOCK / 64 wavefronts per workgroup.
 *
 * route (chooseRoute)  taken when                               RPL   PH  UNROLL PIPE  TAIL  STRIPS BLOCK TILE_BYTES TAIL_EVERY PACKED  rows per workgroup
 *   Wide         wide layout; GATHER, STRIPS, or AUTO's   fp32   WIDE  8   2      true  true  vote   256   0          0          frozen  128
 *                vote for either                          8-byte WIDE  1   8      true  true  vote   256   0          0          frozen  512
 *   Tiled        wide layout; XTILE, or AUTO's vote       fp32   WIDE  8   2      true  true  false  512   32768      0          false   256
 *                for the x tile                           8-byte WIDE  1   4      true  true  false  256   32768      8          false   512
 *   Lean         wide layout, 8-byte, AUTO, hint 1 .. 8,         WIDE  1   4      false true  false  256   0          8          false   512
 *                ELL: maxNnz <= 16
 *   Narrow       any other layout; complex fp64                  1     2   4      true  false false  256   0          0          false   128
 *   NarrowTiled  the same, XTILE                                 1     2   4      true  false false  256   32768      0          false   128
 *   Sweep        SWEEP on a wide layout without a row order (otherwise the call runs as AUTO), or AUTO's vote (8-byte, kAutoSweepRows rows,
 *                no row order): sweepSpmvKernel<T, WIDE, PACKS, IS_HELL, beta != 0, 8-byte>, PACKS = 32 / WIDE (complex fp64: 16); grid
 *                (sweepGrid): 256 * PACKS * WIDE rows per workgroup, 2 048 workgroups at most
 *   probe        formProbeKernel<T, RPL, PH, IS_HELL, PH * UNROLL> of the Wide (narrow layout: the Narrow) shape, kProbeBlocks workgroups of
 *                one wavefront, in front of the SpMV when autoVote says probeBehind; spgpu?SpmvForm launches it alone
 *
 * The form reported (spgpuGetLastSpmvForm): XTILE for the tiled routes, SWEEP for Sweep, GATHER for Lean, else STRIPS / GATHER by the vote.
 * Who tells AUTO the form: the three sample wavefronts of the strip-capable Wide kernel (what a new matrix runs first); for every other
 * form the probe.  A word they leave says 0 nothing yet, 1 scattered, 2 strips, 3 inside a window an x tile holds, 4 (the probe only)
 * scattered and fit for SWEEP; two of three decide (countForms, then autoVote for AUTO and formVerdict for spgpu?SpmvForm).
 */
#include "level1_grid.h" /* wideOf, ceilDiv */

namespace spgpu {

constexpr int kRulesWave = 64;    /* numeric.hip.h's kWave; ellpack_spmv.hip asserts that they agree */
constexpr int kBlockThreads = 256;
constexpr int kTailLanes = 16;    /* switch to whole-wave row processing when <= this many lanes are busy
                                     (measured flat between 4 and 16 for the 1-phase kernel, worse above) */
constexpr int kTailUnroll = 4;    /* entries per lane in flight in tail mode */
/* The x tile.  Workgroup size and tile size go together: the tile has to hold the columns of the workgroup's rows, and LDS (160 KiB
 * per CU) divided by the tile is the number of workgroups a CU overlaps. */
constexpr int kTileBytes = 32768;
constexpr int kTileSpanNum = 5, kTileSpanDen = 4; /* a sample group is "local" up to 1.25 x the tile */
constexpr int kTiledBlockFp32 = 512;
constexpr int kTailEvery = 8;     /* kernels of the 8-byte types with 4-column stages consider the tail where the 8-column kernel does */
constexpr int kLeanMaxHint = 8, kLeanMaxEll = 16;
constexpr int kSweepLaneRows = 32, kSweepPacks16 = 16, kSweepMaxBlocks = 2048;
constexpr int kAutoSweepRows = 2 * 1024 * 1024; /* AUTO: the SWEEP form wants a grid that fills the chip (8 192 rows per workgroup); measured, scattered
                                                  * fp64, 16 and 32 per row: 1 Mi rows 1.5 x SLOWER than the gathers (x fits the L2s), 2 Mi ... 16 Mi rows 0.61 ... 0.89 x their
                                                  * time (profiles/r04_exp_sweep_rows.txt) */
constexpr int kProbeBlocks = 3;   /* of one wavefront each */
enum SpmvForm { kFormAuto, kFormGather, kFormStrips, kFormXtile, kFormSweep }; /* SPGPU_SPMV_FORM_* (include/spgpu/tuning.h) */

/* ---- layout and alignment ---- */
inline bool alignedTo(const void* p, size_t bytes) { return ((uintptr_t)p % bytes) == 0; }

/* A lane reads WIDE consecutive rows of a slab column with one 16-byte load: the strip must not straddle a hack (HELL) or run past the
 * pitch (ELL), and the streams must be 16-byte aligned. */
inline bool wideLayout(size_t elemBytes, bool isHell, int rows, int hackSize, long long valStride, long long idxStride, const void* cM, const void* rP)
{
    const int wide = wideOf(elemBytes);
    const long long stripRows = ceilDiv(rows, wide) * wide;
    const bool layoutOk = isHell ? (hackSize > 0 && hackSize % wide == 0) : (valStride >= stripRows && idxStride >= stripRows);
    return layoutOk && alignedTo(cM, 16) && alignedTo(rP, 4 * wide) && valStride % wide == 0 && idxStride % wide == 0;
}
/* z and y take 16-byte accesses (NULL lies on every boundary) */
inline bool wideIO(const void* z, const void* y) { return alignedTo(z, 16) && alignedTo(y, 16); }
constexpr long long tileSpanLimit(size_t elemBytes) { return (long long)(kTileBytes / elemBytes) * kTileSpanNum / kTileSpanDen; }

/* ---- kernel shapes ---- */
enum class SpmvRoute { Sweep, Tiled, Lean, Wide, NarrowTiled, Narrow };
constexpr bool narrowRoute(SpmvRoute r) { return r == SpmvRoute::Narrow || r == SpmvRoute::NarrowTiled; } /* RPL == 1: y and z are always aligned */
struct SlabShape { /* slabSpmvKernel's template arguments behind T and IS_HELL; NT is true everywhere */
    int rpl, ph, unroll;
    bool pipe, tail, strips;
    int block, tileBytes, tailEvery;
    bool packed;
};
/* Measured on MI355X, 10 M rows x 32 nnz (profiles/): wide where the layout allows it, the next stage prefetched AFTER the current
 * gathers are issued, whole-wave tail rows -- 8-byte types fastest with a lane walking whole rows, 8 slab columns per stage (banded 5.9 TB/s),
 * fp32 with 8 phases x 2 columns (5.4-6.0 TB/s); narrow: 2 phases x 4 columns (5.9 TB/s).  The tiled and lean kernels add in the order of
 * the type's Wide kernel, the narrow tile in that of Narrow, so the form never changes a bit: the 8-byte tile halves the stage (LDS gathers
 * are short, and at 8 the kernel needs 148 VGPRs: one 512-lane workgroup per CU); Lean drops the prefetch ring (a third of the registers). */
constexpr SlabShape slabShape(SpmvRoute route, size_t elemBytes, bool strips = false, bool packed = false)
{
    const int wide = wideOf(elemBytes);
    const bool fp32 = elemBytes == 4;
    switch (route) {
    case SpmvRoute::Wide: return {wide, fp32 ? 2 * wide : 1, fp32 ? 2 : 8, true, true, strips, kBlockThreads, 0, 0, packed};
    case SpmvRoute::Tiled: return {wide, fp32 ? 2 * wide : 1, fp32 ? 2 : 4, true, true, false, fp32 ? kTiledBlockFp32 : kBlockThreads, kTileBytes, fp32 ? 0 : kTailEvery, false};
    case SpmvRoute::Lean: return {wide, 1, 4, false, true, false, kBlockThreads, 0, kTailEvery, false};
    case SpmvRoute::NarrowTiled: return {1, 2, 4, true, false, false, kBlockThreads, kTileBytes, 0, false};
    default: return {1, 2, 4, true, false, false, kBlockThreads, 0, 0, false};
    }
}
constexpr int groupRows(const SlabShape& s) { return kRulesWave / s.ph * s.rpl; } /* rows of a wavefront */
constexpr int wideGroupRows(size_t elemBytes) { return groupRows(slabShape(SpmvRoute::Wide, elemBytes)); }
inline unsigned slabGrid(const SlabShape& s, int rows) { return (unsigned)ceilDiv(ceilDiv(rows, groupRows(s)), s.block / kRulesWave); }

/* SWEEP: kSweepLaneRows rows per lane (kSweepPacks16 packs for 16-byte elements).  8-byte elements add in the order of their Wide kernel
 * (whole-wave tail rows), the others in one phase. */
struct SweepShape { int vec, packs; bool tail; };
constexpr SweepShape sweepShape(size_t elemBytes) { return {wideOf(elemBytes), elemBytes == 16 ? kSweepPacks16 : kSweepLaneRows / wideOf(elemBytes), elemBytes == 8}; }
inline unsigned sweepGrid(size_t elemBytes, int rows)
{
    const SweepShape s = sweepShape(elemBytes);
    const long long blocks = ceilDiv(ceilDiv(rows, s.vec), (long long)kBlockThreads * s.packs);
    return (unsigned)(blocks > kSweepMaxBlocks ? kSweepMaxBlocks : blocks);
}
/* The probe walks the groups and stages of the kernel it answers for. */
struct ProbeShape { int rpl, ph, step; };
constexpr ProbeShape probeShape(const SlabShape& s) { return {s.rpl, s.ph, s.ph * s.unroll}; }

/* ---- votes ---- */
struct FormCounts { int gathers, strips, local, sweeps; };
constexpr FormCounts countForms(int said0, int said1, int said2)
{
    FormCounts c{0, 0, 0, 0};
    for (int said : {said0, said1, said2}) {
        c.gathers += said == 1;
        c.strips += said == 2;
        c.local += said == 3;
        c.sweeps += said == 4;
    }
    return c;
}
/* What AUTO (or the caller's form) decided for rows as they come: the strip-capable kernel; AUTO's x tile; AUTO's SWEEP form; the probe
 * in front of this launch (its answer is for later calls). */
struct FormVote { bool strips, autoTile, autoSweep, probeBehind; };
/* Does the call vote at all?  Wide layout, more than one row per lane, no x tile asked for. */
constexpr bool votes(int form, bool wideOk, size_t elemBytes) { return wideOk && wideOf(elemBytes) > 1 && form != kFormXtile; }
constexpr FormVote fixedVote(int form, bool wideOk, size_t elemBytes) { return {votes(form, wideOk, elemBytes) && form == kFormStrips, false, false, false}; }
/* Two of three samples decide: scattered -> gathers; inside a window -> the LDS tile; otherwise (strips, or nothing known yet) the
 * strip-capable kernel, which reports itself.  SWEEP: scattered over all of x, ascending inside the rows, rows about equally long (only
 * the probe says so) -- same bits as the Wide kernel of the 8-byte types; it needs rows for a resident grid.  The other forms do not
 * report: with their first call (whether "neither strips nor window" is a matrix for SWEEP only the probe finds out) and every fourth
 * three wavefronts look at the matrix again -- another one may live at this address by now.  calls: as spgpuFormFeedback counts them. */
constexpr FormVote autoVote(const FormCounts& c, int calls, int rows, size_t elemBytes, bool sweepKnob, bool rowOrder)
{
    const bool autoTile = c.local >= 2, strips = c.gathers + c.local + c.sweeps < 2;
    return {strips, autoTile, c.sweeps >= 2 && !autoTile && elemBytes == 8 && sweepKnob && !rowOrder && rows >= kAutoSweepRows,
            !strips && (calls % 4 == 0 || calls == 1)};
}
/* spgpu?SpmvForm: SWEEP where AUTO itself would take it. */
constexpr int formVerdict(const FormCounts& c, size_t elemBytes, int rows)
{
    if (c.sweeps >= 2 && elemBytes == 8 && rows >= kAutoSweepRows)
        return kFormSweep;
    return c.strips >= 2 ? kFormStrips : (c.local >= 2 ? kFormXtile : kFormGather);
}

/* ---- route ---- */
/* SWEEP is the caller's choice for scattered columns that ascend inside a row; it needs 16-byte slab accesses and no row order. */
constexpr int callerForm(int form, bool wideOk, bool rowOrder) { return form == kFormSweep && (!wideOk || rowOrder) ? (int)kFormAuto : form; }

struct SpmvChoice {
    SpmvRoute route;
    int noted;            /* what spgpuGetLastSpmvForm reports */
    bool strips, packed;  /* Wide only */
};
/* form: callerForm's; vote: fixedVote's or, under AUTO where the call votes, autoVote's.  Lean: the caller says the rows
 * are short (avgNnzPerRow: the reference's own tuning hint, hell_spmv_base_template.cuh:306-325) -- such a row is one stage; ELL says how
 * long its longest row is: beyond two stages the prefetching kernel stays, whatever the average; HELL has only the hint.  frozen: the
 * matrix has a 16-bit index copy (asked only where the route is Wide without it: the lookup counts a use). */
constexpr SpmvChoice chooseRoute(int form, bool wideOk, size_t elemBytes, bool isHell, const FormVote& vote, int avgNnzPerRow, int maxNnz, bool frozen)
{
    const bool tiled = form == kFormXtile || vote.autoTile;
    const int byVote = vote.strips ? kFormStrips : kFormGather;
    if (form == kFormSweep || vote.autoSweep)
        return {SpmvRoute::Sweep, kFormSweep, false, false};
    if (!wideOk || wideOf(elemBytes) == 1)
        return {tiled ? SpmvRoute::NarrowTiled : SpmvRoute::Narrow, tiled ? kFormXtile : byVote, false, false};
    if (tiled)
        return {SpmvRoute::Tiled, kFormXtile, false, false};
    if (elemBytes == 8 && avgNnzPerRow > 0 && avgNnzPerRow <= kLeanMaxHint && form == kFormAuto && (isHell || maxNnz <= kLeanMaxEll))
        return {SpmvRoute::Lean, kFormGather, false, false};
    return {SpmvRoute::Wide, byVote, vote.strips, frozen};
}

} // namespace spgpu
