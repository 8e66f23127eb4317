#pragma once
/*
 * Where the ELL / HELL SpMV for rows ORDERED BY LENGTH (rIdx given: launchOrdered in ellpack_spmv.hip, launchRagged in ragged_spmv.hip.h,
 * launchPlanned / startPlan / packPlan in planned_spmv.hip, freezeSlab in frozen_slab.hip.h) chooses its launches: which queue kernel
 * runs, over which grid, how a plan's buffer is laid out, when a matrix gets a plan and when a 16-bit index copy -- each rule once.
 * Plain host C++17, no HIP header: the rules compile and run on their own (tests/ordered_dispatch_cases.cpp).
 *
 * raggedSpmvKernel<T, RPL, IS_HELL, UNROLL, WAVES, TILE_BYTES, SUBS, DEEP, ZBYTES, PLAN, PACKED>; RPL = WIDE = 16 / sizeof(T), UNROLL =
 * raggedUnroll(RPL), DEEP is true everywhere; a workgroup of WAVES wavefronts owns SUBS sub-groups of kSubRows rows.
 *
 * shape (queueShape)  taken when                                                      WAVES TILE_BYTES SUBS ZBYTES  rows per workgroup  plan
 *   gather            the caller asked for plain gathers (form GATHER), any type      4     0          16   0       512                 yes
 *   tiled             every other form; SPGPU_RAGGED_SHAPE 0 and the probe did not    8     65536      32   0       1 024               yes
 *                     say "windows" (orderedShapeSaid), or complex fp64, or no row
 *                     order, or (shape not 4) a stream without a deep list
 *   tiled, knob       SPGPU_RAGGED_SHAPE neither 0 nor 4 on a stream with a deep      8     65536      32   0       1 024               never
 *                     list: the same kernel, registered in the deep list (plannable)
 *   staged            4- and 8-byte types, tiled form, SPGPU_RAGGED_SHAPE 4 or the    8     49152      64   17408   2 048               yes
 *                     probe's word 4 or 6 (stagedShape)
 * PLAN: the matrix has a READY plan (or, on a stream without a deep list, none at all: planBlocks NULL); its grid is planGrid, the
 * workgroups of deep sub-groups at every planDeepStride-th place.  PACKED: the plan has a 16-bit index copy (mayPack: tiled and staged
 * shapes of the 4- and 8-byte types).  Without a plan the grid is queueGrid and, where deepKernelsFollow, the deep kernels run behind it.
 * planBlocksKernel<IS_HELL, SUBS> / planPackKernel<IS_HELL, SUBS> analyse and pack in blocks of the shape's SUBS (withPlanSubs).
 */
#include "spmv_rules.h" /* kRulesWave; level1_grid.h: wideOf, ceilDiv */

namespace spgpu {

constexpr int kSubRows = 32;      /* rows of a sub-group: what one wavefront of the queue kernel takes from the queue */
constexpr int kPlanDeepMost = 8;  /* deep sub-groups one batch of wholeSubgroups holds (deep_rows.hip.h: their tables live in LDS) */
constexpr int kStagedShape = 4;   /* SPGPU_RAGGED_SHAPE's and the probe's name of the staged shape; 0 is the default */

/* ---- kernel shapes ---- */
struct QueueShape { int waves, tileBytes, subs, zBytes; }; /* raggedSpmvKernel's WAVES, TILE_BYTES, SUBS, ZBYTES */
constexpr QueueShape kGatherQueue{4, 0, 16, 0}, kTiledQueue{8, 65536, 32, 0}, kStagedQueue{8, 49152, 64, 17408};
/* 2 048 rows per workgroup, results staged by destination.  (16-byte elements: tile + staging leave room for one workgroup per CU --
 * they keep the tiled shape.) */
constexpr bool stagedShape(size_t elemBytes, bool tiled, int shape) { return tiled && elemBytes <= 8 && shape == kStagedShape; }
constexpr QueueShape queueShape(size_t elemBytes, bool tiled, int shape)
{
    return !tiled ? kGatherQueue : (stagedShape(elemBytes, tiled, shape) ? kStagedQueue : kTiledQueue);
}
constexpr int rowsPerWorkgroup(const QueueShape& s) { return s.subs * kSubRows; }

/* ---- the stage, and the chunks of a split sub-group ---- */
/* wave-wide loads per stage; 3 keeps the 8-byte kernels at 112 VGPRs (4 wavefronts per SIMD: two 8-wavefront workgroups per CU) with two stages in flight */
constexpr int raggedUnroll(int rpl) { return rpl >= 4 ? 2 : 3; }
/* slab columns per stage: PH = 64 / (32 / RPL) phases, raggedUnroll loads each */
constexpr int queueStep(size_t elemBytes) { return kRulesWave / (kSubRows / wideOf(elemBytes)) * raggedUnroll(wideOf(elemBytes)); }
/* Most chunks a split sub-group may have: what the tightest tiled shape -- the staged one, 48 KiB of LDS behind 2 048 rows -- can park
 * when every one of its sub-groups is split.  fp64 / complex fp32: 3, fp32: 6, complex fp64: 1 (never split). */
constexpr int raggedMostChunks(size_t elemBytes) { return kStagedQueue.tileBytes / (int)elemBytes / rowsPerWorkgroup(kStagedQueue); }
constexpr int kRaggedSplitColumns = 96;
/* Columns per chunk of a split sub-group (raggedSpmvKernel, SPLIT): about 96 (8 stages of the 8-byte kernels), and large
 * enough that the chunk sums of a workgroup whose sub-groups are ALL deepCap deep -- the hacks of set-aside long rows -- fit
 * behind the x tile, which is of no use to such a workgroup anyway.  The SAME value for every shape and form (the sums must not
 * depend on which of them AUTO takes): tests/oracle_api.py ragged_split restates this.  asked: SPGPU_RAGGED_SPLIT. */
constexpr int raggedSplit(size_t elemBytes, int deepCap, int asked)
{
    const int most = raggedMostChunks(elemBytes), step = queueStep(elemBytes);
    if (most < 2 || deepCap <= 0 || asked == 0)
        return 0;
    const int want = (int)(ceilDiv(asked > 0 ? asked : kRaggedSplitColumns, step) * step);
    const int need = (int)(ceilDiv(ceilDiv(deepCap, most), step) * step);
    return want > need ? want : need;
}

/* ---- grids ---- */
constexpr long long subGroupsOf(int rows) { return ceilDiv(rows, kSubRows); }
inline unsigned queueGrid(int rows, int subs) { return (unsigned)ceilDiv(subGroupsOf(rows), subs); } /* without a plan; a plan's planMainBlocks */
inline unsigned planDeepBlocks(int deep) { return (unsigned)ceilDiv(deep, kPlanDeepMost); }
inline unsigned planGrid(int mainBlocks, int deep) { return (unsigned)mainBlocks + planDeepBlocks(deep); }
constexpr int kPlanDeepReachPct = 60;
/* The workgroups of deep sub-groups spread over the first 60 % of the grid, one at every planDeepStride-th place (0: there are none).
 * Odd: the hardware deals workgroup ids round-robin over the 8 XCDs -- with an even stride the long-lived workgroups would pile up on
 * one or two of them (measured: stride 8, 0.73 -> 0.94 ms, one XCD still busy 250 us after the others).  In the grid: stride <=
 * 1.5 x (reach / deepBlocks) when that is >= 1, so (deepBlocks - 1) x stride < 1.5 x reach <= 0.9 x grid; below that the stride is 1
 * and the grid holds deepBlocks places. */
inline int planDeepStride(unsigned grid, unsigned deepBlocks)
{
    if (deepBlocks == 0u)
        return 0;
    const unsigned long long reach = (unsigned long long)grid * kPlanDeepReachPct / 100ull;
    const unsigned stride = (unsigned)(reach / deepBlocks);
    return (int)(stride < 1u ? 1u : (stride | 1u));
}

/* ---- a plan's device buffer: SpgpuPlanBlock[blocks] | int counts[blocks] | int deepSubs[sub-groups], each part on a 16-byte boundary ---- */
constexpr size_t kPlanRecordBytes = 32; /* sizeof(SpgpuPlanBlock) (spgpu_internal.h); planned_spmv.hip asserts it */
constexpr size_t roundUpTo(size_t v, size_t unit) { return (v + unit - 1) / unit * unit; }
struct PlanLayout { size_t blockBytes, countBytes, listBytes, total; }; /* counts at blockBytes, deepSubs at blockBytes + countBytes */
constexpr PlanLayout planLayout(long long blocks, long long subGroups, size_t recordBytes)
{
    const size_t blockBytes = roundUpTo((size_t)blocks * recordBytes, 16), countBytes = roundUpTo((size_t)blocks * sizeof(int), 16);
    const size_t listBytes = (size_t)subGroups * sizeof(int);
    return {blockBytes, countBytes, listBytes, blockBytes + countBytes + listBytes};
}

/* ---- the ordered path's decisions (launchOrdered, launchPlanned) ---- */
/* orderedProbeKernel's word: 4 the staged shape, 6 the same (the blocks are the windows of an aligned order); anything else the default */
constexpr int orderedShapeSaid(int said) { return said == 4 || said == 6 ? kStagedShape : 0; }
/* The probe runs until it has answered, and again with every 64th call: another matrix may live at this address by now. */
constexpr bool reprobe(int said, int calls) { return said == 0 || calls % 64 == 0; }
/* Is the shape the probe's to say?  SPGPU_RAGGED_SHAPE unset, the tiled form, a row order, a type that has the staged shape. */
constexpr bool probesShape(int knob, bool tiled, bool rowOrder, size_t elemBytes) { return knob == 0 && tiled && rowOrder && elemBytes <= 8; }
/* knob: SPGPU_RAGGED_SHAPE; probed: orderedShapeSaid's answer (read only where probesShape).  A stream without a deep list runs from a
 * plan or stateless, and only the shapes a plan can have do that. */
constexpr int orderedShapeFor(int knob, bool tiled, bool rowOrder, size_t elemBytes, int probed, bool noDeepList)
{
    const int shape = probesShape(knob, tiled, rowOrder, elemBytes) ? probed : knob;
    return noDeepList && shape != kStagedShape ? 0 : shape;
}
constexpr bool plannable(bool tiled, int shape) { return !tiled || shape == 0 || shape == kStagedShape; }
/* ELL says how long its longest row is: when none can exceed the cap nothing registers and the two launches behind the main
 * kernel (~5 us each when empty) are left out; HELL does not say */
constexpr bool deepKernelsFollow(bool isHell, int maxNnz, int deepCap) { return isHell || maxNnz > deepCap; }
constexpr int planSubs(size_t elemBytes, bool tiled, int shape) { return queueShape(elemBytes, tiled, shape).subs; }
/* raggedSpmvKernel<..., PACKED> exists for the tiled shapes of the 4- and 8-byte types; a plan of theirs may get the 16-bit copy */
constexpr bool packedKernels(bool tiled, size_t elemBytes) { return tiled && elemBytes <= 8; }
constexpr bool mayPack(bool tiled, size_t elemBytes, int subs) { return packedKernels(tiled, elemBytes) && (subs == kStagedQueue.subs || subs == kTiledQueue.subs); }
/* A matrix that keeps changing under a young plan is left alone after the third time. */
constexpr bool planGivesUp(int uses, int stales) { return uses < 16 && stales >= 3; }
/* A plan's sub-groups per block as a constant: f(std::integral_constant<int, SUBS>) over the shapes' values (GATHER_TOO: all three;
 * else the two that can be packed). */
template <bool GATHER_TOO, typename F> inline void withPlanSubs(int subs, F&& f)
{
    if (subs == kStagedQueue.subs)
        return f(std::integral_constant<int, kStagedQueue.subs>{});
    if constexpr (GATHER_TOO) {
        if (subs == kGatherQueue.subs)
            return f(std::integral_constant<int, kGatherQueue.subs>{});
    }
    f(std::integral_constant<int, kTiledQueue.subs>{});
}

/* ---- freeze: the 16-bit copy of the column indices (packPlan, freezeSlab) ---- */
/* (a lane's last pack may reach past the last real slot's word: whole 256-byte lines) */
constexpr size_t packedBytes(long long slots) { return roundUpTo((size_t)slots * sizeof(unsigned short), 256); }
/* Scattered columns: the copy would save nothing (an escape costs its rP word on top of the 16-bit one).  Kept with at most pct
 * escapes in a hundred entries (SPGPU_FREEZE_MAX_ESCAPES_PCT; below 0 counts as 0). */
constexpr bool keepsCopy(unsigned long long entries, unsigned long long escapes, int pct)
{
    return escapes * 100ull <= entries * (unsigned long long)(pct < 0 ? 0 : pct);
}

} // namespace spgpu
