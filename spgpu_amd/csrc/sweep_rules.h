#pragma once
/*
 * The launch rules of the multicolour sweep and of the residual on CSR arrays (sweep_device.hip).  Plain host C++17, no HIP header:
 * the rules compile and run on their own (tests/sweep_rules_cases.cpp).
 *
 * PASSES.  A sweep is a list of colour passes: FORWARD the colours 0 .. C-1, BACKWARD the colours C-1 .. 0, SYMMETRIC the forward
 * list and then the backward list -- two lists, each cut on its own, so a symmetric sweep launches what the two calls launch, in
 * that order.  The reversed list is handed to the rule as a pointer array of its own: reversed[k] = rows - colourPtrHost[C - k], so
 * that its level k is colour C - 1 - k (sweepReversed).
 *
 * SEGMENTS.  A list is cut into launches by forEachTrsvSegment of trsv_rules.h, unchanged, with the sweep's own width:
 *   plain    every colour is a launch of its own, grid-strided over its rows;
 *   chained  a colour of more than kSweepChainWidth rows is a launch of its own; a MAXIMAL run of consecutive colours of at most
 *            kSweepChainWidth rows each is walked by ONE workgroup with a barrier between colours.  The sweep call has no device
 *            copy of colourPtr (it reads colourPtrHost at call time), so the bounds of a run travel as kernel arguments, at most
 *            kSweepChainPasses colours a launch: a run of n colours is ceil(n / kSweepChainPasses) launches (sweepChainLaunches),
 *            one for every matrix with at most kSweepChainPasses narrow colours in a row.
 *
 * SHAPES.  A shape is the number of lanes that own a row: SPGPU_SWEEP_SHAPE_THREAD (1), or a GROUP of L lanes of one wavefront, L a
 * power of two in [2, 64].  Every shape gives the same bytes.  The public calls pick the shape from the MEAN number of stored
 * entries per row, entriesCount / rowsCount, compared in integers, by the rule of ilu0Shape (ilu0_rules.h) WITH ITS TWO THRESHOLDS:
 * they are ILU(0)'s, taken over as they stand and NOT MEASURED for these kernels (tools/bench_sweep.py is the run that would move
 * them).
 */
#include "ilu0_rules.h"

namespace spgpu {

constexpr int kSweepThreads = kTrsvThreads;
/* one workgroup-stride of the THREAD shape: a chained colour gives every lane at most one row */
constexpr int kSweepChainWidth = kSweepThreads;
/* the colours one chained launch can walk: their bounds are kernel arguments (SweepBounds of sweep_device.hip) */
constexpr int kSweepChainPasses = 64;

constexpr int SPGPU_SWEEP_SHAPE_THREAD = 1;
constexpr int kSweepGroupNarrow = kIlu0GroupNarrow;
constexpr int kSweepGroupWide = kIlu0GroupWide;
constexpr int kSweepMaxGroup = 64; /* one wavefront */
/* ILU(0)'s thresholds, unmeasured here (head of the file) */
constexpr int kSweepThreadMaxMean = kIlu0ThreadMaxMean;
constexpr int kSweepNarrowMaxMean = kIlu0NarrowMaxMean;

/* the codes of include/spgpu/ext/sweep_device.h (which needs HIP; sweep_device.hip checks that they are the same) */
enum { kSweepForward = 0, kSweepBackward = 1, kSweepSymmetric = 2 };

inline bool sweepShapeKnown(int shape)
{
    return shape >= 1 && shape <= kSweepMaxGroup && (shape & (shape - 1)) == 0;
}

inline bool sweepDirectionKnown(int direction)
{
    return direction == kSweepForward || direction == kSweepBackward || direction == kSweepSymmetric;
}

/* the public calls' shape for a matrix of `rows` rows and `nnz` stored entries; rows <= 0 or nnz < 0 (no such matrix): THREAD */
inline int sweepShape(long long nnz, int rows)
{
    if (rows <= 0 || nnz <= (long long)kSweepThreadMaxMean * rows)
        return SPGPU_SWEEP_SHAPE_THREAD;
    return nnz <= (long long)kSweepNarrowMaxMean * rows ? kSweepGroupNarrow : kSweepGroupWide;
}

/* workgroups of a plain launch over `rows` rows of `shape` lanes each */
inline unsigned sweepGrid(long long rows, int shape, int maxBlocks)
{
    return trsvGrid(rows * shape, maxBlocks);
}

/* reversed[0 .. coloursCount]: the pointer array of the colours in descending order */
inline void sweepReversed(int* reversed, const int* colourPtrHost, int coloursCount)
{
    const int rows = colourPtrHost[coloursCount];
    for (int k = 0; k <= coloursCount; ++k)
        reversed[k] = rows - colourPtrHost[coloursCount - k];
}

/* launches of a chained run of `colours` narrow colours */
inline int sweepChainLaunches(int colours)
{
    return (colours + kSweepChainPasses - 1) / kSweepChainPasses;
}

struct SweepSegment {
    int firstColour; /* the first colour visited; the segment visits `colours` of them, ascending (step 1) or descending (step -1) */
    int colours;
    int step;
    bool chained;
};

/* f(SweepSegment) for every segment of one list, in the order of the visit.  `list` is colourPtrHost for step 1 and the array of
 * sweepReversed for step -1; every segment names the colours of the matrix, not the places of the list. */
template <typename F> inline void forEachSweepSegment(const int* list, int coloursCount, int step, int solve, F&& f)
{
    forEachTrsvSegment(list, coloursCount, solve, kSweepChainWidth, [&](TrsvSegment g) {
        f(SweepSegment{step > 0 ? g.firstLevel : coloursCount - 1 - g.firstLevel, g.levels, step > 0 ? 1 : -1, g.chained});
    });
}

/* the launches of one list */
inline int sweepLaunches(const int* list, int coloursCount, int solve)
{
    int launches = 0;
    forEachTrsvSegment(list, coloursCount, solve, kSweepChainWidth,
                       [&](TrsvSegment g) { launches += g.chained ? sweepChainLaunches(g.levels) : 1; });
    return launches;
}

} // namespace spgpu
