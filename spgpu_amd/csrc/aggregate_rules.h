#pragma once
/*
 * The launch rules of the aggregation (aggregate_device.hip).  Plain host C++17, no HIP header: the rules compile and run on their
 * own (tests/aggregate_rules_cases.cpp).
 *
 * SHAPES.  A shape is the number of lanes that own a row in the max-propagation sweeps of a round and in the mask pass of the
 * strength call: SPGPU_AGG_SHAPE_THREAD (1) -- one thread walks the row -- or a GROUP of L lanes of one wavefront, L a power of two
 * in [2, 64]: lane l takes the entries of the row at positions = l (mod L), and the sweeps combine the lanes' maxima with lane
 * shuffles.  max is exact, so every shape gives the same bytes.  The public calls pick the shape from the MEAN number of stored
 * entries per row, nnz / rows, compared in integers:
 *   mean <= kAggThreadMaxMean  THREAD
 *   mean <= kAggNarrowMaxMean  GROUP of kAggGroupNarrow lanes
 *   otherwise                  GROUP of kAggGroupWide lanes
 *
 * GRID.  A launch over r rows of a shape of L lanes has ceil(r * L / kAggThreads) workgroups, maxBlocks (> 0) or kTrsvMaxBlocks at
 * most, and at least one; the kernels stride over the rest.
 */
#include "ilu0_rules.h"

namespace spgpu {

constexpr int kAggThreads = kTrsvThreads;

constexpr int SPGPU_AGG_SHAPE_THREAD = 1;
constexpr int kAggMaxGroup = 64; /* one wavefront */

/* The thresholds and the two widths.  NOT MEASURED: nobody has timed these kernels on an MI355X.  They are ILU(0)'s, taken over as
 * they stand (ilu0_rules.h, where profiles/csr_ilu0_ab.json backs them for the factorisation): the sweeps walk the same rows in the
 * same two shapes, but they gather one 8-byte word per entry and bisect nothing, so the crossovers need not coincide.  The shipping
 * rule is the project's: tools/bench_aggregate.py times every shape on the 7-point matrix of a 200^3 grid and on the 27-point
 * matrix of a 100^3 grid and writes profiles/csr_aggregate_ab.json; a shape counts as fastest only when its min-max range lies
 * below that of every other shape, and THREAD is the fallback.  Until that file exists these numbers are a starting point, not a
 * finding. */
constexpr int kAggGroupNarrow = kIlu0GroupNarrow;
constexpr int kAggGroupWide = kIlu0GroupWide;
constexpr int kAggThreadMaxMean = kIlu0ThreadMaxMean;
constexpr int kAggNarrowMaxMean = kIlu0NarrowMaxMean;

inline bool aggShapeKnown(int shape)
{
    return shape >= 1 && shape <= kAggMaxGroup && (shape & (shape - 1)) == 0;
}

/* the public calls' shape for a matrix of `rows` rows and `nnz` stored entries; rows <= 0 or nnz < 0 (no such matrix): THREAD */
inline int aggShape(long long nnz, int rows)
{
    if (rows <= 0 || nnz <= (long long)kAggThreadMaxMean * rows)
        return SPGPU_AGG_SHAPE_THREAD;
    return nnz <= (long long)kAggNarrowMaxMean * rows ? kAggGroupNarrow : kAggGroupWide;
}

/* workgroups of a launch over `rows` rows of `shape` lanes each */
inline unsigned aggGrid(long long rows, int shape, int maxBlocks)
{
    return trsvGrid(rows * shape, maxBlocks);
}

} // namespace spgpu
