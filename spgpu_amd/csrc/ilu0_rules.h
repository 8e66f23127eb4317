#pragma once
/*
 * The launch rules of the ILU(0) factorisation (ilu0_device.hip).  Plain host C++17, no HIP header: the rules compile and run on
 * their own (tests/ilu0_rules_cases.cpp).
 *
 * SEGMENTS.  The list of levels is cut into launches by forEachTrsvSegment of trsv_rules.h, with the factorisation's own width:
 *   plain    every level is a launch of its own, grid-strided over its rows;
 *   chained  a level of more than kIlu0ChainWidth rows is a launch of its own; a MAXIMAL run of consecutive levels of at most
 *            kIlu0ChainWidth rows each is ONE launch of ONE workgroup, which walks its levels with a barrier between them.
 *
 * SHAPES.  A shape is the number of lanes that own a row: SPGPU_ILU0_SHAPE_THREAD (1) -- one thread walks row k's upper part and its
 * own row with two pointers -- or a GROUP of L lanes of one wavefront, L a power of two in [2, 64]: lane l owns the entries of the row
 * at positions = l (mod L) and bisects row k's upper part for their columns.  Every shape gives the same bytes.  The public call
 * picks the shape from the MEAN number of stored entries per row, nnz / rows, compared in integers:
 *   mean <= kIlu0ThreadMaxMean  THREAD
 *   mean <= kIlu0NarrowMaxMean  GROUP of kIlu0GroupNarrow lanes
 *   otherwise                   GROUP of kIlu0GroupWide lanes
 */
#include "trsv_rules.h"

namespace spgpu {

constexpr int kIlu0Threads = kTrsvThreads;
/* one workgroup-stride of the THREAD shape: a chained level gives every lane at most one row */
constexpr int kIlu0ChainWidth = kIlu0Threads;

constexpr int SPGPU_ILU0_SHAPE_THREAD = 1;
constexpr int kIlu0GroupNarrow = 8;
constexpr int kIlu0GroupWide = 32;
constexpr int kIlu0MaxGroup = 64; /* one wavefront */

/* The thresholds.  The rule: the public call runs, on the 7-point matrix of a 200^3 grid (mean 6.97) and on the 27-point matrix of a
 * 100^3 grid (mean 26.46), the leg that tools/bench_ilu0.py measured fastest, a leg counting as fastest only when its min-max range
 * lies below that of every other leg; THREAD / plain is the fallback.  On an MI355X, fp64, one launch per level
 * (profiles/csr_ilu0_ab.json): 7-point THREAD 13.55 ms, GROUP 8 6.83 ms (6.78-6.85), GROUP 32 8.99 ms; 27-point
 * THREAD 98.0 ms, GROUP 8 33.3 ms, GROUP 32 20.41 ms (20.36-20.43).  So the second threshold lies between the two means: it is the
 * measured one.  The first is NOT a measured crossover but the fallback's place: THREAD keeps the matrices with at most one
 * off-diagonal entry per row, the only kind on which no GROUP beat it (bidiagonal, mean 2.0: 284 / 289 / 299 ms with ranges of
 * 279-359 that overlap, and launches, not the row shape, dominate there).  The 5-point matrix of a 1024^2 grid (mean 5.0) ran faster
 * with 32 lanes than with the 8 this rule gives it (11.30 against 12.19 ms): its levels are narrow, which a rule on the mean row
 * length cannot see. */
constexpr int kIlu0ThreadMaxMean = 2;
constexpr int kIlu0NarrowMaxMean = 16;

inline bool ilu0ShapeKnown(int shape)
{
    return shape >= 1 && shape <= kIlu0MaxGroup && (shape & (shape - 1)) == 0;
}

/* the public call's shape for a matrix of `rows` rows and `nnz` stored entries; rows <= 0 or nnz < 0 (no such matrix): THREAD */
inline int ilu0Shape(long long nnz, int rows)
{
    if (rows <= 0 || nnz <= (long long)kIlu0ThreadMaxMean * rows)
        return SPGPU_ILU0_SHAPE_THREAD;
    return nnz <= (long long)kIlu0NarrowMaxMean * rows ? kIlu0GroupNarrow : kIlu0GroupWide;
}

/* workgroups of a plain launch over `rows` rows of `shape` lanes each */
inline unsigned ilu0Grid(long long rows, int shape, int maxBlocks)
{
    return trsvGrid(rows * shape, maxBlocks);
}

} // namespace spgpu
