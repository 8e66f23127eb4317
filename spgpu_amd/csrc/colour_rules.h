#pragma once
/*
 * The launch rules of the multicolour ordering (colour_device.hip).  Plain host C++17, no HIP header: the rules compile and run on
 * their own (tests/colour_rules_cases.cpp).
 *
 * SHAPES.  A shape is the number of lanes that own a row in a round of the colouring and in the fill of the permutation:
 * SPGPU_COLOUR_SHAPE_THREAD (1) -- one thread walks the row -- or a GROUP of L lanes of one wavefront, L a power of two in [2, 64]:
 * lane l takes the entries of the row at positions = l (mod L); the round combines the lanes' readiness (AND) and colour masks (OR)
 * with lane shuffles.  AND, OR and "lowest zero bit" are exact, so every shape gives the same bytes.
 *
 * THE RULE is the project's: tools/bench_colour.py times every shape on the 7-point matrix of a 200^3 grid (mean row length 6.97)
 * and on the 27-point matrix of a 100^3 grid (26.46) and writes profiles/csr_colour_ab.json; a shape counts as fastest only when
 * its min-max range lies below that of every other shape, and THREAD is the fallback.  MEASURED on an MI355X, fp64, one run:
 *   the colouring (all rounds, one synchronise each)   THREAD / GROUP 8 / 32 / 64
 *     7-point, 21 rounds     32.7 / 162.0 / 344.0 / 348.2 ms
 *     27-point, 61 rounds    18.3 /  64.6 / 165.0 / 235.7 ms
 *   THREAD wins on both with ranges far apart: after the first rounds most rows are coloured and only copy their colour, and a
 *   GROUP spends L lanes on such a row.  So the thresholds that ILU(0) has (ilu0_rules.h) are NOT taken over: the colouring runs
 *   THREAD at both measured means, and beyond them nothing is measured, where THREAD is the fallback anyway.  colourShape keeps its
 *   arguments for a later measurement on longer rows; the public call does not need rowPtr[rows] and does not read it.
 *   the permutation (lengths, scan, fill)              THREAD / GROUP 8 / 32 / 64
 *     7-point                 6.01 / 1.05 / 3.02 / 5.19 ms
 *     27-point                9.94 / 0.99 / 0.79 / 1.41 ms
 *   The permutation is asynchronous and cannot read rowPtr[rows], so it has ONE FIXED shape for every matrix.  GROUP 8 and GROUP 32
 *   both lie below THREAD on both matrices with ranges apart; GROUP 8 is the fastest on the 7-point matrix and 0.20 ms behind
 *   GROUP 32 on the 27-point one, GROUP 32 is 1.97 ms behind on the 7-point one: kColourPermuteShape is 8.
 *
 * GRID.  A launch over r rows of a shape of L lanes has ceil(r * L / kColourThreads) workgroups, maxBlocks (> 0) or kCsrMaxBlocks
 * at most, and at least one (cappedGrid of csr_host.h); the kernels stride over the rest.
 */
#include "csr_host.h"

namespace spgpu {

constexpr int kColourThreads = 256;

constexpr int SPGPU_COLOUR_SHAPE_THREAD = 1;
constexpr int kColourMaxGroup = 64; /* one wavefront */

/* the permutation's one shape (measured, above) */
constexpr int kColourPermuteShape = 8;

inline bool colourShapeKnown(int shape)
{
    return shape >= 1 && shape <= kColourMaxGroup && (shape & (shape - 1)) == 0;
}

/* the colouring's shape for a matrix of `rows` rows and `nnz` stored entries: THREAD, measured at means 6.97 and 26.46 and the
 * fallback everywhere else */
inline int colourShape(long long nnz, int rows)
{
    (void)nnz;
    (void)rows;
    return SPGPU_COLOUR_SHAPE_THREAD;
}

/* workgroups of a launch over `rows` rows of `shape` lanes each */
inline unsigned colourGrid(long long rows, int shape, int maxBlocks)
{
    return cappedGrid(rows * shape, kColourThreads, maxBlocks);
}

} // namespace spgpu
