#pragma once
/*
 * How the sparse triangular solve (trsv_device.hip) cuts the list of levels into launches.  Plain host C++17, no HIP header: the
 * rule compiles and runs on its own (tests/trsv_rules_cases.cpp).
 *
 * levelPtrHost[0 .. levelsCount] is the Plan's host array: level l holds the rows rowOrder[levelPtrHost[l] .. levelPtrHost[l + 1]).
 *   plain    every level is a launch of its own, grid-strided over its rows;
 *   chained  a level of more than kTrsvChainWidth rows is a launch of its own, as in plain; a MAXIMAL run of consecutive levels of at
 *            most kTrsvChainWidth rows each is ONE launch of ONE workgroup, which walks its levels with a barrier between them.
 * Every level belongs to exactly one segment, and the segments come in the order of the levels: stream order between launches is
 * the only ordering between workgroups.
 */
namespace spgpu {

constexpr int kTrsvThreads = 256;
/* one workgroup-stride: a chained level gives every lane at most one row */
constexpr int kTrsvChainWidth = kTrsvThreads;
constexpr int kTrsvMaxBlocks = 1048576;

enum { SPGPU_TRSV_SOLVE_PLAIN = 0, SPGPU_TRSV_SOLVE_CHAINED = 1 };

struct TrsvSegment {
    int firstLevel; /* levels [firstLevel, firstLevel + levels) */
    int levels;
    bool chained;   /* one workgroup walks them; otherwise levels == 1 and the launch is grid-strided */
};

inline bool trsvNarrow(const int* levelPtrHost, int level, int width)
{
    return (long long)levelPtrHost[level + 1] - levelPtrHost[level] <= width;
}

/* f(TrsvSegment) for every segment, in order.  levelsCount <= 0: nothing. */
template <typename F> inline void forEachTrsvSegment(const int* levelPtrHost, int levelsCount, int solve, int width, F&& f)
{
    int l = 0;
    while (l < levelsCount) {
        if (solve != SPGPU_TRSV_SOLVE_CHAINED || !trsvNarrow(levelPtrHost, l, width)) {
            f(TrsvSegment{l, 1, false});
            ++l;
            continue;
        }
        int end = l + 1;
        while (end < levelsCount && trsvNarrow(levelPtrHost, end, width))
            ++end;
        f(TrsvSegment{l, end - l, true});
        l = end;
    }
}

/* workgroups of a plain launch over `rows` rows: one per kTrsvThreads rows, maxBlocks (> 0) or kTrsvMaxBlocks at most */
inline unsigned trsvGrid(long long rows, int maxBlocks)
{
    const long long cap = maxBlocks > 0 ? (long long)maxBlocks : (long long)kTrsvMaxBlocks;
    const long long blocks = (rows + kTrsvThreads - 1) / kTrsvThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

} // namespace spgpu
