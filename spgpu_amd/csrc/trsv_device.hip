/*
 * The sparse triangular solve x = T^-1 * b on CSR arrays for gfx950, level-scheduled (include/spgpu/ext/trsv_device.h).  New
 * functionality.  No kernel of this file waits for another workgroup: there is no spin loop and no polled flag.  Rows of one level
 * do not depend on one another; levels are ordered by stream order between launches, or by a barrier inside ONE workgroup.
 *
 * THE PLAN is set-up code: repeated sweeps over the rows that have no level yet, which are kept as a list in ascending order.
 * Sweep k gives level k to every listed row whose dependencies all have a level in [0, k) -- a level written in the same sweep reads
 * as -1 or as k, and both mean "not yet" -- and scans the flags of its tile (trsvSweepKernel); the tile totals are scanned
 * (scanTotalsKernel of convert_scan.hip.h); then the rows that got the level are appended to rowOrder and the others to the next
 * list, both in list order, which is row order (trsvScatterKernel).  So rowOrder comes out sorted by (level, row) without a sort,
 * and levelPtr[k + 1] is written on the way.  The host reads the number of rows left once per sweep.  When at most kTrsvFinishRows
 * rows are left, ONE workgroup finishes them in a loop with barriers (trsvFinishKernel), four list entries per lane.  A sweep that
 * assigns nothing while rows remain cannot happen on a triangle (the first row of the list is always ready); it returns
 * SPGPU_UNSPECIFIED and does not loop.  The first pass (trsvInitKernel) checks every column and counts every row's diagonals.
 * Scratch (ints): misc[16] | level[rows] | listA[rows] | listB[rows] | pos[rows] | scan totals; misc[1] the bad-input flag,
 * misc[2] the rows left, misc[3] the levels so far, misc[4] a round that assigned nothing.
 *
 * THE SOLVES.  One thread per row, the row summed in storage order with contraction off (trsvRow, on exactSubMul and exactDiv of
 * csr_shared.hip.h), so both give the same bytes:
 *   plain    (csrTrsvLevelKernel) one launch per level, grid-strided over the level's part of rowOrder;
 *   chained  (csrTrsvChainKernel) the host rule of trsv_rules.h cuts the level list into segments: a level of more than
 *            kTrsvChainWidth rows is a launch as in plain; a maximal run of narrower levels is ONE launch of ONE workgroup, which
 *            walks its levels with __syncthreads() between them.  The bounds of the level loop come from levelPtr and are uniform,
 *            and the row loop of a level is closed before the barrier, so every thread reaches every barrier.  x written before
 *            the barrier and read behind it goes through global memory at workgroup scope: all wavefronts of a workgroup share
 *            their CU's vector L1, which takes that CU's loads and stores in order, so no cache needs invalidating; and
 *            __syncthreads() is a workgroup-scope release and acquire over all address spaces, global memory included, which
 *            also keeps the compiler from moving a load of x across it.  No further fence.
 */
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"
#include "trsv_rules.h"

#include "spgpu/ext/trsv_device.h"

#include <string.h>

namespace spgpu {

constexpr int kTrsvFinishRows = kScanTile; /* the rows one workgroup finishes: kScanPerThread list entries per lane */
/* The solve the public call runs.  The rule: chained if it is faster on the lower solve of the 200^3 7-point matrix with
 * non-overlapping min-max ranges of the two legs, plain otherwise.  tools/bench_trsv.py on an MI355X, fp64, 8 M rows in 598 levels:
 * chained 5.92-5.94 ms in 556 launches, plain 5.98-6.01 ms in 598; a bidiagonal matrix of 100 000 rows: 72 ms in one launch against
 * 322 ms in 100 000 (profiles/csr_trsv_ab.json). */
constexpr int kTrsvDefaultSolve = SPGPU_TRSV_SOLVE_CHAINED;

struct TrsvWork {
    int* misc;
    int* level;
    int* listA;
    int* listB;
    int* pos;
    int* totals;
};

static size_t trsvWorkInts(int rows) { return (size_t)16 + 4 * alignUpCv((size_t)rows, 64) + alignUpCv(scanBlocks(rows) + 2, 64); }

static TrsvWork carveTrsv(void* work, int rows)
{
    const size_t S = alignUpCv((size_t)rows, 64);
    TrsvWork w;
    w.misc = static_cast<int*>(work);
    w.level = w.misc + 16;
    w.listA = w.level + S;
    w.listB = w.listA + S;
    w.pos = w.listB + S;
    w.totals = w.pos + S;
    return w;
}

/* ---- the plan ---- */
/* level = -1, list = every row; a column outside the matrix or, under STORED, a row with no diagonal or with two raises misc[1] */
__global__ __launch_bounds__(kCvThreads) void trsvInitKernel(int* level, int* list, int* levelPtr, int* misc, int rows, const int* ptr,
                                                              const int* idx, int base, int diag)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        const int e1 = ptr[i + 1] - base;
        int diagonals = 0;
        bool bad = false;
        for (int e = ptr[i] - base; e < e1; ++e) {
            const unsigned c = (unsigned)idx[e] - (unsigned)base;
            bad |= c >= (unsigned)rows;
            diagonals += c == (unsigned)i;
        }
        bad |= diag == SPGPU_TRSV_DIAG_STORED && diagonals != 1;
        if (bad)
            misc[1] = 1;
        level[i] = -1;
        list[i] = (int)i;
        if (i == 0)
            levelPtr[0] = 0;
    }
}

/* every dependency of row r has a level in [0, k); a column outside the matrix is no dependency (the Plan refuses it afterwards) */
__device__ inline bool trsvReady(const int* level, int k, int r, int rows, const int* ptr, const int* idx, int base, int side)
{
    const int e1 = ptr[r + 1] - base;
    for (int e = ptr[r] - base; e < e1; ++e) {
        const unsigned c = (unsigned)idx[e] - (unsigned)base;
        if (c >= (unsigned)rows)
            continue;
        if (side == SPGPU_TRSV_LOWER ? (int)c < r : (int)c > r) {
            const int at = level[c];
            if (at < 0 || at >= k)
                return false;
        }
    }
    return true;
}

/* Sweep k over list[0, remaining), a tile of kScanTile entries per workgroup: level[r] = k where r is ready; pos[t] = the number of
 * ready entries of the tile in front of t; totals[tile] = the tile's number. */
__global__ __launch_bounds__(kCvThreads) void trsvSweepKernel(int* pos, int* totals, int* level, const int* list, int remaining, int k, int rows,
                                                               const int* ptr, const int* idx, int base, int side)
{
    __shared__ int waveTotals[kCvThreads / kWave];
    const long long first = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanPerThread;
    int v[kScanPerThread], mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        v[j] = 0;
        if (first + j < remaining) {
            const int r = list[first + j];
            if (trsvReady(level, k, r, rows, ptr, idx, base, side)) {
                level[r] = k;
                v[j] = 1;
            }
        }
        mine += v[j];
    }
    int total;
    int run = blockExclusiveScan(mine, waveTotals, &total);
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        if (first + j < remaining)
            pos[first + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0)
        totals[blockIdx.x] = total;
}

/* The rows of level k behind rowOrder[done), the others into the next list, both in list order; totals[] scanned, totals[tiles] the
 * number of rows of level k. */
__global__ __launch_bounds__(kCvThreads) void trsvScatterKernel(int* rowOrder, int* levelPtr, int* listOut, int* misc, const int* list,
                                                                 const int* pos, const int* totals, long long tiles, int remaining, const int* level,
                                                                 int k, int done)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long t = (long long)blockIdx.x * kCvThreads + threadIdx.x; t < remaining; t += stride) {
        const int r = list[t];
        const int before = pos[t] + totals[t / kScanTile];
        if (level[r] == k)
            rowOrder[(long long)done + before] = r;
        else
            listOut[t - before] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int assigned = totals[tiles];
        levelPtr[k + 1] = done + assigned;
        misc[2] = remaining - assigned;
    }
}

/* ONE workgroup, remaining <= kTrsvFinishRows: lane t owns list[t * kScanPerThread + j].  Every quantity that steers the loop (left,
 * total) is the same in every thread, so every thread reaches every barrier. */
__global__ __launch_bounds__(kCvThreads) void trsvFinishKernel(int* rowOrder, int* levelPtr, int* level, int* misc, const int* list, int remaining,
                                                                int k, int done, int rows, const int* ptr, const int* idx, int base, int side)
{
    __shared__ int waveTotals[kCvThreads / kWave];
    int r[kScanPerThread];
    unsigned open = 0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        const int t = (int)threadIdx.x * kScanPerThread + j;
        r[j] = t < remaining ? list[t] : 0;
        open |= t < remaining ? 1u << j : 0u;
    }
    int left = remaining, stuck = 0;
    while (left > 0) {
        unsigned ready = 0;
#pragma unroll
        for (int j = 0; j < kScanPerThread; ++j)
            if ((open >> j & 1u) && trsvReady(level, k, r[j], rows, ptr, idx, base, side))
                ready |= 1u << j;
        __syncthreads(); /* every level of this round is read before one is written */
#pragma unroll
        for (int j = 0; j < kScanPerThread; ++j)
            if (ready >> j & 1u)
                level[r[j]] = k;
        int total;
        int at = done + blockExclusiveScan(__popc(ready), waveTotals, &total);
#pragma unroll
        for (int j = 0; j < kScanPerThread; ++j)
            if (ready >> j & 1u)
                rowOrder[at++] = r[j];
        open &= ~ready;
        if (total == 0) {
            stuck = 1;
            break;
        }
        done += total;
        left -= total;
        ++k;
        if (threadIdx.x == 0)
            levelPtr[k] = done;
        __syncthreads(); /* the levels written in this round are read in the next (global memory, workgroup scope) */
    }
    if (threadIdx.x == 0) {
        misc[2] = left;
        misc[3] = k;
        if (stuck)
            misc[4] = 1;
    }
}

/* Row i of the contract.  x and b may be the same array: b[i] is read before x[i] is written, and no other row reads b[i]. */
template <typename T>
__device__ inline void trsvRow(T* x, const T* b, int i, const int* ptr, const int* idx, const T* val, int base, int side, int diag)
{
    T acc = b[i];
    T pivot = zeroOf<T>();
    const int e1 = ptr[i + 1] - base;
    for (int e = ptr[i] - base; e < e1; ++e) {
        const int j = idx[e] - base;
        if (j == i) {
            if (diag == SPGPU_TRSV_DIAG_STORED)
                pivot = val[e];
        } else if (side == SPGPU_TRSV_LOWER ? j < i : j > i) {
            acc = exactSubMul(acc, val[e], x[j]);
        }
    }
    x[i] = diag == SPGPU_TRSV_DIAG_STORED ? exactDiv(acc, pivot) : acc;
}

/* plain: the `count` rows of one level, order[0, count) */
template <typename T>
__global__ __launch_bounds__(kTrsvThreads) void csrTrsvLevelKernel(T* x, const T* b, const int* order, int count, const int* ptr, const int* idx,
                                                                   const T* val, int base, int side, int diag)
{
    const long long stride = (long long)gridDim.x * kTrsvThreads;
    for (long long t = (long long)blockIdx.x * kTrsvThreads + threadIdx.x; t < count; t += stride)
        trsvRow(x, b, order[t], ptr, idx, val, base, side, diag);
}

/* chained: ONE workgroup walks levels [firstLevel, firstLevel + levels) (head of the file) */
template <typename T>
__global__ __launch_bounds__(kTrsvThreads) void csrTrsvChainKernel(T* x, const T* b, const int* rowOrder, const int* levelPtr, int firstLevel,
                                                                   int levels, const int* ptr, const int* idx, const T* val, int base, int side,
                                                                   int diag)
{
    for (int l = firstLevel; l < firstLevel + levels; ++l) {
        const int first = levelPtr[l], last = levelPtr[l + 1];
        for (int t = first + (int)threadIdx.x; t < last; t += kTrsvThreads)
            trsvRow(x, b, rowOrder[t], ptr, idx, val, base, side, diag);
        __syncthreads(); /* the x of this level is read by the next */
    }
}

template <typename T>
static void launchCsrTrsv(hipStream_t s, void* x, const void* b, int levelsCount, const int* rowOrder, const int* levelPtr, const int* levelPtrHost,
                          const int* ptr, const int* idx, const void* val, int base, int side, int diag, int solve, int maxBlocks)
{
    forEachTrsvSegment(levelPtrHost, levelsCount, solve, kTrsvChainWidth, [&](TrsvSegment g) {
        if (g.chained) {
            hipLaunchKernelGGL((csrTrsvChainKernel<T>), dim3(1), dim3(kTrsvThreads), 0, s, static_cast<T*>(x), static_cast<const T*>(b), rowOrder,
                               levelPtr, g.firstLevel, g.levels, ptr, idx, static_cast<const T*>(val), base, side, diag);
            return;
        }
        const int first = levelPtrHost[g.firstLevel], count = levelPtrHost[g.firstLevel + 1] - first;
        hipLaunchKernelGGL((csrTrsvLevelKernel<T>), dim3(trsvGrid(count, maxBlocks)), dim3(kTrsvThreads), 0, s, static_cast<T*>(x),
                           static_cast<const T*>(b), rowOrder + first, count, ptr, idx, static_cast<const T*>(val), base, side, diag);
    });
}

static bool trsvSideAndDiagKnown(int side, int diag)
{
    return (side == SPGPU_TRSV_LOWER || side == SPGPU_TRSV_UPPER) && (diag == SPGPU_TRSV_DIAG_STORED || diag == SPGPU_TRSV_DIAG_UNIT);
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_trsv.py and the tests that compare the two solves.  solve: 0 plain, 1 chained, < 0 the
 * public call's choice; maxBlocks > 0 caps the grid of a level's launch (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrTrsvDeviceWith(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int levelsCount, const int* rowOrder,
                                     const int* levelPtr, const int* levelPtrHost, const int* rowPtr, const int* colIndices, const void* values,
                                     int baseIndex, int side, int diag, spgpuType_t valuesType, int solve, int maxBlocks);
int spgpuCsrTrsvDefaultSolve(void);
int spgpuCsrTrsvChainWidth(void); /* the widest level that the chained solve leaves to one workgroup */

int spgpuCsrTrsvDefaultSolve(void) { return kTrsvDefaultSolve; }
int spgpuCsrTrsvChainWidth(void) { return kTrsvChainWidth; }

size_t spgpuCsrTrsvWorkBytes(int rowsCount) { return trsvWorkInts(rowsCount > 0 ? rowsCount : 0) * sizeof(int) + 256; }

spgpuStatus_t spgpuCsrTrsvPlanDevice(spgpuHandle_t handle, int* levelsCount, int* rowOrder, int* levelPtr, int* levelPtrHost, int rowsCount,
                                     const int* rowPtr, const int* colIndices, int baseIndex, int side, int diag, void* work)
{
    *levelsCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!work || !rowOrder || !levelPtr || !levelPtrHost || !trsvSideAndDiagKnown(side, diag))
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const TrsvWork w = carveTrsv(work, rowsCount);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(w.misc, 0, 16 * sizeof(int), s);
    hipLaunchKernelGGL(trsvInitKernel, dim3(gridFor(rowsCount)), dim3(kCvThreads), 0, s, w.level, w.listA, levelPtr, w.misc, rowsCount, rowPtr,
                       colIndices, baseIndex, diag);
    int *list = w.listA, *next = w.listB;
    int remaining = rowsCount, k = 0;
    while (remaining > 0) { /* every round assigns a row or returns: at most rowsCount rounds */
        const bool finish = remaining <= kTrsvFinishRows;
        if (finish) {
            hipLaunchKernelGGL(trsvFinishKernel, dim3(1), dim3(kCvThreads), 0, s, rowOrder, levelPtr, w.level, w.misc, list, remaining, k,
                               rowsCount - remaining, rowsCount, rowPtr, colIndices, baseIndex, side);
        } else {
            const long long tiles = (long long)scanBlocks(remaining);
            hipLaunchKernelGGL(trsvSweepKernel, dim3((unsigned)tiles), dim3(kCvThreads), 0, s, w.pos, w.totals, w.level, list, remaining, k,
                               rowsCount, rowPtr, colIndices, baseIndex, side);
            hipLaunchKernelGGL(scanTotalsKernel, dim3(1), dim3(kCvThreads), 0, s, w.totals, tiles);
            hipLaunchKernelGGL(trsvScatterKernel, dim3(gridFor(remaining)), dim3(kCvThreads), 0, s, rowOrder, levelPtr, next, w.misc, list, w.pos,
                               w.totals, tiles, remaining, w.level, k, rowsCount - remaining);
        }
        (void)hipMemcpyAsync(host, w.misc, 8 * sizeof(int), hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess)
            return SPGPU_UNSPECIFIED;
        spgpuDebugCheck(handle, "csr trsv plan");
        if (host[1])
            return SPGPU_UNSUPPORTED; /* a column outside the matrix, a missing diagonal or a diagonal stored twice */
        const int left = host[2];
        if (host[4] || left < 0 || left >= remaining)
            return SPGPU_UNSPECIFIED; /* a round that assigned nothing: not a triangle's dependencies */
        k = finish ? host[3] : k + 1;
        remaining = left;
        int* t = list;
        list = next;
        next = t;
    }
    (void)hipMemcpyAsync(levelPtrHost, levelPtr, ((size_t)k + 1) * sizeof(int), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    *levelsCount = k;
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrTrsvDeviceWith(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int levelsCount, const int* rowOrder,
                                     const int* levelPtr, const int* levelPtrHost, const int* rowPtr, const int* colIndices, const void* values,
                                     int baseIndex, int side, int diag, spgpuType_t valuesType, int solve, int maxBlocks)
{
    if (rowsCount <= 0 || levelsCount <= 0)
        return SPGPU_SUCCESS;
    if (solve < 0)
        solve = kTrsvDefaultSolve;
    if (solve != SPGPU_TRSV_SOLVE_PLAIN && solve != SPGPU_TRSV_SOLVE_CHAINED)
        return SPGPU_UNSUPPORTED;
    if (!x || !b || !levelPtrHost || !trsvSideAndDiagKnown(side, diag))
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const bool launched = forValueType(valuesType, [&](auto tag) {
        launchCsrTrsv<decltype(tag)>(s, x, b, levelsCount, rowOrder, levelPtr, levelPtrHost, rowPtr, colIndices, values, baseIndex, side, diag,
                                     solve, maxBlocks);
    });
    if (!launched)
        return SPGPU_UNSUPPORTED;
    spgpuDebugCheck(handle, "csr trsv");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrTrsvDevice(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int levelsCount, const int* rowOrder,
                                 const int* levelPtr, const int* levelPtrHost, const int* rowPtr, const int* colIndices, const void* values,
                                 int baseIndex, int side, int diag, spgpuType_t valuesType)
{
    return spgpuCsrTrsvDeviceWith(handle, x, b, rowsCount, levelsCount, rowOrder, levelPtr, levelPtrHost, rowPtr, colIndices, values, baseIndex,
                                  side, diag, valuesType, -1, 0);
}

} // extern "C"
