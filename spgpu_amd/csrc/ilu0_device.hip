/*
 * The incomplete factorisation ILU(0) on CSR arrays for gfx950, level-scheduled (include/spgpu/ext/ilu0_device.h).  New
 * functionality.  No kernel of this file waits for another workgroup: there is no spin loop and no polled flag.  Rows of one level
 * do not depend on one another; levels are ordered by stream order between launches, or by a barrier inside ONE workgroup.
 *
 * THE PLAN is set-up code.  One pass of its own (ilu0CheckKernel) checks every row -- columns inside the matrix, strictly
 * ascending, the diagonal stored -- and writes diagPos; the host reads the flag and the number of stored entries after one
 * synchronise.  The levels are then spgpuCsrTrsvPlanDevice's, called as it stands on the rest of the scratch.
 * Scratch: misc[64 ints] | the scratch of the triangular solve's Plan; misc[1] the bad-input flag, misc[2] the stored entries.
 *
 * THE FACTOR CALL.  Row i is read from a and written to lu by the lanes that own it, then updated in lu; with lu == a the copy is
 * skipped.  A stored entry of row i is read and written by ONE lane from the first touch to the last, so inside a launch no lane
 * reads, through memory, what another lane of the same row wrote: the multiplier lu_ik goes from its owner to the other lanes of
 * the group by a shuffle.  What a row reads of OTHER rows (row k's pivot and upper part) was written in an earlier level:
 *   plain    (csrIlu0LevelKernel) one launch per level, grid-strided over the level's part of rowOrder: stream order;
 *   chained  (csrIlu0ChainKernel) the host rule of ilu0_rules.h / trsv_rules.h cuts the level list into segments: a level of more
 *            than kIlu0ChainWidth rows is a launch as in plain; a maximal run of narrower levels is ONE launch of ONE workgroup,
 *            which walks its levels with __syncthreads() between them.  The bounds of the level loop come from levelPtr and are
 *            uniform, and the row loop of a level is closed before the barrier, so every thread reaches every barrier.  lu written
 *            before the barrier and read behind it goes through global memory at workgroup scope: all wavefronts of a workgroup
 *            share their CU's vector L1, which takes that CU's loads and stores in order, and __syncthreads() is a workgroup-scope
 *            release and acquire over all address spaces, which also keeps the compiler from moving a load of lu across it.  No
 *            further fence -- the argument of the chained triangular solve, unchanged.
 * Two row shapes (ilu0_rules.h), the same bytes:
 *   THREAD   one thread owns the row; row k's upper part and the rest of row i are merged with two pointers (both ascend);
 *   GROUP    L lanes of one wavefront own the row, lane l the positions = l (mod L).  The loop over k is uniform across the group;
 *            each lane bisects row k's upper part for the columns of its own entries beyond k.
 * Each entry's updates come in ascending k because its owner walks k in ascending order, and a k touches it at most once because
 * row k's columns are distinct.  The arithmetic is the triangular solve's: exactDiv and exactSubMul of csr_shared.hip.h.
 */
#include "csr_shared.hip.h"
#include "ilu0_rules.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/ilu0_device.h"
#include "spgpu/ext/trsv_device.h"

namespace spgpu {

constexpr int kIlu0MiscInts = 64; /* 256 bytes: the scratch behind it keeps the alignment the triangular solve's Plan asks for */
/* The segmenting the public call runs.  The rule: the one of the leg that tools/bench_ilu0.py measured fastest on the 200^3 7-point
 * and on the 100^3 27-point matrix, plain where the ranges overlap.  On an MI355X, fp64, plain / chained at the shape that ships:
 * 6.83 / 7.30 ms and 20.41 / 45.98 ms -- a chained level of 256 rows is several passes of ONE workgroup where a launch of its own
 * spreads the groups over 8 or 32.  A bidiagonal matrix of 100 000 rows would gain from the chain (280-299 ms in 100 000 launches
 * against 91 ms in one); the rule does not look at it (profiles/csr_ilu0_ab.json). */
constexpr int kIlu0DefaultSolve = SPGPU_TRSV_SOLVE_PLAIN;

/* ---- the plan ---- */
/* Row i: every column inside the matrix, strictly ascending, the diagonal stored; diagPos[i] = its 0-based position (or -1).  A
 * column is compared, never used as an index, so nothing is read out of bounds whatever it holds. */
__global__ __launch_bounds__(kCvThreads) void ilu0CheckKernel(int* diagPos, int* misc, int rows, const int* ptr, const int* idx, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        const int e1 = ptr[i + 1] - base;
        int at = -1;
        long long before = -1;
        bool bad = false;
        for (int e = ptr[i] - base; e < e1; ++e) {
            const unsigned c = (unsigned)idx[e] - (unsigned)base;
            bad |= c >= (unsigned)rows || (long long)c <= before;
            before = (long long)c;
            if (c == (unsigned)i)
                at = e;
        }
        bad |= at < 0;
        if (bad)
            misc[1] = 1;
        diagPos[i] = at;
        if (i == 0)
            misc[2] = ptr[rows] - base;
    }
}

/* the value of lane `from` of this wavefront; every lane of the group that holds `from` is active at the call */
__device__ inline float ilu0FromLane(float v, int from) { return __shfl(v, from, kWave); }
__device__ inline double ilu0FromLane(double v, int from) { return __shfl(v, from, kWave); }
template <typename R> __device__ inline Cx<R> ilu0FromLane(Cx<R> v, int from)
{
    return Cx<R>{ilu0FromLane(v.x, from), ilu0FromLane(v.y, from)};
}

/* ---- a row ---- */
/* THREAD.  lu and a may be the same array.  Positions [s, d) of row i are its lower part, d its diagonal: the row ascends. */
template <typename T>
__device__ inline void ilu0RowThread(T* lu, const T* a, int i, const int* ptr, const int* idx, const int* diagPos, int base)
{
    const int s = ptr[i] - base, e1 = ptr[i + 1] - base, d = diagPos[i];
    if (lu != a)
        for (int e = s; e < e1; ++e)
            lu[e] = a[e];
    for (int e = s; e < d; ++e) {
        const int k = idx[e] - base;
        const int dk = diagPos[k], endK = ptr[k + 1] - base;
        const T m = exactDiv(lu[e], lu[dk]);
        lu[e] = m;
        int p = dk + 1, q = e + 1;
        while (p < endK && q < e1) {
            const int cp = idx[p], cq = idx[q];
            if (cp == cq) {
                lu[q] = exactSubMul(lu[q], m, lu[p]);
                ++p;
                ++q;
            } else if (cp < cq) {
                ++p;
            } else {
                ++q;
            }
        }
    }
}

/* GROUP of L lanes; `lane` is this lane's number in the group, `first` the wavefront lane of the group's lane 0.  Every quantity
 * that steers the loop over e is the same in every lane of the group, so the group reaches every shuffle together. */
template <typename T>
__device__ inline void ilu0RowGroup(T* lu, const T* a, int i, const int* ptr, const int* idx, const int* diagPos, int base, int L, int lane,
                                    int first)
{
    const int s = ptr[i] - base, e1 = ptr[i + 1] - base, d = diagPos[i];
    if (lu != a)
        for (int e = s + lane; e < e1; e += L)
            lu[e] = a[e];
    for (int e = s; e < d; ++e) {
        const int k = idx[e] - base;
        const int dk = diagPos[k], endK = ptr[k + 1] - base;
        const int owner = (e - s) & (L - 1);
        T m = zeroOf<T>();
        if (lane == owner) {
            m = exactDiv(lu[e], lu[dk]);
            lu[e] = m;
        }
        m = ilu0FromLane(m, first + owner);
        /* this lane's entries behind e: the smallest q > e with (q - s) = lane (mod L), then every L-th */
        for (int q = e + 1 + ((lane - (e + 1 - s)) & (L - 1)); q < e1; q += L) {
            const int c = idx[q];
            int lo = dk + 1, hi = endK;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (idx[mid] < c)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < endK && idx[lo] == c)
                lu[q] = exactSubMul(lu[q], m, lu[lo]);
        }
    }
}

/* ---- plain: the `count` rows of one level, order[0, count) ---- */
template <typename T>
__global__ __launch_bounds__(kIlu0Threads) void csrIlu0LevelKernel(T* lu, const T* a, const int* order, int count, const int* diagPos, const int* ptr,
                                                                   const int* idx, int base)
{
    const long long stride = (long long)gridDim.x * kIlu0Threads;
    for (long long t = (long long)blockIdx.x * kIlu0Threads + threadIdx.x; t < count; t += stride)
        ilu0RowThread(lu, a, order[t], ptr, idx, diagPos, base);
}

template <typename T>
__global__ __launch_bounds__(kIlu0Threads) void csrIlu0LevelGroupKernel(T* lu, const T* a, const int* order, int count, const int* diagPos,
                                                                        const int* ptr, const int* idx, int base, int L)
{
    const int perBlock = kIlu0Threads / L, lane = (int)threadIdx.x & (L - 1), first = ((int)threadIdx.x & (kWave - 1)) - lane;
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long t = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; t < count; t += stride)
        ilu0RowGroup(lu, a, order[t], ptr, idx, diagPos, base, L, lane, first);
}

/* ---- chained: ONE workgroup walks levels [firstLevel, firstLevel + levels) (head of the file) ---- */
template <typename T>
__global__ __launch_bounds__(kIlu0Threads) void csrIlu0ChainKernel(T* lu, const T* a, const int* rowOrder, const int* levelPtr, int firstLevel,
                                                                   int levels, const int* diagPos, const int* ptr, const int* idx, int base)
{
    for (int l = firstLevel; l < firstLevel + levels; ++l) {
        const int begin = levelPtr[l], end = levelPtr[l + 1];
        for (int t = begin + (int)threadIdx.x; t < end; t += kIlu0Threads)
            ilu0RowThread(lu, a, rowOrder[t], ptr, idx, diagPos, base);
        __syncthreads(); /* the rows of this level are read by the next */
    }
}

template <typename T>
__global__ __launch_bounds__(kIlu0Threads) void csrIlu0ChainGroupKernel(T* lu, const T* a, const int* rowOrder, const int* levelPtr, int firstLevel,
                                                                        int levels, const int* diagPos, const int* ptr, const int* idx, int base,
                                                                        int L)
{
    const int perBlock = kIlu0Threads / L, lane = (int)threadIdx.x & (L - 1), first = ((int)threadIdx.x & (kWave - 1)) - lane;
    for (int l = firstLevel; l < firstLevel + levels; ++l) {
        const int begin = levelPtr[l], end = levelPtr[l + 1];
        for (int t = begin + (int)threadIdx.x / L; t < end; t += perBlock)
            ilu0RowGroup(lu, a, rowOrder[t], ptr, idx, diagPos, base, L, lane, first);
        __syncthreads(); /* the rows of this level are read by the next */
    }
}

template <typename T>
static void launchCsrIlu0(hipStream_t s, void* luValues, const void* aValues, int levelsCount, const int* rowOrder, const int* levelPtr,
                          const int* levelPtrHost, const int* diagPos, const int* ptr, const int* idx, int base, int shape, int solve, int maxBlocks)
{
    T* lu = static_cast<T*>(luValues);
    const T* a = static_cast<const T*>(aValues);
    const bool thread = shape == SPGPU_ILU0_SHAPE_THREAD;
    forEachTrsvSegment(levelPtrHost, levelsCount, solve, kIlu0ChainWidth, [&](TrsvSegment g) {
        if (g.chained) {
            if (thread)
                hipLaunchKernelGGL((csrIlu0ChainKernel<T>), dim3(1), dim3(kIlu0Threads), 0, s, lu, a, rowOrder, levelPtr, g.firstLevel, g.levels,
                                   diagPos, ptr, idx, base);
            else
                hipLaunchKernelGGL((csrIlu0ChainGroupKernel<T>), dim3(1), dim3(kIlu0Threads), 0, s, lu, a, rowOrder, levelPtr, g.firstLevel,
                                   g.levels, diagPos, ptr, idx, base, shape);
            return;
        }
        const int first = levelPtrHost[g.firstLevel], count = levelPtrHost[g.firstLevel + 1] - first;
        const dim3 grid(ilu0Grid(count, shape, maxBlocks));
        if (thread)
            hipLaunchKernelGGL((csrIlu0LevelKernel<T>), grid, dim3(kIlu0Threads), 0, s, lu, a, rowOrder + first, count, diagPos, ptr, idx, base);
        else
            hipLaunchKernelGGL((csrIlu0LevelGroupKernel<T>), grid, dim3(kIlu0Threads), 0, s, lu, a, rowOrder + first, count, diagPos, ptr, idx,
                               base, shape);
    });
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_ilu0.py and the tests that compare the shapes.  shape: 1 one thread per row, a power of
 * two in [2, 64] that many lanes per row, <= 0 the public call's choice; solve: 0 plain, 1 chained, < 0 the public call's choice;
 * maxBlocks > 0 caps the grid of a level's launch (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrIlu0DeviceWith(spgpuHandle_t handle, void* luValues, const void* aValues, int rowsCount, int levelsCount,
                                     const int* rowOrder, const int* levelPtr, const int* levelPtrHost, const int* diagPos, const int* rowPtr,
                                     const int* colIndices, int baseIndex, spgpuType_t valuesType, int shape, int solve, int maxBlocks);
int spgpuCsrIlu0DefaultShape(int rowsCount, int nonZerosCount); /* the rule of ilu0_rules.h */
int spgpuCsrIlu0DefaultSolve(void);
int spgpuCsrIlu0ChainWidth(void);    /* the widest level that the chained segmenting leaves to one workgroup */
int spgpuCsrIlu0ShapeConstant(int which); /* 0, 1: the two GROUP widths of the rule; 2, 3: the mean row lengths up to which THREAD and the
                                            * narrow GROUP run */

int spgpuCsrIlu0DefaultShape(int rowsCount, int nonZerosCount) { return ilu0Shape(nonZerosCount, rowsCount); }
int spgpuCsrIlu0DefaultSolve(void) { return kIlu0DefaultSolve; }
int spgpuCsrIlu0ChainWidth(void) { return kIlu0ChainWidth; }
int spgpuCsrIlu0ShapeConstant(int which)
{
    const int constants[4] = {kIlu0GroupNarrow, kIlu0GroupWide, kIlu0ThreadMaxMean, kIlu0NarrowMaxMean};
    return which >= 0 && which < 4 ? constants[which] : -1;
}

size_t spgpuCsrIlu0WorkBytes(int rowsCount) { return kIlu0MiscInts * sizeof(int) + spgpuCsrTrsvWorkBytes(rowsCount); }

spgpuStatus_t spgpuCsrIlu0PlanDevice(spgpuHandle_t handle, int* levelsCount, int* rowOrder, int* levelPtr, int* levelPtrHost, int* diagPos,
                                     int rowsCount, const int* rowPtr, const int* colIndices, int baseIndex, void* work)
{
    *levelsCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!work || !rowOrder || !levelPtr || !levelPtrHost || !diagPos)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    int* misc = static_cast<int*>(work);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(misc, 0, kIlu0MiscInts * sizeof(int), s);
    hipLaunchKernelGGL(ilu0CheckKernel, dim3(gridFor(rowsCount)), dim3(kCvThreads), 0, s, diagPos, misc, rowsCount, rowPtr, colIndices,
                       baseIndex);
    (void)hipMemcpyAsync(host, misc, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    spgpuDebugCheck(handle, "csr ilu0 plan");
    if (host[1])
        return SPGPU_UNSUPPORTED; /* a column outside the matrix, a row that does not ascend strictly or a missing diagonal */
    const int stored = host[2]; /* the Plan of the solve reuses `host` */
    const spgpuStatus_t status = spgpuCsrTrsvPlanDevice(handle, levelsCount, rowOrder, levelPtr, levelPtrHost, rowsCount, rowPtr, colIndices,
                                                        baseIndex, SPGPU_TRSV_LOWER, SPGPU_TRSV_DIAG_STORED, misc + kIlu0MiscInts);
    if (status != SPGPU_SUCCESS) {
        *levelsCount = 0;
        return status;
    }
    levelPtrHost[*levelsCount + 1] = stored; /* the extra slot of the header */
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrIlu0DeviceWith(spgpuHandle_t handle, void* luValues, const void* aValues, int rowsCount, int levelsCount,
                                     const int* rowOrder, const int* levelPtr, const int* levelPtrHost, const int* diagPos, const int* rowPtr,
                                     const int* colIndices, int baseIndex, spgpuType_t valuesType, int shape, int solve, int maxBlocks)
{
    if (rowsCount <= 0 || levelsCount <= 0)
        return SPGPU_SUCCESS;
    if (solve < 0)
        solve = kIlu0DefaultSolve;
    if (solve != SPGPU_TRSV_SOLVE_PLAIN && solve != SPGPU_TRSV_SOLVE_CHAINED)
        return SPGPU_UNSUPPORTED;
    if (!luValues || !aValues || !levelPtrHost)
        return SPGPU_UNSUPPORTED;
    if (shape <= 0)
        shape = ilu0Shape(levelPtrHost[levelsCount + 1], rowsCount);
    if (!ilu0ShapeKnown(shape))
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const bool launched = forValueType(valuesType, [&](auto tag) {
        launchCsrIlu0<decltype(tag)>(s, luValues, aValues, levelsCount, rowOrder, levelPtr, levelPtrHost, diagPos, rowPtr, colIndices, baseIndex,
                                     shape, solve, maxBlocks);
    });
    if (!launched)
        return SPGPU_UNSUPPORTED;
    spgpuDebugCheck(handle, "csr ilu0");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrIlu0Device(spgpuHandle_t handle, void* luValues, const void* aValues, int rowsCount, int levelsCount, const int* rowOrder,
                                 const int* levelPtr, const int* levelPtrHost, const int* diagPos, const int* rowPtr, const int* colIndices,
                                 int baseIndex, spgpuType_t valuesType)
{
    return spgpuCsrIlu0DeviceWith(handle, luValues, aValues, rowsCount, levelsCount, rowOrder, levelPtr, levelPtrHost, diagPos, rowPtr,
                                  colIndices, baseIndex, valuesType, 0, -1, 0);
}

} // extern "C"
