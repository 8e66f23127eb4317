/*
 * The sparse matrix sum C = alpha * A + beta * B on CSR arrays for gfx950 (include/spgpu/ext/add_device.h).  New functionality.
 * Both inputs have ascending columns, so nothing is sorted: the analysis merges, and the fills place every stored entry of A and
 * of B by its RANK in the other matrix's row, without reading the columns of C.
 *
 * THE PLAN is set-up code: one thread per row walks the two rows as a merge and counts len(A_i) + len(B_i) - matches into
 * cRowPtr[i], checking in the same pass that every column lies in the matrix and that both rows ascend strictly (columns are
 * compared, never used as an index); the counts are added into a 64-bit total (integer atomics: order-independent), scanned in
 * place by the three-launch scan of convert_scan.hip.h, and baseIndex is added.  One thread per row reads its rows uncoalesced;
 * that is accepted for a pass that runs once per pattern.  Scratch (ints): misc[16] | scan totals[tiles(rows + 1) + 2]; misc[1]
 * the bad-input flag, misc[2..3] the 64-bit count.
 *
 * THE FILLS.  Entry e of A's row i lands at cRowPtr[i] + (e - aRowPtr[i]) + below, where `below` is the number of columns of B's
 * row i below the entry's column that A's row does not hold: the rank in B's row (a bisection) less the columns the two rows
 * have in common below it (addCommon: a walk over both rows from their starts, as long as the row is up to the entry -- a handful
 * of steps on a stencil, quadratic in the length of a long row).  If the bisection ends on an equal column, that position
 * supplies the b term.  An entry of B whose column A's row does not hold lands at cRowPtr[i] + (f - bRowPtr[i]) + below with the
 * roles exchanged; one that A holds is written by A's entry.  One writer per element, no atomics, and the same arithmetic
 * (exactMul, exactScaledSum of csr_shared.hip.h: contraction off) in both fills, so both give the same bytes:
 *   plain    (csrAddEntryKernel) one thread per stored entry of A and of B, grid-strided; the counts come from the row pointers
 *            on the device; the row by bisection of the row pointer, the rank by bisection of the other row in global memory.
 *            No LDS;
 *   staged   (csrAddTileKernel) a workgroup of 256 owns tile t: the rows that START in entries [t * kAddTile, (t + 1) * kAddTile)
 *            of C, found by two bisections of cRowPtr (two lanes, one each).  All of them but the last end inside the tile, so
 *            only the last can be long.  If it has more than kAddRowCap entries in C it is set aside.  The slices of aColIndices
 *            and bColIndices of the remaining rows are contiguous and no longer than their part of C, at most kAddTile - 1 +
 *            kAddRowCap entries: they are read coalesced into LDS (kAddSlice ints each, 32 KB together, the same for every
 *            type: values never pass through LDS).  Then one thread per entry of A's slice and of B's slice: the row by
 *            bisection of the row pointer between the tile's first and last row, the rank by bisection of the other slice in
 *            LDS; the own value is loaded coalesced, a matching b near-monotone, and the stores fall into the tile's contiguous
 *            range of C in near-monotone order.  The row set aside is done by the plain method in the same launch, the
 *            workgroup striding over its entries: no host knowledge, no second launch.
 */
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/add_device.h"

#include <limits.h>
#include <string.h>

namespace spgpu {

constexpr int kAddThreads = 256;
constexpr int kAddTile = 2048;   /* entries of C whose rows one workgroup owns */
constexpr int kAddRowCap = 2048; /* the longest row of C that is staged; a longer one goes by the plain method */
constexpr int kAddSlice = 4096;  /* ints of LDS per matrix: kAddTile - 1 + kAddRowCap fit */
static_assert(kAddRowCap >= kAddTile, "a row that is not the last of its tile is shorter than the tile and must be staged");
static_assert(kAddTile - 1 + kAddRowCap <= kAddSlice, "the staged rows' slices must fit");
static_assert(2 * kAddSlice * sizeof(int) <= 64 * 1024, "static LDS within 64 KB");
constexpr int kAddFillBlocks = 2048; /* enough workgroups of 256 to fill 256 CUs, where the host does not know C's size */

enum { SPGPU_ADD_FILL_PLAIN = 0, SPGPU_ADD_FILL_STAGED = 1 };
/* The fill the public calls run.  The rule: the one that is faster on M + dt * K of a 3-D 7-point pattern if the min-max ranges of
 * the two legs do not overlap, the plain one otherwise.  tools/bench_csr_add.py on an MI355X, fp64, 8 M rows, values pass: staged
 * 1.93-1.94 ms, plain 2.36-2.37 ms (profiles/csr_add_ab.json). */
constexpr int kAddDefaultFill = SPGPU_ADD_FILL_STAGED;

static size_t addWorkInts(int rows) { return alignUpCv((size_t)16 + scanBlocks((long long)rows + 1) + 2, 64); }

/* ---- the plan ---- */
/* counts[i] = |A_i u B_i| for i < rows, counts[rows] = 0 (the scan's last slot).  A column outside the matrix or a row that does
 * not ascend strictly raises misc[1]; the walk ends all the same, and its count lies in [0, len(A_i) + len(B_i)]. */
__global__ __launch_bounds__(kCvThreads) void csrAddCountKernel(int* counts, int* misc, int rows, int cols, const int* aPtr, const int* aIdx,
                                                                 const int* bPtr, const int* bIdx, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i <= rows; i += stride) {
        int count = 0;
        if (i < rows) {
            int e = aPtr[i] - base, f = bPtr[i] - base;
            const int e0 = e, f0 = f, e1 = aPtr[i + 1] - base, f1 = bPtr[i + 1] - base;
            bool bad = false;
            while (e < e1 || f < f1) {
                /* INT_MAX where a row is used up: never compared, takeA and takeB ask first whether their row still has entries */
                const int ja = e < e1 ? aIdx[e] : INT_MAX, jb = f < f1 ? bIdx[f] : INT_MAX;
                if (e < e1) {
                    bad |= (unsigned)ja - (unsigned)base >= (unsigned)cols;
                    bad |= e > e0 && aIdx[e - 1] >= ja;
                }
                if (f < f1) {
                    bad |= (unsigned)jb - (unsigned)base >= (unsigned)cols;
                    bad |= f > f0 && bIdx[f - 1] >= jb;
                }
                const bool takeA = e < e1 && (f >= f1 || ja <= jb), takeB = f < f1 && (e >= e1 || jb <= ja);
                e += takeA;
                f += takeB;
                ++count;
            }
            if (bad)
                misc[1] = 1;
            if (count)
                atomicAdd(reinterpret_cast<unsigned long long*>(misc + 2), (unsigned long long)count);
        }
        counts[i] = count;
    }
}

__global__ __launch_bounds__(kCvThreads) void csrAddBaseKernel(int* rowPtr, long long n, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < n; i += stride)
        rowPtr[i] += base;
}

/* how many columns own[ownFrom, ownTo) and other[otherFrom, otherTo) -- both ascending -- have in common: a walk over both */
__device__ inline int addCommon(const int* own, int ownFrom, int ownTo, const int* other, int otherFrom, int otherTo)
{
    int common = 0;
    while (ownFrom < ownTo && otherFrom < otherTo) {
        const int jo = own[ownFrom], jt = other[otherFrom];
        common += jo == jt;
        ownFrom += jo <= jt;
        otherFrom += jt <= jo;
    }
    return common;
}

/* the last row i in [lo, hi) with ptr[i] - base <= u (lo < hi, ptr[lo] - base <= u): rows without entries in front of u's are
 * passed over */
__device__ inline int addRowOf(const int* ptr, int lo, int hi, int base, long long u)
{
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ptr[mid] - base <= u)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

/* What the two matrices are to one stored entry: the matrix that stores it (own) and the other one.  OWN_IS_A: the entry is A's,
 * and it writes the sum where B holds the column too; otherwise the entry is B's and leaves such a column to A's entry. */
template <typename T, bool OWN_IS_A, bool FULL>
__device__ inline void addPlace(int* cIdx, T* cVal, int cStart, int offsetInRow, int column, T ownScalar, T ownValue, T otherScalar,
                                const T* otherVal, long long otherAt, int below, bool match)
{
    if (!OWN_IS_A && match)
        return;
    const long long at = (long long)cStart + offsetInRow + below;
    T c;
    if (OWN_IS_A && match)
        c = exactScaledSum(ownScalar, ownValue, otherScalar, otherVal[otherAt]);
    else
        c = exactMul(ownScalar, ownValue);
    cVal[at] = c;
    if (FULL)
        cIdx[at] = column;
}

/* entry u of the own matrix, in row i, by the plain method: the other matrix's row bisected in global memory */
template <typename T, bool OWN_IS_A, bool FULL>
__device__ inline void addEntryPlain(int* cIdx, T* cVal, int i, long long u, T ownScalar, const int* ownPtr, const int* ownIdx, const T* ownVal,
                                     T otherScalar, const int* otherPtr, const int* otherIdx, const T* otherVal, const int* cPtr, int base)
{
    const int column = ownIdx[u];
    const int o0 = otherPtr[i] - base, o1 = otherPtr[i + 1] - base;
    const int lo = lowerBound(otherIdx, o0, o1, column);
    const bool match = lo < o1 && otherIdx[lo] == column;
    if (!OWN_IS_A && match)
        return;
    const int own0 = ownPtr[i] - base;
    const int below = lo - o0 - addCommon(ownIdx, own0, (int)u, otherIdx, o0, lo); /* the other row's columns below that C has not counted yet */
    addPlace<T, OWN_IS_A, FULL>(cIdx, cVal, cPtr[i] - base, (int)u - own0, column, ownScalar, ownVal[u], otherScalar, otherVal, lo, below, match);
}

/* The plain fill: one thread per stored entry of A, then of B.  The numbers of entries are read from the row pointers. */
template <typename T, bool FULL>
__global__ __launch_bounds__(kAddThreads) void csrAddEntryKernel(int* cIdx, T* cVal, int rows, T alphaValue, const T* alphaAt, const int* aPtr,
                                                                 const int* aIdx, const T* aVal, T betaValue, const T* betaAt, const int* bPtr,
                                                                 const int* bIdx, const T* bVal, const int* cPtr, int base)
{
    const T alpha = alphaAt ? *alphaAt : alphaValue, beta = betaAt ? *betaAt : betaValue;
    const long long inA = aPtr[rows] - base, inB = bPtr[rows] - base;
    const long long stride = (long long)gridDim.x * kAddThreads;
    for (long long u = (long long)blockIdx.x * kAddThreads + threadIdx.x; u < inA + inB; u += stride) {
        if (u < inA) {
            const int i = addRowOf(aPtr, 0, rows, base, u);
            addEntryPlain<T, true, FULL>(cIdx, cVal, i, u, alpha, aPtr, aIdx, aVal, beta, bPtr, bIdx, bVal, cPtr, base);
        } else {
            const long long v = u - inA;
            const int i = addRowOf(bPtr, 0, rows, base, v);
            addEntryPlain<T, false, FULL>(cIdx, cVal, i, v, beta, bPtr, bIdx, bVal, alpha, aPtr, aIdx, aVal, cPtr, base);
        }
    }
}

/* the staged rows [r0, rs) of a tile: one thread per entry of the own slice (own0 .. own0 + ownLen in global numbering, its columns
 * in ownCols), the other slice's columns in otherCols (other0 its first global position) */
template <typename T, bool OWN_IS_A, bool FULL>
__device__ inline void addSliceStaged(int* cIdx, T* cVal, int r0, int rs, T ownScalar, const int* ownPtr, const int* ownCols, int own0, int ownLen,
                                      const T* ownVal, T otherScalar, const int* otherPtr, const int* otherCols, int other0, const T* otherVal,
                                      const int* cPtr, int base)
{
    for (int x = threadIdx.x; x < ownLen; x += kAddThreads) {
        const int u = own0 + x;
        const int i = addRowOf(ownPtr, r0, rs, base, u);
        const int column = ownCols[x];
        const int o0 = otherPtr[i] - base - other0, o1 = otherPtr[i + 1] - base - other0;
        const int lo = lowerBound(otherCols, o0, o1, column);
        const bool match = lo < o1 && otherCols[lo] == column;
        if (!OWN_IS_A && match)
            continue;
        const int ownRow = ownPtr[i] - base - own0; /* where the row starts in the own slice */
        const int below = lo - o0 - addCommon(ownCols, ownRow, x, otherCols, o0, lo);
        addPlace<T, OWN_IS_A, FULL>(cIdx, cVal, cPtr[i] - base, x - ownRow, column, ownScalar, ownVal[u], otherScalar, otherVal,
                                    (long long)other0 + lo, below, match);
    }
}

/* row i by the plain method, the workgroup striding over its entries of A and of B */
template <typename T, bool FULL>
__device__ inline void addRowPlain(int* cIdx, T* cVal, int i, T alpha, const int* aPtr, const int* aIdx, const T* aVal, T beta, const int* bPtr,
                                   const int* bIdx, const T* bVal, const int* cPtr, int base)
{
    const int a0 = aPtr[i] - base, a1 = aPtr[i + 1] - base, b0 = bPtr[i] - base, b1 = bPtr[i + 1] - base;
    for (int u = a0 + (int)threadIdx.x; u < a1; u += kAddThreads)
        addEntryPlain<T, true, FULL>(cIdx, cVal, i, u, alpha, aPtr, aIdx, aVal, beta, bPtr, bIdx, bVal, cPtr, base);
    for (int v = b0 + (int)threadIdx.x; v < b1; v += kAddThreads)
        addEntryPlain<T, false, FULL>(cIdx, cVal, i, v, beta, bPtr, bIdx, bVal, alpha, aPtr, aIdx, aVal, cPtr, base);
}

/* The staged fill (head of the file). */
template <typename T, bool FULL>
__global__ __launch_bounds__(kAddThreads) void csrAddTileKernel(int* cIdx, T* cVal, int rows, T alphaValue, const T* alphaAt, const int* aPtr,
                                                                const int* aIdx, const T* aVal, T betaValue, const T* betaAt, const int* bPtr,
                                                                const int* bIdx, const T* bVal, const int* cPtr, int base)
{
    __shared__ int ldsA[kAddSlice];
    __shared__ int ldsB[kAddSlice];
    __shared__ int ldsBounds[2];
    const T alpha = alphaAt ? *alphaAt : alphaValue, beta = betaAt ? *betaAt : betaValue;
    const long long entries = cPtr[rows] - base;
    const long long tiles = (entries + kAddTile - 1) / kAddTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        /* the first row whose entries start at or behind t * kAddTile, and the same for t + 1: rows [0, rows], whose last element
         * starts at `entries` */
        if (threadIdx.x == 0 || threadIdx.x == kWave) {
            const long long from = (t + (threadIdx.x ? 1 : 0)) * kAddTile;
            int lo = 0, hi = rows;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (cPtr[mid] - base < from)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            ldsBounds[threadIdx.x ? 1 : 0] = lo;
        }
        __syncthreads();
        const int r0 = ldsBounds[0], r1 = ldsBounds[1];
        int rs = r1; /* rows [r0, rs) are staged */
        if (r1 > r0 && cPtr[r1] - cPtr[r1 - 1] > kAddRowCap)
            rs = r1 - 1;
        const int a0 = aPtr[r0] - base, b0 = bPtr[r0] - base;
        const int aLen = aPtr[rs] - base - a0, bLen = bPtr[rs] - base - b0;
        if (aLen <= kAddSlice && bLen <= kAddSlice) {
            for (int x = threadIdx.x; x < aLen; x += kAddThreads)
                ldsA[x] = aIdx[a0 + x];
            for (int x = threadIdx.x; x < bLen; x += kAddThreads)
                ldsB[x] = bIdx[b0 + x];
            __syncthreads();
            if (rs > r0) {
                addSliceStaged<T, true, FULL>(cIdx, cVal, r0, rs, alpha, aPtr, ldsA, a0, aLen, aVal, beta, bPtr, ldsB, b0, bVal, cPtr, base);
                addSliceStaged<T, false, FULL>(cIdx, cVal, r0, rs, beta, bPtr, ldsB, b0, bLen, bVal, alpha, aPtr, ldsA, a0, aVal, cPtr, base);
            }
        } else { /* not a cRowPtr of these matrices' Plan: nothing is staged, so nothing leaves the slices */
            rs = r0;
        }
        for (int i = rs; i < r1; ++i)
            addRowPlain<T, FULL>(cIdx, cVal, i, alpha, aPtr, aIdx, aVal, beta, bPtr, bIdx, bVal, cPtr, base);
        __syncthreads(); /* the next tile overwrites the slices and the bounds */
    }
}

/* entries < 0: the host does not know how many entries C has (the values-only calls) */
template <typename T, bool FULL>
static void launchCsrAdd(hipStream_t s, int* cIdx, void* cVal, int entries, int rows, const void* alpha, bool scalarsOnDevice, const int* aPtr,
                         const int* aIdx, const void* aVal, const void* beta, const int* bPtr, const int* bIdx, const void* bVal, const int* cPtr,
                         int base, int fill, int maxBlocks)
{
    T alphaValue = zeroOf<T>(), betaValue = zeroOf<T>();
    const T *alphaAt = nullptr, *betaAt = nullptr;
    if (scalarsOnDevice) {
        alphaAt = static_cast<const T*>(alpha);
        betaAt = static_cast<const T*>(beta);
    } else {
        memcpy(&alphaValue, alpha, sizeof(T));
        memcpy(&betaValue, beta, sizeof(T));
    }
    /* the host does not know the sizes: a workgroup per 16 rows, and at least enough to fill the device; the kernels stride */
    long long unknown = ((long long)rows + 15) / 16;
    if (unknown < kAddFillBlocks)
        unknown = kAddFillBlocks;
    if (fill == SPGPU_ADD_FILL_PLAIN) {
        /* A and B together hold at least as many entries as C and at most twice as many */
        const long long blocks = entries >= 0 ? (2 * (long long)entries + kAddThreads - 1) / kAddThreads : unknown;
        hipLaunchKernelGGL((csrAddEntryKernel<T, FULL>), dim3(cappedGrid(blocks, 1, maxBlocks)), dim3(kAddThreads), 0, s, cIdx, static_cast<T*>(cVal),
                           rows, alphaValue, alphaAt, aPtr, aIdx, static_cast<const T*>(aVal), betaValue, betaAt, bPtr, bIdx,
                           static_cast<const T*>(bVal), cPtr, base);
        return;
    }
    const long long blocks = entries >= 0 ? ((long long)entries + kAddTile - 1) / kAddTile : unknown;
    hipLaunchKernelGGL((csrAddTileKernel<T, FULL>), dim3(cappedGrid(blocks, 1, maxBlocks)), dim3(kAddThreads), 0, s, cIdx, static_cast<T*>(cVal), rows,
                       alphaValue, alphaAt, aPtr, aIdx, static_cast<const T*>(aVal), betaValue, betaAt, bPtr, bIdx, static_cast<const T*>(bVal),
                       cPtr, base);
}

/* fill < 0: the one the public calls run.  cIdx != NULL: the full call (entries > 0); cIdx == NULL: values only, entries < 0. */
static spgpuStatus_t csrAdd(spgpuHandle_t handle, int* cIdx, void* cVal, int entries, int rows, const void* alpha, bool scalarsOnDevice,
                            const int* aPtr, const int* aIdx, const void* aVal, const void* beta, const int* bPtr, const int* bIdx, const void* bVal,
                            const int* cPtr, int base, spgpuType_t type, int fill, int maxBlocks)
{
    if (fill < 0)
        fill = kAddDefaultFill;
    if (fill != SPGPU_ADD_FILL_PLAIN && fill != SPGPU_ADD_FILL_STAGED)
        return SPGPU_UNSUPPORTED;
    if (!alpha || !beta || !cVal)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const bool launched = forValueType(type, [&](auto tag) {
        using T = decltype(tag);
        if (cIdx)
            launchCsrAdd<T, true>(s, cIdx, cVal, entries, rows, alpha, scalarsOnDevice, aPtr, aIdx, aVal, beta, bPtr, bIdx, bVal, cPtr, base, fill,
                                  maxBlocks);
        else
            launchCsrAdd<T, false>(s, cIdx, cVal, entries, rows, alpha, scalarsOnDevice, aPtr, aIdx, aVal, beta, bPtr, bIdx, bVal, cPtr, base, fill,
                                   maxBlocks);
    });
    if (!launched)
        return SPGPU_UNSUPPORTED;
    spgpuDebugCheck(handle, "csr add");
    return SPGPU_SUCCESS;
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_csr_add.py and the tests that compare the two fills.  fill: 0 the plain fill, 1 the
 * staged fill, < 0 the public call's choice; maxBlocks > 0 caps the grid (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrAddDeviceWith(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int rowsCount, const void* alpha,
                                    const int* aRowPtr, const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                    const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType, int fill,
                                    int maxBlocks);
spgpuStatus_t spgpuCsrAddValuesDeviceWith(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                          const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                          const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType,
                                          int fill, int maxBlocks);
spgpuStatus_t spgpuCsrAddValuesDeviceScalarsWith(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                                 const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                                 const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex,
                                                 spgpuType_t valuesType, int fill, int maxBlocks);
int spgpuCsrAddDefaultFill(void);
int spgpuCsrAddTile(void);   /* the entries of C whose rows one workgroup of the staged fill owns */
int spgpuCsrAddRowCap(void); /* the longest row of C that the staged fill stages */

int spgpuCsrAddDefaultFill(void) { return kAddDefaultFill; }
int spgpuCsrAddTile(void) { return kAddTile; }
int spgpuCsrAddRowCap(void) { return kAddRowCap; }

size_t spgpuCsrAddWorkBytes(int rowsCount) { return addWorkInts(rowsCount > 0 ? rowsCount : 0) * sizeof(int) + 256; }

spgpuStatus_t spgpuCsrAddPlanDevice(spgpuHandle_t handle, int* cNonZerosCount, int* cRowPtr, int rowsCount, int columnsCount, const int* aRowPtr,
                                    const int* aColIndices, const int* bRowPtr, const int* bColIndices, int baseIndex, void* work)
{
    *cNonZerosCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!work || !cRowPtr)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    int* misc = static_cast<int*>(work);
    int* totals = misc + 16;
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    const long long n = (long long)rowsCount + 1;
    (void)hipMemsetAsync(misc, 0, 16 * sizeof(int), s);
    hipLaunchKernelGGL(csrAddCountKernel, dim3(gridFor(n)), dim3(kCvThreads), 0, s, cRowPtr, misc, rowsCount, columnsCount > 0 ? columnsCount : 0,
                       aRowPtr, aColIndices, bRowPtr, bColIndices, baseIndex);
    exclusiveScan(s, cRowPtr, cRowPtr, n, 1, totals); /* in place, as in the assembly */
    if (baseIndex != 0)
        hipLaunchKernelGGL(csrAddBaseKernel, dim3(gridFor(n)), dim3(kCvThreads), 0, s, cRowPtr, n, baseIndex);
    (void)hipMemcpyAsync(host, misc, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "csr add plan");
    if (host[1])
        return SPGPU_UNSUPPORTED; /* a column outside the matrix, or a row that does not ascend strictly */
    unsigned long long total;
    memcpy(&total, host + 2, sizeof(total));
    if (total > (unsigned long long)INT_MAX) {
        *cNonZerosCount = -1;
        return SPGPU_UNSUPPORTED;
    }
    *cNonZerosCount = (int)total;
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrAddDeviceWith(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int rowsCount, const void* alpha,
                                    const int* aRowPtr, const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                    const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType, int fill,
                                    int maxBlocks)
{
    if (cNonZerosCount <= 0 || rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!cColIndices)
        return SPGPU_UNSUPPORTED;
    return csrAdd(handle, cColIndices, cValues, cNonZerosCount, rowsCount, alpha, false, aRowPtr, aColIndices, aValues, beta, bRowPtr, bColIndices,
                  bValues, cRowPtr, baseIndex, valuesType, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrAddValuesDeviceWith(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                          const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                          const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType,
                                          int fill, int maxBlocks)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    return csrAdd(handle, nullptr, cValues, -1, rowsCount, alpha, false, aRowPtr, aColIndices, aValues, beta, bRowPtr, bColIndices, bValues, cRowPtr,
                  baseIndex, valuesType, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrAddValuesDeviceScalarsWith(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                                 const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                                 const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex,
                                                 spgpuType_t valuesType, int fill, int maxBlocks)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    return csrAdd(handle, nullptr, cValues, -1, rowsCount, alpha, true, aRowPtr, aColIndices, aValues, beta, bRowPtr, bColIndices, bValues, cRowPtr,
                  baseIndex, valuesType, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrAddDevice(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int rowsCount, const void* alpha,
                                const int* aRowPtr, const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType)
{
    return spgpuCsrAddDeviceWith(handle, cColIndices, cValues, cNonZerosCount, rowsCount, alpha, aRowPtr, aColIndices, aValues, beta, bRowPtr,
                                 bColIndices, bValues, cRowPtr, baseIndex, valuesType, -1, 0);
}

spgpuStatus_t spgpuCsrAddValuesDevice(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                      const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr, const int* bColIndices,
                                      const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType)
{
    return spgpuCsrAddValuesDeviceWith(handle, cValues, rowsCount, alpha, aRowPtr, aColIndices, aValues, beta, bRowPtr, bColIndices, bValues,
                                       cRowPtr, baseIndex, valuesType, -1, 0);
}

spgpuStatus_t spgpuCsrAddValuesDeviceScalars(spgpuHandle_t handle, void* cValues, int rowsCount, const void* alpha, const int* aRowPtr,
                                             const int* aColIndices, const void* aValues, const void* beta, const int* bRowPtr,
                                             const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex,
                                             spgpuType_t valuesType)
{
    return spgpuCsrAddValuesDeviceScalarsWith(handle, cValues, rowsCount, alpha, aRowPtr, aColIndices, aValues, beta, bRowPtr, bColIndices, bValues,
                                              cRowPtr, baseIndex, valuesType, -1, 0);
}

} // extern "C"
