/*
 * Aggregation for algebraic multigrid on CSR arrays for gfx950 (include/spgpu/ext/aggregate_device.h): strength of connection, the
 * aggregates' roots as a distance-2 maximal independent set with fixed priorities, the tentative prolongator.  New functionality.
 * No kernel of this file waits for another workgroup: there is no spin loop and no polled flag.  Rounds, sweeps and passes are ordered
 * by stream order between launches, nothing else, and every kernel reads one array and writes another (or only its own element).
 *
 * STRENGTH.  Two launches: csrDiagAbsKernel (one thread per row: |a_ii| of the first stored diagonal) and the mask, which reads
 * diagAbs of both ends of every entry.  The mask has the two row shapes of aggregate_rules.h; every byte of `strong` has one writer.
 *
 * THE ROUNDS.  A node's tuple (state, hash(i), i) is one 64-bit word, so "larger" is the integer comparison.  A round is
 *   t1 = sweep(t0), t2 = sweep(t1)   sweep: out[i] = max(in[i], max over j in S(i) of in[j]) -- a gather of 8-byte words over the strong
 *                                    pattern, the hot path, in two row shapes (THREAD, or a GROUP of L lanes whose maxima are combined
 *                                    by lane shuffles); max of integers is exact, so the shapes and any grid give the same words;
 *   update(t0, t2)                   every undecided node looks at its own two words and rewrites its own t0; the nodes left
 *                                    undecided are counted with one integer atomic per wavefront (the only atomic of the file);
 * and the host reads the count and the bad-input flag after one synchronise.  An entry whose column lies outside the matrix is never
 * used as an index: it is no neighbour, and it raises the flag (misc[1]), as the Plan of the triangular solve does.
 *
 * AFTER THE ROUNDS.  Root flags, one exclusive scan (convert_scan.hip.h) for the numbers, two joining passes (each reads only the array
 * of the pass before), and the sizes.  The sizes are a histogram, which without atomics is a sort: aggregateOf is sorted by a split
 * per key bit -- flag the zeros of the bit, scan, scatter; each position has one writer -- and aggregate a then owns the sorted
 * positions between the lower bounds of a and a + 1.  (rocPRIM's radix sort would do the same, but its scratch cannot be sized
 * without a device, and the scratch size of this call is a function of the rows alone.)  This is set-up code, one thread per row.
 *
 * Scratch, R = rows rounded up to 64: misc[64 ints] | t0[R] t1[R] t2[R] 8-byte words | a[R] b[R] ints | the scan's totals.
 * After the rounds t1 holds the two arrays of the joining passes and t2 the two arrays of the sort.
 */
#include "aggregate_rules.h"
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/aggregate_device.h"

namespace spgpu {

typedef unsigned long long AggTuple;

constexpr int kAggMiscInts = 64; /* 256 bytes: misc[0] the nodes still undecided, misc[1] the bad-input flag */
constexpr unsigned kAggUndecided = 1u, kAggRoot = 2u; /* OUT = 0 is one step below UNDECIDED */
constexpr int kAggStateShift = 62, kAggHashShift = 31;

/* lowbias32(i) >> 1: 31 bits */
__device__ inline unsigned aggHash(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x >> 1;
}

__device__ inline AggTuple aggTupleOf(unsigned state, int i)
{
    return ((AggTuple)state << kAggStateShift) | ((AggTuple)aggHash((unsigned)i) << kAggHashShift) | (AggTuple)(unsigned)i;
}

/* Entry p of row i: its 0-based column when the entry makes a neighbour, -1 when it does not (masked out, the diagonal, or a column
 * outside the matrix, which raises *bad).  The column is compared before it is used, so nothing is read out of bounds. */
__device__ inline int aggNeighbour(int i, int p, const int* idx, const unsigned char* strong, int base, int rows, int* bad)
{
    if (strong && !strong[p])
        return -1;
    const unsigned c = (unsigned)idx[p] - (unsigned)base;
    if (c >= (unsigned)rows) {
        *bad = 1;
        return -1;
    }
    return (int)c == i ? -1 : (int)c;
}

/* ---- strength ---- */
/* |v| as a bit operation: the sign goes, -0.0 becomes +0 */
__device__ inline float aggAbs(float v) { return __builtin_fabsf(v); }
__device__ inline double aggAbs(double v) { return __builtin_fabs(v); }

/* d_i = |a_ii| of the first stored (i, i), +0 without one */
template <typename T>
__global__ __launch_bounds__(kCvThreads) void csrDiagAbsKernel(T* diagAbs, int rows, const int* ptr, const int* idx, const T* val, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        T d = (T)0;
        const int e1 = ptr[i + 1] - base;
        for (int e = ptr[i] - base; e < e1; ++e)
            if ((unsigned)idx[e] - (unsigned)base == (unsigned)i) {
                d = aggAbs(val[e]);
                break;
            }
        diagAbs[i] = d;
    }
}

/* strong[p] of entry p of row i; every product rounded on its own (there is no sum to fuse, the pragma says it anyway) */
template <typename T> __device__ inline unsigned char aggStrong(int i, int p, int rows, const int* idx, const T* val, const T* diagAbs, int base, T t)
{
#pragma clang fp contract(off)
    const unsigned c = (unsigned)idx[p] - (unsigned)base;
    if (c >= (unsigned)rows || c == (unsigned)i)
        return 0;
    const T a = val[p];
    const T lhs = a * a;
    const T scaled = t * diagAbs[i];
    const T rhs = scaled * diagAbs[c];
    return lhs >= rhs ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(kAggThreads) void csrStrengthKernel(unsigned char* strong, int rows, const int* ptr, const int* idx, const T* val,
                                                                 const T* diagAbs, int base, T t)
{
    const long long stride = (long long)gridDim.x * kAggThreads;
    for (long long i = (long long)blockIdx.x * kAggThreads + threadIdx.x; i < rows; i += stride) {
        const int e1 = ptr[i + 1] - base;
        for (int p = ptr[i] - base; p < e1; ++p)
            strong[p] = aggStrong((int)i, p, rows, idx, val, diagAbs, base, t);
    }
}

template <typename T>
__global__ __launch_bounds__(kAggThreads) void csrStrengthGroupKernel(unsigned char* strong, int rows, const int* ptr, const int* idx, const T* val,
                                                                      const T* diagAbs, int base, T t, int L)
{
    const int perBlock = kAggThreads / L, lane = (int)threadIdx.x & (L - 1);
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long i = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; i < rows; i += stride) {
        const int e1 = ptr[i + 1] - base;
        for (int p = ptr[i] - base + lane; p < e1; p += L)
            strong[p] = aggStrong((int)i, p, rows, idx, val, diagAbs, base, t);
    }
}

/* ---- the rounds ---- */
static __global__ __launch_bounds__(kCvThreads) void aggInitKernel(AggTuple* t0, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        t0[i] = aggTupleOf(kAggUndecided, (int)i);
}

/* THREAD: out[i] = max(in[i], max over j in S(i) of in[j]) */
static __global__ __launch_bounds__(kAggThreads) void aggSweepKernel(AggTuple* out, const AggTuple* in, int* misc, int rows, const int* ptr,
                                                                    const int* idx, const unsigned char* strong, int base)
{
    const long long stride = (long long)gridDim.x * kAggThreads;
    for (long long i = (long long)blockIdx.x * kAggThreads + threadIdx.x; i < rows; i += stride) {
        AggTuple best = in[i];
        const int e1 = ptr[i + 1] - base;
        for (int p = ptr[i] - base; p < e1; ++p) {
            const int j = aggNeighbour((int)i, p, idx, strong, base, rows, misc + 1);
            if (j >= 0) {
                const AggTuple v = in[j];
                best = v > best ? v : best;
            }
        }
        out[i] = best;
    }
}

/* GROUP of L lanes of one wavefront per row.  The row loop's bound is the same in every lane of a group (they share i), so a whole
 * group reaches the shuffles together; a shuffle with a mask below L stays inside the group.  A row longer than L: the lanes stride;
 * a lane without an entry keeps in[i], which every lane of the group loaded. */
static __global__ __launch_bounds__(kAggThreads) void aggSweepGroupKernel(AggTuple* out, const AggTuple* in, int* misc, int rows, const int* ptr,
                                                                         const int* idx, const unsigned char* strong, int base, int L)
{
    const int perBlock = kAggThreads / L, lane = (int)threadIdx.x & (L - 1);
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long i = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; i < rows; i += stride) {
        AggTuple best = in[i];
        const int e1 = ptr[i + 1] - base;
        for (int p = ptr[i] - base + lane; p < e1; p += L) {
            const int j = aggNeighbour((int)i, p, idx, strong, base, rows, misc + 1);
            if (j >= 0) {
                const AggTuple v = in[j];
                best = v > best ? v : best;
            }
        }
        for (int m = L >> 1; m > 0; m >>= 1) {
            const AggTuple other = __shfl_xor(best, m, kWave);
            best = other > best ? other : best;
        }
        if (lane == 0)
            out[i] = best;
    }
}

/* An undecided i with t2[i] == t0[i] becomes ROOT; otherwise, under a ROOT's tuple, OUT; otherwise it stays and is counted.  The
 * loop is closed before the shuffles, so the whole wavefront takes part in them. */
static __global__ __launch_bounds__(kCvThreads) void aggUpdateKernel(AggTuple* t0, const AggTuple* t2, int* misc, int rows)
{
    const AggTuple one = (AggTuple)1 << kAggStateShift;
    int left = 0;
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        const AggTuple me = t0[i];
        if ((unsigned)(me >> kAggStateShift) != kAggUndecided)
            continue;
        const AggTuple top = t2[i];
        if (top == me)
            t0[i] = me + one; /* UNDECIDED -> ROOT */
        else if ((unsigned)(top >> kAggStateShift) == kAggRoot)
            t0[i] = me - one; /* UNDECIDED -> OUT */
        else
            ++left;
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1)
        left += laneXor(left, m);
    if ((threadIdx.x & (kWave - 1)) == 0 && left > 0)
        atomicAdd(&misc[0], left);
}

/* ---- after the rounds ---- */
static __global__ __launch_bounds__(kCvThreads) void aggRootFlagsKernel(int* isRoot, const AggTuple* t0, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        isRoot[i] = (unsigned)(t0[i] >> kAggStateShift) == kAggRoot ? 1 : 0;
}

static __global__ __launch_bounds__(kCvThreads) void aggRootNumbersKernel(int* assigned, const int* isRoot, const int* number, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        assigned[i] = isRoot[i] ? number[i] : -1;
}

/* a joining pass: an unassigned node takes the smallest aggregate number among the assigned nodes of S(i), read from `in` only */
static __global__ __launch_bounds__(kCvThreads) void aggJoinKernel(int* out, const int* in, int* misc, int rows, const int* ptr, const int* idx,
                                                                  const unsigned char* strong, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        int mine = in[i];
        if (mine < 0) {
            const int e1 = ptr[i + 1] - base;
            for (int p = ptr[i] - base; p < e1; ++p) {
                const int j = aggNeighbour((int)i, p, idx, strong, base, rows, misc + 1);
                if (j < 0)
                    continue;
                const int theirs = in[j];
                if (theirs >= 0 && (mine < 0 || theirs < mine))
                    mine = theirs;
            }
        }
        out[i] = mine;
    }
}

/* the split of the sort by one key bit: flag the keys whose bit is 0 ... */
static __global__ __launch_bounds__(kCvThreads) void aggSplitFlagsKernel(int* zero, const int* keys, int rows, int bit)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        zero[i] = (((unsigned)keys[i] >> bit) & 1u) ? 0 : 1;
}

/* ... and, with before[i] = the zeros in front of i and *zeros their number, move key i to its place: the zeros keep their order in
 * front, the ones keep theirs behind.  The places are a permutation of [0, rows): one writer each. */
static __global__ __launch_bounds__(kCvThreads) void aggSplitScatterKernel(int* out, const int* keys, const int* zero, const int* before,
                                                                          const int* zeros, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    const int z = *zeros;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        out[zero[i] ? before[i] : z + ((int)i - before[i])] = keys[i];
}

/* aggregateSize[a], a < count: the sorted positions between the lower bounds of a and of a + 1 */
static __global__ __launch_bounds__(kCvThreads) void aggSizesKernel(int* sizes, const int* sorted, int rows, int count)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long a = (long long)blockIdx.x * kCvThreads + threadIdx.x; a < count; a += stride) {
        int bound[2];
        for (int k = 0; k < 2; ++k) {
            int lo = 0, hi = rows;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (sorted[mid] < (int)a + k)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            bound[k] = lo;
        }
        sizes[a] = bound[1] - bound[0];
    }
}

/* ---- the tentative prolongator; an element is WORDS words of type W, and `one` the bits of the type's real 1 ---- */
template <typename W, int WORDS>
__global__ __launch_bounds__(kCvThreads) void csrTentativeKernel(int* tPtr, int* tIdx, W* tVal, int rows, const int* aggregateOf, const W* candidate,
                                                                 int base, W one)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i <= rows; i += stride) {
        tPtr[i] = (int)i + base;
        if (i == rows)
            break;
        tIdx[i] = aggregateOf[i] + base;
#pragma unroll
        for (int w = 0; w < WORDS; ++w)
            tVal[i * WORDS + w] = candidate ? candidate[i * WORDS + w] : (w == 0 ? one : (W)0);
    }
}

struct AggregateWork {
    int* misc;
    AggTuple *t0, *t1, *t2;
    int *a, *b, *totals;
};

static size_t aggPadded(int rows) { return alignUpCv((size_t)(rows > 0 ? rows : 0), 64); }
static size_t aggTotalsInts(int rows) { return alignUpCv(scanBlocks((long long)(rows > 0 ? rows : 0)) + 2, 64); }

static AggregateWork carveAggregate(void* work, int rows)
{
    const size_t R = aggPadded(rows);
    AggregateWork w;
    w.misc = static_cast<int*>(work);
    w.t0 = reinterpret_cast<AggTuple*>(w.misc + kAggMiscInts);
    w.t1 = w.t0 + R;
    w.t2 = w.t1 + R;
    w.a = reinterpret_cast<int*>(w.t2 + R);
    w.b = w.a + R;
    w.totals = w.b + R;
    return w;
}

template <typename T>
static void launchStrength(hipStream_t s, unsigned char* strong, void* diagAbs, int rows, const int* ptr, const int* idx, const void* values, int base,
                           double theta, int shape, int maxBlocks)
{
    T* d = static_cast<T*>(diagAbs);
    const T* v = static_cast<const T*>(values);
    const T t = (T)(theta * theta); /* the product in double, one conversion */
    hipLaunchKernelGGL((csrDiagAbsKernel<T>), dim3(aggGrid(rows, 1, maxBlocks)), dim3(kCvThreads), 0, s, d, rows, ptr, idx, v, base);
    const dim3 grid(aggGrid(rows, shape, maxBlocks));
    if (shape == SPGPU_AGG_SHAPE_THREAD)
        hipLaunchKernelGGL((csrStrengthKernel<T>), grid, dim3(kAggThreads), 0, s, strong, rows, ptr, idx, v, (const T*)d, base, t);
    else
        hipLaunchKernelGGL((csrStrengthGroupKernel<T>), grid, dim3(kAggThreads), 0, s, strong, rows, ptr, idx, v, (const T*)d, base, t, shape);
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_aggregate.py and the tests that compare the shapes.  shape: 1 one thread per row, a
 * power of two in [2, 64] that many lanes per row, <= 0 the public call's choice; maxBlocks > 0 caps the grid of every launch that
 * has a shape (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrAggregateDeviceWith(spgpuHandle_t handle, int* aggregatesCount, int* roundsCount, int* aggregateOf, int* aggregateSize,
                                          int rowsCount, const int* rowPtr, const int* colIndices, const unsigned char* strong, int baseIndex,
                                          void* work, int shape, int maxBlocks);
spgpuStatus_t spgpuCsrStrengthDeviceWith(spgpuHandle_t handle, unsigned char* strong, void* diagAbs, int rowsCount, const int* rowPtr,
                                         const int* colIndices, const void* values, int baseIndex, double theta, spgpuType_t valuesType, int shape,
                                         int maxBlocks);
int spgpuCsrAggregateDefaultShape(int rowsCount, int nonZerosCount); /* the rule of aggregate_rules.h */

int spgpuCsrAggregateDefaultShape(int rowsCount, int nonZerosCount) { return aggShape(nonZerosCount, rowsCount); }

size_t spgpuCsrAggregateWorkBytes(int rowsCount)
{
    const size_t R = aggPadded(rowsCount);
    return kAggMiscInts * sizeof(int) + 3 * R * sizeof(AggTuple) + (2 * R + aggTotalsInts(rowsCount)) * sizeof(int);
}

spgpuStatus_t spgpuCsrStrengthDeviceWith(spgpuHandle_t handle, unsigned char* strong, void* diagAbs, int rowsCount, const int* rowPtr,
                                         const int* colIndices, const void* values, int baseIndex, double theta, spgpuType_t valuesType, int shape,
                                         int maxBlocks)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (valuesType != SPGPU_TYPE_FLOAT && valuesType != SPGPU_TYPE_DOUBLE)
        return SPGPU_UNSUPPORTED;
    if (!strong || !diagAbs || !rowPtr)
        return SPGPU_UNSUPPORTED;
    /* The call may not synchronise, so it cannot read the number of stored entries that the rule of aggregate_rules.h asks for: the
     * public call runs the fallback, one thread per row. */
    if (shape <= 0)
        shape = SPGPU_AGG_SHAPE_THREAD;
    if (!aggShapeKnown(shape))
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    if (valuesType == SPGPU_TYPE_FLOAT)
        launchStrength<float>(s, strong, diagAbs, rowsCount, rowPtr, colIndices, values, baseIndex, theta, shape, maxBlocks);
    else
        launchStrength<double>(s, strong, diagAbs, rowsCount, rowPtr, colIndices, values, baseIndex, theta, shape, maxBlocks);
    spgpuDebugCheck(handle, "csr strength");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrStrengthDevice(spgpuHandle_t handle, unsigned char* strong, void* diagAbs, int rowsCount, const int* rowPtr,
                                     const int* colIndices, const void* values, int baseIndex, double theta, spgpuType_t valuesType)
{
    return spgpuCsrStrengthDeviceWith(handle, strong, diagAbs, rowsCount, rowPtr, colIndices, values, baseIndex, theta, valuesType, 0, 0);
}

spgpuStatus_t spgpuCsrAggregateDeviceWith(spgpuHandle_t handle, int* aggregatesCount, int* roundsCount, int* aggregateOf, int* aggregateSize,
                                          int rowsCount, const int* rowPtr, const int* colIndices, const unsigned char* strong, int baseIndex,
                                          void* work, int shape, int maxBlocks)
{
    *aggregatesCount = 0;
    *roundsCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!aggregateOf || !aggregateSize || !rowPtr || !work)
        return SPGPU_UNSUPPORTED;
    if (shape > 0 && !aggShapeKnown(shape))
        return SPGPU_UNSUPPORTED;
    const int rows = rowsCount, base = baseIndex;
    hipStream_t s = handle->currentStream;
    const AggregateWork w = carveAggregate(work, rows);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(w.misc, 0, kAggMiscInts * sizeof(int), s);
    hipLaunchKernelGGL(aggInitKernel, dim3(gridFor(rows)), dim3(kCvThreads), 0, s, w.t0, rows);
    if (shape <= 0) { /* the rule wants the mean row length, which lies in HBM */
        (void)hipMemcpyAsync(host, rowPtr + rows, sizeof(int), hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess)
            return SPGPU_UNSPECIFIED;
        shape = aggShape((long long)host[0] - base, rows);
    }
    const dim3 sweepGrid(aggGrid(rows, shape, maxBlocks)), rowGrid(gridFor(rows));
    auto sweep = [&](AggTuple* out, const AggTuple* in) {
        if (shape == SPGPU_AGG_SHAPE_THREAD)
            hipLaunchKernelGGL(aggSweepKernel, sweepGrid, dim3(kAggThreads), 0, s, out, in, w.misc, rows, rowPtr, colIndices, strong, base);
        else
            hipLaunchKernelGGL(aggSweepGroupKernel, sweepGrid, dim3(kAggThreads), 0, s, out, in, w.misc, rows, rowPtr, colIndices, strong, base,
                               shape);
    };
    /* ---- the rounds: at least one node decides in each, so there are at most `rows` ---- */
    int rounds = 0, left = rows;
    while (left > 0 && rounds < rows) {
        (void)hipMemsetAsync(w.misc, 0, sizeof(int), s);
        sweep(w.t1, w.t0);
        sweep(w.t2, w.t1);
        hipLaunchKernelGGL(aggUpdateKernel, rowGrid, dim3(kCvThreads), 0, s, w.t0, (const AggTuple*)w.t2, w.misc, rows);
        (void)hipMemcpyAsync(host, w.misc, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess)
            return SPGPU_UNSPECIFIED;
        spgpuDebugCheck(handle, "csr aggregate round");
        ++rounds;
        if (host[1])
            return SPGPU_UNSUPPORTED; /* a neighbour outside the matrix: the first sweep has seen every entry */
        left = host[0];
    }
    if (left > 0)
        return SPGPU_UNSPECIFIED;
    /* ---- numbers and the two joining passes ---- */
    const size_t R = aggPadded(rows), tiles = scanBlocks(rows);
    int *joined0 = reinterpret_cast<int*>(w.t1), *joined1 = joined0 + R;
    int *keysA = reinterpret_cast<int*>(w.t2), *keysB = keysA + R;
    hipLaunchKernelGGL(aggRootFlagsKernel, rowGrid, dim3(kCvThreads), 0, s, w.a, (const AggTuple*)w.t0, rows);
    exclusiveScan(s, w.b, w.a, rows, 1, w.totals);
    (void)hipMemcpyAsync(host, w.totals + tiles, sizeof(int), hipMemcpyDeviceToHost, s);
    hipLaunchKernelGGL(aggRootNumbersKernel, rowGrid, dim3(kCvThreads), 0, s, joined0, (const int*)w.a, (const int*)w.b, rows);
    hipLaunchKernelGGL(aggJoinKernel, rowGrid, dim3(kCvThreads), 0, s, joined1, (const int*)joined0, w.misc, rows, rowPtr, colIndices, strong, base);
    hipLaunchKernelGGL(aggJoinKernel, rowGrid, dim3(kCvThreads), 0, s, aggregateOf, (const int*)joined1, w.misc, rows, rowPtr, colIndices, strong,
                       base);
    if (hipStreamSynchronize(s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    const int count = host[0];
    if (count < 1 || count > rows)
        return SPGPU_UNSPECIFIED;
    /* ---- the sizes: aggregateOf sorted by a split per bit of the largest number, then two lower bounds per aggregate ---- */
    const int* sorted = aggregateOf;
    int* into = keysA;
    const int bits = bitsFor(count);
    for (int bit = 0; bit < bits; ++bit) {
        hipLaunchKernelGGL(aggSplitFlagsKernel, rowGrid, dim3(kCvThreads), 0, s, w.a, sorted, rows, bit);
        exclusiveScan(s, w.b, w.a, rows, 1, w.totals);
        hipLaunchKernelGGL(aggSplitScatterKernel, rowGrid, dim3(kCvThreads), 0, s, into, sorted, (const int*)w.a, (const int*)w.b,
                           (const int*)(w.totals + tiles), rows);
        sorted = into;
        into = into == keysA ? keysB : keysA;
    }
    hipLaunchKernelGGL(aggSizesKernel, dim3(gridFor(count)), dim3(kCvThreads), 0, s, aggregateSize, sorted, rows, count);
    if (hipStreamSynchronize(s) != hipSuccess) /* `work` may be freed once the call has returned */
        return SPGPU_UNSPECIFIED;
    spgpuDebugCheck(handle, "csr aggregate");
    *aggregatesCount = count;
    *roundsCount = rounds;
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrAggregateDevice(spgpuHandle_t handle, int* aggregatesCount, int* roundsCount, int* aggregateOf, int* aggregateSize,
                                      int rowsCount, const int* rowPtr, const int* colIndices, const unsigned char* strong, int baseIndex, void* work)
{
    return spgpuCsrAggregateDeviceWith(handle, aggregatesCount, roundsCount, aggregateOf, aggregateSize, rowsCount, rowPtr, colIndices, strong,
                                       baseIndex, work, 0, 0);
}

spgpuStatus_t spgpuCsrTentativeDevice(spgpuHandle_t handle, int* tRowPtr, int* tColIndices, void* tValues, int rowsCount, const int* aggregateOf,
                                      const void* candidate, int baseIndex, spgpuType_t valuesType)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (valuesType != SPGPU_TYPE_FLOAT && valuesType != SPGPU_TYPE_DOUBLE && valuesType != SPGPU_TYPE_COMPLEX_FLOAT &&
        valuesType != SPGPU_TYPE_COMPLEX_DOUBLE)
        return SPGPU_UNSUPPORTED;
    if (!tRowPtr || !tColIndices || !tValues || !aggregateOf)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const dim3 grid(gridFor((long long)rowsCount + 1));
    const unsigned oneS = 0x3F800000u;
    const unsigned long long oneD = 0x3FF0000000000000ull;
#define SPGPU_TENTATIVE_LAUNCH(W, WORDS, ONE)                                                                                             \
    hipLaunchKernelGGL((csrTentativeKernel<W, WORDS>), grid, dim3(kCvThreads), 0, s, tRowPtr, tColIndices, static_cast<W*>(tValues), rowsCount, \
                       aggregateOf, static_cast<const W*>(candidate), baseIndex, ONE)
    switch (valuesType) {
    case SPGPU_TYPE_FLOAT:
        SPGPU_TENTATIVE_LAUNCH(unsigned, 1, oneS);
        break;
    case SPGPU_TYPE_DOUBLE:
        SPGPU_TENTATIVE_LAUNCH(unsigned long long, 1, oneD);
        break;
    case SPGPU_TYPE_COMPLEX_FLOAT:
        SPGPU_TENTATIVE_LAUNCH(unsigned, 2, oneS);
        break;
    default:
        SPGPU_TENTATIVE_LAUNCH(unsigned long long, 2, oneD);
        break;
    }
#undef SPGPU_TENTATIVE_LAUNCH
    spgpuDebugCheck(handle, "csr tentative");
    return SPGPU_SUCCESS;
}

} // extern "C"
