/*
 * Multicolour Gauss-Seidel / SOR sweeps and the residual r = b - A * x on CSR arrays for gfx950
 * (include/spgpu/ext/sweep_device.h).  New functionality.  No kernel of this file waits for another workgroup: there is no spin
 * loop and no polled flag.  Rows of one colour do not read one another (the Plan has checked it); colours are ordered by stream
 * order between launches, or by a barrier inside ONE workgroup.  No atomics: the Plan's flag and count are plain stores.
 *
 * THE PLAN is set-up code: one pass, one thread per row (sweepCheckKernel).  Row i finds its colour -- colourOf[i] under an order,
 * the bisection of colourPtr without one --, compares every column before it is used, counts its diagonals and keeps the position of
 * the diagonal, and compares its colour with that of every off-diagonal column.  A column is compared, never used as an index before
 * the comparison, so nothing is read out of bounds whatever it holds.  The host reads the flag, the number of stored entries and
 * colourPtr after ONE synchronise and checks colourPtrHost itself (it starts at 0, never descends and ends at rowsCount): the
 * sweep sizes its launches from it.  Scratch: misc[64 ints]; misc[1] the bad-input flag, misc[2] the stored entries.
 *
 * A ROW, two shapes that give the same bytes (sweep_rules.h):
 *   THREAD   one thread walks the row: acc = exactSubMul(acc, a_e, x[col_e]) in storage order, the diagonal skipped by position;
 *   GROUP    L lanes of one wavefront take the row in chunks of L entries.  Lane l loads entry chunk * L + l and its x[col] and rounds
 *            its own product (exactMul: the product exactSubMul rounds); every lane of the group then runs the SAME chain of
 *            differences over the chunk's products in storage order, product k fetched from lane k by a shuffle, the diagonal's
 *            skipped by position.  The loads are parallel and coalesced, the chain is the contract's.  Lanes past the row's end
 *            bring no product into the chain: its length is the number of entries left.  Every quantity that steers the loops is
 *            the same in every lane of a group, so a group reaches every shuffle together, and a shuffle reads a lane of its own
 *            group.  Lane 0 of the group divides and stores.
 *
 * THE SWEEP.  The host rule of sweep_rules.h / trsv_rules.h cuts the list of colour passes into segments:
 *   plain    (csrSweepColourKernel) one launch per colour, grid-strided over the colour's rows;
 *   chained  (csrSweepChainKernel) a maximal run of colours of at most kSweepChainWidth rows is walked by ONE workgroup with
 *            __syncthreads() between colours; the bounds of its colours are kernel arguments (SweepBounds), at most kSweepChainPasses
 *            colours a launch.  The bounds are uniform and the row loop of a colour is closed before the barrier, so every thread
 *            reaches every barrier.  x written before the barrier and read behind it goes through global memory at workgroup scope:
 *            all wavefronts of a workgroup share their CU's vector L1, which takes that CU's loads and stores in order, and
 *            __syncthreads() is a workgroup-scope release and acquire over all address spaces, which also keeps the compiler from
 *            moving a load of x across it.  No further fence -- the argument of the chained triangular solve.
 * THE RESIDUAL (csrResidualKernel) is one grid-strided launch over all rows with the same two row shapes and nothing skipped.
 */
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"
#include "sweep_rules.h"

#include "spgpu/ext/sweep_device.h"

#include <vector>

namespace spgpu {

static_assert(kSweepForward == SPGPU_SWEEP_FORWARD && kSweepBackward == SPGPU_SWEEP_BACKWARD && kSweepSymmetric == SPGPU_SWEEP_SYMMETRIC,
              "sweep_rules.h restates the direction codes of the header");

constexpr int kSweepMiscInts = 64; /* 256 bytes */
/* The segmenting the public call runs: chained, the point of which is the coarse levels of a hierarchy, where every colour is
 * narrow and a sweep is one launch.  NOT MEASURED against plain for these kernels (tools/bench_sweep.py records both). */
constexpr int kSweepDefaultSolve = SPGPU_TRSV_SOLVE_CHAINED;

/* the bounds of the colours a chained launch visits: pass k covers the places between at[k] and at[k + 1], whichever is smaller
 * first (ascending colours: at ascends; descending colours: at descends) */
struct SweepBounds {
    int at[kSweepChainPasses + 1];
};

/* ---- the plan ---- */
/* the colour of row or column k, k inside the matrix */
__device__ inline int sweepColourAt(int k, const int* order, const int* colourPtr, const int* colourOf, int colours)
{
    return order ? colourOf[k] : lowerBound(colourPtr, 0, colours + 1, k + 1) - 1;
}

__global__ __launch_bounds__(kCvThreads) void sweepCheckKernel(int* diagPos, int* misc, int rows, int colours, const int* order, const int* colourPtr,
                                                               const int* colourOf, const int* ptr, const int* idx, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride) {
        const int mine = sweepColourAt((int)i, order, colourPtr, colourOf, colours);
        bool bad = (unsigned)mine >= (unsigned)colours;
        const int e1 = ptr[i + 1] - base;
        int at = -1, diagonals = 0;
        for (int e = ptr[i] - base; e < e1; ++e) {
            const unsigned c = (unsigned)idx[e] - (unsigned)base;
            if (c >= (unsigned)rows) {
                bad = true; /* clamped out: never an index */
                continue;
            }
            if (c == (unsigned)i) {
                at = e;
                ++diagonals;
            } else {
                bad |= sweepColourAt((int)c, order, colourPtr, colourOf, colours) == mine;
            }
        }
        bad |= diagonals != 1;
        if (bad)
            misc[1] = 1;
        diagPos[i] = at;
        if (i == 0)
            misc[2] = ptr[rows] - base;
    }
}

/* ---- the arithmetic that csr_shared.hip.h does not name: a difference on its own, rounded once (componentwise for complex) ---- */
__device__ inline float sweepSub(float a, float p)
{
#pragma clang fp contract(off)
    return a - p;
}
__device__ inline double sweepSub(double a, double p)
{
#pragma clang fp contract(off)
    return a - p;
}
template <typename R> __device__ inline Cx<R> sweepSub(Cx<R> a, Cx<R> p)
{
#pragma clang fp contract(off)
    const R re = a.x - p.x, im = a.y - p.y;
    return Cx<R>{re, im};
}

/* the value of lane `from` of this wavefront; every lane of the group that holds `from` is active at the call */
__device__ inline float sweepFromLane(float v, int from) { return __shfl(v, from, kWave); }
__device__ inline double sweepFromLane(double v, int from) { return __shfl(v, from, kWave); }
template <typename R> __device__ inline Cx<R> sweepFromLane(Cx<R> v, int from)
{
    return Cx<R>{sweepFromLane(v.x, from), sweepFromLane(v.y, from)};
}

/* ---- a row ---- */
/* start - sum of a_e * x[col_e] over the stored entries of row i in storage order, the entry at position `skip` left out (-1: none) */
template <typename T>
__device__ inline T sweepRowThread(T start, const T* x, int i, const int* ptr, const int* idx, const T* val, int base, int skip)
{
    T acc = start;
    const int e1 = ptr[i + 1] - base;
    for (int e = ptr[i] - base; e < e1; ++e)
        if (e != skip)
            acc = exactSubMul(acc, val[e], x[idx[e] - base]);
    return acc;
}

/* GROUP of L lanes; `lane` is this lane's number in the group, `first` the wavefront lane of the group's lane 0.  Every lane of
 * the group returns the same value. */
template <typename T>
__device__ inline T sweepRowGroup(T start, const T* x, int i, const int* ptr, const int* idx, const T* val, int base, int skip, int L, int lane,
                                  int first)
{
    T acc = start;
    const int e1 = ptr[i + 1] - base;
    for (int chunk = ptr[i] - base; chunk < e1; chunk += L) {
        const int e = chunk + lane;
        T product = zeroOf<T>();
        if (e < e1 && e != skip)
            product = exactMul(val[e], x[idx[e] - base]);
        const int left = e1 - chunk, n = left < L ? left : L;
        for (int k = 0; k < n; ++k) {
            const T p = sweepFromLane(product, first + k);
            if (chunk + k != skip)
                acc = sweepSub(acc, p);
        }
    }
    return acc;
}

/* steps 3 to 5 of a colour pass, by the one lane that stores x_i */
template <typename T> __device__ inline void sweepRelax(T* x, int i, T acc, T pivot, int relax, T omega)
{
    const T g = exactDiv(acc, pivot);
    if (!relax) {
        x[i] = g;
        return;
    }
    const T mine = x[i];
    x[i] = exactMulAdd(mine, omega, sweepSub(g, mine));
}

/* the rows at places [begin, end) of the row list (order, or the places themselves), relaxed by the calling workgroup with a
 * stride of `perStride` rows; `slot` is this lane's first row among them */
template <typename T>
__device__ inline void sweepRows(T* x, const T* b, const int* order, long long begin, long long end, long long slot, long long perStride,
                                 const int* diagPos, const int* ptr, const int* idx, const T* val, int base, int relax, T omega, int L, int lane,
                                 int first)
{
    for (long long t = begin + slot; t < end; t += perStride) {
        const int i = order ? order[t] : (int)t;
        const int d = diagPos[i];
        if (L == 1) {
            sweepRelax(x, i, sweepRowThread(b[i], x, i, ptr, idx, val, base, d), val[d], relax, omega);
        } else {
            const T acc = sweepRowGroup(b[i], x, i, ptr, idx, val, base, d, L, lane, first);
            if (lane == 0)
                sweepRelax(x, i, acc, val[d], relax, omega);
        }
    }
}

/* plain: the rows of one colour, places [begin, begin + count) */
template <typename T>
__global__ __launch_bounds__(kSweepThreads) void csrSweepColourKernel(T* x, const T* b, const int* order, int begin, int count, const int* diagPos,
                                                                      const int* ptr, const int* idx, const T* val, int base, int relax, T omega,
                                                                      int L)
{
    const int perBlock = kSweepThreads / L, lane = (int)threadIdx.x & (L - 1), first = ((int)threadIdx.x & (kWave - 1)) - lane;
    sweepRows(x, b, order, (long long)begin, (long long)begin + count, (long long)blockIdx.x * perBlock + (int)threadIdx.x / L,
              (long long)gridDim.x * perBlock, diagPos, ptr, idx, val, base, relax, omega, L, lane, first);
}

/* chained: ONE workgroup walks `passes` colours (head of the file) */
template <typename T>
__global__ __launch_bounds__(kSweepThreads) void csrSweepChainKernel(T* x, const T* b, const int* order, SweepBounds bounds, int passes,
                                                                     const int* diagPos, const int* ptr, const int* idx, const T* val, int base,
                                                                     int relax, T omega, int L)
{
    const int perBlock = kSweepThreads / L, lane = (int)threadIdx.x & (L - 1), first = ((int)threadIdx.x & (kWave - 1)) - lane;
    for (int k = 0; k < passes; ++k) {
        const int a = bounds.at[k], c = bounds.at[k + 1];
        sweepRows(x, b, order, (long long)(a < c ? a : c), (long long)(a < c ? c : a), (long long)((int)threadIdx.x / L), (long long)perBlock, diagPos,
                  ptr, idx, val, base, relax, omega, L, lane, first);
        __syncthreads(); /* the x of this colour is read by the next */
    }
}

/* r = b - A * x, every stored entry of a row subtracted.  r and b may be the same array: b_i is read by the lanes that own row i
 * before lane 0 of them writes r_i, and no other row reads b_i. */
template <typename T>
__global__ __launch_bounds__(kSweepThreads) void csrResidualKernel(T* r, const T* b, const T* x, int rows, const int* ptr, const int* idx, const T* val,
                                                                   int base, int L)
{
    const int perBlock = kSweepThreads / L, lane = (int)threadIdx.x & (L - 1), first = ((int)threadIdx.x & (kWave - 1)) - lane;
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long i = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; i < rows; i += stride) {
        if (L == 1) {
            r[i] = sweepRowThread(b[i], x, (int)i, ptr, idx, val, base, -1);
        } else {
            const T acc = sweepRowGroup(b[i], x, (int)i, ptr, idx, val, base, -1, L, lane, first);
            if (lane == 0)
                r[i] = acc;
        }
    }
}

/* colourPtrHost describes `rows` rows in `colours` colours: it starts at 0, never descends and ends at rows */
static bool sweepPointersSound(const int* colourPtrHost, int colours, int rows)
{
    if (colourPtrHost[0] != 0 || colourPtrHost[colours] != rows)
        return false;
    for (int c = 0; c < colours; ++c)
        if (colourPtrHost[c] > colourPtrHost[c + 1])
            return false;
    return true;
}

/* one list of colour passes: colourPtrHost itself (step 1) or its reversal (step -1) */
template <typename T>
static void launchSweepList(hipStream_t s, T* x, const T* b, int colours, const int* order, const int* colourPtrHost, const int* list, int step,
                            const int* diagPos, const int* ptr, const int* idx, const T* val, int base, int relax, T omega, int shape, int solve,
                            int maxBlocks)
{
    forEachSweepSegment(list, colours, step, solve, [&](SweepSegment g) {
        if (!g.chained) {
            const int begin = colourPtrHost[g.firstColour], count = colourPtrHost[g.firstColour + 1] - begin;
            hipLaunchKernelGGL((csrSweepColourKernel<T>), dim3(sweepGrid(count, shape, maxBlocks)), dim3(kSweepThreads), 0, s, x, b, order, begin,
                               count, diagPos, ptr, idx, val, base, relax, omega, shape);
            return;
        }
        for (int done = 0; done < g.colours; done += kSweepChainPasses) {
            const int passes = g.colours - done < kSweepChainPasses ? g.colours - done : kSweepChainPasses;
            const int from = g.firstColour + g.step * done; /* the first colour of this launch */
            SweepBounds bounds;
            for (int k = 0; k <= passes; ++k)
                bounds.at[k] = g.step > 0 ? colourPtrHost[from + k] : colourPtrHost[from + 1 - k];
            hipLaunchKernelGGL((csrSweepChainKernel<T>), dim3(1), dim3(kSweepThreads), 0, s, x, b, order, bounds, passes, diagPos, ptr, idx, val,
                               base, relax, omega, shape);
        }
    });
}

template <typename T>
static void launchSweep(hipStream_t s, void* x, const void* b, int colours, const int* order, const int* colourPtrHost, const int* diagPos,
                        const int* ptr, const int* idx, const void* val, int base, int direction, const void* omega, int shape, int solve,
                        int maxBlocks)
{
    const int relax = omega ? 1 : 0;
    const T w = omega ? *static_cast<const T*>(omega) : zeroOf<T>();
    if (direction != SPGPU_SWEEP_BACKWARD)
        launchSweepList<T>(s, static_cast<T*>(x), static_cast<const T*>(b), colours, order, colourPtrHost, colourPtrHost, 1, diagPos, ptr, idx,
                           static_cast<const T*>(val), base, relax, w, shape, solve, maxBlocks);
    if (direction != SPGPU_SWEEP_FORWARD) {
        std::vector<int> reversed((size_t)colours + 1); /* host memory for the length of the call: the list the rule reads */
        sweepReversed(reversed.data(), colourPtrHost, colours);
        launchSweepList<T>(s, static_cast<T*>(x), static_cast<const T*>(b), colours, order, colourPtrHost, reversed.data(), -1, diagPos, ptr, idx,
                           static_cast<const T*>(val), base, relax, w, shape, solve, maxBlocks);
    }
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_sweep.py and the tests that compare the shapes.  shape: 1 one thread per row, a power
 * of two in [2, 64] that many lanes per row, <= 0 the public call's choice; solve: 0 plain, 1 chained, < 0 the public call's
 * choice; maxBlocks > 0 caps the grid of every grid-strided launch (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrSweepDeviceWith(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int coloursCount, const int* order,
                                      const int* colourPtrHost, const int* diagPos, const int* rowPtr, const int* colIndices, const void* values,
                                      int baseIndex, int direction, const void* omega, spgpuType_t valuesType, int entriesCount, int shape,
                                      int solve, int maxBlocks);
spgpuStatus_t spgpuCsrResidualDeviceWith(spgpuHandle_t handle, void* r, const void* b, const void* x, int rowsCount, const int* rowPtr,
                                         const int* colIndices, const void* values, int baseIndex, spgpuType_t valuesType, int entriesCount,
                                         int shape, int maxBlocks);
int spgpuCsrSweepDefaultShape(int rowsCount, int nonZerosCount); /* the rule of sweep_rules.h */
int spgpuCsrSweepDefaultSolve(void);
int spgpuCsrSweepChainWidth(void);  /* the widest colour that the chained sweep leaves to one workgroup */
int spgpuCsrSweepChainPasses(void); /* the colours one chained launch walks */
/* the launches of one sweep call, counted by the rule the call runs; colourPtrHost as the Plan returned it */
int spgpuCsrSweepLaunches(const int* colourPtrHost, int coloursCount, int direction, int solve);

int spgpuCsrSweepDefaultShape(int rowsCount, int nonZerosCount) { return sweepShape(nonZerosCount, rowsCount); }
int spgpuCsrSweepDefaultSolve(void) { return kSweepDefaultSolve; }
int spgpuCsrSweepChainWidth(void) { return kSweepChainWidth; }
int spgpuCsrSweepChainPasses(void) { return kSweepChainPasses; }

int spgpuCsrSweepLaunches(const int* colourPtrHost, int coloursCount, int direction, int solve)
{
    if (!colourPtrHost || coloursCount <= 0 || !sweepDirectionKnown(direction))
        return 0;
    if (solve < 0)
        solve = kSweepDefaultSolve;
    int launches = 0;
    if (direction != SPGPU_SWEEP_BACKWARD)
        launches += sweepLaunches(colourPtrHost, coloursCount, solve);
    if (direction != SPGPU_SWEEP_FORWARD) {
        std::vector<int> reversed((size_t)coloursCount + 1);
        sweepReversed(reversed.data(), colourPtrHost, coloursCount);
        launches += sweepLaunches(reversed.data(), coloursCount, solve);
    }
    return launches;
}

size_t spgpuCsrSweepWorkBytes(int rowsCount)
{
    (void)rowsCount; /* the flag and the count: the Plan keeps nothing per row */
    return kSweepMiscInts * sizeof(int);
}

spgpuStatus_t spgpuCsrSweepPlanDevice(spgpuHandle_t handle, int* entriesCount, int* diagPos, int* colourPtrHost, int rowsCount, int coloursCount,
                                      const int* order, const int* colourPtr, const int* colourOf, const int* rowPtr, const int* colIndices,
                                      int baseIndex, void* work)
{
    *entriesCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (coloursCount <= 0 || !diagPos || !colourPtrHost || !colourPtr || (order && !colourOf) || !rowPtr || !colIndices || !work)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    int* misc = static_cast<int*>(work);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(misc, 0, kSweepMiscInts * sizeof(int), s);
    hipLaunchKernelGGL(sweepCheckKernel, dim3(gridFor(rowsCount)), dim3(kCvThreads), 0, s, diagPos, misc, rowsCount, coloursCount, order, colourPtr,
                       colourOf, rowPtr, colIndices, baseIndex);
    (void)hipMemcpyAsync(host, misc, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(colourPtrHost, colourPtr, ((size_t)coloursCount + 1) * sizeof(int), hipMemcpyDeviceToHost, s);
    if (hipStreamSynchronize(s) != hipSuccess) /* `work` may be freed once the call has returned */
        return SPGPU_UNSPECIFIED;
    spgpuDebugCheck(handle, "csr sweep plan");
    if (host[1] || host[2] < 0 || !sweepPointersSound(colourPtrHost, coloursCount, rowsCount))
        return SPGPU_UNSUPPORTED;
    *entriesCount = host[2];
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrSweepDeviceWith(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int coloursCount, const int* order,
                                      const int* colourPtrHost, const int* diagPos, const int* rowPtr, const int* colIndices, const void* values,
                                      int baseIndex, int direction, const void* omega, spgpuType_t valuesType, int entriesCount, int shape,
                                      int solve, int maxBlocks)
{
    if (rowsCount <= 0 || coloursCount <= 0)
        return SPGPU_SUCCESS;
    if (shape <= 0)
        shape = sweepShape(entriesCount, rowsCount);
    if (solve < 0)
        solve = kSweepDefaultSolve;
    if (!sweepShapeKnown(shape) || (solve != SPGPU_TRSV_SOLVE_PLAIN && solve != SPGPU_TRSV_SOLVE_CHAINED) || !sweepDirectionKnown(direction))
        return SPGPU_UNSUPPORTED;
    if (!forValueType((int)valuesType, [](auto) {}))
        return SPGPU_UNSUPPORTED;
    if (!x || !b || !colourPtrHost || !diagPos || !rowPtr || !colIndices || !values)
        return SPGPU_UNSUPPORTED;
    if (!sweepPointersSound(colourPtrHost, coloursCount, rowsCount)) /* the launches are sized from it */
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    forValueType((int)valuesType, [&](auto tag) {
        launchSweep<decltype(tag)>(s, x, b, coloursCount, order, colourPtrHost, diagPos, rowPtr, colIndices, values, baseIndex, direction, omega,
                                   shape, solve, maxBlocks);
    });
    spgpuDebugCheck(handle, "csr sweep");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrSweepDevice(spgpuHandle_t handle, void* x, const void* b, int rowsCount, int coloursCount, const int* order,
                                  const int* colourPtrHost, const int* diagPos, const int* rowPtr, const int* colIndices, const void* values,
                                  int baseIndex, int direction, const void* omega, spgpuType_t valuesType, int entriesCount)
{
    return spgpuCsrSweepDeviceWith(handle, x, b, rowsCount, coloursCount, order, colourPtrHost, diagPos, rowPtr, colIndices, values, baseIndex,
                                   direction, omega, valuesType, entriesCount, 0, -1, 0);
}

spgpuStatus_t spgpuCsrResidualDeviceWith(spgpuHandle_t handle, void* r, const void* b, const void* x, int rowsCount, const int* rowPtr,
                                         const int* colIndices, const void* values, int baseIndex, spgpuType_t valuesType, int entriesCount,
                                         int shape, int maxBlocks)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (shape <= 0)
        shape = sweepShape(entriesCount, rowsCount); /* entriesCount is this rule's input and nothing else */
    if (!sweepShapeKnown(shape) || !forValueType((int)valuesType, [](auto) {}))
        return SPGPU_UNSUPPORTED;
    if (!r || !b || !x || !rowPtr || !colIndices || !values)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    forValueType((int)valuesType, [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((csrResidualKernel<T>), dim3(sweepGrid(rowsCount, shape, maxBlocks)), dim3(kSweepThreads), 0, s, static_cast<T*>(r),
                           static_cast<const T*>(b), static_cast<const T*>(x), rowsCount, rowPtr, colIndices, static_cast<const T*>(values),
                           baseIndex, shape);
    });
    spgpuDebugCheck(handle, "csr residual");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrResidualDevice(spgpuHandle_t handle, void* r, const void* b, const void* x, int rowsCount, const int* rowPtr,
                                     const int* colIndices, const void* values, int baseIndex, spgpuType_t valuesType, int entriesCount)
{
    return spgpuCsrResidualDeviceWith(handle, r, b, x, rowsCount, rowPtr, colIndices, values, baseIndex, valuesType, entriesCount, 0, 0);
}

} // extern "C"
