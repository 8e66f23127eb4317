/*
 * Multicolour ordering on CSR arrays for gfx950 (include/spgpu/ext/colour_device.h): a colouring with fixed priorities, the rows
 * listed colour by colour, the symmetric permutation B = A(order, order).  New functionality.  No kernel of this file waits for
 * another workgroup: there is no spin loop and no polled flag.  Rounds, splits and passes are ordered by stream order between
 * launches, nothing else, and every kernel reads one array and writes another.
 *
 * THE ROUNDS.  A round reads the colouring c0 and writes c1.  A coloured node copies its colour.  An uncoloured node i walks its row:
 * a coloured neighbour j sets bit c0[j] - w of a 64-bit mask of the window [w, w + 64), an uncoloured one with a larger tuple
 * (hash(j), j) clears `ready`.  A ready node takes w + the lowest zero bit of the mask; if the window is full, w += 64 and the row is
 * walked again (a clique of 130 takes three windows).  This gather of 4-byte colours over the pattern is the hot path, in two row
 * shapes: THREAD, or a GROUP of L lanes whose masks are OR-ed and whose readiness is AND-ed by lane shuffles.  AND, OR and "lowest
 * zero bit" are exact, so the shapes and any grid give the same words.  The nodes left uncoloured are counted with one integer
 * atomicAdd per wavefront and the largest colour + 1 is kept with one integer atomicMax per wavefront (the only atomics of the
 * file); the host reads both and the bad-input flag after one synchronise.  An entry whose column lies outside the matrix is never
 * used as an index: it is no neighbour, and it raises the flag (misc[1]).  In the first round every node is uncoloured, so every
 * entry is seen.
 *
 * THE ORDER.  The rows sorted by colour, stably: one split per bit of coloursCount - 1 -- flag the rows whose colour has the bit 0,
 * scan, scatter; each position has one writer -- as the sizes of aggregate_device.hip do (whose kernels sort keys, these sort rows
 * by a key looked up; folding the two is a later refactor).  Then order / inverse, and colourPtr by one bisection per colour.
 *
 * THE PERMUTATION.  Gathered row lengths, one exclusive scan (convert_scan.hip.h), bRowPtr, and the fill: entry p of a row goes to
 * the slot of its rank, the number of positions q of the row with (new column, q) below (new column, p).  Each slot has one
 * writer; the row is re-read from cache, rank by rank: quadratic in the row length, set-up code.  One kernel serves THREAD (L = 1)
 * and every GROUP: lane l ranks the positions = l (mod L), and no lane needs another's result.
 *
 * Scratch of the colouring and the order, R = rows rounded up to 64: misc[64 ints] | c0[R] c1[R] a[R] b[R] ints | the scan's totals.
 * The order keeps its two row lists in c0 and c1.  Scratch of the permutation, R1 = rows + 1 rounded up to 64: len[R1] scan[R1] ints
 * | the scan's totals.
 */
#include "colour_rules.h"
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/colour_device.h"

namespace spgpu {

constexpr int kColourMiscInts = 64; /* 256 bytes: misc[0] the nodes still uncoloured, misc[1] the bad-input flag, misc[2] 1 + the largest colour */

/* (lowbias32(i) >> 1, i) in one 64-bit word: "larger" is the integer comparison */
__device__ inline unsigned long long colourTuple(int i)
{
    unsigned x = (unsigned)i;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return ((unsigned long long)(x >> 1) << 32) | (unsigned long long)(unsigned)i;
}

/* Entry p of row i against the window [w, w + 64): a coloured neighbour marks its bit, an uncoloured one with a larger tuple clears
 * *ready.  The diagonal is no neighbour; a column outside the matrix is none either and raises *bad.  The column is compared before
 * it is used, so nothing is read out of bounds. */
__device__ inline void colourVisit(int i, unsigned long long mine, int p, int w, const int* idx, const int* c0, int base, int rows, int* bad,
                                   unsigned long long* used, int* ready)
{
    const unsigned c = (unsigned)idx[p] - (unsigned)base;
    if (c >= (unsigned)rows) {
        *bad = 1;
        return;
    }
    if ((int)c == i)
        return;
    const int theirs = c0[c];
    if (theirs >= 0) {
        const unsigned bit = (unsigned)(theirs - w); /* below the window: wraps to a large number */
        if (bit < 64u)
            *used |= 1ull << bit;
    } else if (colourTuple((int)c) > mine) {
        *ready = 0;
    }
}

/* the end of a round's kernel: every lane brings the nodes it left uncoloured and 1 + its largest colour; one atomic of each per
 * wavefront.  Called outside the row loop, so the whole wavefront takes part in the shuffles. */
__device__ inline void colourTally(int* misc, int left, int top)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        left += laneXor(left, m);
        const int other = laneXor(top, m);
        top = other > top ? other : top;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (left > 0)
            atomicAdd(&misc[0], left);
        if (top > 0)
            atomicMax(&misc[2], top);
    }
}

/* THREAD: one thread per row */
static __global__ __launch_bounds__(kColourThreads) void colourRoundKernel(int* c1, const int* c0, int* misc, int rows, const int* ptr, const int* idx,
                                                                          int base)
{
    int left = 0, top = 0;
    const long long stride = (long long)gridDim.x * kColourThreads;
    for (long long i = (long long)blockIdx.x * kColourThreads + threadIdx.x; i < rows; i += stride) {
        int colour = c0[i];
        if (colour < 0) {
            const unsigned long long mine = colourTuple((int)i);
            const int e0 = ptr[i] - base, e1 = ptr[i + 1] - base;
            for (int w = 0;; w += 64) {
                unsigned long long used = 0;
                int ready = 1;
                for (int p = e0; p < e1; ++p)
                    colourVisit((int)i, mine, p, w, idx, c0, base, rows, misc + 1, &used, &ready);
                if (!ready)
                    break;
                if (~used) {
                    colour = w + __builtin_ctzll(~used);
                    break;
                }
            }
            if (colour < 0)
                ++left;
            else
                top = colour + 1 > top ? colour + 1 : top;
        }
        c1[i] = colour;
    }
    colourTally(misc, left, top);
}

/* GROUP of L lanes of one wavefront per row.  The row index, and with it c0[i], is the same in every lane of a group, and after the
 * shuffles so are `ready` and `used`: a whole group reaches every shuffle together, and a shuffle with a mask below L stays inside
 * the group.  A row longer than L: the lanes stride; a lane without an entry brings ready = 1 and an empty mask. */
static __global__ __launch_bounds__(kColourThreads) void colourRoundGroupKernel(int* c1, const int* c0, int* misc, int rows, const int* ptr,
                                                                               const int* idx, int base, int L)
{
    int left = 0, top = 0;
    const int perBlock = kColourThreads / L, lane = (int)threadIdx.x & (L - 1);
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long i = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; i < rows; i += stride) {
        int colour = c0[i];
        if (colour < 0) {
            const unsigned long long mine = colourTuple((int)i);
            const int e0 = ptr[i] - base, e1 = ptr[i + 1] - base;
            for (int w = 0;; w += 64) {
                unsigned long long used = 0;
                int ready = 1;
                for (int p = e0 + lane; p < e1; p += L)
                    colourVisit((int)i, mine, p, w, idx, c0, base, rows, misc + 1, &used, &ready);
                for (int m = L >> 1; m > 0; m >>= 1) {
                    used |= __shfl_xor(used, m, kWave);
                    ready &= __shfl_xor(ready, m, kWave);
                }
                if (!ready)
                    break;
                if (~used) {
                    colour = w + __builtin_ctzll(~used);
                    break;
                }
            }
            if (lane == 0) {
                if (colour < 0)
                    ++left;
                else
                    top = colour + 1 > top ? colour + 1 : top;
            }
        }
        if (lane == 0)
            c1[i] = colour;
    }
    colourTally(misc, left, top);
}

/* ---- the order ---- */
static __global__ __launch_bounds__(kCvThreads) void colourIotaKernel(int* out, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < rows; i += stride)
        out[i] = (int)i;
}

/* the split by one bit of the colour: flag the listed rows whose colour has the bit 0 ... */
static __global__ __launch_bounds__(kCvThreads) void colourSplitFlagsKernel(int* zero, const int* list, const int* colourOf, int rows, int bit)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long k = (long long)blockIdx.x * kCvThreads + threadIdx.x; k < rows; k += stride)
        zero[k] = (((unsigned)colourOf[list[k]] >> bit) & 1u) ? 0 : 1;
}

/* ... and, with before[k] = the zeros in front of k and *zeros their number, move row list[k] to its place: the zeros keep their
 * order in front, the ones keep theirs behind.  The places are a permutation of [0, rows): one writer each. */
static __global__ __launch_bounds__(kCvThreads) void colourSplitScatterKernel(int* out, const int* list, const int* zero, const int* before,
                                                                             const int* zeros, int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    const int z = *zeros;
    for (long long k = (long long)blockIdx.x * kCvThreads + threadIdx.x; k < rows; k += stride)
        out[zero[k] ? before[k] : z + ((int)k - before[k])] = list[k];
}

/* the sorted list becomes order and inverse; sorted[k] keeps the colour of place k for the bisections below */
static __global__ __launch_bounds__(kCvThreads) void colourOrderKernel(int* order, int* inverse, int* sorted, const int* list, const int* colourOf,
                                                                      int rows)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long k = (long long)blockIdx.x * kCvThreads + threadIdx.x; k < rows; k += stride) {
        const int row = list[k];
        order[k] = row;
        inverse[row] = (int)k;
        sorted[k] = colourOf[row];
    }
}

/* colourPtr[c], c <= count: the first place whose colour is not below c */
static __global__ __launch_bounds__(kCvThreads) void colourPtrKernel(int* colourPtr, const int* sorted, int rows, int count)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long c = (long long)blockIdx.x * kCvThreads + threadIdx.x; c <= count; c += stride)
        colourPtr[c] = lowerBound(sorted, 0, rows, (int)c);
}

/* ---- the permutation ---- */
/* len[k] = the length of row order[k] of A, k < rows; len[rows] = 0, so that the scan's last element is the number of entries */
static __global__ __launch_bounds__(kCvThreads) void permuteLengthsKernel(int* len, int rows, const int* order, const int* aPtr)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long k = (long long)blockIdx.x * kCvThreads + threadIdx.x; k <= rows; k += stride) {
        int length = 0;
        if (k < rows) {
            const int row = order[k];
            length = aPtr[row + 1] - aPtr[row];
        }
        len[k] = length;
    }
}

static __global__ __launch_bounds__(kCvThreads) void permuteRowPtrKernel(int* bPtr, const int* scan, int rows, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long k = (long long)blockIdx.x * kCvThreads + threadIdx.x; k <= rows; k += stride)
        bPtr[k] = scan[k] + base;
}

struct alignas(16) Word16 {
    unsigned long long lo, hi;
};
template <size_t BYTES> struct WordOf;
template <> struct WordOf<4> { typedef unsigned type; };
template <> struct WordOf<8> { typedef unsigned long long type; };
template <> struct WordOf<16> { typedef Word16 type; };

/* The fill, L lanes per row (L = 1: THREAD).  Lane l places the positions = l (mod L) of row order[k]: position p goes to the slot
 * of its rank among (new column, position).  W is the word a value is moved as. */
template <typename W>
__global__ __launch_bounds__(kColourThreads) void permuteFillKernel(int* bIdx, W* bVal, int rows, const int* scan, const int* order, const int* inverse,
                                                                    const int* aPtr, const int* aIdx, const W* aVal, int base, int L)
{
    const int perBlock = kColourThreads / L, lane = (int)threadIdx.x & (L - 1);
    const long long stride = (long long)gridDim.x * perBlock;
    for (long long k = (long long)blockIdx.x * perBlock + (int)threadIdx.x / L; k < rows; k += stride) {
        const int row = order[k];
        const int a0 = aPtr[row] - base, length = aPtr[row + 1] - base - a0, b0 = scan[k];
        for (int p = lane; p < length; p += L) {
            const int column = inverse[aIdx[a0 + p] - base];
            int rank = 0;
            for (int q = 0; q < length; ++q) {
                const int other = inverse[aIdx[a0 + q] - base];
                rank += (other < column || (other == column && q < p)) ? 1 : 0;
            }
            bIdx[b0 + rank] = column + base;
            bVal[b0 + rank] = aVal[a0 + p];
        }
    }
}

struct ColourWork {
    int *misc, *c0, *c1, *a, *b, *totals;
};

static size_t colourPadded(long long n) { return alignUpCv((size_t)(n > 0 ? n : 0), 64); }
static size_t colourTotalsInts(long long n) { return alignUpCv(scanBlocks(n > 0 ? n : 0) + 2, 64); }

static ColourWork carveColour(void* work, int rows)
{
    const size_t R = colourPadded(rows);
    ColourWork w;
    w.misc = static_cast<int*>(work);
    w.c0 = w.misc + kColourMiscInts;
    w.c1 = w.c0 + R;
    w.a = w.c1 + R;
    w.b = w.a + R;
    w.totals = w.b + R;
    return w;
}

template <typename W>
static void launchPermuteFill(hipStream_t s, int* bIdx, void* bVal, int rows, const int* scan, const int* order, const int* inverse, const int* aPtr,
                              const int* aIdx, const void* aVal, int base, int shape, int maxBlocks)
{
    hipLaunchKernelGGL((permuteFillKernel<W>), dim3(colourGrid(rows, shape, maxBlocks)), dim3(kColourThreads), 0, s, bIdx, static_cast<W*>(bVal), rows,
                       scan, order, inverse, aPtr, aIdx, static_cast<const W*>(aVal), base, shape);
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_colour.py and the tests that compare the shapes.  shape: 1 one thread per row, a power
 * of two in [2, 64] that many lanes per row, <= 0 the public call's choice; maxBlocks > 0 caps the grid of every launch that has a
 * shape (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrColourDeviceWith(spgpuHandle_t handle, int* coloursCount, int* roundsCount, int* colourOf, int rowsCount, const int* rowPtr,
                                       const int* colIndices, int baseIndex, void* work, int shape, int maxBlocks);
spgpuStatus_t spgpuCsrPermuteDeviceWith(spgpuHandle_t handle, int* bRowPtr, int* bColIndices, void* bValues, int rowsCount, const int* order,
                                        const int* inverse, const int* aRowPtr, const int* aColIndices, const void* aValues, int baseIndex,
                                        spgpuType_t valuesType, void* work, int shape, int maxBlocks);
int spgpuCsrColourDefaultShape(int rowsCount, int nonZerosCount); /* the rule of colour_rules.h */

int spgpuCsrColourDefaultShape(int rowsCount, int nonZerosCount) { return colourShape(nonZerosCount, rowsCount); }

size_t spgpuCsrColourWorkBytes(int rowsCount)
{
    return (kColourMiscInts + 4 * colourPadded(rowsCount) + colourTotalsInts(rowsCount)) * sizeof(int);
}

size_t spgpuCsrPermuteWorkBytes(int rowsCount)
{
    const long long n = (long long)(rowsCount > 0 ? rowsCount : 0) + 1;
    return (2 * colourPadded(n) + colourTotalsInts(n)) * sizeof(int);
}

spgpuStatus_t spgpuCsrColourDeviceWith(spgpuHandle_t handle, int* coloursCount, int* roundsCount, int* colourOf, int rowsCount, const int* rowPtr,
                                       const int* colIndices, int baseIndex, void* work, int shape, int maxBlocks)
{
    *coloursCount = 0;
    *roundsCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!colourOf || !rowPtr || !colIndices || !work)
        return SPGPU_UNSUPPORTED;
    if (shape > 0 && !colourShapeKnown(shape))
        return SPGPU_UNSUPPORTED;
    const int rows = rowsCount, base = baseIndex;
    hipStream_t s = handle->currentStream;
    const ColourWork w = carveColour(work, rows);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(w.misc, 0, kColourMiscInts * sizeof(int), s);
    hipLaunchKernelGGL(csrSetIntsKernel, dim3(gridFor(rows)), dim3(kCvThreads), 0, s, w.c0, (long long)rows, -1);
    if (shape <= 0) /* the measured rule does not depend on the number of stored entries, so rowPtr[rows] is not fetched for it */
        shape = colourShape(-1, rows);
    const dim3 grid(colourGrid(rows, shape, maxBlocks));
    /* ---- the rounds: the uncoloured node with the largest tuple is coloured in each, so there are at most `rows` ---- */
    int *from = w.c0, *into = w.c1;
    int rounds = 0, left = rows, colours = 0;
    while (left > 0 && rounds < rows) {
        (void)hipMemsetAsync(w.misc, 0, sizeof(int), s);
        if (shape == SPGPU_COLOUR_SHAPE_THREAD)
            hipLaunchKernelGGL(colourRoundKernel, grid, dim3(kColourThreads), 0, s, into, (const int*)from, w.misc, rows, rowPtr, colIndices, base);
        else
            hipLaunchKernelGGL(colourRoundGroupKernel, grid, dim3(kColourThreads), 0, s, into, (const int*)from, w.misc, rows, rowPtr, colIndices, base,
                               shape);
        (void)hipMemcpyAsync(host, w.misc, 3 * sizeof(int), hipMemcpyDeviceToHost, s);
        if (hipStreamSynchronize(s) != hipSuccess)
            return SPGPU_UNSPECIFIED;
        spgpuDebugCheck(handle, "csr colour round");
        ++rounds;
        if (host[1])
            return SPGPU_UNSUPPORTED; /* a column outside the matrix: the first round has seen every entry */
        left = host[0];
        colours = host[2];
        int* const swap = from;
        from = into;
        into = swap;
    }
    if (left > 0 || colours < 1 || colours > rows)
        return SPGPU_UNSPECIFIED;
    (void)hipMemcpyAsync(colourOf, from, (size_t)rows * sizeof(int), hipMemcpyDeviceToDevice, s);
    if (hipStreamSynchronize(s) != hipSuccess) /* `work` may be freed once the call has returned */
        return SPGPU_UNSPECIFIED;
    spgpuDebugCheck(handle, "csr colour");
    *coloursCount = colours;
    *roundsCount = rounds;
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrColourDevice(spgpuHandle_t handle, int* coloursCount, int* roundsCount, int* colourOf, int rowsCount, const int* rowPtr,
                                   const int* colIndices, int baseIndex, void* work)
{
    return spgpuCsrColourDeviceWith(handle, coloursCount, roundsCount, colourOf, rowsCount, rowPtr, colIndices, baseIndex, work, 0, 0);
}

spgpuStatus_t spgpuCsrColourOrderDevice(spgpuHandle_t handle, int* order, int* inverse, int* colourPtr, int rowsCount, int coloursCount,
                                        const int* colourOf, void* work)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!order || !inverse || !colourPtr || !colourOf || !work || coloursCount < 1 || coloursCount > rowsCount)
        return SPGPU_UNSUPPORTED;
    const int rows = rowsCount;
    hipStream_t s = handle->currentStream;
    const ColourWork w = carveColour(work, rows);
    const dim3 rowGrid(gridFor(rows));
    const size_t tiles = scanBlocks(rows);
    int *list = w.c0, *into = w.c1;
    hipLaunchKernelGGL(colourIotaKernel, rowGrid, dim3(kCvThreads), 0, s, list, rows);
    const int bits = bitsFor(coloursCount);
    for (int bit = 0; bit < bits; ++bit) {
        hipLaunchKernelGGL(colourSplitFlagsKernel, rowGrid, dim3(kCvThreads), 0, s, w.a, (const int*)list, colourOf, rows, bit);
        exclusiveScan(s, w.b, w.a, rows, 1, w.totals);
        hipLaunchKernelGGL(colourSplitScatterKernel, rowGrid, dim3(kCvThreads), 0, s, into, (const int*)list, (const int*)w.a, (const int*)w.b,
                           (const int*)(w.totals + tiles), rows);
        int* const swap = list;
        list = into;
        into = swap;
    }
    hipLaunchKernelGGL(colourOrderKernel, rowGrid, dim3(kCvThreads), 0, s, order, inverse, w.a, (const int*)list, colourOf, rows);
    hipLaunchKernelGGL(colourPtrKernel, dim3(gridFor((long long)coloursCount + 1)), dim3(kCvThreads), 0, s, colourPtr, (const int*)w.a, rows,
                       coloursCount);
    spgpuDebugCheck(handle, "csr colour order");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrPermuteDeviceWith(spgpuHandle_t handle, int* bRowPtr, int* bColIndices, void* bValues, int rowsCount, const int* order,
                                        const int* inverse, const int* aRowPtr, const int* aColIndices, const void* aValues, int baseIndex,
                                        spgpuType_t valuesType, void* work, int shape, int maxBlocks)
{
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!forValueType((int)valuesType, [](auto) {}))
        return SPGPU_UNSUPPORTED;
    if (!bRowPtr || !bColIndices || !bValues || !order || !inverse || !aRowPtr || !aColIndices || !aValues || !work)
        return SPGPU_UNSUPPORTED;
    /* The call may not synchronise, so it cannot read the number of stored entries: the public call runs one fixed shape, the one
     * profiles/csr_colour_ab.json backs (colour_rules.h). */
    if (shape <= 0)
        shape = kColourPermuteShape;
    if (!colourShapeKnown(shape))
        return SPGPU_UNSUPPORTED;
    const int rows = rowsCount, base = baseIndex;
    hipStream_t s = handle->currentStream;
    const long long n = (long long)rows + 1;
    int* len = static_cast<int*>(work);
    int* scan = len + colourPadded(n);
    int* totals = scan + colourPadded(n);
    const dim3 ptrGrid(gridFor(n));
    hipLaunchKernelGGL(permuteLengthsKernel, ptrGrid, dim3(kCvThreads), 0, s, len, rows, order, aRowPtr);
    exclusiveScan(s, scan, len, n, 1, totals);
    hipLaunchKernelGGL(permuteRowPtrKernel, ptrGrid, dim3(kCvThreads), 0, s, bRowPtr, (const int*)scan, rows, base);
    forValueType((int)valuesType, [&](auto tag) {
        using W = typename WordOf<sizeof(decltype(tag))>::type; /* double and complex float share the 8-byte kernel */
        launchPermuteFill<W>(s, bColIndices, bValues, rows, scan, order, inverse, aRowPtr, aColIndices, aValues, base, shape, maxBlocks);
    });
    spgpuDebugCheck(handle, "csr permute");
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrPermuteDevice(spgpuHandle_t handle, int* bRowPtr, int* bColIndices, void* bValues, int rowsCount, const int* order,
                                    const int* inverse, const int* aRowPtr, const int* aColIndices, const void* aValues, int baseIndex,
                                    spgpuType_t valuesType, void* work)
{
    return spgpuCsrPermuteDeviceWith(handle, bRowPtr, bColIndices, bValues, rowsCount, order, inverse, aRowPtr, aColIndices, aValues, baseIndex,
                                     valuesType, work, 0, 0);
}

} // extern "C"
