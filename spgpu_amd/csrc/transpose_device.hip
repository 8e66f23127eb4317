/*
 * Device-side transpose of a stored HELL or ELL matrix into HELL arrays, for gfx950 (include/spgpu/ext/transpose_device.h).
 * New functionality; the arrays are byte-identical to what the host converters (conv_ell.c, conv_hell.c) and the COO route
 * (convert_device.hip) give for the COO listing of A^T by ascending matrix row, then ascending slot.
 *
 * Scratch layout (ints), S = slots rounded up to 64:
 *   head[fixedInts(cols)]   misc[16] | colStart[cols+1] | (depth[cols] | scanTotals: spgpuHellPlanDevice's, called in between)
 *   src[fixedInts(rows)]    srcStart[rows+1] | rowLen[rows] | scanTotals
 *   keysA[2S] | keysB[2S]   64-bit sort keys as emitted / sorted: (column << rowBits) | i; a column outside the matrix becomes `cols`
 *   slotA[S] | slotB[S]     the source slot (position in rP) of the entry, as emitted / sorted
 *   rocPRIM temp
 *   misc[0] longest row of A^T, misc[1] bad-input flag
 *
 * Pass A  one lane per storage row: validates rS / rIdx / the reach of the row, rowLen[r] = rS[r]; exclusive scan -> srcStart.
 *         The host reads the entry count (the sort needs it) and the flag.
 * Pass B  the front end: one lane per storage row of a hack, stepping through the slots by hackSize (ELL: by the pitch), so a
 *         wavefront's loads of rP are coalesced; never past rS[r].  Emits key and slot at srcStart[r] + k.
 * Sort    ONE stable radix sort of (key, slot) pairs (rocPRIM).  Entries are emitted by ascending storage row, then slot: without
 *         rIdx that is ascending i already and only the column bits are sorted; with rIdx all bits of the key are.
 * Then    colStart by binary search in the sorted keys (rowStartKernel of convert_scan.hip.h), lengths, longest; the fill writes
 *         the entry at sorted position p to slot p - colStart[column] of its destination row.
 */
#include "convert_scan.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/transpose_device.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace spgpu {

typedef unsigned long long TrKey;

struct TransposeWork {
    int* misc;
    int* colStart;
    int* srcStart;
    int* rowLen;
    int* srcTotals;
    TrKey *keysA, *keysB;
    int *slotA, *slotB;
    void* temp;
};

/* How the slots of the source are addressed: HELL (pitch == 0) through hackOffsets, ELL by r + k * pitch. */
struct SourceLayout {
    const int* hackOffsets;
    int hackSize;
    int pitch;
    __device__ long long first(int r) const
    {
        if (pitch)
            return r;
        const int hack = r / hackSize;
        return (long long)hackOffsets[hack] + (r - hack * hackSize);
    }
    __host__ __device__ int step() const { return pitch ? pitch : hackSize; }
};

static size_t slotInts(int slots) { return alignUpCv((size_t)(slots > 0 ? slots : 0), 64); }

static TransposeWork carveTranspose(void* work, int rows, int cols, int slots)
{
    TransposeWork w;
    int* p = static_cast<int*>(work);
    w.misc = p;
    w.colStart = p + 16;
    p += fixedInts(cols);
    w.srcStart = p;
    w.rowLen = p + (size_t)rows + 1;
    w.srcTotals = w.rowLen + (size_t)rows;
    p += fixedInts(rows);
    const size_t S = slotInts(slots);
    w.keysA = reinterpret_cast<TrKey*>(p);
    p += 2 * S;
    w.keysB = reinterpret_cast<TrKey*>(p);
    p += 2 * S;
    w.slotA = p;
    p += S;
    w.slotB = p;
    p += S;
    w.temp = p;
    return w;
}

static hipError_t transposeSortTempBytes(size_t n, size_t* bytes)
{
    size_t need = 0;
    const hipError_t err = rocprim::radix_sort_pairs(nullptr, need, (const TrKey*)nullptr, (TrKey*)nullptr, (const int*)nullptr,
                                                     (int*)nullptr, n);
    *bytes = alignUpCv(need, 256);
    return err;
}

/* smallest b with 2^b >= n (n >= 1) */
static int bitsFor(long long n)
{
    int b = 0;
    while (((long long)1 << b) < n)
        ++b;
    return b;
}

/* Pass A: rowLen[r] = rS[r] where the row can be read, 0 and the flag otherwise. */
__global__ __launch_bounds__(kCvThreads) void sourceRowsKernel(int* rowLen, int* misc, SourceLayout src, const int* rS,
                                                               const int* rIdx, int rows, int slots)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long t = (long long)blockIdx.x * kCvThreads + threadIdx.x; t < rows; t += stride) {
        const int r = (int)t;
        const int len = rS[r];
        bool bad = len < 0;
        if (rIdx)
            bad |= (unsigned)rIdx[r] >= (unsigned)rows;
        if (len > 0) {
            const long long first = src.first(r);
            bad |= first < 0 || first + (long long)(len - 1) * src.step() >= (long long)slots;
        }
        rowLen[r] = bad ? 0 : len;
        if (bad)
            misc[1] = 1;
    }
}

/* Pass B: lane r walks the slots of storage row r; lanes of a wavefront read consecutive words of rP at every step. */
__global__ __launch_bounds__(kCvThreads) void emitKeysKernel(TrKey* keys, int* slotOf, SourceLayout src, const int* rP,
                                                             const int* rowLen, const int* srcStart, const int* rIdx, int rows,
                                                             int cols, int base, int rowBits)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long t = (long long)blockIdx.x * kCvThreads + threadIdx.x; t < rows; t += stride) {
        const int r = (int)t;
        const int len = rowLen[r];
        if (len <= 0)
            continue;
        const TrKey i = (TrKey)(unsigned)(rIdx ? rIdx[r] : r);
        const long long first = src.first(r);
        const int step = src.step();
        const long long out = srcStart[r];
        for (int k = 0; k < len; ++k) {
            const long long a = first + (long long)k * step;
            const unsigned c = (unsigned)(rP[a] - base);
            keys[out + k] = ((TrKey)(c < (unsigned)cols ? c : (unsigned)cols) << rowBits) | i;
            slotOf[out + k] = (int)a;
        }
    }
}

/* misc[0] = the longest row of A^T, misc[1] set if some key carries a column outside the matrix; tLengths is not touched yet */
__global__ __launch_bounds__(kCvThreads) void columnMaxKernel(const int* colStart, int cols, int nnz, int* misc)
{
    int best = 0;
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long j = (long long)blockIdx.x * kCvThreads + threadIdx.x; j < cols; j += stride) {
        const int len = colStart[j + 1] - colStart[j];
        best = len > best ? len : best;
    }
    best = waveMax(best);
    if ((threadIdx.x & (kWave - 1)) == 0 && best > 0)
        atomicMax(&misc[0], best);
    if (blockIdx.x == 0 && threadIdx.x == 0 && colStart[cols] < nnz)
        misc[1] = 1;
}

struct Words128 { unsigned long long lo, hi; };

/* One thread per sorted position: destination row j = column of the entry, place k = p - colStart[j]. */
template <typename ELEM>
__global__ __launch_bounds__(kCvThreads) void transposeFillKernel(ELEM* tValues, int* tIndices, const int* tHackOffsets, int tHackSize,
                                                                  int tBase, const ELEM* cM, int valuesPitch, int indicesPitch,
                                                                  int cols, const int* misc, const int* colStart,
                                                                  const TrKey* keys, const int* slotOf, int rowBits)
{
    if (misc[1])
        return; /* the lengths call refused the source */
    const long long stride = (long long)gridDim.x * kCvThreads;
    const int valid = colStart[cols];
    const TrKey rowMask = ((TrKey)1 << rowBits) - 1;
    for (long long p = (long long)blockIdx.x * kCvThreads + threadIdx.x; p < valid; p += stride) {
        const TrKey key = keys[p];
        const int j = (int)(key >> rowBits);
        const int i = (int)(key & rowMask);
        const int k = (int)p - colStart[j];
        const int a = slotOf[p];
        const long long from = indicesPitch ? (long long)(a % indicesPitch) + (long long)(a / indicesPitch) * valuesPitch : (long long)a;
        const int hack = j / tHackSize;
        const long long slot = (long long)tHackOffsets[hack] + (j - hack * tHackSize) + (long long)k * tHackSize;
        tIndices[slot] = i + tBase;
        tValues[slot] = cM[from];
    }
}

static spgpuStatus_t transposeLengths(spgpuHandle_t handle, int* tLengths, int* maxRowSize, int* nonZerosCount, const int* rP,
                                      SourceLayout src, const int* rS, const int* rIdx, int rows, int cols, int base, int slots,
                                      void* work)
{
    *maxRowSize = 0;
    *nonZerosCount = 0;
    if (rows <= 0 || cols <= 0)
        return SPGPU_SUCCESS;
    if (src.step() <= 0 || !rS || !work)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const TransposeWork w = carveTranspose(work, rows, cols, slots);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(w.misc, 0, 16 * sizeof(int), s);
    hipLaunchKernelGGL(sourceRowsKernel, dim3(gridFor(rows)), dim3(kCvThreads), 0, s, w.rowLen, w.misc, src, rS, rIdx, rows, slots);
    exclusiveScan(s, w.srcStart, w.rowLen, (long long)rows, 1, w.srcTotals);
    (void)hipMemcpyAsync(host, w.srcTotals + scanBlocks(rows), sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(host + 1, w.misc + 1, sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    const int nnz = host[0];
    if (host[1] || nnz < 0 || nnz > slots) {
        (void)hipMemsetAsync(w.misc + 1, 0xff, sizeof(int), s); /* a fill on this work writes nothing */
        spgpuDebugCheck(handle, "transpose lengths");
        return SPGPU_UNSUPPORTED;
    }
    if (nnz == 0) {
        (void)hipMemsetAsync(w.colStart, 0, ((size_t)cols + 1) * sizeof(int), s);
        (void)hipMemsetAsync(tLengths, 0, (size_t)cols * sizeof(int), s);
        spgpuDebugCheck(handle, "transpose lengths");
        return SPGPU_SUCCESS;
    }
    const int rowBits = bitsFor(rows), colBits = bitsFor((long long)cols + 1);
    hipLaunchKernelGGL(emitKeysKernel, dim3(gridFor(rows)), dim3(kCvThreads), 0, s, w.keysA, w.slotA, src, rP, (const int*)w.rowLen,
                       (const int*)w.srcStart, rIdx, rows, cols, base, rowBits);
    size_t bytes = 0, room = 0; /* `work` was sized for `slots` entries: never hand rocPRIM more than that gave it */
    if (transposeSortTempBytes((size_t)nnz, &bytes) != hipSuccess || transposeSortTempBytes((size_t)slots, &room) != hipSuccess ||
        bytes > room)
        return SPGPU_UNSPECIFIED;
    if (rocprim::radix_sort_pairs(w.temp, bytes, (const TrKey*)w.keysA, w.keysB, (const int*)w.slotA, w.slotB, (size_t)nnz,
                                  (unsigned)(rIdx ? 0 : rowBits), (unsigned)(rowBits + colBits), s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    hipLaunchKernelGGL(rowStartKernel<TrKey>, dim3(gridFor((long long)cols + 1)), dim3(kCvThreads), 0, s, w.colStart, cols,
                       (const TrKey*)w.keysB, rowBits, nnz);
    hipLaunchKernelGGL(columnMaxKernel, dim3(gridFor(cols)), dim3(kCvThreads), 0, s, (const int*)w.colStart, cols, nnz, w.misc);
    (void)hipMemcpyAsync(host, w.misc, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "transpose lengths");
    if (host[1])
        return SPGPU_UNSUPPORTED; /* a stored column outside the matrix: misc[1] stays set, tLengths untouched */
    hipLaunchKernelGGL(rowLengthsKernel, dim3(gridFor(cols)), dim3(kCvThreads), 0, s, tLengths, (const int*)w.colStart, cols, nnz, w.misc);
    *maxRowSize = host[0];
    *nonZerosCount = nnz;
    return SPGPU_SUCCESS;
}

static spgpuStatus_t transposeFill(spgpuHandle_t handle, void* tValues, int* tIndices, const int* tHackOffsets, int tHackSize,
                                   int tBase, const void* cM, int valuesPitch, int indicesPitch, int rows, int cols, int slots,
                                   spgpuType_t type, void* work)
{
    if (rows <= 0 || cols <= 0)
        return SPGPU_SUCCESS;
    const size_t size = spgpuSizeOf(type);
    if ((size != 4 && size != 8 && size != 16) || tHackSize <= 0 || !work)
        return SPGPU_UNSUPPORTED;
    if (slots <= 0)
        return SPGPU_SUCCESS; /* no stored slot, no entry */
    hipStream_t s = handle->currentStream;
    const TransposeWork w = carveTranspose(work, rows, cols, slots);
    const int rowBits = bitsFor(rows);
    const dim3 grid(gridFor(slots)), block(kCvThreads);
    switch (size) {
    case 4:
        hipLaunchKernelGGL(transposeFillKernel<unsigned>, grid, block, 0, s, static_cast<unsigned*>(tValues), tIndices, tHackOffsets,
                           tHackSize, tBase, static_cast<const unsigned*>(cM), valuesPitch, indicesPitch, cols, (const int*)w.misc,
                           (const int*)w.colStart, (const TrKey*)w.keysB, (const int*)w.slotB, rowBits);
        break;
    case 8:
        hipLaunchKernelGGL(transposeFillKernel<unsigned long long>, grid, block, 0, s, static_cast<unsigned long long*>(tValues),
                           tIndices, tHackOffsets, tHackSize, tBase, static_cast<const unsigned long long*>(cM), valuesPitch,
                           indicesPitch, cols, (const int*)w.misc, (const int*)w.colStart, (const TrKey*)w.keysB, (const int*)w.slotB,
                           rowBits);
        break;
    default:
        hipLaunchKernelGGL(transposeFillKernel<Words128>, grid, block, 0, s, static_cast<Words128*>(tValues), tIndices, tHackOffsets,
                           tHackSize, tBase, static_cast<const Words128*>(cM), valuesPitch, indicesPitch, cols, (const int*)w.misc,
                           (const int*)w.colStart, (const TrKey*)w.keysB, (const int*)w.slotB, rowBits);
        break;
    }
    spgpuDebugCheck(handle, "transpose fill");
    return SPGPU_SUCCESS;
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

size_t spgpuHellTransposeWorkBytes(int rowsCount, int columnsCount, int slots)
{
    const int rows = rowsCount > 0 ? rowsCount : 0, cols = columnsCount > 0 ? columnsCount : 0;
    size_t temp = 0;
    if (slots > 0 && transposeSortTempBytes((size_t)slots, &temp) != hipSuccess)
        return 0; /* no GPU to ask for rocPRIM's share */
    return (fixedInts(cols) + fixedInts(rows) + 6 * slotInts(slots)) * sizeof(int) + temp + 256;
}

spgpuStatus_t spgpuHellTransposeLengthsDevice(spgpuHandle_t handle, int* tLengths, int* maxRowSize, int* nonZerosCount,
                                              const int* rP, int hackSize, const int* hackOffsets, const int* rS, const int* rIdx,
                                              int rowsCount, int columnsCount, int baseIndex, int slots, void* work)
{
    return transposeLengths(handle, tLengths, maxRowSize, nonZerosCount, rP, SourceLayout{hackOffsets, hackSize, 0}, rS, rIdx,
                            rowsCount, columnsCount, baseIndex, slots, work);
}

spgpuStatus_t spgpuHellTransposeDevice(spgpuHandle_t handle, void* tValues, int* tIndices, const int* tHackOffsets, int tHackSize,
                                       int tBaseIndex, const void* cM, const int* rP, int hackSize, const int* hackOffsets,
                                       const int* rS, const int* rIdx, int rowsCount, int columnsCount, int baseIndex, int slots,
                                       spgpuType_t valuesType, const int* tLengths, void* work)
{
    (void)rP, (void)hackSize, (void)hackOffsets, (void)rS, (void)rIdx, (void)baseIndex, (void)tLengths; /* all in `work` by now */
    return transposeFill(handle, tValues, tIndices, tHackOffsets, tHackSize, tBaseIndex, cM, 0, 0, rowsCount, columnsCount, slots,
                         valuesType, work);
}

spgpuStatus_t spgpuEllTransposeLengthsDevice(spgpuHandle_t handle, int* tLengths, int* maxRowSize, int* nonZerosCount,
                                             const int* rP, int ellIndicesPitch, const int* rS, const int* rIdx, int rowsCount,
                                             int columnsCount, int baseIndex, int slots, void* work)
{
    if (rowsCount > 0 && columnsCount > 0 && ellIndicesPitch < rowsCount) {
        *maxRowSize = 0;
        *nonZerosCount = 0;
        return SPGPU_UNSUPPORTED;
    }
    return transposeLengths(handle, tLengths, maxRowSize, nonZerosCount, rP, SourceLayout{nullptr, 0, ellIndicesPitch}, rS, rIdx,
                            rowsCount, columnsCount, baseIndex, slots, work);
}

spgpuStatus_t spgpuEllTransposeDevice(spgpuHandle_t handle, void* tValues, int* tIndices, const int* tHackOffsets, int tHackSize,
                                      int tBaseIndex, const void* cM, const int* rP, int ellValuesPitch, int ellIndicesPitch,
                                      const int* rS, const int* rIdx, int rowsCount, int columnsCount, int baseIndex, int slots,
                                      spgpuType_t valuesType, const int* tLengths, void* work)
{
    (void)rP, (void)rS, (void)rIdx, (void)baseIndex, (void)tLengths;
    if (rowsCount > 0 && columnsCount > 0 && (ellIndicesPitch < rowsCount || ellValuesPitch < rowsCount))
        return SPGPU_UNSUPPORTED;
    return transposeFill(handle, tValues, tIndices, tHackOffsets, tHackSize, tBaseIndex, cM, ellValuesPitch, ellIndicesPitch,
                         rowsCount, columnsCount, slots, valuesType, work);
}

} // extern "C"
