/*
 * Device-side CSR -> ELL / HELL construction for gfx950 (include/spgpu/ext/csr_device.h).
 * New functionality; the arrays are byte-identical to the COO route's (convert_device.hip) for the same matrix as row-major
 * COO, and so to the host converters' (conv_ell.c, conv_hell.c; reference ell.c:5-80, hell.c:4-104).
 *
 * The conversion is a transposition.  On the CSR side a row is a contiguous run of entries; on the slab side a slab column
 * is a contiguous run of 32 rows (hackSize in general).  One thread per entry coalesces the reads and scatters the writes
 * (placeKernel of the COO route); one thread per row does the opposite (csrRowFillKernel below, the plain fill).
 *
 * THE TRANSPOSING FILL (csrTransposeFillKernel): a wavefront owns a GROUP of up to 32 destination rows of one hack (a hack of
 * hackSize rows is ceil(hackSize / 32) groups; ELL is a single hack of pitch ellValuesPitch / ellIndicesPitch) and walks it in
 * chunks of kCsrChunk = 16 slab columns:
 *   read    8 passes; in a pass the 64 lanes are 4 rows x 16 consecutive entries of each row's run: for fp64 a 128-byte run
 *           of values and a 64-byte run of columns per row.  Element loads: a run starts at any element offset;
 *   park    entry k of row r goes to tile[k * kCsrTileLd + r] in LDS.  kCsrTileLd = 36: the 16 k of a pass fall 4 banks
 *           apart (two to a bank in a 32-lane group, which a 4-byte LDS store takes at full rate), and the read-out has
 *           lanes along r, consecutive words;
 *   write   8 steps; in a step the 64 lanes are 2 slab columns x 32 rows: whole 128-byte (4-byte types and the indices) or
 *           256-byte runs, and with hackSize == 32 the 16 columns of the chunk are one contiguous block.  A slot beyond its
 *           row's end is not written (the caller zeroed it).
 * A row of any length is so many chunks: no LDS that grows with the row.  A row order changes only where a row's run starts.
 * Lengths come from csrRowPtr.  No atomics, each slot has one writer: the arrays do not depend on scheduling.  A wavefront's
 * tile is its own; its LDS operations execute in order, the wave barriers only keep the compiler from moving them.
 */
#include "csr_host.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/csr_device.h"

namespace spgpu {

constexpr int kCsrThreads = 256;
constexpr int kCsrWaves = kCsrThreads / kWave;
constexpr int kCsrGroupRows = 32;                                   /* destination rows a wavefront owns */
constexpr int kCsrChunk = 16;                                       /* slab columns per trip */
constexpr int kCsrTileLd = 36;                                      /* padded row count of the LDS tile */
constexpr int kCsrReadPasses = kCsrGroupRows * kCsrChunk / kWave;   /* 8: 4 rows x 16 entries per pass */
constexpr int kCsrWriteSteps = kCsrGroupRows * kCsrChunk / kWave;   /* 8: 2 columns x 32 rows per step */
constexpr int kCsrRowsPerPass = kWave / kCsrChunk;                  /* 4 */
constexpr int kCsrColsPerStep = kWave / kCsrGroupRows;              /* 2 */

enum { SPGPU_CSR_FILL_PLAIN = 0, SPGPU_CSR_FILL_TRANSPOSE = 1 };
constexpr int kCsrDefaultFill = SPGPU_CSR_FILL_TRANSPOSE;

struct CsrBits128 { unsigned long long lo, hi; };

/* Where the slots of the destination lie.  HELL: slot(row, k) = hackOffsets[row / hackSize] + row % hackSize + k * hackSize;
 * ELL (hackOffsets == NULL): row + k * pitch, with a pitch each for values and indices. */
struct CsrSlabs {
    const int* hackOffsets;
    int hackSize;
    long long valStride, idxStride;
};

/* The run of CSR entries that becomes destination row `row`: first entry (0-based) and length.  A row pointer that descends
 * or an order entry outside the matrix gives an empty row. */
__device__ inline void csrRunOf(int row, int rows, const int* rowPtr, int csrBase, const int* rIdx, int& start, int& len)
{
    start = 0;
    len = 0;
    const int src = rIdx ? rIdx[row] : row;
    if ((unsigned)src < (unsigned)rows) {
        const int a = rowPtr[src], b = rowPtr[src + 1];
        start = a - csrBase;
        len = b > a ? b - a : 0;
    }
}

/* The plain fill: one thread per destination row.  Neighbouring lanes write neighbouring slots; each reads its own run. */
template <typename ELEM, bool TO_HELL>
__global__ __launch_bounds__(kCsrThreads) void csrRowFillKernel(ELEM* values, int* indices, CsrSlabs slabs, int outBase, int rows,
                                                                const int* rowPtr, const int* csrCols, const ELEM* csrVals,
                                                                int csrBase, const int* rIdx)
{
    const long long stride = (long long)gridDim.x * kCsrThreads;
    for (long long row = (long long)blockIdx.x * kCsrThreads + threadIdx.x; row < rows; row += stride) {
        int start, len;
        csrRunOf((int)row, rows, rowPtr, csrBase, rIdx, start, len);
        long long slot = row;
        if constexpr (TO_HELL) {
            const int hack = (int)(row / slabs.hackSize);
            slot = (long long)slabs.hackOffsets[hack] + (row - (long long)hack * slabs.hackSize);
        }
        for (int k = 0; k < len; ++k) {
            indices[slot + k * slabs.idxStride] = csrCols[start + k] - csrBase + outBase;
            values[slot + k * slabs.valStride] = csrVals[start + k];
        }
    }
}

/* The transposing fill (head of the file).  `groups` = hacks * subsPerHack groups of up to 32 rows, grid-strided by wavefront. */
template <typename ELEM, bool TO_HELL>
__global__ __launch_bounds__(kCsrThreads) void csrTransposeFillKernel(ELEM* values, int* indices, CsrSlabs slabs, int subsPerHack,
                                                                      long long groups, int outBase, int rows, const int* rowPtr,
                                                                      const int* csrCols, const ELEM* csrVals, int csrBase,
                                                                      const int* rIdx)
{
    __shared__ ELEM tileVals[kCsrWaves][kCsrChunk * kCsrTileLd];
    __shared__ int tileCols[kCsrWaves][kCsrChunk * kCsrTileLd];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    ELEM* tv = tileVals[wave];
    int* tc = tileCols[wave];
    const int myRow = lane & (kCsrGroupRows - 1);        /* write side: lanes along the rows ... */
    const int myCol = lane / kCsrGroupRows;              /* ... 2 slab columns per step */
    const int readK = lane & (kCsrChunk - 1);            /* read side: lanes along a row's run ... */
    const int readRow = lane / kCsrChunk;                /* ... 4 rows per pass */
    const long long stride = (long long)gridDim.x * kCsrWaves;
    for (long long g = (long long)blockIdx.x * kCsrWaves + wave; g < groups; g += stride) {
        long long firstRow, slot0;
        int rowsHere;
        if constexpr (TO_HELL) {
            const long long hack = g / subsPerHack;
            const int inHack = (int)(g - hack * subsPerHack) * kCsrGroupRows;
            firstRow = hack * slabs.hackSize + inHack;
            rowsHere = slabs.hackSize - inHack;
            if (firstRow >= rows) /* wavefront-uniform: the last hack is partly filled */
                continue;
            slot0 = (long long)slabs.hackOffsets[hack] + inHack;
        } else {
            firstRow = g * kCsrGroupRows;
            rowsHere = kCsrGroupRows;
            slot0 = firstRow;
        }
        if (rowsHere > kCsrGroupRows)
            rowsHere = kCsrGroupRows;
        if (rowsHere > rows - firstRow)
            rowsHere = (int)(rows - firstRow);
        int start = 0, len = 0; /* of row firstRow + myRow: both halves of the wavefront hold it */
        if (myRow < rowsHere)
            csrRunOf((int)firstRow + myRow, rows, rowPtr, csrBase, rIdx, start, len);
        const int longest = waveMax(len);
        for (int k0 = 0; k0 < longest; k0 += kCsrChunk) {
            int col[kCsrReadPasses];
            ELEM val[kCsrReadPasses];
            bool mine[kCsrReadPasses];
#pragma unroll
            for (int p = 0; p < kCsrReadPasses; ++p) {
                const int r = p * kCsrRowsPerPass + readRow;
                const int from = __shfl(start, r, kWave), have = __shfl(len, r, kWave);
                mine[p] = k0 + readK < have;
                if (mine[p]) {
                    col[p] = csrCols[(long long)from + k0 + readK];
                    val[p] = csrVals[(long long)from + k0 + readK];
                }
            }
            __builtin_amdgcn_wave_barrier(); /* the previous trip's read-out precedes these stores */
#pragma unroll
            for (int p = 0; p < kCsrReadPasses; ++p)
                if (mine[p]) {
                    tc[readK * kCsrTileLd + p * kCsrRowsPerPass + readRow] = col[p] - csrBase + outBase;
                    tv[readK * kCsrTileLd + p * kCsrRowsPerPass + readRow] = val[p];
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int s = 0; s < kCsrWriteSteps; ++s) {
                const int kk = s * kCsrColsPerStep + myCol;
                if (k0 + kk < len) {
                    indices[slot0 + myRow + (long long)(k0 + kk) * slabs.idxStride] = tc[kk * kCsrTileLd + myRow];
                    values[slot0 + myRow + (long long)(k0 + kk) * slabs.valStride] = tv[kk * kCsrTileLd + myRow];
                }
            }
        }
    }
}

/* differences, their maximum and the two checks in one grid-strided pass; misc[0] longest row, misc[1] != 0: csrRowPtr[0] is
 * not the base or the pointers descend somewhere */
__global__ __launch_bounds__(kCsrThreads) void csrRowLengthsKernel(int* rowLengths, int rows, const int* rowPtr, int csrBase, int* misc)
{
    int best = 0, bad = 0;
    const long long stride = (long long)gridDim.x * kCsrThreads;
    for (long long r = (long long)blockIdx.x * kCsrThreads + threadIdx.x; r < rows; r += stride) {
        const int a = rowPtr[r], b = rowPtr[r + 1];
        rowLengths[r] = b - a;
        best = b - a > best ? b - a : best;
        bad |= (b < a) | (r == 0 && a != csrBase);
    }
    best = waveMax(best);
    bad = waveMax(bad);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (best > 0)
            atomicMax(&misc[0], best);
        if (bad)
            atomicMax(&misc[1], 1);
    }
}

template <typename ELEM, bool TO_HELL>
static void launchCsrFill(hipStream_t s, void* values, int* indices, const CsrSlabs& slabs, int outBase, int rows, const int* rowPtr,
                          const int* csrCols, const void* csrVals, int csrBase, const int* rIdx, int fill, int maxBlocks)
{
    if (fill == SPGPU_CSR_FILL_PLAIN) {
        hipLaunchKernelGGL((csrRowFillKernel<ELEM, TO_HELL>), dim3(cappedGrid(rows, kCsrThreads, maxBlocks)), dim3(kCsrThreads), 0, s,
                           static_cast<ELEM*>(values), indices, slabs, outBase, rows, rowPtr, csrCols, static_cast<const ELEM*>(csrVals),
                           csrBase, rIdx);
        return;
    }
    const int subsPerHack = TO_HELL ? (slabs.hackSize + kCsrGroupRows - 1) / kCsrGroupRows : 1;
    const long long hacks = TO_HELL ? ((long long)rows + slabs.hackSize - 1) / slabs.hackSize : ((long long)rows + kCsrGroupRows - 1) / kCsrGroupRows;
    const long long groups = hacks * subsPerHack;
    hipLaunchKernelGGL((csrTransposeFillKernel<ELEM, TO_HELL>), dim3(cappedGrid(groups, kCsrWaves, maxBlocks)), dim3(kCsrThreads), 0, s,
                       static_cast<ELEM*>(values), indices, slabs, subsPerHack, groups, outBase, rows, rowPtr, csrCols,
                       static_cast<const ELEM*>(csrVals), csrBase, rIdx);
}

template <bool TO_HELL>
static spgpuStatus_t csrFill(spgpuHandle_t handle, void* values, int* indices, const CsrSlabs& slabs, int outBase, int rows,
                             const int* rowPtr, const int* csrCols, const void* csrVals, int csrBase, spgpuType_t type,
                             const int* rIdx, int fill, int maxBlocks)
{
    if (rows <= 0)
        return SPGPU_SUCCESS;
    if (TO_HELL && slabs.hackSize <= 0)
        return SPGPU_UNSUPPORTED;
    if (fill != SPGPU_CSR_FILL_PLAIN && fill != SPGPU_CSR_FILL_TRANSPOSE)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    switch (spgpuSizeOf(type)) {
    case 4:
        launchCsrFill<unsigned, TO_HELL>(s, values, indices, slabs, outBase, rows, rowPtr, csrCols, csrVals, csrBase, rIdx, fill, maxBlocks);
        break;
    case 8:
        launchCsrFill<unsigned long long, TO_HELL>(s, values, indices, slabs, outBase, rows, rowPtr, csrCols, csrVals, csrBase, rIdx, fill,
                                                   maxBlocks);
        break;
    case 16:
        launchCsrFill<CsrBits128, TO_HELL>(s, values, indices, slabs, outBase, rows, rowPtr, csrCols, csrVals, csrBase, rIdx, fill,
                                           maxBlocks);
        break;
    default:
        return SPGPU_UNSUPPORTED;
    }
    spgpuDebugCheck(handle, "csr conversion");
    return SPGPU_SUCCESS;
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_convert_csr.py and the tests that compare the two fills.  fill: 0 the plain
 * fill, 1 the transposing fill; maxBlocks > 0 caps the grid (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrToEllDeviceWith(spgpuHandle_t handle, void* ellValues, int* ellIndices, int ellValuesPitch,
                                      int ellIndicesPitch, int ellBaseIndex, int rowsCount, const int* csrRowPtr,
                                      const int* csrColIndices, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                      const int* rIdx, int fill, int maxBlocks);
spgpuStatus_t spgpuCsrToHellDeviceWith(spgpuHandle_t handle, void* hellValues, int* hellIndices, const int* hackOffsets,
                                       int hackSize, int hellBaseIndex, int rowsCount, const int* csrRowPtr,
                                       const int* csrColIndices, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                       const int* rIdx, int fill, int maxBlocks);
/* slab columns per trip of the transposing fill, and the fill the public calls run */
int spgpuCsrFillChunk(void);
int spgpuCsrDefaultFill(void);

int spgpuCsrFillChunk(void) { return kCsrChunk; }
int spgpuCsrDefaultFill(void) { return kCsrDefaultFill; }

spgpuStatus_t spgpuCsrRowLengthsDevice(spgpuHandle_t handle, int* rowLengths, int* maxRowSize, int rowsCount, const int* csrRowPtr,
                                       int csrBaseIndex)
{
    if (maxRowSize)
        *maxRowSize = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!maxRowSize)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    /* the handle's reduction scratch and its pinned mirror: one reduction of a handle at a time, as everywhere */
    int* misc = static_cast<int*>(spgpuPrivate(handle)->reduceScratch);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(misc, 0, 2 * sizeof(int), s);
    hipLaunchKernelGGL(csrRowLengthsKernel, dim3(cappedGrid(rowsCount, kCsrThreads, 4096)), dim3(kCsrThreads), 0, s, rowLengths, rowsCount,
                       csrRowPtr, csrBaseIndex, misc);
    (void)hipMemcpyAsync(host, misc, 2 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "csr row lengths");
    if (host[1])
        return SPGPU_UNSUPPORTED;
    *maxRowSize = host[0];
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrToEllDeviceWith(spgpuHandle_t handle, void* ellValues, int* ellIndices, int ellValuesPitch,
                                      int ellIndicesPitch, int ellBaseIndex, int rowsCount, const int* csrRowPtr,
                                      const int* csrColIndices, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                      const int* rIdx, int fill, int maxBlocks)
{
    const CsrSlabs slabs = {nullptr, 0, ellValuesPitch, ellIndicesPitch};
    return csrFill<false>(handle, ellValues, ellIndices, slabs, ellBaseIndex, rowsCount, csrRowPtr, csrColIndices, csrValues,
                          csrBaseIndex, valuesType, rIdx, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrToHellDeviceWith(spgpuHandle_t handle, void* hellValues, int* hellIndices, const int* hackOffsets,
                                       int hackSize, int hellBaseIndex, int rowsCount, const int* csrRowPtr,
                                       const int* csrColIndices, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                       const int* rIdx, int fill, int maxBlocks)
{
    const CsrSlabs slabs = {hackOffsets, hackSize, hackSize, hackSize};
    return csrFill<true>(handle, hellValues, hellIndices, slabs, hellBaseIndex, rowsCount, csrRowPtr, csrColIndices, csrValues,
                         csrBaseIndex, valuesType, rIdx, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrToEllDevice(spgpuHandle_t handle, void* ellValues, int* ellIndices, int ellValuesPitch, int ellIndicesPitch,
                                  int ellBaseIndex, int rowsCount, const int* csrRowPtr, const int* csrColIndices,
                                  const void* csrValues, int csrBaseIndex, spgpuType_t valuesType, const int* rIdx)
{
    return spgpuCsrToEllDeviceWith(handle, ellValues, ellIndices, ellValuesPitch, ellIndicesPitch, ellBaseIndex, rowsCount, csrRowPtr,
                                   csrColIndices, csrValues, csrBaseIndex, valuesType, rIdx, kCsrDefaultFill, 0);
}

spgpuStatus_t spgpuCsrToHellDevice(spgpuHandle_t handle, void* hellValues, int* hellIndices, const int* hackOffsets, int hackSize,
                                   int hellBaseIndex, int rowsCount, const int* csrRowPtr, const int* csrColIndices,
                                   const void* csrValues, int csrBaseIndex, spgpuType_t valuesType, const int* rIdx)
{
    return spgpuCsrToHellDeviceWith(handle, hellValues, hellIndices, hackOffsets, hackSize, hellBaseIndex, rowsCount, csrRowPtr,
                                    csrColIndices, csrValues, csrBaseIndex, valuesType, rIdx, kCsrDefaultFill, 0);
}

} // extern "C"
