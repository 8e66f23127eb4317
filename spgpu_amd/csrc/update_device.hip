/*
 * New coefficients for a stored HELL / ELL matrix on gfx950 (include/spgpu/ext/update_device.h).  New functionality: the value
 * refill writes the bytes spgpuCsrToHellDevice / spgpuCsrToEllDevice (convert_csr_device.hip) would write into the value
 * array and touches no column index; spgpu?hellcsput is ellCsputKernel (ell_csput.hip.h) on HELL storage, with a row order.
 *
 * THE TRANSPOSING REFILL (csrValuesTransposeKernel) has the shape of csrTransposeFillKernel -- a wavefront owns a GROUP of up
 * to 32 destination rows of one hack (ELL: one hack of pitch ellValuesPitch) and walks it in chunks of kUpChunk = 16 slab
 * columns -- with the index stream gone and the write side widened:
 *   read    8 passes; in a pass the 64 lanes are 4 rows x 16 consecutive entries of each row's run (fp64: a 128-byte run per
 *           row).  Element loads: a run starts at any element offset, csrValues has the alignment of its element only;
 *   park    entry k of row r goes to tile[k * kUpTileLd + r] in LDS.  kUpTileLd = 36 as in the full fill (the 16 k of a pass
 *           fall 4 banks apart), and 36 elements of 4, 8 or 16 bytes are a multiple of 16 bytes: every slab column of the
 *           tile starts on a 16-byte boundary;
 *   write   WIDE, when the group's first slot is 16-byte aligned and the slab-column stride is a multiple of 16 bytes
 *           (wavefront-uniform; always so for hackSize % 32 == 0 and a 16-byte aligned cM): a lane takes 16 bytes -- 4, 2 or 1
 *           neighbouring rows of one slab column -- from LDS in one read and stores them in one 16-byte store, so the 64
 *           lanes write 1 KiB, 8 / 4 / 2 whole slab columns, per instruction; with hackSize == 32 that is one contiguous
 *           run.  A lane whose rows do not all reach the column stores the live ones element by element: a slot beyond its
 *           row's end is not written.  Otherwise NARROW: 8 steps of 2 slab columns x 32 rows, element stores, as the full fill.
 * A row of any length is so many chunks: no LDS that grows with the row.  A row order changes only where a row's run starts.
 * Lengths come from csrRowPtr.  No atomics, each slot has one writer.  A wavefront's tile is its own; its LDS operations
 * execute in order, the wave barriers only keep the compiler from moving them.
 *
 * The plain refill (csrValuesRowKernel), one thread per destination row, serves every hackSize that is no multiple of 32
 * (a group would be mostly idle lanes) and is the second implementation the tests compare bytes with.
 */
#include "csr_host.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/update_device.h"

#include <cstdint>
#include <type_traits>

namespace spgpu {

constexpr int kUpThreads = 256;
constexpr int kUpWaves = kUpThreads / kWave;
constexpr int kUpGroupRows = 32;                                 /* destination rows a wavefront owns */
constexpr int kUpChunk = 16;                                     /* slab columns per trip */
constexpr int kUpTileLd = 36;                                    /* padded row count of the LDS tile */
constexpr int kUpReadPasses = kUpGroupRows * kUpChunk / kWave;   /* 8: 4 rows x 16 entries per pass */
constexpr int kUpRowsPerPass = kWave / kUpChunk;                 /* 4 */

enum { SPGPU_UPDATE_FILL_PLAIN = 0, SPGPU_UPDATE_FILL_TRANSPOSE = 1 };

struct UpBits128 { unsigned long long lo, hi; };                 /* in HBM: the alignment of the caller's element type, 8 bytes */
struct alignas(16) UpTile128 { unsigned long long lo, hi; };      /* in registers and LDS: 16 bytes, so that one element is one 16-byte LDS access */
struct alignas(16) UpVec16 { unsigned w[4]; };                   /* what a lane moves in a wide step */
template <typename ELEM> struct UpTileOf { typedef ELEM type; };
template <> struct UpTileOf<UpBits128> { typedef UpTile128 type; };
template <typename TO, typename FROM> __device__ inline TO upAs(const FROM& v)
{
    if constexpr (std::is_same<TO, FROM>::value) {
        return v;
    } else {
        TO t;
        t.lo = v.lo, t.hi = v.hi;
        return t;
    }
}

/* Where the value slots lie.  HELL: slot(row, k) = hackOffsets[row / hackSize] + row % hackSize + k * hackSize; ELL
 * (hackOffsets == NULL): row + k * stride. */
struct UpSlabs {
    const int* hackOffsets;
    int hackSize;
    long long stride;
};

/* The run of CSR entries that is destination row `row`: first entry (0-based) and length.  A row pointer that descends or an
 * order entry outside the matrix gives an empty run, as in the full fill. */
__device__ inline void upRunOf(int row, int rows, const int* rowPtr, int csrBase, const int* rIdx, int& start, int& len)
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

/* The plain refill: one thread per destination row.  Neighbouring lanes write neighbouring slots; each reads its own run. */
template <typename ELEM, bool TO_HELL>
__global__ __launch_bounds__(kUpThreads) void csrValuesRowKernel(ELEM* values, UpSlabs slabs, int rows, const int* rowPtr,
                                                                 const ELEM* csrVals, int csrBase, const int* rIdx)
{
    const long long stride = (long long)gridDim.x * kUpThreads;
    for (long long row = (long long)blockIdx.x * kUpThreads + threadIdx.x; row < rows; row += stride) {
        int start, len;
        upRunOf((int)row, rows, rowPtr, csrBase, rIdx, start, len);
        long long slot = row;
        if constexpr (TO_HELL) {
            const long long hack = row / slabs.hackSize;
            slot = (long long)slabs.hackOffsets[hack] + (row - hack * slabs.hackSize);
        }
        for (int k = 0; k < len; ++k)
            values[slot + k * slabs.stride] = csrVals[(long long)start + k];
    }
}

/* The transposing refill (head of the file).  `groups` = hacks * subsPerHack groups of up to 32 rows, grid-strided by wavefront. */
template <typename ELEM, bool TO_HELL>
__global__ __launch_bounds__(kUpThreads) void csrValuesTransposeKernel(ELEM* values, UpSlabs slabs, int subsPerHack, long long groups,
                                                                       int rows, const int* rowPtr, const ELEM* csrVals, int csrBase,
                                                                       const int* rIdx)
{
    constexpr int kVec = 16 / (int)sizeof(ELEM);          /* rows a lane stores in a wide step: 4, 2, 1 */
    constexpr int kLanesPerCol = kUpGroupRows / kVec;     /* 8, 16, 32 */
    constexpr int kColsPerStep = kWave / kLanesPerCol;    /* 8, 4, 2 */
    constexpr int kWideSteps = kUpChunk / kColsPerStep;   /* 2, 4, 8 */
    constexpr int kNarrowCols = kWave / kUpGroupRows;     /* 2 slab columns x 32 rows per narrow step */
    constexpr int kNarrowSteps = kUpChunk / kNarrowCols;  /* 8 */
    typedef typename UpTileOf<ELEM>::type TILE;
    __shared__ __attribute__((aligned(16))) TILE tiles[kUpWaves][kUpChunk * kUpTileLd];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    TILE* tile = tiles[wave];
    const int myRow = lane & (kUpGroupRows - 1);          /* holds the run of row firstRow + myRow; narrow write: lanes along the rows */
    const int readK = lane & (kUpChunk - 1);              /* read side: lanes along a row's run ... */
    const int readRow = lane / kUpChunk;                  /* ... 4 rows per pass */
    const int wideRow = (lane % kLanesPerCol) * kVec;     /* wide write: the first of the lane's kVec rows ... */
    const int wideCol = lane / kLanesPerCol;              /* ... of this slab column of the step */
    const long long stride = (long long)gridDim.x * kUpWaves;
    for (long long g = (long long)blockIdx.x * kUpWaves + wave; g < groups; g += stride) {
        long long firstRow, slot0;
        int rowsHere;
        if constexpr (TO_HELL) {
            const long long hack = g / subsPerHack;
            const int inHack = (int)(g - hack * subsPerHack) * kUpGroupRows;
            firstRow = hack * slabs.hackSize + inHack;
            rowsHere = slabs.hackSize - inHack;
            if (firstRow >= rows) /* wavefront-uniform: the last hack is partly filled */
                continue;
            slot0 = (long long)slabs.hackOffsets[hack] + inHack;
        } else {
            firstRow = g * kUpGroupRows;
            rowsHere = kUpGroupRows;
            slot0 = firstRow;
        }
        if (rowsHere > kUpGroupRows)
            rowsHere = kUpGroupRows;
        if (rowsHere > rows - firstRow)
            rowsHere = (int)(rows - firstRow);
        int start = 0, len = 0; /* of row firstRow + myRow: both halves of the wavefront hold it */
        if (myRow < rowsHere)
            upRunOf((int)firstRow + myRow, rows, rowPtr, csrBase, rIdx, start, len);
        const int longest = waveMax(len);
        ELEM* out = values + slot0;
        /* wavefront-uniform: every 16-byte piece of every slab column of the group lies on a 16-byte boundary */
        const bool wide = ((uintptr_t)out & 15) == 0 && (slabs.stride * (long long)sizeof(ELEM)) % 16 == 0;
        int lenOf[kVec], all = 0x7fffffff; /* wide write: how far the lane's rows reach, and how far all of them do */
#pragma unroll
        for (int v = 0; v < kVec; ++v) {
            lenOf[v] = __shfl(len, wideRow + v, kWave);
            all = lenOf[v] < all ? lenOf[v] : all;
        }
        for (int k0 = 0; k0 < longest; k0 += kUpChunk) {
            TILE val[kUpReadPasses];
            bool mine[kUpReadPasses];
#pragma unroll
            for (int p = 0; p < kUpReadPasses; ++p) {
                const int r = p * kUpRowsPerPass + readRow;
                const int from = __shfl(start, r, kWave), have = __shfl(len, r, kWave);
                mine[p] = k0 + readK < have;
                if (mine[p])
                    val[p] = upAs<TILE>(csrVals[(long long)from + k0 + readK]);
            }
            __builtin_amdgcn_wave_barrier(); /* the previous trip's read-out precedes these stores */
#pragma unroll
            for (int p = 0; p < kUpReadPasses; ++p)
                if (mine[p])
                    tile[readK * kUpTileLd + p * kUpRowsPerPass + readRow] = val[p];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (wide) {
#pragma unroll
                for (int s = 0; s < kWideSteps; ++s) {
                    const int kk = s * kColsPerStep + wideCol, k = k0 + kk;
                    ELEM* to = out + wideRow + (long long)k * slabs.stride;
                    if (k < all) {
                        UpVec16 piece;
                        __builtin_memcpy(&piece, __builtin_assume_aligned(&tile[kk * kUpTileLd + wideRow], 16), 16);
                        __builtin_memcpy(__builtin_assume_aligned(to, 16), &piece, 16);
                    } else {
#pragma unroll
                        for (int v = 0; v < kVec; ++v)
                            if (k < lenOf[v])
                                to[v] = upAs<ELEM>(tile[kk * kUpTileLd + wideRow + v]);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < kNarrowSteps; ++s) {
                    const int kk = s * kNarrowCols + lane / kUpGroupRows;
                    if (k0 + kk < len)
                        out[myRow + (long long)(k0 + kk) * slabs.stride] = upAs<ELEM>(tile[kk * kUpTileLd + myRow]);
                }
            }
        }
    }
}

/* ---- spgpu?hellcsput: ellCsputKernel (ell_csput.hip.h) on HELL storage, the storage row through rowOf ---- */
template <typename T>
__global__ __launch_bounds__(kUpThreads) void hellCsputKernel(T* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                                                              const int* rowOf, int rows, int nnz, const int* aI, const int* aJ,
                                                              const T* aVal, int baseIndex)
{
    const long long i = (long long)blockIdx.x * kUpThreads + threadIdx.x;
    if (i >= nnz)
        return;
    int row = aI[i] - baseIndex;
    if (row < 0 || row >= rows)
        return;
    if (rowOf) {
        row = rowOf[row];
        if ((unsigned)row >= (unsigned)rows)
            return;
    }
    const int column = aJ[i];
    const int hack = row / hackSize;
    const long long first = (long long)hackOffsets[hack] + (row - hack * hackSize);
    int lower = 0, upper = rS[row] - 1;
    while (lower <= upper) { /* the row's stored indices ascend */
        const int mid = (int)(((long long)lower + upper) / 2);
        const long long slot = first + (long long)mid * hackSize;
        const int stored = rP[slot];
        if (stored == column) {
            cM[slot] = aVal[i];
            return;
        }
        if (stored < column)
            lower = mid + 1;
        else
            upper = mid - 1;
    }
}

__global__ __launch_bounds__(kUpThreads) void invertRowOrderKernel(int* rowOf, const int* rIdx, int rows)
{
    const long long stride = (long long)gridDim.x * kUpThreads;
    for (long long r = (long long)blockIdx.x * kUpThreads + threadIdx.x; r < rows; r += stride) {
        const int i = rIdx[r];
        if ((unsigned)i < (unsigned)rows)
            rowOf[i] = (int)r;
    }
}

template <typename ELEM, bool TO_HELL>
static void launchRefill(hipStream_t s, void* values, const UpSlabs& slabs, int rows, const int* rowPtr, const void* csrVals, int csrBase,
                         const int* rIdx, int fill, int maxBlocks)
{
    if (fill == SPGPU_UPDATE_FILL_PLAIN) {
        hipLaunchKernelGGL((csrValuesRowKernel<ELEM, TO_HELL>), dim3(cappedGrid(rows, kUpThreads, maxBlocks)), dim3(kUpThreads), 0, s,
                           static_cast<ELEM*>(values), slabs, rows, rowPtr, static_cast<const ELEM*>(csrVals), csrBase, rIdx);
        return;
    }
    const int subsPerHack = TO_HELL ? (slabs.hackSize + kUpGroupRows - 1) / kUpGroupRows : 1;
    const long long hacks = TO_HELL ? ((long long)rows + slabs.hackSize - 1) / slabs.hackSize : ((long long)rows + kUpGroupRows - 1) / kUpGroupRows;
    const long long groups = hacks * subsPerHack;
    hipLaunchKernelGGL((csrValuesTransposeKernel<ELEM, TO_HELL>), dim3(cappedGrid(groups, kUpWaves, maxBlocks)), dim3(kUpThreads), 0, s,
                       static_cast<ELEM*>(values), slabs, subsPerHack, groups, rows, rowPtr, static_cast<const ELEM*>(csrVals), csrBase, rIdx);
}

/* fill < 0: the one the public calls run -- transposing where a group of 32 rows lies within a hack (ELL; hackSize a multiple of
 * 32), else plain. */
template <bool TO_HELL>
static spgpuStatus_t refill(spgpuHandle_t handle, void* values, const UpSlabs& slabs, int rows, const int* rowPtr, const void* csrVals,
                            int csrBase, spgpuType_t type, const int* rIdx, int fill, int maxBlocks)
{
    if (rows <= 0)
        return SPGPU_SUCCESS;
    if (TO_HELL && slabs.hackSize <= 0)
        return SPGPU_UNSUPPORTED;
    if (fill < 0)
        fill = !TO_HELL || slabs.hackSize % kUpGroupRows == 0 ? SPGPU_UPDATE_FILL_TRANSPOSE : SPGPU_UPDATE_FILL_PLAIN;
    if (fill != SPGPU_UPDATE_FILL_PLAIN && fill != SPGPU_UPDATE_FILL_TRANSPOSE)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    switch (spgpuSizeOf(type)) {
    case 4:
        launchRefill<unsigned, TO_HELL>(s, values, slabs, rows, rowPtr, csrVals, csrBase, rIdx, fill, maxBlocks);
        break;
    case 8:
        launchRefill<unsigned long long, TO_HELL>(s, values, slabs, rows, rowPtr, csrVals, csrBase, rIdx, fill, maxBlocks);
        break;
    case 16:
        launchRefill<UpBits128, TO_HELL>(s, values, slabs, rows, rowPtr, csrVals, csrBase, rIdx, fill, maxBlocks);
        break;
    default:
        return SPGPU_UNSUPPORTED;
    }
    spgpuDebugCheck(handle, "csr value refill");
    return SPGPU_SUCCESS;
}

template <typename T, typename ApiT>
static void hellCsput(spgpuHandle_t handle, ApiT* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS, const int* rowOf,
                      int rows, int nnz, const int* aI, const int* aJ, const ApiT* aVal, int baseIndex)
{
    if (nnz <= 0 || rows <= 0 || hackSize <= 0)
        return;
    const unsigned blocks = (unsigned)(((long long)nnz + kUpThreads - 1) / kUpThreads);
    hipLaunchKernelGGL((hellCsputKernel<T>), dim3(blocks), dim3(kUpThreads), 0, handle->currentStream, reinterpret_cast<T*>(cM), rP, hackSize,
                       hackOffsets, rS, rowOf, rows, nnz, aI, aJ, reinterpret_cast<const T*>(aVal), baseIndex);
    spgpuDebugCheck(handle, "hellcsput");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_update.py and the tests that compare the two refills.  fill: 0 the plain refill,
 * 1 the transposing refill, < 0 the public call's choice; maxBlocks > 0 caps the grid (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrToHellValuesDeviceWith(spgpuHandle_t handle, void* hellValues, const int* hackOffsets, int hackSize, int rowsCount,
                                             const int* csrRowPtr, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                             const int* rIdx, int fill, int maxBlocks);
spgpuStatus_t spgpuCsrToEllValuesDeviceWith(spgpuHandle_t handle, void* ellValues, int ellValuesPitch, int rowsCount, const int* csrRowPtr,
                                            const void* csrValues, int csrBaseIndex, spgpuType_t valuesType, const int* rIdx, int fill,
                                            int maxBlocks);

spgpuStatus_t spgpuCsrToHellValuesDeviceWith(spgpuHandle_t handle, void* hellValues, const int* hackOffsets, int hackSize, int rowsCount,
                                             const int* csrRowPtr, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                             const int* rIdx, int fill, int maxBlocks)
{
    const UpSlabs slabs = {hackOffsets, hackSize, hackSize};
    return refill<true>(handle, hellValues, slabs, rowsCount, csrRowPtr, csrValues, csrBaseIndex, valuesType, rIdx, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrToEllValuesDeviceWith(spgpuHandle_t handle, void* ellValues, int ellValuesPitch, int rowsCount, const int* csrRowPtr,
                                            const void* csrValues, int csrBaseIndex, spgpuType_t valuesType, const int* rIdx, int fill,
                                            int maxBlocks)
{
    const UpSlabs slabs = {nullptr, 0, ellValuesPitch};
    return refill<false>(handle, ellValues, slabs, rowsCount, csrRowPtr, csrValues, csrBaseIndex, valuesType, rIdx, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrToHellValuesDevice(spgpuHandle_t handle, void* hellValues, const int* hackOffsets, int hackSize, int rowsCount,
                                         const int* csrRowPtr, const void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                         const int* rIdx)
{
    return spgpuCsrToHellValuesDeviceWith(handle, hellValues, hackOffsets, hackSize, rowsCount, csrRowPtr, csrValues, csrBaseIndex, valuesType,
                                          rIdx, -1, 0);
}

spgpuStatus_t spgpuCsrToEllValuesDevice(spgpuHandle_t handle, void* ellValues, int ellValuesPitch, int rowsCount, const int* csrRowPtr,
                                        const void* csrValues, int csrBaseIndex, spgpuType_t valuesType, const int* rIdx)
{
    return spgpuCsrToEllValuesDeviceWith(handle, ellValues, ellValuesPitch, rowsCount, csrRowPtr, csrValues, csrBaseIndex, valuesType, rIdx, -1,
                                         0);
}

spgpuStatus_t spgpuInvertRowOrderDevice(spgpuHandle_t handle, int* rowOf, const int* rIdx, int rows)
{
    if (rows <= 0)
        return SPGPU_SUCCESS;
    hipLaunchKernelGGL(invertRowOrderKernel, dim3(cappedGrid(rows, kUpThreads, 4096)), dim3(kUpThreads), 0, handle->currentStream, rowOf, rIdx,
                       rows);
    spgpuDebugCheck(handle, "invert row order");
    return SPGPU_SUCCESS;
}

/* alpha is accepted and not applied, as in spgpu?ellcsput (reference ell_csput_base.cuh:35,44,66). */
#define SPGPU_HELLCSPUT_ABI(L, T, ApiT)                                                                                                  \
    void spgpu##L##hellcsput(spgpuHandle_t handle, ApiT alpha, ApiT* cM, const int* rP, int hackSize, const int* hackOffsets,            \
                             const int* rS, const int* rowOf, int rows, int nnz, int* aI, int* aJ, ApiT* aVal, int baseIndex)           \
    { (void)alpha; hellCsput<T>(handle, cM, rP, hackSize, hackOffsets, rS, rowOf, rows, nnz, aI, aJ, aVal, baseIndex); }

SPGPU_HELLCSPUT_ABI(S, float, float)
SPGPU_HELLCSPUT_ABI(D, double, double)
SPGPU_HELLCSPUT_ABI(C, cfloat, hipFloatComplex)
SPGPU_HELLCSPUT_ABI(Z, cdouble, hipDoubleComplex)

} // extern "C"
