/*
 * Device-side HELL / ELL -> CSR construction for gfx950 (include/spgpu/ext/to_csr_device.h).  New functionality: the
 * transposition of convert_csr_device.hip run the other way.  On the slab side a slab column is a contiguous run of 32 rows
 * (hackSize in general); on the CSR side a row is a contiguous run of entries.
 *
 * ROW POINTERS.  toCsrLengthsKernel, one lane per storage row: validates rS / rIdx / the reach of the row, stores the length at
 * the MATRIX row's place in `work` and, with rIdx, counts the storage rows that name each matrix row (integer atomics: the
 * counts, and so the flag, do not depend on the order).  The longest row, the flag and the 64-bit sum of the lengths go to the
 * host through the handle's reduction scratch; a refused source ends there.  Then the three-launch exclusiveScan of
 * convert_scan.hip.h over the lengths straight into csrRowPtr, and one pass that adds csrBaseIndex and writes the grand total.
 *   work (ints): lengths[rows] | hits[rows] | scan totals[tiles + 2], rounded up to 64 ints.
 *
 * THE PLAIN FILL (toCsrRowFillKernel): one thread per storage row.  Neighbouring lanes read neighbouring slots; each writes its
 * own CSR run.
 *
 * THE TRANSPOSING FILL (toCsrTransposeFillKernel), the mirror of csrTransposeFillKernel: a wavefront owns a GROUP of up to 32
 * storage rows of one hack (a hack of hackSize rows is ceil(hackSize / 32) groups; ELL is a single hack of the two pitches) and
 * walks it in chunks of kToCsrChunk = 16 slab columns:
 *   read    8 steps; in a step the 64 lanes are 2 slab columns x 32 rows: whole 128-byte (4-byte types and the indices) or
 *           256-byte runs, and with hackSize == 32 the 16 columns of a chunk are one contiguous block.  The predicate is
 *           k < rS[r]: a padding slot is never loaded;
 *   park    slot k of row r goes to tile[k * kToCsrTileLd + r] in LDS: lanes along r, consecutive words, which every LDS store
 *           takes without a conflict;
 *   write   8 passes; in a pass the 64 lanes are 4 rows x 16 consecutive entries of each row's CSR run: for fp64 a 128-byte run
 *           of values and a 64-byte run of columns per row.  Element stores: a run starts at any element offset.
 * kToCsrTileLd = 34, not the 36 of the CSR -> slab fill, because here the STRIDED side is the LDS read, and reads are banked
 * differently from stores (4-byte reads: 32 banks, groups of 32 lanes; 8- and 16-byte reads: 64 banks, groups of 32 / 16 lanes).
 * A read group holds lanes (row, k) with element address 34 k + row:
 *   4 bytes   rows {0,1} x 16 k: banks (2 k + row) mod 32 -- all 32 distinct (36 gives 4 k + row: k and k + 8 collide);
 *   8 bytes   rows {0,1} x 16 k: words 68 k + 2 row = 4 k + 2 row mod 64, two banks each -- all 64 distinct (36: 8 k + 2 row, 2-way);
 *   16 bytes  8 k of one row and the other 8 k of the next: words 136 k + 4 row = 8 k + 4 row mod 64, four banks each -- 64 distinct.
 * The 16-byte line holds for ONE 16-byte read per lane: the tile's element type is 16-byte aligned (ToCsrTile128) although the
 * caller's arrays need 8 only, and the compiler then emits ds_read_b128 / ds_write_b128 for it (seen in the ISA; with an 8-byte
 * aligned tile type it emitted ds_read2_b64, which banks over 32 dwords).  All three lines are DERIVED from the banking rules;
 * no bank-conflict counter has been collected.
 * A row of any length is so many chunks: no LDS that grows with the row.  A row order changes only where a row's run starts.
 * No atomics, each CSR element has one writer: the arrays do not depend on scheduling.  A wavefront's tile is its own; its LDS
 * operations execute in order, the wave barriers only keep the compiler from moving them.
 */
#include "convert_scan.hip.h"
#include "csr_host.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/to_csr_device.h"

#include <string.h>
#include <type_traits>

namespace spgpu {

constexpr int kToCsrThreads = kCvThreads;
constexpr int kToCsrWaves = kToCsrThreads / kWave;
constexpr int kToCsrGroupRows = 32;                                       /* storage rows a wavefront owns */
constexpr int kToCsrChunk = 16;                                           /* slab columns per trip */
constexpr int kToCsrTileLd = 34;                                          /* padded row count of the LDS tile (head of the file) */
constexpr int kToCsrReadSteps = kToCsrGroupRows * kToCsrChunk / kWave;    /* 8: 2 columns x 32 rows per step */
constexpr int kToCsrWritePasses = kToCsrGroupRows * kToCsrChunk / kWave;  /* 8: 4 rows x 16 entries per pass */
constexpr int kToCsrColsPerStep = kWave / kToCsrGroupRows;                /* 2 */
constexpr int kToCsrRowsPerPass = kWave / kToCsrChunk;                    /* 4 */

enum { SPGPU_TO_CSR_FILL_PLAIN = 0, SPGPU_TO_CSR_FILL_TRANSPOSE = 1 };
constexpr int kToCsrDefaultFill = SPGPU_TO_CSR_FILL_TRANSPOSE;

struct ToCsrBits128 { unsigned long long lo, hi; };          /* in HBM: the alignment of the caller's element type, 8 bytes */
struct alignas(16) ToCsrTile128 { unsigned long long lo, hi; }; /* in LDS: 16 bytes, so that one slot is one 16-byte read or store */
template <typename ELEM> struct ToCsrTileOf { typedef ELEM type; };
template <> struct ToCsrTileOf<ToCsrBits128> { typedef ToCsrTile128 type; };
template <typename TO, typename FROM> __device__ inline TO toCsrAs(const FROM& v)
{
    if constexpr (std::is_same<TO, FROM>::value) {
        return v;
    } else {
        TO t;
        t.lo = v.lo, t.hi = v.hi;
        return t;
    }
}

/* Where the slots of the source lie.  HELL: slot(r, k) = hackOffsets[r / hackSize] + r % hackSize + k * hackSize; ELL
 * (hackOffsets == NULL): r + k * pitch, with a pitch each for values and indices. */
struct ToCsrSlabs {
    const int* hackOffsets;
    int hackSize;
    long long valStride, idxStride;
    __device__ long long first(int r) const
    {
        if (!hackOffsets)
            return r;
        const int hack = r / hackSize;
        return (long long)hackOffsets[hack] + (r - hack * hackSize);
    }
};

/* misc words of the row-pointer call in the handle's reduction scratch */
enum { TO_CSR_LONGEST = 0, TO_CSR_BAD = 1, TO_CSR_TOTAL = 2 /* 64 bits: ints 2 and 3 */, TO_CSR_MISC_INTS = 4 };

__device__ inline unsigned long long waveSum64(unsigned long long v)
{
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1)
        v += __shfl_xor(v, m, kWave);
    return v;
}

/* lengths[i] = rS[r] of the storage row r that holds matrix row i (0 and the flag where the row cannot be read); hits[i] counts
 * those storage rows when there is a row order.  `hits` was zeroed by the caller. */
__global__ __launch_bounds__(kToCsrThreads) void toCsrLengthsKernel(int* lengths, int* hits, int* misc, ToCsrSlabs src, const int* rS,
                                                                    const int* rIdx, int rows, int slots)
{
    int best = 0, flag = 0;
    unsigned long long sum = 0;
    const long long stride = (long long)gridDim.x * kToCsrThreads;
    for (long long t = (long long)blockIdx.x * kToCsrThreads + threadIdx.x; t < rows; t += stride) {
        const int r = (int)t;
        const int len = rS[r];
        bool bad = len < 0;
        if (len > 0) {
            const long long first = src.first(r);
            bad |= first < 0 || first + (long long)(len - 1) * src.idxStride >= (long long)slots;
        }
        int i = r;
        if (rIdx) {
            i = rIdx[r];
            if ((unsigned)i >= (unsigned)rows)
                bad = true, i = -1;
            else
                bad |= atomicAdd(&hits[i], 1) != 0; /* whoever comes second to a matrix row sees it: some lane does, in any order */
        }
        const int kept = bad ? 0 : len;
        if (i >= 0)
            lengths[i] = kept; /* two storage rows with one rIdx value both store here: whichever lands, the hit count has raised the
                                * flag, the call is refused on the host and `lengths` is never read */
        best = kept > best ? kept : best;
        sum += (unsigned long long)kept;
        flag |= bad;
    }
    best = waveMax(best);
    flag = waveMax(flag);
    sum = waveSum64(sum);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (best > 0)
            atomicMax(&misc[TO_CSR_LONGEST], best);
        if (flag)
            atomicMax(&misc[TO_CSR_BAD], 1);
        if (sum)
            atomicAdd(reinterpret_cast<unsigned long long*>(misc + TO_CSR_TOTAL), sum);
    }
}

/* csrRowPtr[0 .. rows) holds the exclusive sums: add the base, and write base + grand total behind them */
__global__ __launch_bounds__(kToCsrThreads) void toCsrFinishKernel(int* rowPtr, int rows, int csrBase, const int* grandTotal)
{
    if (csrBase) {
        const long long stride = (long long)gridDim.x * kToCsrThreads;
        for (long long i = (long long)blockIdx.x * kToCsrThreads + threadIdx.x; i < rows; i += stride)
            rowPtr[i] += csrBase;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        rowPtr[rows] = *grandTotal + csrBase;
}

/* The CSR run of storage row `r`: first element (0-based) and length.  The length is rS[r], which the row-pointer call has
 * checked; bounded by the run csrRowPtr leaves for the row, so no element outside [0, nonZerosCount) is written whatever rS
 * says by now. */
__device__ inline void toCsrRunOf(int r, int rows, const int* rowPtr, int csrBase, const int* rS, const int* rIdx, long long& out, int& len)
{
    out = 0;
    len = 0;
    const int i = rIdx ? rIdx[r] : r;
    if ((unsigned)i < (unsigned)rows) {
        const int a = rowPtr[i], room = rowPtr[i + 1] - a, have = rS[r];
        out = (long long)a - csrBase;
        len = have < room ? have : room;
        if (len < 0 || out < 0)
            len = 0;
    }
}

/* The plain fill: one thread per storage row. */
template <typename ELEM>
__global__ __launch_bounds__(kToCsrThreads) void toCsrRowFillKernel(int* csrCols, ELEM* csrVals, const int* rowPtr, int csrBase,
                                                                    const ELEM* values, const int* indices, ToCsrSlabs src,
                                                                    const int* rS, const int* rIdx, int rows, int srcBase)
{
    const long long stride = (long long)gridDim.x * kToCsrThreads;
    for (long long row = (long long)blockIdx.x * kToCsrThreads + threadIdx.x; row < rows; row += stride) {
        long long out;
        int len;
        toCsrRunOf((int)row, rows, rowPtr, csrBase, rS, rIdx, out, len);
        if (len <= 0)
            continue;
        const long long slot = src.first((int)row);
        for (int k = 0; k < len; ++k) {
            csrCols[out + k] = indices[slot + k * src.idxStride] - srcBase + csrBase;
            csrVals[out + k] = values[slot + k * src.valStride];
        }
    }
}

/* The transposing fill (head of the file).  `groups` = hacks * subsPerHack groups of up to 32 rows, grid-strided by wavefront. */
template <typename ELEM>
__global__ __launch_bounds__(kToCsrThreads) void toCsrTransposeFillKernel(int* csrCols, ELEM* csrVals, const int* rowPtr, int csrBase,
                                                                          const ELEM* values, const int* indices, ToCsrSlabs src,
                                                                          int subsPerHack, long long groups, const int* rS,
                                                                          const int* rIdx, int rows, int srcBase)
{
    typedef typename ToCsrTileOf<ELEM>::type TILE;
    __shared__ TILE tileVals[kToCsrWaves][kToCsrChunk * kToCsrTileLd];
    __shared__ int tileCols[kToCsrWaves][kToCsrChunk * kToCsrTileLd];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    TILE* tv = tileVals[wave];
    int* tc = tileCols[wave];
    const int myRow = lane & (kToCsrGroupRows - 1);      /* read side: lanes along the rows ... */
    const int myCol = lane / kToCsrGroupRows;            /* ... 2 slab columns per step */
    const int writeK = lane & (kToCsrChunk - 1);         /* write side: lanes along a row's run ... */
    const int writeRow = lane / kToCsrChunk;             /* ... 4 rows per pass */
    const long long stride = (long long)gridDim.x * kToCsrWaves;
    for (long long g = (long long)blockIdx.x * kToCsrWaves + wave; g < groups; g += stride) {
        long long firstRow, slot0;
        int rowsHere;
        if (src.hackOffsets) {
            const long long hack = g / subsPerHack;
            const int inHack = (int)(g - hack * subsPerHack) * kToCsrGroupRows;
            firstRow = hack * src.hackSize + inHack;
            rowsHere = src.hackSize - inHack;
            if (firstRow >= rows) /* wavefront-uniform: the last hack is partly filled */
                continue;
            slot0 = (long long)src.hackOffsets[hack] + inHack;
        } else {
            firstRow = g * kToCsrGroupRows;
            rowsHere = kToCsrGroupRows;
            slot0 = firstRow;
        }
        if (rowsHere > kToCsrGroupRows)
            rowsHere = kToCsrGroupRows;
        if (rowsHere > rows - firstRow)
            rowsHere = (int)(rows - firstRow);
        long long out = 0; /* of row firstRow + myRow: both halves of the wavefront hold it */
        int len = 0;
        if (myRow < rowsHere)
            toCsrRunOf((int)firstRow + myRow, rows, rowPtr, csrBase, rS, rIdx, out, len);
        const int longest = waveMax(len);
        for (int k0 = 0; k0 < longest; k0 += kToCsrChunk) {
            int col[kToCsrReadSteps];
            ELEM val[kToCsrReadSteps];
#pragma unroll
            for (int s = 0; s < kToCsrReadSteps; ++s) {
                const int kk = s * kToCsrColsPerStep + myCol;
                if (k0 + kk < len) {
                    col[s] = indices[slot0 + myRow + (long long)(k0 + kk) * src.idxStride];
                    val[s] = values[slot0 + myRow + (long long)(k0 + kk) * src.valStride];
                }
            }
            __builtin_amdgcn_wave_barrier(); /* the previous trip's read-out precedes these stores */
#pragma unroll
            for (int s = 0; s < kToCsrReadSteps; ++s) {
                const int kk = s * kToCsrColsPerStep + myCol;
                if (k0 + kk < len) {
                    tc[kk * kToCsrTileLd + myRow] = col[s] - srcBase + csrBase;
                    tv[kk * kToCsrTileLd + myRow] = toCsrAs<TILE>(val[s]);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int p = 0; p < kToCsrWritePasses; ++p) {
                const int r = p * kToCsrRowsPerPass + writeRow;
                const long long to = __shfl(out, r, kWave);
                const int have = __shfl(len, r, kWave);
                if (k0 + writeK < have) {
                    csrCols[to + k0 + writeK] = tc[writeK * kToCsrTileLd + r];
                    csrVals[to + k0 + writeK] = toCsrAs<ELEM>(tv[writeK * kToCsrTileLd + r]);
                }
            }
        }
    }
}

static size_t toCsrWorkInts(int rows) { return alignUpCv(2 * (size_t)rows + scanBlocks(rows) + 2, 64); }

static spgpuStatus_t toCsrRowPtr(spgpuHandle_t handle, int* csrRowPtr, int* nonZerosCount, int* maxRowSize, int csrBase,
                                 const ToCsrSlabs& src, const int* rS, const int* rIdx, int rows, int slots, void* work)
{
    if (nonZerosCount)
        *nonZerosCount = 0;
    if (maxRowSize)
        *maxRowSize = 0;
    if (rows <= 0)
        return SPGPU_SUCCESS;
    if (!nonZerosCount || !maxRowSize || !csrRowPtr || !rS || !work || src.idxStride <= 0)
        return SPGPU_UNSUPPORTED;
    if (!src.hackOffsets && src.idxStride < rows)
        return SPGPU_UNSUPPORTED; /* an ELL pitch below the row count: rows would share slots */
    hipStream_t s = handle->currentStream;
    int* lengths = static_cast<int*>(work);
    int* hits = lengths + (size_t)rows;
    int* totals = hits + (size_t)rows;
    /* the handle's reduction scratch and its pinned mirror: one reduction of a handle at a time, as everywhere */
    int* misc = static_cast<int*>(spgpuPrivate(handle)->reduceScratch);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    (void)hipMemsetAsync(misc, 0, TO_CSR_MISC_INTS * sizeof(int), s);
    if (rIdx)
        (void)hipMemsetAsync(hits, 0, (size_t)rows * sizeof(int), s);
    hipLaunchKernelGGL(toCsrLengthsKernel, dim3(cappedGrid(rows, kToCsrThreads, 4096)), dim3(kToCsrThreads), 0, s, lengths, hits, misc,
                       src, rS, rIdx, rows, slots);
    (void)hipMemcpyAsync(host, misc, TO_CSR_MISC_INTS * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "to-csr row lengths");
    unsigned long long total;
    memcpy(&total, host + TO_CSR_TOTAL, sizeof(total));
    const int longest = host[TO_CSR_LONGEST];
    if (host[TO_CSR_BAD] || total > (unsigned long long)(slots > 0 ? slots : 0))
        return SPGPU_UNSUPPORTED; /* with every matrix row named once and no more entries than slots, the sums below fit an int */
    exclusiveScan(s, csrRowPtr, lengths, (long long)rows, 1, totals);
    hipLaunchKernelGGL(toCsrFinishKernel, dim3(csrBase ? cappedGrid(rows, kToCsrThreads, 4096) : 1u), dim3(kToCsrThreads), 0, s, csrRowPtr,
                       rows, csrBase, (const int*)(totals + scanBlocks(rows)));
    (void)hipStreamSynchronize(s); /* `work` is the caller's again on return */
    spgpuDebugCheck(handle, "to-csr row pointers");
    *nonZerosCount = (int)total;
    *maxRowSize = longest;
    return SPGPU_SUCCESS;
}

template <typename ELEM>
static void launchToCsrFill(hipStream_t s, int* csrCols, void* csrVals, const int* rowPtr, int csrBase, const void* values,
                            const int* indices, const ToCsrSlabs& src, const int* rS, const int* rIdx, int rows, int srcBase, int fill,
                            int maxBlocks)
{
    if (fill == SPGPU_TO_CSR_FILL_PLAIN) {
        hipLaunchKernelGGL(toCsrRowFillKernel<ELEM>, dim3(cappedGrid(rows, kToCsrThreads, maxBlocks)), dim3(kToCsrThreads), 0, s, csrCols,
                           static_cast<ELEM*>(csrVals), rowPtr, csrBase, static_cast<const ELEM*>(values), indices, src, rS, rIdx, rows,
                           srcBase);
        return;
    }
    const bool hell = src.hackOffsets != nullptr;
    const int subsPerHack = hell ? (src.hackSize + kToCsrGroupRows - 1) / kToCsrGroupRows : 1;
    const long long hacks = hell ? ((long long)rows + src.hackSize - 1) / src.hackSize : ((long long)rows + kToCsrGroupRows - 1) / kToCsrGroupRows;
    const long long groups = hacks * subsPerHack;
    hipLaunchKernelGGL(toCsrTransposeFillKernel<ELEM>, dim3(cappedGrid(groups, kToCsrWaves, maxBlocks)), dim3(kToCsrThreads), 0, s,
                       csrCols, static_cast<ELEM*>(csrVals), rowPtr, csrBase, static_cast<const ELEM*>(values), indices, src, subsPerHack,
                       groups, rS, rIdx, rows, srcBase);
}

static spgpuStatus_t toCsrFill(spgpuHandle_t handle, int* csrCols, void* csrVals, const int* rowPtr, int csrBase, const void* values,
                               const int* indices, const ToCsrSlabs& src, const int* rS, const int* rIdx, int rows, int srcBase,
                               spgpuType_t type, int fill, int maxBlocks)
{
    if (rows <= 0)
        return SPGPU_SUCCESS;
    if (src.idxStride <= 0 || src.valStride <= 0 || !rS || !rowPtr)
        return SPGPU_UNSUPPORTED;
    if (!src.hackOffsets && (src.idxStride < rows || src.valStride < rows))
        return SPGPU_UNSUPPORTED;
    if (fill != SPGPU_TO_CSR_FILL_PLAIN && fill != SPGPU_TO_CSR_FILL_TRANSPOSE)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    switch (spgpuSizeOf(type)) {
    case 4:
        launchToCsrFill<unsigned>(s, csrCols, csrVals, rowPtr, csrBase, values, indices, src, rS, rIdx, rows, srcBase, fill, maxBlocks);
        break;
    case 8:
        launchToCsrFill<unsigned long long>(s, csrCols, csrVals, rowPtr, csrBase, values, indices, src, rS, rIdx, rows, srcBase, fill,
                                            maxBlocks);
        break;
    case 16:
        launchToCsrFill<ToCsrBits128>(s, csrCols, csrVals, rowPtr, csrBase, values, indices, src, rS, rIdx, rows, srcBase, fill, maxBlocks);
        break;
    default:
        return SPGPU_UNSUPPORTED;
    }
    spgpuDebugCheck(handle, "to-csr fill");
    return SPGPU_SUCCESS;
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_to_csr.py and the tests that compare the two fills.  fill: 0 the plain fill, 1 the
 * transposing fill; maxBlocks > 0 caps the grid (the grid stride on a small matrix). */
spgpuStatus_t spgpuHellToCsrDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr,
                                       int csrBaseIndex, const void* cM, const int* rP, int hackSize, const int* hackOffsets,
                                       const int* rS, const int* rIdx, int rowsCount, int hellBaseIndex, spgpuType_t valuesType,
                                       int fill, int maxBlocks);
spgpuStatus_t spgpuEllToCsrDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr,
                                      int csrBaseIndex, const void* cM, const int* rP, int ellValuesPitch, int ellIndicesPitch,
                                      const int* rS, const int* rIdx, int rowsCount, int ellBaseIndex, spgpuType_t valuesType,
                                      int fill, int maxBlocks);
/* slab columns per trip of the transposing fill, and the fill the public calls run */
int spgpuToCsrFillChunk(void);
int spgpuToCsrDefaultFill(void);

int spgpuToCsrFillChunk(void) { return kToCsrChunk; }
int spgpuToCsrDefaultFill(void) { return kToCsrDefaultFill; }

size_t spgpuToCsrWorkBytes(int rowsCount)
{
    return rowsCount > 0 ? toCsrWorkInts(rowsCount) * sizeof(int) : 0;
}

spgpuStatus_t spgpuHellToCsrRowPtrDevice(spgpuHandle_t handle, int* csrRowPtr, int* nonZerosCount, int* maxRowSize, int csrBaseIndex,
                                         int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int rowsCount, int slots,
                                         void* work)
{
    if (rowsCount > 0 && (!hackOffsets || hackSize <= 0)) {
        if (nonZerosCount)
            *nonZerosCount = 0;
        if (maxRowSize)
            *maxRowSize = 0;
        return SPGPU_UNSUPPORTED;
    }
    const ToCsrSlabs src = {hackOffsets, hackSize, hackSize, hackSize};
    return toCsrRowPtr(handle, csrRowPtr, nonZerosCount, maxRowSize, csrBaseIndex, src, rS, rIdx, rowsCount, slots, work);
}

spgpuStatus_t spgpuEllToCsrRowPtrDevice(spgpuHandle_t handle, int* csrRowPtr, int* nonZerosCount, int* maxRowSize, int csrBaseIndex,
                                        int ellIndicesPitch, const int* rS, const int* rIdx, int rowsCount, int slots, void* work)
{
    const ToCsrSlabs src = {nullptr, 0, ellIndicesPitch, ellIndicesPitch};
    return toCsrRowPtr(handle, csrRowPtr, nonZerosCount, maxRowSize, csrBaseIndex, src, rS, rIdx, rowsCount, slots, work);
}

spgpuStatus_t spgpuHellToCsrDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr,
                                       int csrBaseIndex, const void* cM, const int* rP, int hackSize, const int* hackOffsets,
                                       const int* rS, const int* rIdx, int rowsCount, int hellBaseIndex, spgpuType_t valuesType,
                                       int fill, int maxBlocks)
{
    if (rowsCount > 0 && !hackOffsets)
        return SPGPU_UNSUPPORTED;
    const ToCsrSlabs src = {hackOffsets, hackSize, hackSize, hackSize};
    return toCsrFill(handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, src, rS, rIdx, rowsCount, hellBaseIndex,
                     valuesType, fill, maxBlocks);
}

spgpuStatus_t spgpuEllToCsrDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr,
                                      int csrBaseIndex, const void* cM, const int* rP, int ellValuesPitch, int ellIndicesPitch,
                                      const int* rS, const int* rIdx, int rowsCount, int ellBaseIndex, spgpuType_t valuesType,
                                      int fill, int maxBlocks)
{
    const ToCsrSlabs src = {nullptr, 0, ellValuesPitch, ellIndicesPitch};
    return toCsrFill(handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, src, rS, rIdx, rowsCount, ellBaseIndex,
                     valuesType, fill, maxBlocks);
}

spgpuStatus_t spgpuHellToCsrDevice(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr, int csrBaseIndex,
                                   const void* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS, const int* rIdx,
                                   int rowsCount, int hellBaseIndex, spgpuType_t valuesType)
{
    return spgpuHellToCsrDeviceWith(handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, hackSize, hackOffsets, rS, rIdx,
                                    rowsCount, hellBaseIndex, valuesType, kToCsrDefaultFill, 0);
}

spgpuStatus_t spgpuEllToCsrDevice(spgpuHandle_t handle, int* csrColIndices, void* csrValues, const int* csrRowPtr, int csrBaseIndex,
                                  const void* cM, const int* rP, int ellValuesPitch, int ellIndicesPitch, const int* rS, const int* rIdx,
                                  int rowsCount, int ellBaseIndex, spgpuType_t valuesType)
{
    return spgpuEllToCsrDeviceWith(handle, csrColIndices, csrValues, csrRowPtr, csrBaseIndex, cM, rP, ellValuesPitch, ellIndicesPitch,
                                   rS, rIdx, rowsCount, ellBaseIndex, valuesType, kToCsrDefaultFill, 0);
}

} // extern "C"
