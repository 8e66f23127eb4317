/*
 * Assembly of a COO list with duplicates into CSR on gfx950 (include/spgpu/ext/assemble_device.h).  New functionality: the plan
 * sorts the list once and writes down, per matrix entry, which contributions belong to it; the fills add them up, left to right.
 *
 * THE PLAN is set-up code.  Scratch layout (ints), S = nonZerosCount rounded up to 64:
 *   head    misc[16] | rowStart[rows+1] | scanTotals[tiles+2], rounded up to 64 ints;   misc[1] bad-input flag
 *   keysA[2S] | keysB[2S]   64-bit sort keys as emitted / sorted: (row << colBits) | column, both 0-based; an entry outside the
 *                           matrix raises the flag and gets key 0, so that every later kernel stays inside its arrays
 *   idA[S]                  the COO position of the entry, as emitted; sorted, it is the caller's perm
 *   entryOf[S]              head flags (1 where a sorted position starts a new key), scanned in place: the matrix entry u of
 *                           every sorted position
 *   rocPRIM temp
 * Emit -> ONE stable radix sort of (key, id) pairs over rowBits + colBits bits (rocPRIM) -> head flags -> the three-launch scan of
 * convert_scan.hip.h -> a head at position p writes segPtr[entryOf[p]] = p -> row starts by binary search in the sorted keys
 * (rowStartKernel of convert_scan.hip.h) -> csrRowPtr[r] = entryOf[rowStart[r]], the entries in front of the row.  The host reads
 * the entry count and the flag.
 *
 * THE FILLS add in the contract's order and give the same bytes:
 *   plain    (assembleEntryKernel) one thread per matrix entry walks its own segPtr range: a chain of dependent loads
 *            perm -> value per thread, as long as the entry has contributions;
 *   staged   (assembleStagedKernel) a workgroup takes a TILE of kAsmTile = 256 consecutive matrix entries, one per thread.  The
 *            tile's range of perm -- segPtr[first entry] .. segPtr[last entry + 1] -- is cut into CHUNKS of kAsmChunk = 1024
 *            positions counted from the tile's first position.  Per chunk every thread reads kAsmChunk / 256 = 4 words of perm,
 *            coalesced, issues its 4 value gathers together and lands them in LDS at their position in the chunk; then every
 *            thread adds the part of its own segment that lies in the chunk, from LDS, in order.  A segment that crosses a
 *            chunk keeps its running sum in the thread and goes on in the next chunk: a segment of any length is so many chunks.
 *            A tile whose segments all have length 1 (workgroup-uniform: its range is as long as the tile) is a straight gather.
 * Both start a sum from the first contribution and move a single contribution as it is.  No atomics, one writer per element.
 * The head flags, the fill of an empty plan's row pointer, the key bits and the grid rule are those of csr_shared.hip.h / csr_host.h.
 */
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/assemble_device.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace spgpu {

typedef unsigned long long AsmKey;

constexpr int kAsmThreads = 256;
constexpr int kAsmTile = kAsmThreads;                 /* matrix entries a workgroup owns: one per thread */
constexpr int kAsmLoads = 4;                          /* gathers a thread issues together */
constexpr int kAsmChunk = kAsmThreads * kAsmLoads;    /* positions of perm landed in LDS per trip */

enum { SPGPU_ASSEMBLE_FILL_PLAIN = 0, SPGPU_ASSEMBLE_FILL_STAGED = 1 };
/* The fill the public calls run: the faster one on the element-by-element listing of a 3-D stencil pattern, 10 M rows, 5-6
 * contributions per entry (tools/bench_assemble.py, profiles/assemble_ab.json). */
constexpr int kAsmDefaultFill = SPGPU_ASSEMBLE_FILL_STAGED;

struct AssembleWork {
    int* misc;
    int* rowStart;
    int* totals;
    AsmKey *keysA, *keysB;
    int* idA;
    int* entryOf;
    void* temp;
};

static size_t asmHeadInts(int rows, size_t nnz)
{
    return alignUpCv((size_t)16 + (size_t)rows + 1 + scanBlocks((long long)nnz) + 2, 64);
}

static AssembleWork carveAssemble(void* work, int rows, size_t nnz)
{
    AssembleWork w;
    int* p = static_cast<int*>(work);
    w.misc = p;
    w.rowStart = p + 16;
    w.totals = w.rowStart + (size_t)rows + 1;
    p += asmHeadInts(rows, nnz);
    const size_t S = alignUpCv(nnz, 64);
    w.keysA = reinterpret_cast<AsmKey*>(p);
    p += 2 * S;
    w.keysB = reinterpret_cast<AsmKey*>(p);
    p += 2 * S;
    w.idA = p;
    p += S;
    w.entryOf = p;
    p += S;
    w.temp = p;
    return w;
}

static hipError_t asmSortTempBytes(size_t n, size_t* bytes)
{
    size_t need = 0;
    const hipError_t err = rocprim::radix_sort_pairs(nullptr, need, (const AsmKey*)nullptr, (AsmKey*)nullptr, (const int*)nullptr,
                                                     (int*)nullptr, n);
    *bytes = alignUpCv(need, 256);
    return err;
}

/* ---- the plan ---- */
__global__ __launch_bounds__(kCvThreads) void asmEmitKeysKernel(AsmKey* keys, int* ids, int* misc, int rows, int cols, int nnz,
                                                                const int* cooRows, const int* cooCols, int cooBase, int colBits)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < nnz; i += stride) {
        const unsigned r = (unsigned)cooRows[i] - (unsigned)cooBase, c = (unsigned)cooCols[i] - (unsigned)cooBase;
        const bool bad = r >= (unsigned)rows || c >= (unsigned)cols;
        if (bad)
            misc[1] = 1;
        keys[i] = bad ? (AsmKey)0 : ((AsmKey)r << colBits) | c;
        ids[i] = (int)i;
    }
}

/* a head at sorted position p is the first contribution of entry entryOf[p]; *unique = the number of heads */
__global__ __launch_bounds__(kCvThreads) void asmSegPtrKernel(int* segPtr, const int* entryOf, const AsmKey* keys, int nnz, const int* unique)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long p = (long long)blockIdx.x * kCvThreads + threadIdx.x; p < nnz; p += stride) {
        if (p == 0 || keys[p] != keys[p - 1])
            segPtr[entryOf[p]] = (int)p;
        if (p == 0)
            segPtr[*unique] = nnz;
    }
}

/* rowStart[r] is a head, or nnz: the entries in front of it are the entries of the rows < r */
__global__ __launch_bounds__(kCvThreads) void asmRowPtrKernel(int* csrRowPtr, const int* rowStart, const int* entryOf, int rows, int nnz,
                                                              const int* unique, int csrBase)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long r = (long long)blockIdx.x * kCvThreads + threadIdx.x; r <= rows; r += stride) {
        const int at = rowStart[r];
        csrRowPtr[r] = csrBase + (at < nnz ? entryOf[at] : *unique);
    }
}

/* ---- the fills ---- */
__global__ __launch_bounds__(kAsmThreads) void asmColumnsKernel(int* csrCols, int unique, const int* cooCols, int shift, const int* perm,
                                                                const int* segPtr)
{
    const long long stride = (long long)gridDim.x * kAsmThreads;
    for (long long u = (long long)blockIdx.x * kAsmThreads + threadIdx.x; u < unique; u += stride)
        csrCols[u] = cooCols[perm[segPtr[u]]] + shift;
}

/* The plain fill: one thread per matrix entry. */
template <typename T>
__global__ __launch_bounds__(kAsmThreads) void assembleEntryKernel(T* csrVals, int unique, const T* cooVals, const int* perm, const int* segPtr)
{
    const long long stride = (long long)gridDim.x * kAsmThreads;
    for (long long u = (long long)blockIdx.x * kAsmThreads + threadIdx.x; u < unique; u += stride) {
        const int first = segPtr[u], end = segPtr[u + 1];
        if (first >= end)
            continue; /* not a segment of a plan: nothing to add, nothing written */
        T run = cooVals[perm[first]];
        for (int p = first + 1; p < end; ++p)
            run = add(run, cooVals[perm[p]]);
        csrVals[u] = run;
    }
}

/* The staged fill (head of the file).  `tiles` tiles of kAsmTile entries, grid-strided by workgroup. */
template <typename T>
__global__ __launch_bounds__(kAsmThreads) void assembleStagedKernel(T* csrVals, int unique, long long tiles, const T* cooVals, const int* perm,
                                                                    const int* segPtr)
{
    __shared__ T landed[kAsmChunk];
    const int t = threadIdx.x;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long u0 = tile * kAsmTile, u = u0 + t;
        const int inTile = unique - u0 < kAsmTile ? (int)(unique - u0) : kAsmTile;
        const int tileFirst = segPtr[u0], tileEnd = segPtr[u0 + inTile]; /* the same in every thread */
        int first = 0, end = 0;
        if (t < inTile)
            first = segPtr[u], end = segPtr[u + 1];
        if (tileEnd - tileFirst == inTile) { /* workgroup-uniform: every segment of the tile is one contribution */
            if (t < inTile)
                csrVals[u] = cooVals[perm[first]];
            continue;
        }
        T run = zeroOf<T>(); /* never read before the segment's first contribution replaces it */
        for (int c0 = tileFirst; c0 < tileEnd; c0 += kAsmChunk) {
            const int here = tileEnd - c0 < kAsmChunk ? tileEnd - c0 : kAsmChunk;
            int from[kAsmLoads];
#pragma unroll
            for (int k = 0; k < kAsmLoads; ++k)
                from[k] = k * kAsmThreads + t < here ? perm[c0 + k * kAsmThreads + t] : -1;
            T got[kAsmLoads]; /* loaded without a branch (a position beyond the range re-reads contribution 0 and is dropped): the
                               * four gathers leave together, and a 16-byte element stays in registers */
#pragma unroll
            for (int k = 0; k < kAsmLoads; ++k)
                got[k] = cooVals[from[k] >= 0 ? from[k] : 0];
#pragma unroll
            for (int k = 0; k < kAsmLoads; ++k)
                if (from[k] >= 0)
                    landed[k * kAsmThreads + t] = got[k];
            __syncthreads();
            const int lo = first > c0 ? first : c0, hi = end < c0 + here ? end : c0 + here;
            if (lo < hi) {
                int i = lo - c0;
                if (lo == first)
                    run = landed[i++];
                for (; i < hi - c0; ++i)
                    run = add(run, landed[i]);
                if (hi == end)
                    csrVals[u] = run;
            }
            __syncthreads(); /* the next trip lands on what this one read */
        }
    }
}

template <typename T>
static void launchValues(hipStream_t s, void* csrVals, int unique, const void* cooVals, const int* perm, const int* segPtr, int fill, int maxBlocks)
{
    if (fill == SPGPU_ASSEMBLE_FILL_PLAIN) {
        hipLaunchKernelGGL(assembleEntryKernel<T>, dim3(cappedGrid(unique, kAsmThreads, maxBlocks)), dim3(kAsmThreads), 0, s,
                           static_cast<T*>(csrVals), unique, static_cast<const T*>(cooVals), perm, segPtr);
        return;
    }
    const long long tiles = ((long long)unique + kAsmTile - 1) / kAsmTile;
    hipLaunchKernelGGL(assembleStagedKernel<T>, dim3(cappedGrid(tiles, 1, maxBlocks)), dim3(kAsmThreads), 0, s, static_cast<T*>(csrVals), unique,
                       tiles, static_cast<const T*>(cooVals), perm, segPtr);
}

/* fill < 0: the one the public calls run.  csrCols == NULL: values only. */
static spgpuStatus_t assemble(spgpuHandle_t handle, int* csrCols, void* csrVals, int unique, int nnz, const int* cooCols, const void* cooVals,
                              int cooBase, int csrBase, spgpuType_t type, const int* perm, const int* segPtr, int fill, int maxBlocks)
{
    if (nnz <= 0 || unique <= 0)
        return SPGPU_SUCCESS;
    if (fill < 0)
        fill = kAsmDefaultFill;
    if (fill != SPGPU_ASSEMBLE_FILL_PLAIN && fill != SPGPU_ASSEMBLE_FILL_STAGED)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const bool launched = forValueType(type, [&](auto tag) {
        if (csrCols)
            hipLaunchKernelGGL(asmColumnsKernel, dim3(cappedGrid(unique, kAsmThreads, maxBlocks)), dim3(kAsmThreads), 0, s, csrCols, unique,
                               cooCols, csrBase - cooBase, perm, segPtr);
        launchValues<decltype(tag)>(s, csrVals, unique, cooVals, perm, segPtr, fill, maxBlocks);
    });
    if (!launched)
        return SPGPU_UNSUPPORTED;
    spgpuDebugCheck(handle, "coo assemble");
    return SPGPU_SUCCESS;
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_assemble.py and the tests that compare the two fills.  fill: 0 the plain fill, 1 the
 * staged fill, < 0 the public call's choice; maxBlocks > 0 caps the grid (the grid stride on a small list). */
spgpuStatus_t spgpuCooAssembleDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, int uniqueCount, int nonZerosCount,
                                         const int* cooColsIndices, const void* cooValues, int cooBaseIndex, int csrBaseIndex,
                                         spgpuType_t valuesType, const int* perm, const int* segPtr, int fill, int maxBlocks);
spgpuStatus_t spgpuCooAssembleValuesDeviceWith(spgpuHandle_t handle, void* csrValues, int uniqueCount, int nonZerosCount, const void* cooValues,
                                               spgpuType_t valuesType, const int* perm, const int* segPtr, int fill, int maxBlocks);
int spgpuCooAssembleDefaultFill(void);
int spgpuCooAssembleTile(void);  /* matrix entries per workgroup of the staged fill */
int spgpuCooAssembleChunk(void); /* positions of perm per trip through LDS, counted from the tile's first position */

int spgpuCooAssembleDefaultFill(void) { return kAsmDefaultFill; }
int spgpuCooAssembleTile(void) { return kAsmTile; }
int spgpuCooAssembleChunk(void) { return kAsmChunk; }

size_t spgpuCooAssembleWorkBytes(int rowsCount, int columnsCount, int nonZerosCount)
{
    (void)columnsCount; /* the columns cost key bits, not scratch */
    const int rows = rowsCount > 0 ? rowsCount : 0;
    const size_t nnz = nonZerosCount > 0 ? (size_t)nonZerosCount : 0;
    size_t temp = 0;
    if (nnz > 0 && asmSortTempBytes(nnz, &temp) != hipSuccess)
        return 0; /* no GPU to ask for rocPRIM's share */
    return (asmHeadInts(rows, nnz) + 6 * alignUpCv(nnz, 64)) * sizeof(int) + temp + 256;
}

spgpuStatus_t spgpuCooAssemblePlanDevice(spgpuHandle_t handle, int* uniqueCount, int* csrRowPtr, int* perm, int* segPtr, int rowsCount,
                                         int columnsCount, int nonZerosCount, const int* cooRowIndices, const int* cooColsIndices,
                                         int cooBaseIndex, int csrBaseIndex, void* work)
{
    *uniqueCount = 0;
    if (rowsCount <= 0)
        return SPGPU_SUCCESS;
    hipStream_t s = handle->currentStream;
    if (nonZerosCount <= 0) {
        hipLaunchKernelGGL(csrSetIntsKernel, dim3(gridFor((long long)rowsCount + 1)), dim3(kCvThreads), 0, s, csrRowPtr, (long long)rowsCount + 1,
                           csrBaseIndex);
        (void)hipMemsetAsync(segPtr, 0, sizeof(int), s);
        spgpuDebugCheck(handle, "coo assemble plan");
        return SPGPU_SUCCESS;
    }
    if (columnsCount <= 0 || !work)
        return SPGPU_UNSUPPORTED;
    const int nnz = nonZerosCount;
    const AssembleWork w = carveAssemble(work, rowsCount, (size_t)nnz);
    const int rowBits = bitsFor(rowsCount), colBits = bitsFor(columnsCount);
    const size_t tiles = scanBlocks(nnz);
    const int* unique = w.totals + tiles; /* the scan's grand total */
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    size_t bytes = 0;
    if (asmSortTempBytes((size_t)nnz, &bytes) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    (void)hipMemsetAsync(w.misc, 0, 16 * sizeof(int), s);
    hipLaunchKernelGGL(asmEmitKeysKernel, dim3(gridFor(nnz)), dim3(kCvThreads), 0, s, w.keysA, w.idA, w.misc, rowsCount, columnsCount, nnz,
                       cooRowIndices, cooColsIndices, cooBaseIndex, colBits);
    /* at least one bit: a 1 x 1 matrix has keys of no bits at all */
    if (rocprim::radix_sort_pairs(w.temp, bytes, (const AsmKey*)w.keysA, w.keysB, (const int*)w.idA, perm, (size_t)nnz, 0u,
                                  (unsigned)(rowBits + colBits > 0 ? rowBits + colBits : 1), s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    hipLaunchKernelGGL(csrHeadFlagsKernel, dim3(gridFor(nnz)), dim3(kCvThreads), 0, s, w.entryOf, (const AsmKey*)w.keysB, nnz);
    exclusiveScan(s, w.entryOf, w.entryOf, (long long)nnz, 1, w.totals); /* in place: a thread reads its four flags before it writes them */
    hipLaunchKernelGGL(asmSegPtrKernel, dim3(gridFor(nnz)), dim3(kCvThreads), 0, s, segPtr, (const int*)w.entryOf, (const AsmKey*)w.keysB, nnz,
                       unique);
    hipLaunchKernelGGL(rowStartKernel<AsmKey>, dim3(gridFor((long long)rowsCount + 1)), dim3(kCvThreads), 0, s, w.rowStart, rowsCount,
                       (const AsmKey*)w.keysB, colBits, nnz);
    hipLaunchKernelGGL(asmRowPtrKernel, dim3(gridFor((long long)rowsCount + 1)), dim3(kCvThreads), 0, s, csrRowPtr, (const int*)w.rowStart,
                       (const int*)w.entryOf, rowsCount, nnz, unique, csrBaseIndex);
    (void)hipMemcpyAsync(host, unique, sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(host + 1, w.misc + 1, sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "coo assemble plan");
    if (host[1])
        return SPGPU_UNSUPPORTED; /* an entry outside the matrix: the arrays hold the plan of some other list */
    *uniqueCount = host[0];
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCooAssembleDeviceWith(spgpuHandle_t handle, int* csrColIndices, void* csrValues, int uniqueCount, int nonZerosCount,
                                         const int* cooColsIndices, const void* cooValues, int cooBaseIndex, int csrBaseIndex,
                                         spgpuType_t valuesType, const int* perm, const int* segPtr, int fill, int maxBlocks)
{
    if (nonZerosCount > 0 && uniqueCount > 0 && !csrColIndices)
        return SPGPU_UNSUPPORTED;
    return assemble(handle, csrColIndices, csrValues, uniqueCount, nonZerosCount, cooColsIndices, cooValues, cooBaseIndex, csrBaseIndex, valuesType,
                    perm, segPtr, fill, maxBlocks);
}

spgpuStatus_t spgpuCooAssembleValuesDeviceWith(spgpuHandle_t handle, void* csrValues, int uniqueCount, int nonZerosCount, const void* cooValues,
                                               spgpuType_t valuesType, const int* perm, const int* segPtr, int fill, int maxBlocks)
{
    return assemble(handle, nullptr, csrValues, uniqueCount, nonZerosCount, nullptr, cooValues, 0, 0, valuesType, perm, segPtr, fill, maxBlocks);
}

spgpuStatus_t spgpuCooAssembleDevice(spgpuHandle_t handle, int* csrColIndices, void* csrValues, int uniqueCount, int nonZerosCount,
                                     const int* cooColsIndices, const void* cooValues, int cooBaseIndex, int csrBaseIndex,
                                     spgpuType_t valuesType, const int* perm, const int* segPtr)
{
    return spgpuCooAssembleDeviceWith(handle, csrColIndices, csrValues, uniqueCount, nonZerosCount, cooColsIndices, cooValues, cooBaseIndex,
                                      csrBaseIndex, valuesType, perm, segPtr, -1, 0);
}

spgpuStatus_t spgpuCooAssembleValuesDevice(spgpuHandle_t handle, void* csrValues, int uniqueCount, int nonZerosCount, const void* cooValues,
                                           spgpuType_t valuesType, const int* perm, const int* segPtr)
{
    return spgpuCooAssembleValuesDeviceWith(handle, csrValues, uniqueCount, nonZerosCount, cooValues, valuesType, perm, segPtr, -1, 0);
}

} // extern "C"
