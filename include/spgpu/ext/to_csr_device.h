#pragma once
/*
 * Device-side construction of CSR arrays FROM a stored HELL or ELL matrix, entirely in HBM (no counterpart in the reference,
 * which has no way back from its formats at all).
 *
 * NEW: the way back out for whoever speaks CSR -- rocSPARSE, torch.sparse_csr, PETSc, PSBLAS -- after spgpu/ext/csr_device.h
 * (or the COO route of spgpu/convert_device.h) brought the matrix in: an AMG setup, a vendor SpGEMM / ILU, a checkpoint, a
 * comparison.  With spgpu/ext/transpose_device.h in front, the CSR arrays of A^T are the CSC arrays of A.
 *
 * All array arguments are DEVICE pointers unless marked host.  The calls run on handle->currentStream.  The two row-pointer
 * calls return host scalars and therefore synchronise that stream, like spgpuCsrRowLengthsDevice; the two fill calls are
 * asynchronous on it and allocate nothing.
 *
 * THE SOURCE is read as spgpu?hellspmv / spgpu?ellspmv read it: cM / rP, hackOffsets, rS, rIdx and the base index mean what
 * they mean there.  Storage row r holds matrix row i = rIdx[r] (0-based) when rIdx != NULL, i = r otherwise; its entries are
 * the slots k = 0 .. rS[r]-1 (HELL: hackOffsets[r / hackSize] + r % hackSize + k * hackSize; ELL: r + k * pitch).  rS is
 * required.  `slots` is the number of stored slots of the source (HELL: hackSize * allocationHeight; ELL: ellIndicesPitch *
 * maxRowSize).
 *
 * THE CONTRACT
 *   - row pointers: csrRowPtr[i] = csrBaseIndex + the lengths of the matrix rows before i, in MATRIX-row order;
 *     csrRowPtr[rowsCount] - csrBaseIndex is the number of stored entries, returned in *nonZerosCount; the longest row in
 *     *maxRowSize;
 *   - entry order: the k-th CSR entry of matrix row i is slot k of its storage row: duplicates are kept, nothing is sorted.
 *     spgpuCsrToHellDevice followed by these calls, with the same rIdx, gives back the caller's CSR arrays byte for byte; the
 *     opposite round trip gives back every stored slot;
 *   - a column index becomes rP[slot] - hellBaseIndex (ellBaseIndex) + csrBaseIndex;
 *   - values are moved as 4-, 8- or 16-byte words (spgpuSizeOf(valuesType)), never as numbers: NaN payloads and -0.0 survive.
 *     Any other element size returns SPGPU_UNSUPPORTED.  csrValues / csrColIndices need the alignment of their element type
 *     only (4 or 8 bytes);
 *   - padding: slots with k >= rS[r] are never read, neither as an index nor as a value;
 *   - writes: exactly nonZerosCount elements of csrColIndices and of csrValues are written, each once, by one writer; no
 *     atomics touch the data, so the arrays do not depend on scheduling.  Nothing else of the caller's is touched;
 *   - rowsCount <= 0 returns SPGPU_SUCCESS, both scalars 0, before anything is launched: nothing is written;
 *   - SPGPU_UNSUPPORTED from a row-pointer call -- an rS[r] that is negative, a row whose last slot lies at or beyond `slots`, an
 *     rIdx[r] outside [0, rowsCount), two storage rows that name one matrix row (a matrix row that no storage row names cannot
 *     then occur), an ELL pitch below rowsCount -- is reported and never dereferenced further: nothing but `work` and csrRowPtr
 *     has been written.  The fill calls trust what the row-pointer call accepted.
 *
 * `work` is caller-provided scratch of spgpuToCsrWorkBytes(rowsCount) bytes with the alignment of an int: the lengths in matrix order,
 * the count of storage rows per matrix row (integer atomics: order-independent) and the tile totals of the scan.  It is free
 * again when the row-pointer call returns.
 *
 * CSR arrays of a HELL matrix, and of its transpose (the CSC arrays of A):
 *
 *     work = malloc(spgpuToCsrWorkBytes(rows));
 *     spgpuHellToCsrRowPtrDevice(h, rowPtr, &nnz, &longest, base, hackSize, hackOffsets, rS, rIdx, rows, slots, work);
 *     (allocate cols: nnz ints, vals: nnz elements)
 *     spgpuHellToCsrDevice(h, cols, vals, rowPtr, base, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, base, type);
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `work` for a source of rowsCount rows.  Host arithmetic only (no GPU is asked); a multiple of 256; 0 for
 * rowsCount <= 0. */
size_t spgpuToCsrWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  Fills csrRowPtr[rowsCount + 1] on the device; the number of stored entries and the
 * longest row come back on the host (synchronises the stream). */
spgpuStatus_t spgpuHellToCsrRowPtrDevice(spgpuHandle_t handle, __device int* csrRowPtr, __host int* nonZerosCount,
                                         __host int* maxRowSize, int csrBaseIndex, int hackSize,
                                         const __device int* hackOffsets, const __device int* rS, const __device int* rIdx,
                                         int rowsCount, int slots, __device void* work);

/* NEW (no counterpart in the reference).  Fills csrColIndices and csrValues (nonZerosCount elements each); csrRowPtr as the
 * call above left it for the same source. */
spgpuStatus_t spgpuHellToCsrDevice(spgpuHandle_t handle, __device int* csrColIndices, __device void* csrValues,
                                   const __device int* csrRowPtr, int csrBaseIndex, const __device void* cM,
                                   const __device int* rP, int hackSize, const __device int* hackOffsets,
                                   const __device int* rS, const __device int* rIdx, int rowsCount, int hellBaseIndex,
                                   spgpuType_t valuesType);

/* NEW (no counterpart in the reference).  The same with an ELL source (slot k of storage row r at r + k * pitch). */
spgpuStatus_t spgpuEllToCsrRowPtrDevice(spgpuHandle_t handle, __device int* csrRowPtr, __host int* nonZerosCount,
                                        __host int* maxRowSize, int csrBaseIndex, int ellIndicesPitch,
                                        const __device int* rS, const __device int* rIdx, int rowsCount, int slots,
                                        __device void* work);

/* NEW (no counterpart in the reference). */
spgpuStatus_t spgpuEllToCsrDevice(spgpuHandle_t handle, __device int* csrColIndices, __device void* csrValues,
                                  const __device int* csrRowPtr, int csrBaseIndex, const __device void* cM,
                                  const __device int* rP, int ellValuesPitch, int ellIndicesPitch, const __device int* rS,
                                  const __device int* rIdx, int rowsCount, int ellBaseIndex, spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
