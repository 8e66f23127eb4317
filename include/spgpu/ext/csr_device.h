#pragma once
/*
 * Device-side format construction FROM CSR: CSR -> ELL and CSR -> HELL entirely in HBM (no counterpart in the reference,
 * which converts COO on one host thread).
 *
 * NEW: the front door for whoever holds CSR -- rocSPARSE, torch.sparse_csr, PETSc, PSBLAS.  The COO route of
 * spgpu/convert_device.h sorts all nonzeros to recover a grouping that CSR already has (and, for a row order, rewrites every
 * COO row index and sorts again).  From CSR a row's length is a difference of two csrRowPtr entries, a row's entries are
 * one contiguous run and a row order is one indirection per row: these calls read the CSR arrays once, write every stored
 * slot once, and need NO scratch and no sort.
 *
 * All array arguments are DEVICE pointers unless marked host.  The calls run on handle->currentStream; only
 * spgpuCsrRowLengthsDevice returns a host scalar and therefore synchronises that stream.
 *
 * THE ARRAYS are, byte for byte, what the COO route gives for the same matrix as row-major COO (and so what the host
 * converters computeEllRowLenghts / cooToEll / computeHellAllocSize / ellToHell give), for any hackSize -- multiples of 32 or
 * not:
 *   - destination arrays are zeroed by the caller; slots beyond a row's end are not written;
 *   - the k-th stored entry of a row is its k-th CSR entry: duplicates are kept, nothing is sorted;
 *   - a column index becomes csrColIndices[e] - csrBaseIndex + ellBaseIndex (or hellBaseIndex);
 *   - values are moved as 4-, 8- or 16-byte words (spgpuSizeOf(valuesType)), never as numbers: NaN payloads survive.  Any
 *     other element size returns SPGPU_UNSUPPORTED.  csrValues needs the alignment of its real type only (4 or 8 bytes);
 *   - rIdx == NULL: destination row i is CSR row i.  rIdx != NULL: destination row i is CSR row rIdx[i] (0-based) -- the
 *     meaning rIdx has in spgpuOellOrderDevice (spgpu/oell_device.h) and in the SpMV calls; the arrays are then those of
 *     spgpuCooPermuteRowsDevice followed by the COO route.  An rIdx[i] outside [0, rowsCount) leaves row i empty;
 *   - rowsCount <= 0 returns SPGPU_SUCCESS before anything is launched; a matrix without entries writes nothing.
 *
 * hackOffsets comes from spgpuHellPlanDevice (spgpu/convert_device.h), called on the row lengths IN DESTINATION ORDER:
 * rowLengths of spgpuCsrRowLengthsDevice without a row order, the dstRs that spgpuOellOrder*Device returns with one.  That
 * call touches only the fixed head of its `work` area: spgpuCooConvertWorkBytes(rowsCount, 0) bytes are enough for it.
 *
 * The ordered HELL matrix of a CSR holder, with no pass over the nonzeros but the fill:
 *
 *     spgpuCsrRowLengthsDevice(h, lengths, &longest, rows, rowPtr, base);
 *     spgpuOellOrderAlignedDevice(h, rIdx, sortedLengths, lengths, rows, 2048, 256, orderWork);
 *     spgpuHellPlanDevice(h, &height, hackOffsets, 32, rows, sortedLengths, work);
 *     spgpuCsrToHellDevice(h, cM, rP, hackOffsets, 32, base, rows, rowPtr, cols, vals, base, type, rIdx);
 *     spgpuDhellspmv(h, z, y, alpha, cM, rP, 32, hackOffsets, sortedLengths, rIdx, avg, rows, x, beta, base);
 *
 * The opposite direction, CSR arrays from a stored HELL or ELL matrix, is ext/to_csr_device.h.  New coefficients for a matrix
 * these calls built, its pattern unchanged (no column index read or written again), are ext/update_device.h.  The product of
 * two CSR matrices, whose result these calls take, is ext/spgemm_device.h.  Their sum alpha * A + beta * B is ext/add_device.h.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rowLengths[i] = csrRowPtr[i+1] - csrRowPtr[i]; the longest row comes back on the host
 * (synchronises the stream, like spgpuCooRowLengthsDevice).
 * SPGPU_UNSUPPORTED if csrRowPtr[0] != csrBaseIndex or csrRowPtr descends anywhere:
 * reported, never dereferenced further. */
spgpuStatus_t spgpuCsrRowLengthsDevice(spgpuHandle_t handle, __device int* rowLengths, __host int* maxRowSize,
                                       int rowsCount, const __device int* csrRowPtr, int csrBaseIndex);

spgpuStatus_t spgpuCsrToEllDevice(spgpuHandle_t handle, __device void* ellValues, __device int* ellIndices,
                                  int ellValuesPitch, int ellIndicesPitch, int ellBaseIndex, int rowsCount,
                                  const __device int* csrRowPtr, const __device int* csrColIndices,
                                  const __device void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                  const __device int* rIdx);

spgpuStatus_t spgpuCsrToHellDevice(spgpuHandle_t handle, __device void* hellValues, __device int* hellIndices,
                                   const __device int* hackOffsets, int hackSize, int hellBaseIndex, int rowsCount,
                                   const __device int* csrRowPtr, const __device int* csrColIndices,
                                   const __device void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                   const __device int* rIdx);

#ifdef __cplusplus
}
#endif
