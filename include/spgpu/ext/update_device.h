#pragma once
/*
 * New coefficients for a HELL or ELL matrix the caller already holds in HBM, its sparsity pattern unchanged (the reference has
 * spgpu?ellcsput for ELL only, and nothing for HELL or for a matrix with a row order).
 *
 * NEW: what a time-stepping or Newton solver does at every step -- PSBLAS drives the reference this way through psb_spins /
 * csput -- without rebuilding the matrix.  spgpuCsrToHellDevice (spgpu/ext/csr_device.h) would do, but it reads and writes every
 * column index again (24 bytes per fp64 entry instead of 16), and the calls here touch no index at all: rP, the row order, a
 * plan of the ordered SpMV and a frozen record (spgpu?SpmvFreeze, spgpu/tuning.h) stay valid, so a FROZEN matrix takes new
 * values with no Thaw -- the coefficients are always read from the caller's cM.  An ADOPTED matrix (spgpu?SpmvAdopt) is
 * different: the library multiplies by its own ordered copy of cM, which these calls do not see.  Thaw an adopted matrix
 * (spgpuSpmvThaw) before its coefficients change, and adopt it again afterwards.
 *
 * All array arguments are DEVICE pointers.  Every call runs asynchronously on handle->currentStream, allocates nothing, keeps
 * no state and never synchronises: it can be captured into a HIP graph.
 *
 * THE CONTRACT of the value refill (spgpuCsrToHellValuesDevice / spgpuCsrToEllValuesDevice), worded against the full fill
 * spgpuCsrToHellDevice / spgpuCsrToEllDevice of spgpu/ext/csr_device.h:
 *   - the calls write exactly the value slots the full fill writes for the same csrRowPtr, rIdx, hackOffsets and hackSize (ELL:
 *     pitch), with the bytes the full fill would write there for these csrValues;
 *   - destination row i is CSR row rIdx[i] (0-based), or row i when rIdx == NULL; slot k of that row gets the row's k-th CSR
 *     entry.  An rIdx[i] outside [0, rowsCount) leaves row i untouched;
 *   - values are moved as 4-, 8- or 16-byte words (spgpuSizeOf(valuesType)), never as numbers: NaN payloads and -0.0 survive.
 *     Any other element size returns SPGPU_UNSUPPORTED.  csrValues needs the alignment of its element type only (4 or 8 bytes);
 *   - no column index is read or written: neither csrColIndices nor rP is an argument.  Slots beyond a row's end are neither
 *     read nor written;
 *   - each element has one writer and no atomics are used: the array does not depend on scheduling;
 *   - the caller vouches that csrRowPtr (and rIdx, hackOffsets, hackSize or the pitch) is what the matrix was built from: the
 *     calls trust it as the full fill does, and as the to-CSR fill calls trust what their row-pointer call accepted;
 *   - rowsCount <= 0 returns SPGPU_SUCCESS before anything touches the stream.
 *
 * THE CONTRACT of spgpu?hellcsput is spgpu?ellcsput's (spgpu/ell.h), word for word, on HELL storage:
 *   - for every i < nnz the matrix row is aI[i] - baseIndex; a negative row is ignored;
 *   - the first rS[row] stored indices of the row -- which must ascend -- are searched by bisection for aJ[i], compared with
 *     the STORED indices as they are (same base as rP); the coefficient found is overwritten with aVal[i]; an entry that is
 *     not found is ignored;
 *   - alpha is accepted and not applied;
 *   - rowOf == NULL: the storage row is the matrix row.  rowOf != NULL (a matrix with a row order): the storage row is
 *     rowOf[matrix row], the inverse of the rIdx the matrix is stored with (spgpuInvertRowOrderDevice).  A matrix row or a
 *     storage row outside [0, rows) is ignored: `rows` stands where spgpu?hellspmv has it;
 *   - two list entries that name the same stored entry leave ONE of the two values there, which one is not defined;
 *   - nnz <= 0 returns before anything is launched.
 *
 * spgpuInvertRowOrderDevice writes rowOf[rIdx[r]] = r for every r < rows; an rIdx[r] outside [0, rows) is skipped; rows <= 0
 * does nothing.  Entries of rowOf that no rIdx[r] names are left as they are (fill rowOf with -1 first if rIdx may be partial).
 *
 * A solver that re-assembles an ordered, frozen HELL matrix at every step:
 *
 *     (once)  spgpuCsrToHellDevice(h, cM, rP, hackOffsets, 32, base, rows, rowPtr, cols, vals, base, type, rIdx);
 *             spgpuHellSpmvFreeze(h, type, cM, rP, 32, hackOffsets, sortedLengths, rIdx, rows, base);
 *             spgpuInvertRowOrderDevice(h, rowOf, rIdx, rows);
 *     (step)  spgpuCsrToHellValuesDevice(h, cM, hackOffsets, 32, rows, rowPtr, vals, base, type, rIdx);        all of them, or
 *             spgpuDhellcsput(h, 1.0, cM, rP, 32, hackOffsets, sortedLengths, rowOf, rows, n, aI, aJ, aVal, base);   some
 *             spgpuDhellspmv(h, z, y, alpha, cM, rP, 32, hackOffsets, sortedLengths, rIdx, avg, rows, x, beta, base);
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  hellValues as spgpuCsrToHellDevice filled it; only value slots are written. */
spgpuStatus_t spgpuCsrToHellValuesDevice(spgpuHandle_t handle, __device void* hellValues, const __device int* hackOffsets,
                                         int hackSize, int rowsCount, const __device int* csrRowPtr,
                                         const __device void* csrValues, int csrBaseIndex, spgpuType_t valuesType,
                                         const __device int* rIdx);

/* NEW (no counterpart in the reference).  The same with an ELL destination (slot k of row i at i + k * ellValuesPitch). */
spgpuStatus_t spgpuCsrToEllValuesDevice(spgpuHandle_t handle, __device void* ellValues, int ellValuesPitch, int rowsCount,
                                        const __device int* csrRowPtr, const __device void* csrValues, int csrBaseIndex,
                                        spgpuType_t valuesType, const __device int* rIdx);

/* NEW (no counterpart in the reference).  rowOf[rIdx[r]] = r: the storage row of every matrix row. */
spgpuStatus_t spgpuInvertRowOrderDevice(spgpuHandle_t handle, __device int* rowOf, const __device int* rIdx, int rows);

/* NEW (the reference has csput for ELL only: ell.h:194-302). */
void spgpuShellcsput(spgpuHandle_t handle, float alpha, __device float* cM, __device const int* rP, int hackSize,
                     __device const int* hackOffsets, __device const int* rS, __device const int* rowOf, int rows, int nnz,
                     __device int* aI, __device int* aJ, __device float* aVal, int baseIndex);
void spgpuDhellcsput(spgpuHandle_t handle, double alpha, __device double* cM, __device const int* rP, int hackSize,
                     __device const int* hackOffsets, __device const int* rS, __device const int* rowOf, int rows, int nnz,
                     __device int* aI, __device int* aJ, __device double* aVal, int baseIndex);
void spgpuChellcsput(spgpuHandle_t handle, hipFloatComplex alpha, __device hipFloatComplex* cM, __device const int* rP,
                     int hackSize, __device const int* hackOffsets, __device const int* rS, __device const int* rowOf, int rows,
                     int nnz, __device int* aI, __device int* aJ, __device hipFloatComplex* aVal, int baseIndex);
void spgpuZhellcsput(spgpuHandle_t handle, hipDoubleComplex alpha, __device hipDoubleComplex* cM, __device const int* rP,
                     int hackSize, __device const int* hackOffsets, __device const int* rS, __device const int* rowOf, int rows,
                     int nnz, __device int* aI, __device int* aJ, __device hipDoubleComplex* aVal, int baseIndex);

#ifdef __cplusplus
}
#endif
