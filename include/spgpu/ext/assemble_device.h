#pragma once
/*
 * Assembly on the device: a COO list of (row, column, value) CONTRIBUTIONS in any order, in which one matrix entry may appear
 * several times, becomes the CSR arrays of the matrix whose entries are the SUMS (the reference has nothing of the kind: its
 * cooToEll keeps every duplicate, and so does spgpuCooToHellDevice of spgpu/convert_device.h, byte for byte).
 *
 * NEW: what a finite-element, finite-volume or graph code does before anything else -- PETSc offers the same pair as
 * MatSetPreallocationCOO / MatSetValuesCOO -- without a round trip through the host.  The pair is an ANALYSIS of the pattern, once
 * (spgpuCooAssemblePlanDevice: one stable radix sort, rocPRIM), and a pass over the values at every step
 * (spgpuCooAssembleValuesDevice).  The CSR arrays have ascending, duplicate-free columns in every row, so the matrix built from
 * them (spgpu/ext/csr_device.h) streams no duplicate in an SpMV, takes the partial updates of spgpu?hellcsput and spgpu?ellcsput,
 * which bisect for the column, and the refill spgpuCsrToHellValuesDevice (spgpu/ext/update_device.h).
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.  The plan returns a host
 * scalar and therefore synchronises that stream; the two fills are asynchronous, allocate nothing, need no scratch, keep no
 * state and never synchronise: they can be captured into a HIP graph.
 *
 * THE CONTRACT
 * Matrix entries
 *   - a matrix entry is a distinct (row, column) pair of the list; entries are numbered u = 0 .. uniqueCount-1 by ascending row,
 *     then ascending column;
 *   - the output is CSR with ascending, duplicate-free columns in every row: csrRowPtr[r] - csrBaseIndex is the number of
 *     entries in rows < r, csrRowPtr[rowsCount] - csrBaseIndex == uniqueCount, and a row without contributions is empty.
 * The plan arrays
 *   - perm lists the COO entry ids (0-based positions in the list) grouped by matrix entry; within one matrix entry they stand
 *     in ascending COO position: the sort is stable, and its key is (row, column) over exactly the bits rowsCount and
 *     columnsCount need;
 *   - segPtr[u] .. segPtr[u+1] is the range of perm that belongs to entry u (0-based); segPtr[uniqueCount] == nonZerosCount;
 *     elements of segPtr beyond uniqueCount are not written;
 *   - the plan arrays are self-contained: after the plan returns, `work` may be freed; neither fill reads it.
 * Columns and values
 *   - csrColIndices[u] = cooColsIndices[perm[segPtr[u]]] - cooBaseIndex + csrBaseIndex;
 *   - csrValues[u] is the sum of the contributions in perm order, left to right: ((v0 + v1) + v2) + ...; each addition is
 *     rounded in the element type, complex sums are componentwise;
 *   - the sum starts from the first contribution, not from zero: an entry with a single contribution is moved as bits, so -0.0
 *     and NaN payloads survive;
 *   - each element has one writer and no atomics are used: the arrays do not depend on scheduling, and a repeated call gives
 *     the same bytes;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED (the
 *     fills add, so they must know the type: the element size is not enough);
 *   - spgpuCooAssembleValuesDevice reads and writes no index other than perm and segPtr.
 * Errors and degenerate inputs
 *   - a row outside [cooBaseIndex, cooBaseIndex + rowsCount) or a column outside [cooBaseIndex, cooBaseIndex + columnsCount)
 *     makes the plan return SPGPU_UNSUPPORTED (the convention of spgpuCooRowLengthsDevice); no output array then has a defined
 *     content, and nothing out of bounds is read or written;
 *   - nonZerosCount <= 0: the plan writes csrRowPtr (all csrBaseIndex) and segPtr[0] = 0, sets *uniqueCount = 0 and succeeds;
 *     the two fills return SPGPU_SUCCESS before touching the stream (as they do for uniqueCount <= 0);
 *   - rowsCount <= 0: SPGPU_SUCCESS with nothing launched, *uniqueCount = 0;
 *   - the fills trust perm and segPtr as the refill of spgpu/ext/update_device.h trusts csrRowPtr.
 *
 * `work` is caller-provided scratch of spgpuCooAssembleWorkBytes(rowsCount, columnsCount, nonZerosCount) bytes (about 24 bytes
 * per contribution plus rocPRIM's share; 0 if no GPU can be asked for that share).
 *
 * A solver that assembles a HELL matrix once and re-assembles its coefficients at every step:
 *
 *     (once)  spgpuCooAssemblePlanDevice(h, &unique, rowPtr, perm, segPtr, rows, cols, nnz, cooRows, cooCols, base, base, work);
 *             spgpuCooAssembleDevice(h, csrCols, csrVals, unique, nnz, cooCols, cooVals, base, base, type, perm, segPtr);
 *             spgpuCsrRowLengthsDevice / spgpuHellPlanDevice / spgpuCsrToHellDevice(h, cM, rP, ..., rowPtr, csrCols, csrVals, ...);
 *     (step)  spgpuCooAssembleValuesDevice(h, csrVals, unique, nnz, cooVals, type, perm, segPtr);
 *             spgpuCsrToHellValuesDevice(h, cM, hackOffsets, 32, rows, rowPtr, csrVals, base, type, NULL);
 *             spgpuDhellspmv(...);
 *
 * The assembled CSR arrays are also what the sparse product of ext/spgemm_device.h takes on either side (its B wants ascending
 * columns): a Galerkin operator P^T * A * P follows the assembly, and its values-only pass this one's, without leaving HBM.
 * Two separately assembled matrices -- a mass and a stiffness matrix -- are added as M + dt * K by ext/add_device.h.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCooAssemblePlanDevice. */
size_t spgpuCooAssembleWorkBytes(int rowsCount, int columnsCount, int nonZerosCount);

/* NEW (no counterpart in the reference).  Analysis, once per pattern.  Synchronises the stream (returns a host scalar).
 * csrRowPtr[rowsCount + 1] in csrBaseIndex; perm[nonZerosCount]: sorted position -> COO entry; segPtr[nonZerosCount + 1], of
 * which the first *uniqueCount + 1 are written. */
spgpuStatus_t spgpuCooAssemblePlanDevice(spgpuHandle_t handle, __host int* uniqueCount, __device int* csrRowPtr,
                                         __device int* perm, __device int* segPtr, int rowsCount, int columnsCount,
                                         int nonZerosCount, const __device int* cooRowIndices,
                                         const __device int* cooColsIndices, int cooBaseIndex, int csrBaseIndex,
                                         __device void* work);

/* NEW (no counterpart in the reference).  Pattern + values: csrColIndices[uniqueCount], csrValues[uniqueCount]. */
spgpuStatus_t spgpuCooAssembleDevice(spgpuHandle_t handle, __device int* csrColIndices, __device void* csrValues,
                                     int uniqueCount, int nonZerosCount, const __device int* cooColsIndices,
                                     const __device void* cooValues, int cooBaseIndex, int csrBaseIndex,
                                     spgpuType_t valuesType, const __device int* perm, const __device int* segPtr);

/* NEW (no counterpart in the reference).  Values only: what runs at every time step. */
spgpuStatus_t spgpuCooAssembleValuesDevice(spgpuHandle_t handle, __device void* csrValues, int uniqueCount,
                                           int nonZerosCount, const __device void* cooValues, spgpuType_t valuesType,
                                           const __device int* perm, const __device int* segPtr);

#ifdef __cplusplus
}
#endif
