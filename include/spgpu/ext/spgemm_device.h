#pragma once
/*
 * The sparse matrix product C = A * B on CSR arrays, built on the device (the reference has no sparse x sparse, and neither had
 * this library).
 *
 * NEW: the Galerkin coarse operator A_c = P^T * A * P of an algebraic multigrid set-up without a round trip through the host.
 * A comes out of the assembly (spgpu/ext/assemble_device.h) in CSR with ascending columns, P^T out of spgpuHellTransposeDevice
 * and spgpuHellToCsrDevice (spgpu/ext/transpose_device.h, spgpu/ext/to_csr_device.h) with ascending columns, and
 * spgpuCsrToHellDevice (spgpu/ext/csr_device.h) turns the result into something the SpMV runs on.  The product is an ANALYSIS of
 * the pattern, once (spgpuCsrSpgemmProductsDevice, spgpuCsrSpgemmPlanDevice: expand, one radix sort of rocPRIM, compress), and a
 * pass over the values at every step (spgpuCsrSpgemmValuesDevice), which can sit in a captured graph beside
 * spgpuCooAssembleValuesDevice and spgpuCsrToHellValuesDevice.
 *
 * All three matrices are CSR with int indices and ONE common baseIndex (0 or 1), so a chain (P^T * A) * P needs no conversion.
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.  The Products and the
 * Plan call each return a host scalar and therefore synchronise that stream, once; the two fills are asynchronous, allocate
 * nothing, keep no state and never synchronise; spgpuCsrSpgemmValuesDevice needs no scratch either and can be captured into a
 * HIP graph.
 *
 * THE CONTRACT
 * Inputs
 *   - the rows of A may list their columns in any order and may list a column more than once: each stored entry is one term;
 *   - the rows of B have strictly ascending columns (the assembly and the transpose -> to-CSR route both produce that).
 * Pattern
 *   - the pattern of C is symbolic: (i, j) is an entry of C if some stored a(i,k) and some stored b(k,j) exist.  The columns of
 *     a row are ascending and duplicate-free.  An entry whose terms cancel stays, with the value the sum gives;
 *   - cRowPtr[i] - baseIndex is the number of entries in rows < i; cRowPtr[aRowsCount] - baseIndex == *cNonZerosCount;
 *   - a row of A without entries, or whose k all name empty rows of B, gives an empty row of C.
 * Values
 *   - c(i,j) = (((0 + p0) + p1) + ...): the p_t are taken over the positions of row i of A in STORAGE ORDER, for those whose row
 *     k of B holds column j;
 *   - p_t = a * b is rounded once in the element type, then added and rounded again: no fused multiply-add joins the product
 *     to the sum;
 *   - complex: re = ar*br - ai*bi, im = ar*bi + ai*br, every multiply and every add / subtract rounded separately; complex
 *     sums are componentwise.  This is NOT the hipCfma expression tree of the SpMV kernels: separately rounded operations are
 *     what numpy can restate exactly (spgpu_amd.formats.csr_spgemm), and the tests compare bytes;
 *   - the sum starts from +0, not from the first product: a lone product -0.0 is therefore stored as +0.0;
 *   - each element has one writer and no atomics are used: the bytes do not depend on scheduling or on which of the library's
 *     two fills ran, and a repeated call gives the same bytes;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED
 *     before a launch.
 * Refusals: SPGPU_UNSUPPORTED, each reported after the call's one synchronise with nothing read or written out of bounds (the
 * offending index is clamped and a flag raised); no output array then has a defined content
 *   - a column of A outside [baseIndex, baseIndex + aColumnsCount)                                   (Products, and Plan again);
 *   - a column of B outside [baseIndex, baseIndex + bColumnsCount)                                   (Plan);
 *   - a row of B that A names and that is not strictly ascending                                      (Plan);
 *   - more than INT_MAX products: *productsCount = -1                                                (Products);
 *   - a productsCount that is not what spgpuCsrSpgemmProductsDevice returns for these matrices         (Plan).
 * Degenerate inputs
 *   - aRowsCount <= 0: SPGPU_SUCCESS with nothing launched, the counts 0;
 *   - productsCount <= 0: the Plan writes cRowPtr (all baseIndex), sets *cNonZerosCount = 0 and succeeds;
 *   - the two fills return SPGPU_SUCCESS before touching the stream for cNonZerosCount <= 0 or aRowsCount <= 0;
 *   - the fills trust their index arrays, as the refill of spgpu/ext/update_device.h trusts csrRowPtr.
 *
 * `work` is caller-provided scratch of spgpuCsrSpgemmWorkBytes(aRowsCount, bColumnsCount, productsCount) bytes, 256-byte aligned
 * (about 20 bytes per product -- two buffers of 64-bit keys and the entry numbers -- plus 8 bytes per row of A plus rocPRIM's
 * share; 0 if no GPU can be asked for that share).  spgpuCsrSpgemmProductsDevice needs only the size for productsCount = 0.  The
 * Plan leaves the columns of C in `work`; spgpuCsrSpgemmDevice copies them out, and once that call has passed on the stream
 * `work` may be freed: spgpuCsrSpgemmValuesDevice never reads it.
 *
 * The coarse operator of a two-grid method, once and then at every step (PT = P^T, all CSR, one base):
 *
 *     (once)  spgpuCsrSpgemmProductsDevice(h, &products, ptRows, ptCols, ptPtr, ptIdx, aPtr, base, small);
 *             spgpuCsrSpgemmPlanDevice(h, &nnzR, rPtr, ptRows, ptCols, aCols, ptPtr, ptIdx, aPtr, aIdx, base, products, work);
 *             spgpuCsrSpgemmDevice(h, rIdx, rVal, nnzR, ptRows, ptPtr, ptIdx, ptVal, aPtr, aIdx, aVal, rPtr, base, type, work);
 *             (the same three calls for A_c = R * P)
 *             spgpuCsrRowLengthsDevice / spgpuHellPlanDevice / spgpuCsrToHellDevice on A_c
 *     (step)  spgpuCsrSpgemmValuesDevice(h, rVal, ptRows, ptPtr, ptIdx, ptVal, aPtr, aIdx, aVal, rPtr, rIdx, base, type);
 *             spgpuCsrSpgemmValuesDevice(h, cVal, ptRows, rPtr, rIdx, rVal, pPtr, pIdx, pVal, cPtr, cIdx, base, type);
 *             spgpuCsrToHellValuesDevice(...);  spgpuDhellspmv(...);
 *
 * The sum of two CSR matrices -- the smoothed prolongator P = T - omega * (A * T) after this product -- is ext/add_device.h.
 * A Gauss-Seidel smoother for the hierarchy these products build is the triangular solve of ext/trsv_device.h.
 * The tentative prolongator T itself -- strength of connection, aggregates, T in CSR -- comes out of ext/aggregate_device.h.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for the calls below; monotone in productsCount. */
size_t spgpuCsrSpgemmWorkBytes(int aRowsCount, int bColumnsCount, int productsCount);

/* NEW (no counterpart in the reference).  How many a(i,k) * b(k,j) terms there are.  Synchronises the stream (returns a host
 * scalar).  aColumnsCount is the number of rows of B: bRowPtr has aColumnsCount + 1 elements. */
spgpuStatus_t spgpuCsrSpgemmProductsDevice(spgpuHandle_t handle, __host int* productsCount, int aRowsCount, int aColumnsCount,
                                           const __device int* aRowPtr, const __device int* aColIndices,
                                           const __device int* bRowPtr, int baseIndex, __device void* work);

/* NEW (no counterpart in the reference).  Pattern analysis, once per pattern.  Synchronises the stream (returns a host scalar).
 * Writes cRowPtr[aRowsCount + 1] and leaves the columns of C in `work`. */
spgpuStatus_t spgpuCsrSpgemmPlanDevice(spgpuHandle_t handle, __host int* cNonZerosCount, __device int* cRowPtr, int aRowsCount,
                                       int aColumnsCount, int bColumnsCount, const __device int* aRowPtr,
                                       const __device int* aColIndices, const __device int* bRowPtr,
                                       const __device int* bColIndices, int baseIndex, int productsCount, __device void* work);

/* NEW (no counterpart in the reference).  Columns (copied out of `work`) and values: cColIndices[cNonZerosCount],
 * cValues[cNonZerosCount].  Asynchronous. */
spgpuStatus_t spgpuCsrSpgemmDevice(spgpuHandle_t handle, __device int* cColIndices, __device void* cValues, int cNonZerosCount,
                                   int aRowsCount, const __device int* aRowPtr, const __device int* aColIndices,
                                   const __device void* aValues, const __device int* bRowPtr, const __device int* bColIndices,
                                   const __device void* bValues, const __device int* cRowPtr, int baseIndex,
                                   spgpuType_t valuesType, const __device void* work);

/* NEW (no counterpart in the reference).  Values only: what runs at every step.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrSpgemmValuesDevice(spgpuHandle_t handle, __device void* cValues, int aRowsCount,
                                         const __device int* aRowPtr, const __device int* aColIndices,
                                         const __device void* aValues, const __device int* bRowPtr,
                                         const __device int* bColIndices, const __device void* bValues,
                                         const __device int* cRowPtr, const __device int* cColIndices, int baseIndex,
                                         spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
