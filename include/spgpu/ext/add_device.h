#pragma once
/*
 * The sparse matrix sum C = alpha * A + beta * B on CSR arrays, built on the device (the reference adds no two sparse matrices,
 * and neither did this library).
 *
 * NEW: M + dt * K of a time stepper or J = M - theta * dt * K of a Newton solver at every step, the smoothed prolongator
 * P = T - omega * (A * T) of an algebraic multigrid set-up, the symmetrised pattern A + A^T, a shifted system A - sigma * B -- all
 * without a round trip through the host.  A and B come out of the assembly (spgpu/ext/assemble_device.h), of the way back to CSR
 * (spgpu/ext/to_csr_device.h, after spgpu/ext/transpose_device.h for A^T) or of the product (spgpu/ext/spgemm_device.h), all of
 * which give ascending columns, and spgpuCsrToHellDevice (spgpu/ext/csr_device.h) turns the result into something the SpMV runs
 * on.  The sum is an ANALYSIS of the pattern, once (spgpuCsrAddPlanDevice: the length of every row's union, counted by merging,
 * and a scan; no sort), and a pass over the values at every step (spgpuCsrAddValuesDevice), which can sit in a captured graph
 * beside spgpuCooAssembleValuesDevice, spgpuCsrSpgemmValuesDevice and spgpuCsrToHellValuesDevice.
 *
 * All three matrices are CSR with int indices and ONE common baseIndex (0 or 1); A and B are both rowsCount x columnsCount.
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.  The Plan returns a host
 * scalar and therefore synchronises that stream, once; the fills are asynchronous, take no scratch, allocate nothing, keep no
 * state and never synchronise, and the values-only calls can be captured into a HIP graph.
 *
 * THE CONTRACT
 * Inputs
 *   - every row of A and every row of B has strictly ascending columns; an empty row is fine on either side or on both.
 * Pattern
 *   - the pattern of C is symbolic: (i, j) is an entry of C if A or B stores it.  The columns of a row are ascending and
 *     duplicate-free.  An entry whose two terms cancel stays, with the value the sum gives;
 *   - cRowPtr[i] - baseIndex is the number of entries in rows < i; cRowPtr[rowsCount] - baseIndex == *cNonZerosCount.
 * Values
 *   - alpha and beta each point to ONE element of valuesType.  The host forms read them at call time; the device form
 *     (spgpuCsrAddValuesDeviceScalars) reads them in the kernel, so a captured graph follows a dt that another kernel writes;
 *   - where both matrices store the entry: c = (alpha * a) + (beta * b), each product rounded once in the element type, then the
 *     sum rounded: no fused multiply-add joins a product to the sum;
 *   - where only A stores the entry: c = alpha * a, the product alone and not + 0; where only B stores it: c = beta * b;
 *   - complex: a product s * v is re = sr*vr - si*vi, im = sr*vi + si*vr, every multiply and the add / subtract rounded
 *     separately -- six operations; the complex sum is componentwise.  This is NOT the hipCfma expression tree of the SpMV
 *     kernels: separately rounded operations are what numpy can restate exactly (spgpu_amd.formats.csr_add), and the tests
 *     compare bytes;
 *   - real types: alpha = 1 therefore stores a lone finite a with its own bits, -0.0 included.  For the complex types the
 *     restatement above is the law, and no moved bits are promised (1 * (-0.0 + 0i) has the imaginary part (1 * 0) + (0 * -0.0));
 *   - each element has one writer and no atomics are used: the bytes do not depend on scheduling or on which of the library's
 *     two fills ran, and a repeated call gives the same bytes;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED
 *     before a launch;
 *   - outputs must not overlap inputs.
 * Refusals: SPGPU_UNSUPPORTED from the Plan, each reported after its one synchronise with nothing read or written out of bounds
 * (the Plan compares columns and never uses one as an index; an offending index is clamped and a flag raised); cRowPtr then
 * has no defined content
 *   - a column of A or of B outside [baseIndex, baseIndex + columnsCount):                   *cNonZerosCount = 0;
 *   - a row of A or of B that does not ascend strictly (it descends or repeats a column):   *cNonZerosCount = 0;
 *   - more than INT_MAX entries in the union: the Plan adds the row counts into a 64-bit total, which decides -- the int scan
 *     does not:                                                                              *cNonZerosCount = -1.
 * Degenerate inputs
 *   - rowsCount <= 0: SPGPU_SUCCESS with nothing launched, *cNonZerosCount = 0;
 *   - spgpuCsrAddDevice returns SPGPU_SUCCESS before touching the stream for rowsCount <= 0 or cNonZerosCount <= 0;
 *   - the values-only calls do not know the count: they return before touching the stream for rowsCount <= 0 and otherwise
 *     read the count on the device, from the row pointers;
 *   - the fills trust their index arrays, as the fills of spgpu/ext/spgemm_device.h do: they are meant for matrices and a
 *     cRowPtr that the Plan accepted.
 *
 * `work` is caller-provided scratch of spgpuCsrAddWorkBytes(rowsCount) bytes, 256-byte aligned: the scan's tile totals, the
 * 64-bit count and the flag word -- about 4 bytes per 1024 rows.  Only the Plan uses it; once the Plan has returned, `work`
 * may be freed: no fill ever reads it.  Neither fill reads the columns of C either: entry e of A's row i lands at
 * cRowPtr[i] + (e - aRowPtr[i]) + (the number of columns of B's row i below its own that A's row does not hold), and an entry of
 * B that A does not hold likewise; that is why spgpuCsrAddValuesDevice takes no cColIndices.  Both numbers come from the two
 * input rows alone; finding them walks both rows up to the entry, so a row of many thousands of entries costs its length squared.
 *
 * M + dt * K, once and then at every step (all CSR, one base):
 *
 *     (once)  spgpuCsrAddPlanDevice(h, &nnzC, cPtr, rows, cols, mPtr, mIdx, kPtr, kIdx, base, work);
 *             spgpuCsrAddDevice(h, cIdx, cVal, nnzC, rows, &one, mPtr, mIdx, mVal, &dt, kPtr, kIdx, kVal, cPtr, base, type);
 *             spgpuCsrRowLengthsDevice / spgpuHellPlanDevice / spgpuCsrToHellDevice on C
 *     (step)  spgpuCsrAddValuesDevice(h, cVal, rows, &one, mPtr, mIdx, mVal, &dt, kPtr, kIdx, kVal, cPtr, base, type);
 *             spgpuCsrToHellValuesDevice(...);  spgpuDhellspmv(...);
 *
 * Solving with a triangle of the CSR matrix this builds -- a Gauss-Seidel sweep on M + dt * K -- is ext/trsv_device.h.
 * The tentative prolongator T of P = T - omega * (A * T) comes out of ext/aggregate_device.h.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrAddPlanDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrAddWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  Pattern analysis, once per pair of patterns.  Synchronises the stream (returns a host
 * scalar).  Writes cRowPtr[rowsCount + 1]. */
spgpuStatus_t spgpuCsrAddPlanDevice(spgpuHandle_t handle, __host int* cNonZerosCount, __device int* cRowPtr, int rowsCount,
                                    int columnsCount, const __device int* aRowPtr, const __device int* aColIndices,
                                    const __device int* bRowPtr, const __device int* bColIndices, int baseIndex,
                                    __device void* work);

/* NEW (no counterpart in the reference).  Columns and values: cColIndices[cNonZerosCount], cValues[cNonZerosCount].
 * Asynchronous, no scratch. */
spgpuStatus_t spgpuCsrAddDevice(spgpuHandle_t handle, __device int* cColIndices, __device void* cValues, int cNonZerosCount,
                                int rowsCount, const __host void* alpha, const __device int* aRowPtr,
                                const __device int* aColIndices, const __device void* aValues, const __host void* beta,
                                const __device int* bRowPtr, const __device int* bColIndices, const __device void* bValues,
                                const __device int* cRowPtr, int baseIndex, spgpuType_t valuesType);

/* NEW (no counterpart in the reference).  Values only: what runs at every step.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrAddValuesDevice(spgpuHandle_t handle, __device void* cValues, int rowsCount, const __host void* alpha,
                                      const __device int* aRowPtr, const __device int* aColIndices,
                                      const __device void* aValues, const __host void* beta, const __device int* bRowPtr,
                                      const __device int* bColIndices, const __device void* bValues,
                                      const __device int* cRowPtr, int baseIndex, spgpuType_t valuesType);

/* NEW (no counterpart in the reference).  The same with alpha and beta in device memory, read by the kernel when it runs. */
spgpuStatus_t spgpuCsrAddValuesDeviceScalars(spgpuHandle_t handle, __device void* cValues, int rowsCount,
                                             const __device void* alpha, const __device int* aRowPtr,
                                             const __device int* aColIndices, const __device void* aValues,
                                             const __device void* beta, const __device int* bRowPtr,
                                             const __device int* bColIndices, const __device void* bValues,
                                             const __device int* cRowPtr, int baseIndex, spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
