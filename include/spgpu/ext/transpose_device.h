#pragma once
/*
 * The transpose of a stored HELL or ELL matrix, built on the device as an ordinary HELL matrix (no counterpart in the
 * reference, whose users leave the GPU for trans = 'T').
 *
 * NEW: every product of the library is A*x.  These calls build the HELL arrays of A^T ONCE, entirely in HBM, and every path
 * the library has then works on A^T unchanged and reproducibly: spgpu?hellspmv with plan / freeze / adopt / hold,
 * spgpu?hellspmm, spgpu?hellspmmMv, spgpu?hellspmvDotDevice, spgpuHellDiag, the ordered calls.  There is NO transposed SpMV
 * call: it would scatter into z with floating-point atomics, and its results would change from run to run.
 *
 * All array arguments are DEVICE pointers unless marked host.  The calls run on handle->currentStream and allocate nothing;
 * only `work` and the named destinations are written.  The two "lengths" calls return host scalars and therefore synchronise
 * that stream, like spgpuCooRowLengthsDevice.
 *
 * THE SOURCE is read as it is stored: cM / rP (or the ELL values / indices), hackOffsets, rS, rIdx and baseIndex mean what they
 * mean in spgpu?hellspmv / spgpu?ellspmv.  Storage row r holds matrix row i = rIdx[r] (0-based) when rIdx != NULL, i = r
 * otherwise; its entries are the slots k = 0 .. rS[r]-1.  rS is required.  `slots` is the number of stored slots of the source
 * (HELL: hackSize * allocationHeight; ELL: ellIndicesPitch * maxRowSize): it sizes `work`, and a row whose last slot would lie
 * beyond it is refused.
 *
 * THE CONTRACT
 *   - entry order: the k-th stored entry of row j of A^T is the k-th entry of column j of A, the entries of A taken by
 *     ascending matrix row i and within a row by ascending slot (of several storage rows with one rIdx value, by ascending
 *     storage row);
 *   - the arrays are, byte for byte, what computeEllRowLenghts -> cooToEll -> computeHellAllocSize -> ellToHell give for the COO
 *     listing of A^T in that order (and so what the COO route of spgpu/convert_device.h gives), for any tHackSize -- multiples
 *     of 32 or not; destination arrays are zeroed by the caller, slots beyond a row's end are not written;
 *   - a column index of the result is i + tBaseIndex; duplicates are kept;
 *   - values are moved as 4-, 8- or 16-byte words (spgpuSizeOf(valuesType)), never as numbers: NaN payloads survive, all four
 *     types work, and this is the plain transpose, not the conjugate one.  Any other element size returns SPGPU_UNSUPPORTED;
 *   - padding: slots with k >= rS[r] are never read, neither as an index nor as a value;
 *   - determinism: one sort key per stored entry, a stable radix sort, row starts by binary search, a destination position =
 *     sorted position - column start.  No floating-point atomics, no order left to the hardware: the arrays do not depend on
 *     scheduling;
 *   - rowsCount <= 0 or columnsCount <= 0 returns SPGPU_SUCCESS before anything is launched, the lengths calls then return 0
 *     and 0; a matrix without entries writes only tLengths (zeros);
 *   - SPGPU_UNSUPPORTED from a lengths call -- an rIdx[r] outside [0, rowsCount), an rS[r] that is negative or reaches beyond
 *     `slots`, a stored column index outside [baseIndex, baseIndex + columnsCount) -- is reported and never dereferenced
 *     further: nothing but `work` has been written, and a fill call on that `work` writes nothing.
 *
 * `work` is caller-provided scratch of spgpuHellTransposeWorkBytes bytes, 256-byte aligned; the lengths call leaves in it what
 * the fill needs.  Its head has the layout spgpuHellPlanDevice uses for columnsCount rows, so the SAME `work` is passed to that
 * call in between, as in the COO route.  Cost: 24 bytes per source slot (two buffers of 64-bit keys, two of source slots) plus
 * rocPRIM's temporary storage, plus 8 bytes per row and per column.
 *
 * The key is (column << rowBits) | i in 64 bits.  With rIdx the sort runs over all of its bits; without, the entries are
 * already emitted by ascending i and the stable sort runs over the column bits only -- as many radix passes as the COO route.
 *
 * A^T of a HELL matrix, then z = beta*y + alpha*A^T*x:
 *
 *     work = malloc(spgpuHellTransposeWorkBytes(rows, cols, slots));
 *     spgpuHellTransposeLengthsDevice(h, tLengths, &longest, &nnz, rP, hackSize, hackOffsets, rS, rIdx, rows, cols, base, slots, work);
 *     spgpuHellPlanDevice(h, &tHeight, tHackOffsets, 32, cols, tLengths, work);
 *     (allocate and zero tValues, tIndices: 32 * tHeight slots)
 *     spgpuHellTransposeDevice(h, tValues, tIndices, tHackOffsets, 32, base, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, cols,
 *                              base, slots, type, tLengths, work);
 *     spgpuDhellspmv(h, z, y, alpha, tValues, tIndices, 32, tHackOffsets, tLengths, NULL, longest, cols, x, beta, base);
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of scratch the calls below need for a source of `slots` stored slots (0 if no GPU can be asked for rocPRIM's share,
 * as spgpuCooConvertWorkBytes). */
size_t spgpuHellTransposeWorkBytes(int rowsCount, int columnsCount, int slots);

/* Fills tLengths[columnsCount], the row lengths of A^T, on the device; returns the longest of them and the number of stored
 * entries on the host (synchronises the stream).  Leaves in `work` what spgpuHellTransposeDevice needs. */
spgpuStatus_t spgpuHellTransposeLengthsDevice(spgpuHandle_t handle, __device int* tLengths, __host int* maxRowSize,
                                              __host int* nonZerosCount, const __device int* rP, int hackSize,
                                              const __device int* hackOffsets, const __device int* rS,
                                              const __device int* rIdx, int rowsCount, int columnsCount, int baseIndex,
                                              int slots, __device void* work);

/* Fills the HELL arrays of A^T (columnsCount rows, rowsCount columns).  tHackOffsets from spgpuHellPlanDevice on tLengths with
 * columnsCount rows; `work` as left by spgpuHellTransposeLengthsDevice for the same source. */
spgpuStatus_t spgpuHellTransposeDevice(spgpuHandle_t handle, __device void* tValues, __device int* tIndices,
                                       const __device int* tHackOffsets, int tHackSize, int tBaseIndex,
                                       const __device void* cM, const __device int* rP, int hackSize,
                                       const __device int* hackOffsets, const __device int* rS, const __device int* rIdx,
                                       int rowsCount, int columnsCount, int baseIndex, int slots, spgpuType_t valuesType,
                                       const __device int* tLengths, __device void* work);

/* The same with an ELL source (slot k of storage row r at r + k * pitch); the destination is HELL. */
spgpuStatus_t spgpuEllTransposeLengthsDevice(spgpuHandle_t handle, __device int* tLengths, __host int* maxRowSize,
                                             __host int* nonZerosCount, const __device int* rP, int ellIndicesPitch,
                                             const __device int* rS, const __device int* rIdx, int rowsCount,
                                             int columnsCount, int baseIndex, int slots, __device void* work);

spgpuStatus_t spgpuEllTransposeDevice(spgpuHandle_t handle, __device void* tValues, __device int* tIndices,
                                      const __device int* tHackOffsets, int tHackSize, int tBaseIndex,
                                      const __device void* cM, const __device int* rP, int ellValuesPitch,
                                      int ellIndicesPitch, const __device int* rS, const __device int* rIdx,
                                      int rowsCount, int columnsCount, int baseIndex, int slots, spgpuType_t valuesType,
                                      const __device int* tLengths, __device void* work);

#ifdef __cplusplus
}
#endif
