#pragma once
/*
 * The incomplete factorisation ILU(0) of a CSR matrix, A ~ L * U in A's own pattern, level-scheduled on the device (the reference
 * factorises nothing, and neither did this library).
 *
 * NEW: the producer of the factor that spgpu/ext/trsv_device.h was built to apply.  The result lies in A's pattern -- unit L strictly
 * below the diagonal, U on and above it -- which is the layout the triangular solve reads from one array with two plans.  The
 * factorisation is an ANALYSIS of the pattern, once (spgpuCsrIlu0PlanDevice), and a pass over the values at every new set of
 * coefficients (spgpuCsrIlu0Device), which can sit in a captured graph in front of the two solves.
 * The number of levels belongs to the row order: spgpu/ext/colour_device.h reorders a matrix so that it has about as many as colours.
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.
 *
 * THE CONTRACT
 * Matrix
 *   - one square CSR matrix of rowsCount rows with int indices and baseIndex 0 or 1;
 *   - every row has strictly ascending columns, which is what spgpu/ext/assemble_device.h, spgemm_device.h, add_device.h and the
 *     transpose followed by to_csr_device.h all emit;
 *   - every row stores its diagonal.
 * Plan
 *   - runs once per pattern and synchronises the stream (it returns host data);
 *   - writes rowOrder[rowsCount], the first *levelsCount + 1 ints of levelPtr and of levelPtrHost, and *levelsCount: byte for byte
 *     what spgpuCsrTrsvPlanDevice(..., SPGPU_TRSV_LOWER, SPGPU_TRSV_DIAG_STORED, ...) writes -- it is that call.  Row i depends on
 *     the rows k < i with (i, k) stored, so the levels of the lower solve are the levels of the factorisation;
 *   - the same arrays then serve spgpuCsrTrsvDevice with SPGPU_TRSV_LOWER and SPGPU_TRSV_DIAG_UNIT for the L solve: the levels of
 *     a triangle do not depend on how its diagonal is treated.  The U solve needs a trsv plan of its own (SPGPU_TRSV_UPPER,
 *     SPGPU_TRSV_DIAG_STORED);
 *   - THE EXTRA SLOT: levelPtrHost[*levelsCount + 1] receives the number of stored entries, rowPtr[rowsCount] - baseIndex, so
 *     levelPtrHost holds rowsCount + 2 ints (levelPtr rowsCount + 1).  spgpuCsrIlu0Device reads the slot on the host, without a
 *     synchronise, to choose its kernel shape from the mean row length; the slot changes the speed, never the bytes.  Nothing
 *     else is touched beyond the first *levelsCount + 1 ints of either level array;
 *   - writes diagPos[i], i < rowsCount: the 0-based position in colIndices of entry (i, i);
 *   - `work` is caller-provided scratch of spgpuCsrIlu0WorkBytes(rowsCount) bytes, 256-byte aligned -- about 16 bytes per row.  Only
 *     the Plan uses it; once the Plan has returned, `work` may be freed.
 * Refusals: SPGPU_UNSUPPORTED from the Plan with *levelsCount = 0, each reported after its synchronise with nothing read or
 * written out of bounds; rowOrder, diagPos and the level arrays then have no defined content
 *   - a column outside [baseIndex, baseIndex + rowsCount);
 *   - a row that does not ascend strictly (it descends, or repeats a column);
 *   - a missing diagonal.
 * Values
 *   - lu starts as a copy of a.  Row i is then processed as follows: take the stored entries (i, k) with k < i in ascending k.
 *     For each one, first lu_ik = lu_ik / lu_kk with one correctly rounded division.  Then take every stored entry (k, j) of row k
 *     with j > k, in ascending j: if row i stores (i, j), lu_ij = lu_ij - (lu_ik * lu_kj), the product rounded, then the
 *     difference; no fused multiply-add joins them.  If row i does not store (i, j), the term is dropped: there is no fill;
 *   - row k is final when row i reads it, because level(k) < level(i);
 *   - the result is unit L strictly below the diagonal (the ones are not stored) and U on and above it;
 *   - a row without lower entries moves its bits, -0.0 included;
 *   - a zero pivot is not looked for: IEEE division decides.  Nothing is pivoted or shifted;
 *   - complex, word for word as in spgpu/ext/trsv_device.h: the product a * x is re = ar*xr - ai*xi, im = ar*xi + ai*xr, every
 *     multiply and the add / subtract rounded separately -- six operations; the difference is componentwise.  The quotient n / d is
 *     den = (dr*dr) + (di*di), re = ((nr*dr) + (ni*di)) / den, im = ((ni*dr) - (nr*di)) / den, every operation rounded separately.
 *     This form is NOT safe against overflow (or underflow) of den.  For the complex types this restatement is the law;
 *   - every stored entry has one writer; its updates come in ascending k, and each k touches it at most once; no atomics are used.
 *     So the bytes do not depend on scheduling, on the kernel shape or on the grid, a repeated call gives the same bytes, and numpy
 *     can restate the result (spgpu_amd.formats.csr_ilu0): the tests compare bytes;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED
 *     before a launch;
 *   - luValues == aValues exactly (in place) is allowed; any other overlap is not.  Out of place, aValues is left untouched.
 * Degenerate inputs
 *   - rowsCount <= 0: the Plan returns SPGPU_SUCCESS with nothing launched, *levelsCount = 0;
 *   - spgpuCsrIlu0Device returns SPGPU_SUCCESS before touching the stream for rowsCount <= 0 or levelsCount <= 0;
 *   - the factor call trusts its index arrays: it is meant for a matrix and a plan that the Plan accepted.
 * State
 *   - the Plan synchronises once for its own checks and then as often as spgpuCsrTrsvPlanDevice does (about once per level);
 *   - the factor call never synchronises, allocates nothing and keeps no state.  It reads levelPtrHost at call time, which is also
 *     capture time: its launches can be captured into a HIP graph and replayed after aValues changed in place;
 *   - no kernel waits for another workgroup: levels are ordered by stream order between launches and by __syncthreads() inside
 *     one workgroup, nothing else.
 *
 * A preconditioner M = L * U, once per pattern, once per set of coefficients and then at every application (A in CSR):
 *
 *     (pattern) spgpuCsrIlu0PlanDevice(h, &levels, order, lvlPtr, lvlPtrHost, diagPos, rows, aPtr, aIdx, base, work);
 *               spgpuCsrTrsvPlanDevice(h, &uLevels, uOrder, uLvlPtr, uLvlPtrHost, rows, aPtr, aIdx, base, SPGPU_TRSV_UPPER,
 *                                      SPGPU_TRSV_DIAG_STORED, trsvWork);
 *     (values)  spgpuCsrIlu0Device(h, lu, aVal, rows, levels, order, lvlPtr, lvlPtrHost, diagPos, aPtr, aIdx, base, SPGPU_TYPE_DOUBLE);
 *     (apply)   spgpuCsrTrsvDevice(h, y, b, rows, levels, order, lvlPtr, lvlPtrHost, aPtr, aIdx, lu, base, SPGPU_TRSV_LOWER,
 *                                  SPGPU_TRSV_DIAG_UNIT, SPGPU_TYPE_DOUBLE);
 *               spgpuCsrTrsvDevice(h, x, y, rows, uLevels, uOrder, uLvlPtr, uLvlPtrHost, aPtr, aIdx, lu, base, SPGPU_TRSV_UPPER,
 *                                  SPGPU_TRSV_DIAG_STORED, SPGPU_TYPE_DOUBLE);
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrIlu0PlanDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrIlu0WorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  Pattern analysis, once per pattern.  Synchronises the stream (returns host data).  Writes
 * rowOrder[rowsCount], diagPos[rowsCount], the first *levelsCount + 1 ints of levelPtr and the first *levelsCount + 2 ints of
 * levelPtrHost (rowsCount + 1 and rowsCount + 2 ints hold every case). */
spgpuStatus_t spgpuCsrIlu0PlanDevice(spgpuHandle_t handle, __host int* levelsCount, __device int* rowOrder, __device int* levelPtr,
                                     __host int* levelPtrHost, __device int* diagPos, int rowsCount, const __device int* rowPtr,
                                     const __device int* colIndices, int baseIndex, __device void* work);

/* NEW (no counterpart in the reference).  lu = ILU(0) of a.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrIlu0Device(spgpuHandle_t handle, __device void* luValues, const __device void* aValues, int rowsCount,
                                 int levelsCount, const __device int* rowOrder, const __device int* levelPtr,
                                 const __host int* levelPtrHost, const __device int* diagPos, const __device int* rowPtr,
                                 const __device int* colIndices, int baseIndex, spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
