#pragma once
/*
 * The sparse triangular solve x = T^-1 * b on CSR arrays, level-scheduled on the device (the reference solves no triangular
 * system, and neither did this library).
 *
 * NEW: Gauss-Seidel and SSOR applied to a zero initial guess, that is, as a preconditioner that is stronger than the diagonal of
 * spgpu/ext/precond.h, on the matrices that spgpu/ext/spgemm_device.h and spgpu/ext/add_device.h build, and the application half
 * of every ILU(0) or IC(0), wherever the factor came from (ext/ilu0_device.h makes the ILU(0)).  The solve computes T^-1 * b and
 * nothing else: a sweep with a guess, x <- (D + L)^-1 * (b - U * x), as a smoother needs it, is spgpu/ext/sweep_device.h.  T is one
 * triangle of a matrix A that is given WHOLE: (D + L)^-1 and (D + U)^-1 come from A's own arrays, and an ILU(0) stored in A's
 * pattern (unit L below, U on and above the diagonal) is solved from one array with two plans.  The solve is an ANALYSIS of the
 * dependencies, once (spgpuCsrTrsvPlanDevice: the level of every row, the rows listed level by level), and a pass over the
 * values at every application (spgpuCsrTrsvDevice), which can sit in a captured graph.
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.
 *
 * THE CONTRACT
 * Matrix
 *   - one square CSR matrix of rowsCount rows with int indices and baseIndex 0 or 1, holding the whole of A;
 *   - side says which triangle the solve uses: SPGPU_TRSV_LOWER the entries with column < row, SPGPU_TRSV_UPPER those with
 *     column > row.  Stored entries on the other side are never read as values and never count as dependencies;
 *   - the columns of a row need not ascend;
 *   - diag = SPGPU_TRSV_DIAG_UNIT: the diagonal of T is 1 and a stored diagonal is never read.  SPGPU_TRSV_DIAG_STORED: every
 *     row must store its diagonal exactly once.
 * Levels
 *   - level(i) = 0 if row i stores no off-diagonal entry on `side`; otherwise 1 + the largest level(j) over those entries (i, j).
 *     This is symbolic: a stored zero is a dependency;
 *   - rowOrder lists the rows by (level, row index) ascending; it holds 0-based row numbers whatever baseIndex is;
 *   - levelPtr[l] is the number of rows in levels < l, 0-based; levelPtr[*levelsCount] == rowsCount;
 *   - levelPtrHost holds the same first *levelsCount + 1 ints on the host.  Neither level array is touched beyond that;
 *   - all of this is unique, so it is comparable byte for byte (spgpu_amd.formats.csr_trsv_plan restates it).
 * Values
 *   - row i starts with acc = b_i.  For each stored off-diagonal entry (i, j) on `side`, in storage order:
 *     acc = acc - (a_ij * x_j), the product rounded, then the difference; no fused multiply-add joins them;
 *   - then x_i = acc / a_ii with one correctly rounded division, or x_i = acc for SPGPU_TRSV_DIAG_UNIT.  A UNIT row without
 *     dependencies therefore moves b_i's bits, -0.0 included;
 *   - a zero pivot is not looked for: IEEE division decides;
 *   - complex: the product a * x is re = ar*xr - ai*xi, im = ar*xi + ai*xr, every multiply and the add / subtract rounded
 *     separately -- six operations, as in spgpu/ext/spgemm_device.h; the difference is componentwise.  The quotient n / d is
 *     den = (dr*dr) + (di*di), re = ((nr*dr) + (ni*di)) / den, im = ((ni*dr) - (nr*di)) / den, every operation rounded separately.
 *     This form is NOT safe against overflow (or underflow) of den: a pivot beyond the square root of the type's range gives
 *     inf or 0 where a scaled algorithm would not.  For the complex types this restatement is the law;
 *   - each row is summed by one thread, so numpy can restate the result (spgpu_amd.formats.csr_trsv) and the tests compare bytes;
 *   - each element has one writer and no atomics are used: the bytes do not depend on scheduling or on which of the library's
 *     two solves ran, and a repeated call gives the same bytes;
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED
 *     before a launch, as does a side or diag that is none of the above;
 *   - x == b exactly (in place) is allowed; any other overlap is not.
 * Refusals: SPGPU_UNSUPPORTED from the Plan with *levelsCount = 0, each reported after its synchronise with nothing read or
 * written out of bounds (an offending column is clamped -- it is no dependency -- and a flag raised); rowOrder and the level
 * arrays then have no defined content
 *   - a column outside [baseIndex, baseIndex + rowsCount), on either side of the diagonal;
 *   - a missing diagonal under SPGPU_TRSV_DIAG_STORED;
 *   - a diagonal stored twice under SPGPU_TRSV_DIAG_STORED.
 * Degenerate inputs
 *   - rowsCount <= 0: SPGPU_SUCCESS with nothing launched, *levelsCount = 0;
 *   - spgpuCsrTrsvDevice returns SPGPU_SUCCESS before touching the stream for rowsCount <= 0 or levelsCount <= 0;
 *   - the solve trusts its index arrays: it is meant for a matrix and a plan that the Plan accepted.
 * State
 *   - the Plan returns host data and therefore synchronises the stream -- once per sweep of its analysis, so about once per
 *     level: it is set-up code, and on a matrix of many thousands of levels (a bidiagonal one has rowsCount of them) it takes
 *     that many round trips;
 *   - the number of levels belongs to the row order: spgpu/ext/colour_device.h reorders a matrix so that it has about as many as colours;
 *   - the solve never synchronises, allocates nothing and keeps no state.  It reads levelPtrHost at call time, which is also
 *     capture time: its launches can be captured into a HIP graph and replayed after b and values changed in place;
 *   - no kernel of the Plan or of the solve waits for another workgroup: levels are ordered by stream order between launches
 *     and by barriers inside one workgroup, nothing else.
 *
 * `work` is caller-provided scratch of spgpuCsrTrsvWorkBytes(rowsCount) bytes, 256-byte aligned -- about 16 bytes per row.  Only
 * the Plan uses it; once the Plan has returned, `work` may be freed: the solve never reads it.
 *
 * A forward Gauss-Seidel sweep x = (D + L)^-1 * b, once and then at every application (A in CSR):
 *
 *     (once)   spgpuCsrTrsvPlanDevice(h, &levels, order, lvlPtr, lvlPtrHost, rows, aPtr, aIdx, base, SPGPU_TRSV_LOWER,
 *                                     SPGPU_TRSV_DIAG_STORED, work);
 *     (apply)  spgpuCsrTrsvDevice(h, x, b, rows, levels, order, lvlPtr, lvlPtrHost, aPtr, aIdx, aVal, base, SPGPU_TRSV_LOWER,
 *                                 SPGPU_TRSV_DIAG_STORED, SPGPU_TYPE_DOUBLE);
 */
#include "../core.h"

#define SPGPU_TRSV_LOWER 0
#define SPGPU_TRSV_UPPER 1
#define SPGPU_TRSV_DIAG_STORED 0
#define SPGPU_TRSV_DIAG_UNIT 1

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrTrsvPlanDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrTrsvWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  Dependency analysis, once per pattern, side and diag.  Synchronises the stream (returns
 * host data).  Writes rowOrder[rowsCount] and the first *levelsCount + 1 ints of levelPtr and of levelPtrHost (rowsCount + 1 ints
 * each hold every case). */
spgpuStatus_t spgpuCsrTrsvPlanDevice(spgpuHandle_t handle, __host int* levelsCount, __device int* rowOrder, __device int* levelPtr,
                                     __host int* levelPtrHost, int rowsCount, const __device int* rowPtr,
                                     const __device int* colIndices, int baseIndex, int side, int diag, __device void* work);

/* NEW (no counterpart in the reference).  x = T^-1 * b.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrTrsvDevice(spgpuHandle_t handle, __device void* x, const __device void* b, int rowsCount, int levelsCount,
                                 const __device int* rowOrder, const __device int* levelPtr, const __host int* levelPtrHost,
                                 const __device int* rowPtr, const __device int* colIndices, const __device void* values,
                                 int baseIndex, int side, int diag, spgpuType_t valuesType);

#ifdef __cplusplus
}
#endif
