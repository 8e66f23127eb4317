#pragma once
/*
 * Multicolour Gauss-Seidel / SOR sweeps in place, and the residual r = b - A * x, on CSR arrays in HBM (the reference relaxes
 * nothing and forms no residual on CSR arrays, and neither did this library).
 *
 * NEW: a smoothing step with a non-zero guess, x <- (D + L)^-1 * (b - U * x), which the triangular solve of
 * spgpu/ext/trsv_device.h cannot express (it computes T^-1 * b and nothing else), and the residual that every multigrid cycle and
 * every stopping test needs.  The colouring of spgpu/ext/colour_device.h supplies what a direct sweep needs: rows of one colour do
 * not read each other, so one launch per colour relaxes them in place, on A ITSELF -- no level analysis, no permuted copy, no
 * gather or scatter of a vector.  The 7-point matrix of a 200^3 grid takes 7 launches a sweep where its lower solve takes 598 in
 * the natural order.  With these calls the solve phase of a hierarchy built by spgpu/ext/spgemm_device.h and
 * spgpu/ext/aggregate_device.h runs without leaving HBM.
 *
 * All array arguments are DEVICE pointers unless marked host.  Every call runs on handle->currentStream.
 *
 * THE CONTRACT
 * Matrix
 *   - one square CSR matrix of rowsCount rows with int indices and baseIndex 0 or 1, holding the whole of A;
 *   - the columns of a row need not ascend; every row stores its diagonal exactly once; an off-diagonal column may be stored
 *     twice (it is subtracted twice);
 *   - a colouring in coloursCount colours: colourPtr[coloursCount + 1] as spgpuCsrColourOrderDevice writes it, and `order`, which
 *     has the meaning rIdx has elsewhere in the library;
 *   - order != NULL: the rows of colour c are order[colourPtr[c] .. colourPtr[c + 1]), and the colour of column j is colourOf[j];
 *   - order == NULL: the matrix is already in colour order, for instance B of spgpuCsrPermuteDevice.  The rows of colour c are
 *     colourPtr[c] .. colourPtr[c + 1] themselves, the colour of row or column k is the c with colourPtr[c] <= k < colourPtr[c + 1],
 *     found by bisection on colourPtr, and colourOf is not read and may be null.
 * Plan (spgpuCsrSweepPlanDevice), once per pattern and colouring
 *   - diagPos[i], i < rowsCount, is the position of row i's diagonal entry in colIndices and values: a 0-based entry index whatever
 *     baseIndex is;
 *   - colourPtrHost holds the coloursCount + 1 ints of colourPtr on the host; nothing behind them is touched;
 *   - *entriesCount = rowPtr[rowsCount] - baseIndex;
 *   - all of this is unique, so it is comparable byte for byte (spgpu_amd.formats.csr_sweep_plan restates it);
 *   - the Plan synchronises the stream once (it returns host data), not once per colour, and cannot be captured;
 *   - the Plan trusts `order` to be the permutation that belongs to colourPtr;
 *   - `work` is caller-provided scratch of spgpuCsrSweepWorkBytes(rowsCount) bytes, 256-byte aligned.  Only the Plan uses it; it
 *     may be freed once the Plan has returned.
 * Refusals: SPGPU_UNSUPPORTED from the Plan with *entriesCount = 0, each reported after the synchronise with nothing read or
 * written out of bounds (an offending column is clamped out -- it is compared, never used as an index -- and a flag is raised, as
 * the Plan of spgpu/ext/trsv_device.h does); diagPos and colourPtrHost then have no defined content
 *   - a column outside [baseIndex, baseIndex + rowsCount);
 *   - a row without a stored diagonal, or with its diagonal stored twice;
 *   - a colourOf[i] outside [0, coloursCount) when order != NULL;
 *   - a stored entry (i, j) with j != i whose two nodes have the same colour;
 *   - a colourPtr that does not start at 0, descends somewhere or does not end at rowsCount (the sweep sizes its launches from it).
 *   The fourth refusal is what makes the sweep free of races: row i reads x_j only for stored (i, j), and no row of i's own colour
 *   is among them.  Properness is needed only in the direction of the stored entries.  The colouring of an UNSYMMETRIC pattern may
 *   fail this check: node j may take the colour of a node i that stores no entry (i, j) while (j, i) is stored
 *   (spgpu/ext/colour_device.h explains why).  The remedy is to colour the pattern of A + A^T, which spgpu/ext/add_device.h builds
 *   with the transpose of spgpu/ext/transpose_device.h, and to sweep on A with that colouring.
 * Sweep (spgpuCsrSweepDevice), relaxation in place
 *   - direction: SPGPU_SWEEP_FORWARD visits the colours 0 .. C-1, SPGPU_SWEEP_BACKWARD the colours C-1 .. 0, SPGPU_SWEEP_SYMMETRIC
 *     is forward then backward, 2C colour passes, and gives the bytes of the two calls in that order;
 *   - one colour pass, for every row i of the colour: acc = b_i; for each stored entry e of row i in storage order, except the one
 *     at diagPos[i], acc = acc - (a_e * x[col_e]), the product rounded, then the difference; no fused multiply-add joins them;
 *     g = acc / a_ii with one correctly rounded division;
 *   - omega == NULL (plain Gauss-Seidel): x_i = g.  Otherwise omega is a HOST pointer to one element of the value type:
 *     d = g - x_i, componentwise and rounded, then x_i = x_i + (omega * d), the product rounded, then the sum.  omega = 1 given
 *     explicitly is a different expression tree from omega == NULL and need not give the same bytes;
 *   - a zero pivot is not looked for: IEEE division decides;
 *   - complex: the products a * x and omega * d are re = ar*xr - ai*xi, im = ar*xi + ai*xr, every multiply and the add / subtract
 *     rounded separately -- six operations, as everywhere in this family; differences and sums are componentwise.  The quotient
 *     n / d is den = (dr*dr) + (di*di), re = ((nr*dr) + (ni*di)) / den, im = ((ni*dr) - (nr*di)) / den, every operation rounded
 *     separately, and NOT safe against overflow or underflow of den, as in spgpu/ext/trsv_device.h;
 *   - the Plan has guaranteed that no row of a colour reads another row of that colour, each x_i has one writer per pass and no
 *     atomics are used.  So the bytes of x after a pass do not depend on scheduling, on the row shape, on the grid, on chaining
 *     or on the order of rows inside a colour; a repeated call on the same input gives the same bytes, and numpy can restate them
 *     (spgpu_amd.formats.csr_sweep): the tests compare bytes;
 *   - x may not overlap b.
 * Residual (spgpuCsrResidualDevice), r = b - A * x
 *   - needs no Plan and no colouring;
 *   - r_i starts as b_i; every stored entry of row i, the diagonal included, is subtracted as above, in storage order.  An empty
 *     row gives r_i = b_i, its bits moved;
 *   - r == b exactly (in place) is allowed; r may not overlap x;
 *   - entriesCount only chooses the row shape; entriesCount <= 0 with rows to do still computes every r_i;
 *   - spgpu_amd.formats.csr_residual restates it.
 * Values
 *   - valuesType is SPGPU_TYPE_FLOAT, _DOUBLE, _COMPLEX_FLOAT or _COMPLEX_DOUBLE; anything else returns SPGPU_UNSUPPORTED before a
 *     launch.
 * Row shapes and launches
 *   - both calls have two row shapes that give the same bytes: one thread per row, or a group of 8 or 32 lanes of one wavefront
 *     that loads a row in chunks, rounds one product per lane and runs the contract's chain of differences over them in storage
 *     order.  The calls pick the shape from entriesCount / rowsCount.  The two thresholds of that rule are those of
 *     spgpu/ext/ilu0_device.h and are NOT MEASURED for these kernels;
 *   - a colour of more than 256 rows is a launch of its own; a maximal run of narrower colours is one launch of one workgroup with a
 *     barrier between colours (at most 64 colours a launch).  So on the coarse levels of a hierarchy, where every colour is narrow,
 *     a forward sweep is one launch and a symmetric sweep is two: the backward list is cut by the same rule, on its own.
 * Degenerate inputs
 *   - rowsCount <= 0: every call returns SPGPU_SUCCESS before the stream is touched; the Plan sets *entriesCount = 0.  The sweep
 *     does the same for coloursCount <= 0;
 *   - an unknown direction or valuesType, or a null array that would be read or written: SPGPU_UNSUPPORTED before a launch.  The
 *     sweep also refuses, before a launch, a colourPtrHost that the Plan would have refused;
 *   - the sweep and the residual trust their index arrays: they are meant for a matrix that a Plan accepted.
 * State
 *   - no call allocates device memory or keeps state;
 *   - the sweep and the residual are asynchronous.  The sweep reads colourPtrHost and *omega at call time, which is also capture
 *     time: both calls can be captured into a HIP graph and replayed after b, x and values changed in place;
 *   - no kernel waits for another workgroup: colours are ordered by stream order between launches and by barriers inside one
 *     workgroup, nothing else.
 *
 * Symmetric Gauss-Seidel on A itself until the residual is small (A in CSR, fp64):
 *
 *     spgpuCsrColourDevice(h, &colours, &rounds, colourOf, rows, aPtr, aIdx, base, work);
 *     spgpuCsrColourOrderDevice(h, order, inverse, colourPtr, rows, colours, colourOf, work);
 *     spgpuCsrSweepPlanDevice(h, &entries, diagPos, colourPtrHost, rows, colours, order, colourPtr, colourOf, aPtr, aIdx, base,
 *                             sweepWork);
 *     (repeat) spgpuCsrSweepDevice(h, x, b, rows, colours, order, colourPtrHost, diagPos, aPtr, aIdx, aVal, base,
 *                                  SPGPU_SWEEP_SYMMETRIC, NULL, SPGPU_TYPE_DOUBLE, entries);
 *              spgpuCsrResidualDevice(h, r, b, x, rows, aPtr, aIdx, aVal, base, SPGPU_TYPE_DOUBLE, entries);
 *              (until spgpuDnrm2(h, rows, r) is small)
 */
#include "../core.h"

#define SPGPU_SWEEP_FORWARD 0
#define SPGPU_SWEEP_BACKWARD 1
#define SPGPU_SWEEP_SYMMETRIC 2

#ifdef __cplusplus
extern "C" {
#endif

/* NEW (no counterpart in the reference).  Bytes of scratch for spgpuCsrSweepPlanDevice; monotone in rowsCount, and the same for
 * rowsCount <= 0 as for rowsCount == 0. */
size_t spgpuCsrSweepWorkBytes(int rowsCount);

/* NEW (no counterpart in the reference).  The checks and the diagonal positions, once per pattern and colouring.  Synchronises the
 * stream (returns host data).  Writes diagPos[rowsCount] and coloursCount + 1 ints of colourPtrHost. */
spgpuStatus_t spgpuCsrSweepPlanDevice(spgpuHandle_t handle, __host int* entriesCount, __device int* diagPos, __host int* colourPtrHost,
                                      int rowsCount, int coloursCount, const __device int* order, const __device int* colourPtr,
                                      const __device int* colourOf, const __device int* rowPtr, const __device int* colIndices,
                                      int baseIndex, __device void* work);

/* NEW (no counterpart in the reference).  One sweep over x in place.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrSweepDevice(spgpuHandle_t handle, __device void* x, const __device void* b, int rowsCount, int coloursCount,
                                  const __device int* order, const __host int* colourPtrHost, const __device int* diagPos,
                                  const __device int* rowPtr, const __device int* colIndices, const __device void* values,
                                  int baseIndex, int direction, const __host void* omega, spgpuType_t valuesType, int entriesCount);

/* NEW (no counterpart in the reference).  r = b - A * x.  Asynchronous, no scratch, no state. */
spgpuStatus_t spgpuCsrResidualDevice(spgpuHandle_t handle, __device void* r, const __device void* b, const __device void* x,
                                     int rowsCount, const __device int* rowPtr, const __device int* colIndices,
                                     const __device void* values, int baseIndex, spgpuType_t valuesType, int entriesCount);

#ifdef __cplusplus
}
#endif
