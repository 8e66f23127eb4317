#pragma once
/*
 * THE FUSED SpMV + DOT OF A CAPTURED CG ITERATION, FOR HDIA AND DIA MATRICES (no counterpart in the reference, whose reductions
 * return host scalars; the HELL form is spgpu?hellspmvDotDevice, spgpu/device_scalars.h).
 *
 * A stencil matrix is stored and multiplied best in HDIA (spgpu/hdia.h: no column indices).  With these calls a CG iteration on
 * such a matrix is 5 kernels instead of 8, as it is on a HELL matrix:
 *
 *     spgpuDhdiaspmvDotDevice(h, pAp, NULL, Ap, NULL, 1.0, dM, offsets, hackSize, hackOffsets, rows, rows, p, 0.0);
 *     spgpuDaxpbyPairDotDevice(h, rrNew, rows, x, x, p, r, r, Ap, rrOld, pAp);                 x += a p, r -= a Ap, |r|^2
 *     spgpuDaxpbyQuotDevice(h, p, rows, rrNew, rrOld, p, NULL, NULL, 0, r);                    p = r + (|r|^2 / |r|^2 old) p
 *
 * and Jacobi PCG the same with spgpu?hdiaDiag and spgpu?axpbyPairAxyDotDevice (spgpu/ext/precond.h).  tools/cg_hdia_amd.c runs
 * both against the unfused iteration (spgpu?hdiaspmv + spgpu?dotDevice + ...) and compares the iterates bit for bit.
 *
 *   spgpu?hdiaspmvDotDevice(result, w, z, y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, x, beta)
 *   spgpu?diaspmvDotDevice (result, w, z, y, alpha, dM, offsets, dMPitch, rows, cols, diags, x, beta)
 *       z = alpha*A*x + beta*y,  *result = w . z
 *
 * ARGUMENTS.  All arrays are device pointers; `result` is one cell in device memory.  After result and w the lists are those of
 * spgpu?hdiaspmv (spgpu/hdia.h) and spgpu?diaspmv (spgpu/dia.h), in the same order and with the same meaning.  Only S and D are
 * offered, as for the other device-scalar calls.
 *   - BITS OF z.  z holds the bits spgpu?hdiaspmv / spgpu?diaspmv writes for the same arguments, for EVERY matrix: a row's
 *     products over the in-range slots (0 <= offsets[d] + row < cols) are added with one fused multiply-add each in ascending
 *     stored diagonal d, starting from +0, then z = alpha*sum (+ beta*y, one more fused multiply-add).  The SpMV adds in that order
 *     on each of its paths, so the contract has no exception (the HELL call has one).  A hack without diagonals gives
 *     z = alpha*0 + beta*y.
 *   - BITS OF *result.  *result holds the bits spgpu?dotDevice(result, rows, w, z) would leave for the stored z: the call IS the
 *     first stage of that dot -- its grid, its element -> lane mapping, its order of additions -- with the second operand
 *     produced on the fly, followed by the dot's second stage.  So it is also what spgpu?dot(rows, w, z) returns.
 *   - w == NULL stands for w = x (the p . Ap of CG).  x has `cols` elements and the dot reads `rows` of them: this needs
 *     cols >= rows.
 *   - beta == 0: y is never read (it may be NULL or hold anything).
 *   - ALIASING.  z may alias y exactly.  z must not alias x or w.
 *   - NO-OPS.  rows <= 0 or hackSize (dMPitch) <= 0: no vector is touched and *result = +0 (the second stage still runs).
 *   - NEIGHBOURS.  z[rows] and beyond are never written; nothing but z, *result and the handle's reduction scratch is written.
 *   - EXECUTION.  Asynchronous on handle->currentStream.  No allocation, no host synchronisation: the calls can be captured into
 *     a HIP graph.  Two kernels each.
 *   - ALIGNMENT.  None is demanded.  16-byte accesses are chosen as spgpu?dotDevice chooses them, from w (x when w == NULL) and z.
 *     Where they are chosen, hackSize (dMPitch) is a multiple of 16 / sizeof(T) and dM lies on a 16-byte boundary, a lane reads
 *     the coefficients of its 16 / sizeof(T) rows with one load per diagonal.  y and x may lie anywhere.  The values are the
 *     same on every path.
 *   - SIZE.  The dot's grid is at most 1024 workgroups of 256 lanes: the calls are for systems whose iteration is bound by its
 *     chain of dependent launches (DESIGN.md says where they stop paying).
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

void spgpuShdiaspmvDotDevice(spgpuHandle_t handle, __device float* result, const __device float* w, __device float* z,
                             const __device float* y, float alpha, const __device float* dM, const __device int* offsets,
                             int hackSize, const __device int* hackOffsets, int rows, int cols, const __device float* x,
                             float beta);
void spgpuDhdiaspmvDotDevice(spgpuHandle_t handle, __device double* result, const __device double* w, __device double* z,
                             const __device double* y, double alpha, const __device double* dM, const __device int* offsets,
                             int hackSize, const __device int* hackOffsets, int rows, int cols, const __device double* x,
                             double beta);

void spgpuSdiaspmvDotDevice(spgpuHandle_t handle, __device float* result, const __device float* w, __device float* z,
                            const __device float* y, float alpha, const __device float* dM, const __device int* offsets,
                            int dMPitch, int rows, int cols, int diags, const __device float* x, float beta);
void spgpuDdiaspmvDotDevice(spgpuHandle_t handle, __device double* result, const __device double* w, __device double* z,
                            const __device double* y, double alpha, const __device double* dM, const __device int* offsets,
                            int dMPitch, int rows, int cols, int diags, const __device double* x, double beta);

#ifdef __cplusplus
}
#endif
