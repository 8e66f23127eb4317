#pragma once
/*
 * JACOBI PRECONDITIONING: the diagonal of a matrix the library already holds, and the preconditioner step of CG fused into the
 * device-scalar calls of a captured iteration (no counterpart in the reference, which has no preconditioner and whose
 * reductions return host scalars).
 *
 * With these calls a Jacobi-preconditioned CG iteration is 5 kernels, as many as plain CG from spgpu/device_scalars.h:
 *
 *     spgpuDhellDiag(h, dinv, cM, rP, hackSize, hackOffsets, rS, rows, base, 1);              once per matrix
 *     ...
 *     spgpuDhellspmvDotDevice(h, pAp, NULL, Ap, NULL, 1.0, cM, rP, hackSize, hackOffsets, rS, rows, p, 0.0, base);
 *     spgpuDaxpbyPairAxyDotDevice(h, rzNew, rows, x, x, p, r, r, Ap, z, dinv, rzOld, pAp);    rzNew[0] = r.z, rzNew[1] = |r|^2
 *     spgpuDaxpbyQuotDevice(h, p, rows, rzNew, rzOld, p, NULL, NULL, 0, z);                   p = z + (r.z / r.z old) p
 *
 * tools/pcg_amd.c runs that loop against the same iteration written with host scalars; INTEGRATION.md shows it in full.
 * A stronger preconditioner than the diagonal -- Gauss-Seidel, SSOR, the application of an ILU(0) -- is the sparse triangular
 * solve of ext/trsv_device.h; the ILU(0) factor itself comes from ext/ilu0_device.h.
 *
 * ARGUMENTS.  All arrays are device pointers.  The matrix arguments of a ?Diag call are the leading matrix arguments of the
 * matching SpMV (spgpu/hell.h, spgpu/ell.h, spgpu/hdia.h), in the same order and with the same meaning.  Only S and D are
 * offered, as for the other device-scalar calls.
 *
 * ---- DIAGONAL EXTRACTION: spgpu?hellDiag, spgpu?ellDiag, spgpu?hdiaDiag ------------------------------------------------------
 *   - VALUE.  d[i] is the sum of the stored entries of row i whose column is i, added in ascending slot k, starting from +0.  A
 *     row without such an entry gets +0.
 *       ELL / HELL: slot k of row i counts iff k < rS[i] (ELL with rS == NULL: every one of the maxNnzPerRow slots counts) and
 *       rP[slot] - baseIndex == i.  Slots beyond rS[i] are never used, whatever they hold; cM is read only where the column
 *       matched.
 *       HDIA: the sum runs over the diagonals of the row's hack whose offsets[] entry is 0, for i < cols; rows i >= cols get +0.
 *   - INVERT.  invert != 0 stores 1 / d[i] instead: one IEEE division, so a zero diagonal gives inf as it would on the host.
 *   - EXECUTION.  Asynchronous on handle->currentStream.  No allocation, no state kept, no host synchronisation: the call can
 *     be captured into a HIP graph.  One kernel.
 *   - NO-OPS.  rows <= 0 or hackSize <= 0 (HELL, HDIA): the call returns before anything touches the stream.
 *   - NEIGHBOURS.  d[rows] and beyond are never written; nothing but d is written.  d must not overlap the matrix arrays.
 *   - ALIGNMENT.  None is demanded.  ELL / HELL read four rows' column indices with one 16-byte load where rP lies on a 16-byte
 *     boundary and hackSize (ELL: rPPitch) is a multiple of 4; otherwise index by index.  The values are the same either way.
 *   - The call runs once per matrix and is not tuned.
 *
 * ---- FUSED STEPS, ONE VECTOR: spgpu?axyDotDevice, spgpu?axpbyPairAxyDotDevice -------------------------------------------------
 *   spgpu?axyDotDevice(result, n, z, d, r):  z = d o r (element-wise), *result = r . z -- the z = M^-1 r, r.z of the start of PCG.
 *   - BITS.  z has the bits of spgpu?axy(z, n, 1, d, r); *result has the bits spgpu?dotDevice(result, n, r, z) leaves for the
 *     stored z.
 *   - ALIASING.  z must not alias d or r.
 *   spgpu?axpbyPairAxyDotDevice(result, n, z1, y1, x1, z2, y2, x2, w, d, alphaNum, alphaDen):  with a = *alphaNum / *alphaDen
 *   (a NULL operand stands for 1): z1 = y1 + a*x1, z2 = y2 - a*x2, w = d o z2, result[0] = z2 . w, result[1] = z2 . z2 -- the
 *   x += alpha p, r -= alpha Ap, z = M^-1 r, r.z and |r|^2 of PCG.  `result` has TWO cells.
 *   - BITS.  z1, z2 and result[1] have the bits of spgpu?axpbyPairDotDevice(result + 1, n, z1, y1, x1, z2, y2, x2, alphaNum,
 *     alphaDen); w has the bits of spgpu?axy(w, n, 1, d, z2); result[0] has the bits of spgpu?dotDevice(result, n, z2, w) for
 *     the stored vectors -- for a w that lies on a 16-byte boundary whenever z2 does.  (Both sums run on ONE grid, that of
 *     z2 . z2, which z2's alignment decides.  A w off the boundary under an aligned z2 is read and written element-aligned;
 *     result[0] is then what spgpu?dotDevice leaves for z2 and a copy of the stored w placed on a 16-byte boundary.)
 *   - ALIASING.  z1 may alias y1 exactly, z2 may alias y2 exactly.  w aliases nothing.
 *   - EXECUTION.  As above; each call is two kernels (the block partials; one launch that combines them in the fixed order of
 *     spgpu?dotDevice).  n <= 0: every result is +0 and no vector is touched.
 *   - ALIGNMENT.  None is demanded.  16-byte accesses are chosen as spgpu?dotDevice chooses them for the operands of the dot
 *     (r and z; z2); d and w never decide it.
 *
 * ---- FUSED STEPS ON PITCH MULTIVECTORS: spgpu?maxyDotDevice, spgpu?maxpbyPairAxyDotDevice --------------------------------------
 *   The argument lists above followed by count, pitch (spgpu/ext/device_scalars_mv.h: vector j of every multivector at
 *   base + j*pitch, one result and one coefficient per vector).
 *   - d IS A PITCH MULTIVECTOR TOO: d_j at d + j*pitch.  A caller with one matrix passes `count` copies of its diagonal.
 *   - RESULTS.  spgpu?maxyDotDevice: result has count cells.  spgpu?maxpbyPairAxyDotDevice: result has 2*count cells,
 *     result[j] = z2_j . w_j, result[count + j] = z2_j . z2_j.
 *   - BITS.  The vectors have the bits of the single-vector call on vector j with element j of alphaNum / alphaDen.
 *     result[j] of spgpu?maxyDotDevice has the bits of spgpu?mdotDevice(result, n, r, z, count, pitch) for the stored z;
 *     result[count + j] those of spgpu?maxpbyPairDotDevice; result[j] of the pair call those of spgpu?mdotDevice(result, n, z2,
 *     w, count, pitch) under the same proviso as above (w's vectors on a 16-byte boundary whenever z2's are).
 *   - NO-OPS.  count <= 0: the call returns before anything touches the stream.  n <= 0 with count > 0: every result is +0.
 *   - NEIGHBOURS.  Elements between the end of a vector and the next pitch, and behind the last vector, are never read or
 *     written; result[count] (pair: result[2*count]) and beyond are never written.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

void spgpuShellDiag(spgpuHandle_t handle, __device float* d, const __device float* cM, const __device int* rP, int hackSize,
                    const __device int* hackOffsets, const __device int* rS, int rows, int baseIndex, int invert);
void spgpuDhellDiag(spgpuHandle_t handle, __device double* d, const __device double* cM, const __device int* rP, int hackSize,
                    const __device int* hackOffsets, const __device int* rS, int rows, int baseIndex, int invert);

void spgpuSellDiag(spgpuHandle_t handle, __device float* d, const __device float* cM, const __device int* rP, int cMPitch,
                   int rPPitch, const __device int* rS, int maxNnzPerRow, int rows, int baseIndex, int invert);
void spgpuDellDiag(spgpuHandle_t handle, __device double* d, const __device double* cM, const __device int* rP, int cMPitch,
                   int rPPitch, const __device int* rS, int maxNnzPerRow, int rows, int baseIndex, int invert);

void spgpuShdiaDiag(spgpuHandle_t handle, __device float* d, const __device float* dM, const __device int* offsets, int hackSize,
                    const __device int* hackOffsets, int rows, int cols, int invert);
void spgpuDhdiaDiag(spgpuHandle_t handle, __device double* d, const __device double* dM, const __device int* offsets, int hackSize,
                    const __device int* hackOffsets, int rows, int cols, int invert);

void spgpuSaxyDotDevice(spgpuHandle_t handle, __device float* result, int n, __device float* z, const __device float* d,
                        const __device float* r);
void spgpuDaxyDotDevice(spgpuHandle_t handle, __device double* result, int n, __device double* z, const __device double* d,
                        const __device double* r);

void spgpuSaxpbyPairAxyDotDevice(spgpuHandle_t handle, __device float* result, int n, __device float* z1,
                                 const __device float* y1, const __device float* x1, __device float* z2,
                                 const __device float* y2, const __device float* x2, __device float* w,
                                 const __device float* d, const __device float* alphaNum, const __device float* alphaDen);
void spgpuDaxpbyPairAxyDotDevice(spgpuHandle_t handle, __device double* result, int n, __device double* z1,
                                 const __device double* y1, const __device double* x1, __device double* z2,
                                 const __device double* y2, const __device double* x2, __device double* w,
                                 const __device double* d, const __device double* alphaNum, const __device double* alphaDen);

void spgpuSmaxyDotDevice(spgpuHandle_t handle, __device float* result, int n, __device float* z, const __device float* d,
                         const __device float* r, int count, int pitch);
void spgpuDmaxyDotDevice(spgpuHandle_t handle, __device double* result, int n, __device double* z, const __device double* d,
                         const __device double* r, int count, int pitch);

void spgpuSmaxpbyPairAxyDotDevice(spgpuHandle_t handle, __device float* result, int n, __device float* z1,
                                  const __device float* y1, const __device float* x1, __device float* z2,
                                  const __device float* y2, const __device float* x2, __device float* w,
                                  const __device float* d, const __device float* alphaNum, const __device float* alphaDen,
                                  int count, int pitch);
void spgpuDmaxpbyPairAxyDotDevice(spgpuHandle_t handle, __device double* result, int n, __device double* z1,
                                  const __device double* y1, const __device double* x1, __device double* z2,
                                  const __device double* y2, const __device double* x2, __device double* w,
                                  const __device double* d, const __device double* alphaNum, const __device double* alphaDen,
                                  int count, int pitch);

#ifdef __cplusplus
}
#endif
