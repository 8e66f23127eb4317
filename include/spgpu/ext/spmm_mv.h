#pragma once
/*
 * HELL SpMM ON THE REFERENCE'S MULTIVECTOR LAYOUT (no counterpart in the reference, which has no SpMM).
 *
 *     Z[j*pitchYZ + i] = alpha * sum_k A[i,k] * X[j*pitchX + col(i,k)] + beta * Y[j*pitchYZ + i],     j < count
 *
 * NEW: the layout.  Vector j of X, Y and Z starts at base + j*pitch -- what spgpu?mdot, spgpu?mnrm2, spgpu?maxpby, spgpu?maxy,
 * spgpu?maxypbz, spgpu?mamax and spgpu?masum take (spgpu/vector.h; reference vector.h:75-91, 187-194, 387-403) and what a
 * block Krylov solver or a multi-rhs preconditioner written against spGPU holds.  spgpu?hellspmm (spgpu/spmm.h) wants
 * interleaved rows, M[i*ld + j]; a holder of pitch vectors paid spgpu?mvInterleave of X and spgpu?mvDeinterleave of Z (and
 * the transpose of Y when beta != 0) around every product.  This call takes the vectors as they are.
 *
 * MIRRORS spgpu?hellspmm in everything else:
 *   - A is given by the HELL arguments of spgpu?hellspmv, unchanged (hell.h:45-59): any hackSize, baseIndex 0 or 1, rIdx NULL or
 *     a row order (the result of matrix row i goes to row rIdx[i] of Z, and Y is read there);
 *   - asynchronous on handle->currentStream, no allocation, no state kept, no host synchronisation: it can be captured into a
 *     HIP graph as it is;
 *   - count <= 0 or rows <= 0: no-op.  Any count; more than 16 vectors run as passes of 16 (the matrix is read once per pass);
 *   - Y == NULL or beta == 0: Y is not read.  Z may alias Y exactly.  With Z == Y and beta == 1 (Z += alpha*A*X) the rows with
 *     rS[i] == 0 are neither read nor written;
 *   - per (row, vector) the products are added in ascending k with the same fused multiply-adds: the result is BIT-IDENTICAL
 *     to spgpu?mvInterleave -> spgpu?hellspmm -> spgpu?mvDeinterleave on the same data.
 *
 * pitchX and pitchYZ are element strides, >= the vector lengths (the columns of A for X, rows for Y and Z).  Elements
 * between the end of a vector and the next pitch, and behind the last vector, are never read or written.
 *
 * No alignment is demanded: any pointers and pitches give the right result.  The FAST PATH needs what spGPU's own
 * allocations give: hackSize a multiple of 32 and cM, rP 16-byte aligned (the strip kernel of spgpu?hellspmm, here with
 * the vectors transposed into its LDS tile as they are loaded); and, for 16-byte loads and stores along the vectors,
 * X, Y, Z 16-byte aligned, pitchX and pitchYZ multiples of 16 bytes, rIdx == NULL.  With rIdx the rows of Z are scattered:
 * every element of Y and Z is then a load or store of its own (4 or 8 bytes) -- inherent to a row order in this layout.
 *
 * WHEN TO USE WHICH.  A workgroup of this call stages the X rows its 256 matrix rows name in LDS when they span at most
 * about 300 rows (16 vectors of doubles; twice that for up to 8), i.e. for band, stencil and FEM-like matrices in a local
 * order: there the pitch layout costs only the transposing fill.  Columns outside such a window are fetched as ONE GATHER
 * PER VECTOR -- 16 cache lines per nonzero where an interleaved row is one -- so for matrices with scattered columns
 * converting (spgpu?mvInterleave -> spgpu?hellspmm -> spgpu?mvDeinterleave), or staying interleaved, remains the faster route.
 * Measured on MI355X, fp64, 5 M rows x 32, 16 vectors, this call / the converting route / spgpu?hellspmm on interleaved data:
 * banded 0.711 / 1.133 / 0.567 ms; columns random within +-32 768 of the row 34.8 / 3.05 / 2.48 ms; random over all of X
 * 46.1 / 3.86 / 3.28 ms (tools/bench_spmm_mv.py, profiles/spmm_mv_ab.json).
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

void spgpuShellspmmMv(spgpuHandle_t handle, __device float* Z, const __device float* Y, float alpha,
                      const __device float* cM, const __device int* rP, int hackSize,
                      const __device int* hackOffsets, const __device int* rS, const __device int* rIdx,
                      int avgNnzPerRow, int rows, const __device float* X, float beta, int baseIndex,
                      int count, int pitchX, int pitchYZ);

void spgpuDhellspmmMv(spgpuHandle_t handle, __device double* Z, const __device double* Y, double alpha,
                      const __device double* cM, const __device int* rP, int hackSize,
                      const __device int* hackOffsets, const __device int* rS, const __device int* rIdx,
                      int avgNnzPerRow, int rows, const __device double* X, double beta, int baseIndex,
                      int count, int pitchX, int pitchYZ);

#ifdef __cplusplus
}
#endif
