#pragma once
/*
 * HDIA AND DIA SpMM ON THE REFERENCE'S MULTIVECTOR LAYOUT (no counterpart in the reference, which has no SpMM).
 *
 *     Z[j*pitchYZ + i] = alpha * sum_d dM(i,d) * X[j*pitchX + offsets[d] + i] + beta * Y[j*pitchYZ + i],     j < count
 *
 * Vector j of X, Y and Z starts at base + j*pitch -- the layout of spgpu?mdot, spgpu?maxpby and spgpu?hellspmmMv
 * (spgpu/vector.h, spgpu/ext/spmm_mv.h).  The matrix is given by the leading arguments of spgpu?hdiaspmv (spgpu/hdia.h) resp.
 * spgpu?diaspmv (spgpu/dia.h), unchanged; count, pitchX and pitchYZ follow as in spmm_mv.h.  In HDIA the column of a slot is
 * offsets[d] + row, so a wavefront reads X contiguously along the rows: this layout is the coalesced one for the format and
 * there is no interleaved twin.  One call streams the coefficients once per pass where `count` SpMV calls stream them `count`
 * times.
 *
 * CONTRACT
 *   - RESULT.  A stored slot (diagonal d, row i) contributes iff 0 <= offsets[d] + i < cols; the products of a row are added
 *     in ascending stored diagonal with the multiply-add and the epilogue of the SpMV.
 *   - BIT-IDENTICAL.  Vector j of Z has the bits spgpu?hdiaspmv (resp. spgpu?diaspmv) gives when called on vector j alone.
 *   - PITCHES.  pitchX >= cols and pitchYZ >= rows are element strides.  Elements between the end of a vector and the next
 *     pitch, and behind the last vector, are never read or written.
 *   - Y.  Y == NULL or beta == 0: Y is not read.  Z may alias Y exactly.
 *   - NO-OPS.  count <= 0, rows <= 0 or hackSize <= 0 (dMPitch <= 0 for DIA): nothing is done, and the call returns before
 *     anything touches the handle's stream.
 *   - ANY COUNT.  A pass holds up to 8 vectors; more run as further passes of 8, and what is left over as one pass of a kernel
 *     for 1, 2, 4 or 8 vectors (3 run in the kernel for 4, 5 to 7 in the kernel for 8).  The matrix is read once per pass.
 *     count == 1 is the SpMV call itself.
 *   - ALIGNMENT.  None is demanded: any pointers and pitches give the right result.  The FAST PATH (one 16-byte coefficient
 *     load per lane and diagonal, 16 / sizeof(T) rows per lane) needs what the SpMV's needs: dM 16-byte aligned and hackSize
 *     (dMPitch) a multiple of 16 / sizeof(T).  For 16-byte loads of Y and stores of Z it also needs Z and Y 16-byte aligned
 *     and pitchYZ * sizeof(T) a multiple of 16; otherwise Y and Z move element by element.  X is read with 16-byte loads at
 *     any element address, whatever pitchX is, wherever no strip of the wavefront crosses an edge of the matrix.
 *   - EXECUTION.  Asynchronous on handle->currentStream; no allocation, no state kept, no host synchronisation: the call can
 *     be captured into a HIP graph as it is.
 *
 * Only S and D are offered, as for the HELL SpMM.  Measurements: tools/bench_hdia_spmm.py, DESIGN.md section 3.8.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

void spgpuShdiaspmmMv(spgpuHandle_t handle, __device float* Z, const __device float* Y, float alpha,
                      const __device float* dM, const __device int* offsets, int hackSize,
                      const __device int* hackOffsets, int rows, int cols,
                      const __device float* X, float beta, int count, int pitchX, int pitchYZ);

void spgpuDhdiaspmmMv(spgpuHandle_t handle, __device double* Z, const __device double* Y, double alpha,
                      const __device double* dM, const __device int* offsets, int hackSize,
                      const __device int* hackOffsets, int rows, int cols,
                      const __device double* X, double beta, int count, int pitchX, int pitchYZ);

void spgpuSdiaspmmMv(spgpuHandle_t handle, __device float* Z, const __device float* Y, float alpha,
                     const __device float* dM, const __device int* offsets, int dMPitch, int rows, int cols,
                     int diags, const __device float* X, float beta, int count, int pitchX, int pitchYZ);

void spgpuDdiaspmmMv(spgpuHandle_t handle, __device double* Z, const __device double* Y, double alpha,
                     const __device double* dM, const __device int* offsets, int dMPitch, int rows, int cols,
                     int diags, const __device double* X, double beta, int count, int pitchX, int pitchYZ);

#ifdef __cplusplus
}
#endif
