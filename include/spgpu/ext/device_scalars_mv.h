#pragma once
/*
 * DEVICE-SCALAR LEVEL-1 CALLS ON PITCH MULTIVECTORS (no counterpart in the reference, whose multivector calls take and return
 * host scalars).
 *
 * Vector j of every multivector starts at base + j*pitch -- the layout of spgpu?mdot, spgpu?maxpby (spgpu/vector.h) and of the
 * SpMM calls spgpu?hellspmmMv (spgpu/ext/spmm_mv.h) and spgpu?hdiaspmmMv / spgpu?diaspmmMv (spgpu/ext/hdia_spmm.h).  These are
 * the calls of spgpu/device_scalars.h for `count` vectors at once: one result per vector left in device memory, one coefficient
 * per vector taken from device memory.  A solver that carries `count` right-hand sides through one matrix runs its whole
 * iteration -- one SpMM, these calls -- from one captured graph; tools/cg_multi_amd.c does.
 *
 * ARGUMENTS.  All arrays are device pointers.  `count` and `pitch` are those of spgpu?mdot.  Every per-vector scalar array
 * (result, out, num, den, alpha, beta, alphaNum, alphaDen, betaNum, betaDen) has `count` elements; element j belongs to vector j.
 * A NULL scalar array stands for 1 in every vector, as a NULL operand does in spgpu?axpbyQuotDevice.
 *
 * CONTRACT
 *   - EXECUTION.  Asynchronous on handle->currentStream; no allocation, no host synchronisation: every call can be captured into
 *     a HIP graph as it is.  count <= 0: the call returns before anything touches the stream.
 *   - REDUCTIONS.  result[j] of spgpu?mdotDevice has the bits of y[j] of spgpu?mdot with the same arguments; spgpu?mnrm2Device
 *     matches spgpu?mnrm2 the same way.  (The first stage, its grid and its choice of 16-byte loads are those of spgpu?mdot:
 *     passes of at most 1024 vectors, the vectors of a pass sharing 1024 workgroups; then one wavefront per vector adds the
 *     block partials in the fixed order the host uses.)  n <= 0 with count > 0: every result[j] is +0.
 *   - REDUCTIONS AGAINST THE SINGLE-VECTOR CALLS.  result[j] also has the bits of spgpu?dotDevice / spgpu?nrm2Device on vector j
 *     alone whenever (1) the bases are 16-byte aligned, (2) pitch * sizeof(T) is a multiple of 16 and (3) the cap on workgroups
 *     per vector does not bind:  ceil(ceil(n / (16 / sizeof(T))) / 1024) * count <= 1024.
 *   - UPDATES.  Vector j of z has the bits spgpu?axpbyQuotDevice (resp. spgpu?axpbyDevice) leaves when called on vector j with
 *     pointers to element j of each scalar array: beta_j = betaNum[j] / betaDen[j], alpha_j = (negateAlpha ? -1 : 1) *
 *     alphaNum[j] / alphaDen[j], one IEEE division each.  Whether y is read is decided per vector: where beta_j is 0, or beta is
 *     NULL in spgpu?maxpbyDevice, vector j of y is not read.  z may alias y exactly.
 *   - PAIR-DOT.  With a_j = alphaNum[j] / alphaDen[j]: z1_j = y1_j + a_j*x1_j, z2_j = y2_j - a_j*x2_j with the bits of
 *     spgpu?axpbyPairDotDevice on vector j; result[j] has the bits spgpu?mdotDevice(result, n, z2, z2, count, pitch) would leave
 *     for the stored z2.  z1 may alias y1 exactly, z2 may alias y2 exactly.
 *   - DIVISION.  spgpu?mdivDevice: out[j] = (negate ? -1 : 1) * (num[j] / den[j]), one IEEE division as in spgpu?divDevice.  0/0
 *     gives NaN here and in the quotients above, as in the single-vector calls: a caller stops a column before it has converged
 *     to zero.
 *   - PITCH AND NEIGHBOURS.  pitch >= n is an element stride.  Elements between the end of a vector and the next pitch, and
 *     behind the last vector, are never read or written.  result[count] (out[count]) and beyond are never written.
 *   - ALIGNMENT.  None is demanded.  The updates use 16-byte accesses when z, x and a y that may be read (given, and beta not
 *     NULL) are 16-byte aligned and pitch * sizeof(T) is a multiple of 16 (any pitch for count == 1); otherwise they go element
 *     by element.  The values are the same either way.
 *
 * Only S and D are offered, as for the SpMM and the single-vector device-scalar calls.  Measurements: tools/bench_mv_level1.py,
 * DESIGN.md section 3.9.
 * The pair-dot with the Jacobi step of preconditioned CG inside (spgpu?maxpbyPairAxyDotDevice): spgpu/ext/precond.h.
 */
#include "../core.h"

#ifdef __cplusplus
extern "C" {
#endif

void spgpuSmdotDevice(spgpuHandle_t handle, __device float* result, int n, const __device float* a, const __device float* b,
                      int count, int pitch);
void spgpuDmdotDevice(spgpuHandle_t handle, __device double* result, int n, const __device double* a, const __device double* b,
                      int count, int pitch);

void spgpuSmnrm2Device(spgpuHandle_t handle, __device float* result, int n, const __device float* x, int count, int pitch);
void spgpuDmnrm2Device(spgpuHandle_t handle, __device double* result, int n, const __device double* x, int count, int pitch);

void spgpuSmdivDevice(spgpuHandle_t handle, __device float* out, const __device float* num, const __device float* den,
                      int negate, int count);
void spgpuDmdivDevice(spgpuHandle_t handle, __device double* out, const __device double* num, const __device double* den,
                      int negate, int count);

void spgpuSmaxpbyDevice(spgpuHandle_t handle, __device float* z, int n, const __device float* beta, const __device float* y,
                        const __device float* alpha, const __device float* x, int count, int pitch);
void spgpuDmaxpbyDevice(spgpuHandle_t handle, __device double* z, int n, const __device double* beta, const __device double* y,
                        const __device double* alpha, const __device double* x, int count, int pitch);

void spgpuSmaxpbyQuotDevice(spgpuHandle_t handle, __device float* z, int n, const __device float* betaNum,
                            const __device float* betaDen, const __device float* y, const __device float* alphaNum,
                            const __device float* alphaDen, int negateAlpha, const __device float* x, int count, int pitch);
void spgpuDmaxpbyQuotDevice(spgpuHandle_t handle, __device double* z, int n, const __device double* betaNum,
                            const __device double* betaDen, const __device double* y, const __device double* alphaNum,
                            const __device double* alphaDen, int negateAlpha, const __device double* x, int count, int pitch);

void spgpuSmaxpbyPairDotDevice(spgpuHandle_t handle, __device float* result, int n, __device float* z1,
                               const __device float* y1, const __device float* x1, __device float* z2,
                               const __device float* y2, const __device float* x2, const __device float* alphaNum,
                               const __device float* alphaDen, int count, int pitch);
void spgpuDmaxpbyPairDotDevice(spgpuHandle_t handle, __device double* result, int n, __device double* z1,
                               const __device double* y1, const __device double* x1, __device double* z2,
                               const __device double* y2, const __device double* x2, const __device double* alphaNum,
                               const __device double* alphaDen, int count, int pitch);

#ifdef __cplusplus
}
#endif
