#pragma once
/* The layout conversions of spgpu/ext/spmm_mv.h: pitch layout (vector j at j*pitch) <-> interleaved multivectors. */
#include "spgpu_internal.h"

namespace spgpu {

/* Layout conversion through a 32x33 LDS tile so that both sides are coalesced. */
template <typename T, bool TO_INTERLEAVED>
__global__ __launch_bounds__(256) void mvTransposeKernel(T* dst, long long dstLd, const T* src, long long srcLd, int n,
                                                         int count)
{
    __shared__ T tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5; /* 32 x 8 */
    /* "long" axis i (0..n), "short" axis j (0..count) */
    const long long i0 = (long long)blockIdx.x * 32;
    const int j0 = blockIdx.y * 32;
    if constexpr (TO_INTERLEAVED) {
        /* src[j*srcLd + i] -> dst[i*dstLd + j] */
        for (int jj = ty; jj < 32; jj += 8)
            if (i0 + tx < n && j0 + jj < count)
                tile[jj][tx] = src[(long long)(j0 + jj) * srcLd + i0 + tx];
        __syncthreads();
        for (int ii = ty; ii < 32; ii += 8)
            if (i0 + ii < n && j0 + tx < count)
                dst[(i0 + ii) * dstLd + j0 + tx] = tile[tx][ii];
    } else {
        /* src[i*srcLd + j] -> dst[j*dstLd + i] */
        for (int ii = ty; ii < 32; ii += 8)
            if (i0 + ii < n && j0 + tx < count)
                tile[ii][tx] = src[(i0 + ii) * srcLd + j0 + tx];
        __syncthreads();
        for (int jj = ty; jj < 32; jj += 8)
            if (i0 + tx < n && j0 + jj < count)
                dst[(long long)(j0 + jj) * dstLd + i0 + tx] = tile[tx][jj];
    }
}

template <typename T, bool TO_INTERLEAVED>
static void mvTranspose(spgpuHandle_t handle, T* dst, int dstLd, const T* src, int srcLd, int n, int count)
{
    if (n <= 0 || count <= 0)
        return;
    const dim3 grid((unsigned)(((long long)n + 31) / 32), (unsigned)((count + 31) / 32));
    hipLaunchKernelGGL((mvTransposeKernel<T, TO_INTERLEAVED>), grid, dim3(256), 0, handle->currentStream, dst,
                       (long long)dstLd, src, (long long)srcLd, n, count);
    spgpuDebugCheck(handle, "mvTranspose");
}

} // namespace spgpu
