/* Included by ellpack_spmv.hip (namespace spgpu); launched by ellCsput there. */

/* ---- ELL coefficient update (include/spgpu/ell.h; reference ell_csput_base.cuh:33-75) ---- */
template <typename T>
__global__ __launch_bounds__(kBlockThreads) void ellCsputKernel(T* cM, const int* rP, long long cMPitch, long long rPPitch,
                                                               const int* rS, int nnz, const int* aI, const int* aJ,
                                                               const T* aVal, int baseIndex)
{
    const long long i = (long long)blockIdx.x * kBlockThreads + threadIdx.x;
    if (i >= nnz)
        return;
    const int row = aI[i] - baseIndex;
    if (row < 0)
        return;
    const int column = aJ[i];
    int lower = 0, upper = rS[row] - 1;
    while (lower <= upper) { /* the row's stored indices ascend */
        const int mid = (lower + upper) / 2;
        const int stored = rP[row + mid * rPPitch];
        if (stored == column) {
            cM[row + mid * cMPitch] = aVal[i];
            return;
        }
        if (stored < column)
            lower = mid + 1;
        else
            upper = mid - 1;
    }
}
