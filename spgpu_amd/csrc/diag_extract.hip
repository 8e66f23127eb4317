/*
 * The diagonal of an ELL, HELL or HDIA matrix, for gfx950 (MI355X): what a Jacobi preconditioner needs from a matrix the
 * library already holds.
 *
 * C ABI: spgpu{S,D}hellDiag, spgpu{S,D}ellDiag, spgpu{S,D}hdiaDiag (include/spgpu/ext/precond.h).  NEW: the reference has no such
 * call; its user keeps the COO copy and picks the diagonal out on the host.
 *
 * ELL / HELL: a lane owns one row -- or four consecutive rows of one hack where their column indices are one 16-byte load --,
 * the lanes of a wavefront own consecutive rows: the index reads of a slot column are coalesced.  A coefficient is read only
 * where the column matched, so a slot costs the 4 bytes of its index, not 12.  Entries of a row are added in ascending k from
 * +0, one lane per row: no cross-lane step, no atomics.
 * HDIA: a lane owns one row; it walks offsets[hackOffsets[h] .. hackOffsets[h+1]) of its hack (the same address in every lane of
 * the hack: a broadcast) and reads dM only on a diagonal whose offset is 0 -- consecutive lanes, consecutive addresses.
 *
 * The call runs once per matrix: it is written to be simple and has not been tuned.
 * Roofline: HBM.  Algorithmic bytes: 4 per stored slot (ELL / HELL) or per stored diagonal and hack (HDIA), + sizeof(T) per row
 * read and written.
 */
#include "level1_grid.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/precond.h"

namespace spgpu {

constexpr int kDiagThreads = 256;
constexpr int kDiagPack = 4; /* rows whose column indices are one 16-byte load */

/* ELL is HELL with one hack that holds every row: slot of (row r, entry k) = r + k * pitch (hackOffsets == NULL). */
template <typename T> struct DiagArgs {
    T* d;
    const T* cM;
    const int* rP;
    const int* hackOffsets; /* NULL: ELL */
    const int* rS;          /* NULL (ELL only): every row has maxNnz slots */
    long long cMStride, rPStride; /* HELL: hackSize both; ELL: the two pitches */
    int hackSize, maxNnz, rows, baseIndex, invert;
};

template <typename T> __device__ inline T diagOut(T sum, int invert) { return invert ? T(1) / sum : sum; }

/* VEC consecutive rows from `row` on (inside one hack when VEC > 1), their diagonal entries added in ascending k. */
template <typename T, int VEC> __device__ inline void diagRows(const DiagArgs<T>& a, long long row)
{
    long long first = row; /* slot of the row's entry 0; entry k lies k strides further */
    if (a.hackOffsets)
        first = (long long)a.hackOffsets[row / a.hackSize] + row % a.hackSize;
    int len[VEC], longest = 0;
    T sum[VEC];
#pragma unroll
    for (int t = 0; t < VEC; ++t) {
        len[t] = a.rS ? a.rS[row + t] : a.maxNnz;
        longest = len[t] > longest ? len[t] : longest;
        sum[t] = zeroOf<T>();
    }
    for (int k = 0; k < longest; ++k) {
        const long long slot = first + k * a.rPStride;
        int column[VEC];
        if constexpr (VEC > 1) {
            const Pack<int, VEC> c = loadPackElementAligned<int, VEC>(a.rP + slot);
#pragma unroll
            for (int t = 0; t < VEC; ++t)
                column[t] = c.v[t];
        } else
            column[0] = a.rP[slot];
#pragma unroll
        for (int t = 0; t < VEC; ++t)
            if (k < len[t] && (long long)column[t] - a.baseIndex == row + t)
                sum[t] = add(sum[t], a.cM[first + k * a.cMStride + t]);
    }
#pragma unroll
    for (int t = 0; t < VEC; ++t)
        a.d[row + t] = diagOut(sum[t], a.invert);
}

template <typename T, int VEC> __global__ __launch_bounds__(kDiagThreads) void ellDiagKernel(DiagArgs<T> a)
{
    const long long lane = (long long)blockIdx.x * kDiagThreads + threadIdx.x;
    const long long packs = a.rows / VEC;
    if (lane < packs)
        diagRows<T, VEC>(a, lane * VEC);
    if constexpr (VEC > 1) { /* the rows % VEC rows behind the last pack */
        const long long tail = packs * VEC + lane;
        if (tail < a.rows)
            diagRows<T, 1>(a, tail);
    }
}

/* Four rows' indices as one load: the four rows lie in one hack, and with hackOffsets[] multiples of hackSize -- as the converters
 * leave them -- at a slot on a 16-byte boundary.  (The load itself promises element alignment only: a hackOffsets[] that is not
 * such a multiple costs speed, nothing else.) */
static bool packedIndices(long long rPStride, int hackSize, const int* rP)
{
    return rPStride % kDiagPack == 0 && hackSize % kDiagPack == 0 && allAligned(sizeof(int) * kDiagPack, {rP});
}

template <typename T> static void ellDiag(spgpuHandle_t handle, const DiagArgs<T>& a, const char* what)
{
    withConstants([&](auto packed) {
        constexpr int VEC = packed ? kDiagPack : 1;
        const long long packs = a.rows / VEC, tail = a.rows % VEC; /* the tail rows go to the first lanes */
        hipLaunchKernelGGL((ellDiagKernel<T, VEC>), dim3((unsigned)ceilDiv(packs > tail ? packs : tail, kDiagThreads)), dim3(kDiagThreads), 0,
                           handle->currentStream, a);
    }, packedIndices(a.rPStride, a.hackSize, a.rP));
    spgpuDebugCheck(handle, what);
}

template <typename T>
static void hellDiag(spgpuHandle_t handle, T* d, const T* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                     int rows, int baseIndex, int invert)
{
    if (rows <= 0 || hackSize <= 0)
        return;
    const DiagArgs<T> a = {d, cM, rP, hackOffsets, rS, hackSize, hackSize, hackSize, 0, rows, baseIndex, invert};
    ellDiag<T>(handle, a, "hellDiag");
}

template <typename T>
static void ellDiagOf(spgpuHandle_t handle, T* d, const T* cM, const int* rP, int cMPitch, int rPPitch, const int* rS,
                      int maxNnzPerRow, int rows, int baseIndex, int invert)
{
    if (rows <= 0)
        return;
    /* no hacks: a pack of kDiagPack rows below `rows` never leaves the allocation, whose pitches are at least `rows` */
    const DiagArgs<T> a = {d, cM, rP, nullptr, rS, cMPitch, rPPitch, kDiagPack, maxNnzPerRow, rows, baseIndex, invert};
    ellDiag<T>(handle, a, "ellDiag");
}

template <typename T>
__global__ __launch_bounds__(kDiagThreads) void hdiaDiagKernel(T* d, const T* dM, const int* offsets, int hackSize,
                                                              const int* hackOffsets, int rows, int cols, int invert)
{
    const long long row = (long long)blockIdx.x * kDiagThreads + threadIdx.x;
    if (row >= rows)
        return;
    const long long hack = row / hackSize, inHack = row % hackSize;
    T sum = zeroOf<T>();
    if (row < cols) {
        const int last = hackOffsets[hack + 1];
        for (int diag = hackOffsets[hack]; diag < last; ++diag)
            if (offsets[diag] == 0)
                sum = add(sum, dM[(long long)diag * hackSize + inHack]);
    }
    d[row] = diagOut(sum, invert);
}

template <typename T>
static void hdiaDiag(spgpuHandle_t handle, T* d, const T* dM, const int* offsets, int hackSize, const int* hackOffsets, int rows,
                     int cols, int invert)
{
    if (rows <= 0 || hackSize <= 0)
        return;
    hipLaunchKernelGGL((hdiaDiagKernel<T>), dim3((unsigned)ceilDiv(rows, kDiagThreads)), dim3(kDiagThreads), 0, handle->currentStream,
                       d, dM, offsets, hackSize, hackOffsets, rows, cols, invert);
    spgpuDebugCheck(handle, "hdiaDiag");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

#define SPGPU_DIAG(L, T)                                                                                                  \
    void spgpu##L##hellDiag(spgpuHandle_t h, T* d, const T* cM, const int* rP, int hackSize, const int* hackOffsets,      \
                            const int* rS, int rows, int baseIndex, int invert)                                           \
    { hellDiag<T>(h, d, cM, rP, hackSize, hackOffsets, rS, rows, baseIndex, invert); }                                    \
    void spgpu##L##ellDiag(spgpuHandle_t h, T* d, const T* cM, const int* rP, int cMPitch, int rPPitch, const int* rS,    \
                           int maxNnzPerRow, int rows, int baseIndex, int invert)                                         \
    { ellDiagOf<T>(h, d, cM, rP, cMPitch, rPPitch, rS, maxNnzPerRow, rows, baseIndex, invert); }                          \
    void spgpu##L##hdiaDiag(spgpuHandle_t h, T* d, const T* dM, const int* offsets, int hackSize, const int* hackOffsets, \
                            int rows, int cols, int invert)                                                               \
    { hdiaDiag<T>(h, d, dM, offsets, hackSize, hackOffsets, rows, cols, invert); }

SPGPU_DIAG(S, float)
SPGPU_DIAG(D, double)

} // extern "C"
