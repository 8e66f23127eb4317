/*
 * HDIA / DIA SpMM on pitch-layout multivectors for gfx950 (MI355X):  Z_j = alpha*A*X_j + beta*Y_j,  j < count,
 * vector j at base + j*pitch.
 *
 * C ABI: spgpu{S,D}hdiaspmmMv, spgpu{S,D}diaspmmMv (include/spgpu/ext/hdia_spmm.h).  No counterpart in the reference.
 *
 * ---- Wavefront design -------------------------------------------------------
 * hdiaSpmvKernel (hdia_spmv.hip) with V vectors per pass.  A lane owns a strip of RPL = 16 B / sizeof(T) consecutive rows
 * (RPL 1 where dM or hackSize do not allow 16-byte coefficient loads), a wavefront 64*RPL consecutive rows.  A stage of
 * UNROLL diagonals loads its coefficient packs and its offsets ONCE -- one stage ahead, non-temporal -- and uses them for
 * all V vectors: V x loads per diagonal, sum[V][RPL] accumulators.  The column of a slot is offsets[d] + row whatever the
 * vector, so the masks of a slot, and the wave-uniform choice between one element-aligned 16-byte x load per strip and
 * element loads at the edges of the matrix, are computed once per diagonal and hold for every vector: an element-aligned
 * load does not care where pitchX puts vector j.  No cross-lane reduction, no LDS, no barrier; per (row, vector) the
 * products are added in ascending stored diagonal with the SpMV's multiply-add and epilogue: the SpMV's bits.
 *
 * A pass of `nvec` < V vectors (3 in the kernel for 4; 5, 6, 7 in the kernel for 8) reads the last live vector of X again
 * for the absent ones -- an address the caller owns, served by the L1 -- and stores nothing for them.
 *
 * Roofline: HBM bandwidth.  Algorithmic bytes per pass: the matrix once (sizeof(T) per stored in-range slot, 4 per stored
 * diagonal, 4 per hack), and per vector sizeof(T) per column and per row [+ y when beta != 0].
 */
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/dia.h"
#include "spgpu/ext/hdia_spmm.h"
#include "spgpu/hdia.h"

#include <stdlib.h>

namespace spgpu {

template <typename T> struct HdiaMmArgs {
    T* z;
    const T* y;
    const T* x;
    const T* dM;
    const int* offsets;
    const int* hackOffsets; /* NULL: plain DIA -- one hack holding all rows, `flatDiags` diagonals */
    T alpha, beta;
    long long pitchX, pitchYZ; /* elements */
    int rows, cols, hackSize;
    int flatDiags;
    int wideIO;
    int nvec; /* 1 .. V: the vectors of this pass */
};

constexpr int kHdiaMmThreads = 512; /* as kHdiaThreads */
constexpr int kHdiaMmMaxV = 8;      /* vectors of a full pass */

/* Diagonals per stage.  The x packs of a stage are all in flight before its first multiply-add: UNROLL * V packs of 16 bytes
 * per lane.  4 * 1 is the SpMV's own stage.  8 vectors: 2 diagonals need 128 VGPRs with doubles (4 wavefronts per SIMD, as 1
 * diagonal would have with half the loads in flight) but 144 with floats (2 resident, workgroups being 8 wavefronts): 1 there. */
template <typename T, int V> constexpr int hdiaMmUnroll() { return V <= 2 ? 4 : V <= 4 || sizeof(T) == 8 ? 2 : 1; }

template <typename T, int RPL, int V>
__global__ __launch_bounds__(kHdiaMmThreads) void hdiaSpmmMvKernel(const HdiaMmArgs<T> a)
{
    constexpr int UNROLL = hdiaMmUnroll<T, V>();
    constexpr bool NT = true; /* coefficients are streamed once per pass */
    const long long strip = (long long)blockIdx.x * kHdiaMmThreads + threadIdx.x;
    const long long waveRow0 = (strip - (threadIdx.x & (kWave - 1))) * RPL;
    if (waveRow0 >= a.rows)
        return; /* whole wavefront leaves together */

    const long long row0 = strip * RPL;
    const bool live = row0 < a.rows;

    int firstDiag = 0, diags = 0;
    long long slab = 0;
    if (live) {
        if (a.hackOffsets) {
            const unsigned r0 = (unsigned)row0, hs = (unsigned)a.hackSize;
            const unsigned hack = r0 / hs;
            firstDiag = a.hackOffsets[hack];
            diags = a.hackOffsets[hack + 1] - firstDiag;
            slab = (long long)firstDiag * hs + (r0 - hack * hs);
        } else { /* DIA: dM[row + d*pitch], every row sees every stored diagonal */
            diags = a.flatDiags;
            slab = row0;
        }
    }
    const int waveDiags = waveMax(diags); /* wave-uniform trip count */
    const bool stripInside = row0 + RPL <= a.rows;

    T sum[V][RPL];
#pragma unroll
    for (int j = 0; j < V; ++j)
#pragma unroll
        for (int t = 0; t < RPL; ++t)
            sum[j][t] = zeroOf<T>();

    const T* __restrict__ vals = a.dM + slab;
    const int* __restrict__ offs = a.offsets + firstDiag;
    /* vector j of X; an absent vector of a partial pass reads the last live one again */
    const T* __restrict__ xj[V];
#pragma unroll
    for (int j = 0; j < V; ++j)
        xj[j] = a.x + (long long)(j < a.nvec ? j : a.nvec - 1) * a.pitchX;

    /* coefficients and offsets of a stage are requested one stage ahead, once for all vectors */
    Pack<T, RPL> v[UNROLL], vNext[UNROLL];
    int off[UNROLL], offNext[UNROLL];
    auto fetch = [&](int dBase, Pack<T, RPL>* vv, int* oo) {
        /* a full stage everywhere in the wavefront: its UNROLL offsets are consecutive ints, one element-aligned load */
        const bool whole = __ballot(dBase + UNROLL > diags) == 0ull;
        if (whole) {
            const Pack<int, UNROLL> o = loadPackElementAligned<int, UNROLL>(offs + dBase);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                vv[u] = loadPack<NT, T, RPL>(vals + (long long)(dBase + u) * a.hackSize);
                oo[u] = o.v[u];
            }
            return;
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            if (dBase + u < diags) {
                vv[u] = loadPack<NT, T, RPL>(vals + (long long)(dBase + u) * a.hackSize);
                oo[u] = offs[dBase + u];
            } else {
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    vv[u].v[t] = zeroOf<T>();
                oo[u] = 0;
            }
        }
    };
    fetch(0, v, off);
    for (int dBase = 0; dBase < waveDiags; dBase += UNROLL) {
        if (dBase + UNROLL < waveDiags) /* wave-uniform */
            fetch(dBase + UNROLL, vNext, offNext);
        Pack<T, RPL> xv[UNROLL][V];
        bool use[UNROLL][RPL];
        bool ragged = false; /* a live diagonal whose strip crosses an edge of the matrix */
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const long long col0 = row0 + off[u];
            const bool dLive = dBase + u < diags;
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                const long long col = col0 + t;
                use[u][t] = dLive && row0 + t < a.rows && col >= 0 && col < a.cols;
            }
            ragged |= dLive && !(stripInside && col0 >= 0 && col0 + RPL <= a.cols);
        }
        /* Wavefront-uniform choice, the same for every vector: when no strip of the wavefront crosses an edge, the RPL
         * consecutive columns of a strip are ONE 16-byte load per vector, aligned to the element size only. */
        if (RPL > 1 && a.cols >= RPL && __ballot(ragged) == 0ull) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long at = dBase + u < diags ? row0 + off[u] : 0;
#pragma unroll
                for (int j = 0; j < V; ++j)
                    xv[u][j] = loadPackElementAligned<T, RPL>(xj[j] + at);
            }
        } else {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u)
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    const long long at = use[u][t] ? row0 + off[u] + t : 0;
#pragma unroll
                    for (int j = 0; j < V; ++j)
                        xv[u][j].v[t] = xj[j][at];
                }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j)
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    sum[j][t] = pick(use[u][t], mulAdd(v[u].v[t], xv[u][j].v[t], sum[j][t]), sum[j][t]);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            v[u] = vNext[u];
            off[u] = offNext[u];
        }
    }

    if (!live)
        return;

    const bool hasBeta = isNotZero(a.beta);
    const bool widePack = a.wideIO && stripInside;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (j >= a.nvec) /* wave-uniform */
            break;
        T* __restrict__ z = a.z + (long long)j * a.pitchYZ;
        const T* __restrict__ y = a.y + (long long)j * a.pitchYZ; /* not read unless hasBeta */
        if (widePack) {
            Pack<T, RPL> out;
            if (hasBeta) {
                const Pack<T, RPL> yv = loadPack<false, T, RPL>(y + row0);
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    out.v[t] = epilogue<true>(a.alpha, sum[j][t], a.beta, yv.v[t]);
            } else {
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    out.v[t] = epilogue<false>(a.alpha, sum[j][t], a.beta, zeroOf<T>());
            }
            storePackMaybeNT<NT, T, RPL>(z + row0, out); /* z is written once and not read again by this call */
        } else {
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                if (row0 + t < a.rows)
                    z[row0 + t] = hasBeta ? epilogue<true>(a.alpha, sum[j][t], a.beta, y[row0 + t])
                                          : epilogue<false>(a.alpha, sum[j][t], a.beta, zeroOf<T>());
            }
        }
    }
}

template <typename T, int RPL, int V>
static void launchHdiaMm(hipStream_t stream, const HdiaMmArgs<T>& a)
{
    const long long strips = ((long long)a.rows + RPL - 1) / RPL;
    const unsigned blocks = (unsigned)((strips + kHdiaMmThreads - 1) / kHdiaMmThreads);
    hipLaunchKernelGGL((hdiaSpmmMvKernel<T, RPL, V>), dim3(blocks), dim3(kHdiaMmThreads), 0, stream, a);
}

/* One pass of a.nvec vectors in the smallest kernel that holds them: 1, 2, 4 or 8. */
template <typename T, int RPL>
static void launchHdiaMmPass(hipStream_t stream, const HdiaMmArgs<T>& a)
{
    if (a.nvec <= 1)
        launchHdiaMm<T, RPL, 1>(stream, a);
    else if (a.nvec <= 2)
        launchHdiaMm<T, RPL, 2>(stream, a);
    else if (a.nvec <= 4)
        launchHdiaMm<T, RPL, 4>(stream, a);
    else
        launchHdiaMm<T, RPL, kHdiaMmMaxV>(stream, a);
}

template <typename T>
static void hdiaSpmmMv(spgpuHandle_t handle, T* z, const T* y, T alpha, const T* dM, const int* offsets, int hackSize,
                       const int* hackOffsets, int rows, int cols, const T* x, T beta, int flatDiags, int count,
                       int pitchX, int pitchYZ)
{
    HdiaMmArgs<T> a;
    a.dM = dM;
    a.offsets = offsets;
    a.hackOffsets = hackOffsets;
    a.alpha = alpha;
    a.beta = y ? beta : zeroOf<T>(); /* Y == NULL: not read */
    a.pitchX = pitchX;
    a.pitchYZ = pitchYZ;
    a.rows = rows;
    a.cols = cols;
    a.hackSize = hackSize;
    a.flatDiags = flatDiags;

    constexpr int WIDE = 16 / (int)sizeof(T);
    const bool wideOk = hackSize % WIDE == 0 && ((uintptr_t)dM % 16 == 0);
    /* every vector of Y and Z on a 16-byte boundary (a NULL Y is on one) */
    a.wideIO = !wideOk || (((uintptr_t)z % 16 == 0) && ((uintptr_t)y % 16 == 0) && ((size_t)pitchYZ * sizeof(T)) % 16 == 0);

    hipStream_t stream = handle->currentStream;
    for (int first = 0; first < count; first += kHdiaMmMaxV) {
        a.nvec = count - first < kHdiaMmMaxV ? count - first : kHdiaMmMaxV;
        a.z = z + (long long)first * pitchYZ;
        a.y = y ? y + (long long)first * pitchYZ : nullptr;
        a.x = x + (long long)first * pitchX;
        if (wideOk)
            launchHdiaMmPass<T, WIDE>(stream, a);
        else
            launchHdiaMmPass<T, 1>(stream, a);
    }
    spgpuDebugCheck(handle, "hdiaspmmMv");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* count <= 0, rows <= 0, hackSize <= 0: returned before anything touches the handle; count == 1 is the SpMV itself */

void spgpuShdiaspmmMv(spgpuHandle_t handle, float* Z, const float* Y, float alpha, const float* dM, const int* offsets,
                      int hackSize, const int* hackOffsets, int rows, int cols, const float* X, float beta, int count,
                      int pitchX, int pitchYZ)
{
    if (count <= 0 || rows <= 0 || hackSize <= 0)
        return;
    if (count == 1)
        return spgpuShdiaspmv(handle, Z, Y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, X, Y ? beta : 0);
    hdiaSpmmMv<float>(handle, Z, Y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, X, beta, 0, count, pitchX, pitchYZ);
}

void spgpuDhdiaspmmMv(spgpuHandle_t handle, double* Z, const double* Y, double alpha, const double* dM, const int* offsets,
                      int hackSize, const int* hackOffsets, int rows, int cols, const double* X, double beta, int count,
                      int pitchX, int pitchYZ)
{
    if (count <= 0 || rows <= 0 || hackSize <= 0)
        return;
    if (count == 1)
        return spgpuDhdiaspmv(handle, Z, Y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, X, Y ? beta : 0);
    hdiaSpmmMv<double>(handle, Z, Y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, X, beta, 0, count, pitchX, pitchYZ);
}

/* DIA: the same kernel over one all-rows hack, hackSize = dMPitch, hackOffsets = NULL */

void spgpuSdiaspmmMv(spgpuHandle_t handle, float* Z, const float* Y, float alpha, const float* dM, const int* offsets,
                     int dMPitch, int rows, int cols, int diags, const float* X, float beta, int count, int pitchX,
                     int pitchYZ)
{
    if (count <= 0 || rows <= 0 || dMPitch <= 0)
        return;
    if (count == 1)
        return spgpuSdiaspmv(handle, Z, Y, alpha, dM, offsets, dMPitch, rows, cols, diags, X, Y ? beta : 0);
    hdiaSpmmMv<float>(handle, Z, Y, alpha, dM, offsets, dMPitch, nullptr, rows, cols, X, beta, diags, count, pitchX, pitchYZ);
}

void spgpuDdiaspmmMv(spgpuHandle_t handle, double* Z, const double* Y, double alpha, const double* dM, const int* offsets,
                     int dMPitch, int rows, int cols, int diags, const double* X, double beta, int count, int pitchX,
                     int pitchYZ)
{
    if (count <= 0 || rows <= 0 || dMPitch <= 0)
        return;
    if (count == 1)
        return spgpuDdiaspmv(handle, Z, Y, alpha, dM, offsets, dMPitch, rows, cols, diags, X, Y ? beta : 0);
    hdiaSpmmMv<double>(handle, Z, Y, alpha, dM, offsets, dMPitch, nullptr, rows, cols, X, beta, diags, count, pitchX, pitchYZ);
}

} // extern "C"
