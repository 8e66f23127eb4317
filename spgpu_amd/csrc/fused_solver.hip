/*
 * Fused steps of a Krylov iteration on small systems, for gfx950 (MI355X).
 *
 * C ABI: spgpu{S,D}hellspmvDotDevice, spgpu{S,D}axpbyPairDotDevice (include/spgpu/device_scalars.h),
 * spgpu{S,D}maxpbyPairDotDevice (include/spgpu/ext/device_scalars_mv.h) and the Jacobi steps spgpu{S,D}axyDotDevice,
 * spgpu{S,D}axpbyPairAxyDotDevice and their m-forms (include/spgpu/ext/precond.h).  NEW: the
 * reference has no fused calls; a CG iteration written with it is hellspmv + dot + 2 axpby + dot + axpby, each
 * reduction a host round trip (vector.h:61-120, ddot.cu:120-150).  On the 1024 x 1024 Laplacian (BASELINE
 * configs[0]) every one of those kernels moves 8-60 MB that sit in the Infinity Cache: the iteration is bound by
 * the number of dependent launches, not by bytes.  These two calls take three launches and two re-reads of a vector
 * out of it.
 *
 * Both kernels ARE the first stage of the dot (reduce.hip.h: same grid, same element -> lane mapping, same order of
 * additions) with the second operand produced on the fly:
 *   hellspmvDot   element i of the second operand = row i of alpha*A*x + beta*y, computed by the lane that owns
 *                 element i of the dot and stored to z; the row sum runs over the row's entries in ascending
 *                 k (the reference's one-thread-per-row order, hell_spmv_base_template.cuh:104-215);
 *   axpbyPairDot  element i = y2[i] - a*x2[i] (stored to z2), next to z1 = y1 + a*x1.
 * So *result has the bits spgpu?dotDevice / spgpu?dot would return for the stored vectors, and z the bits of
 * orc_?hellspmv with one phase -- which are spgpu?hellspmv's own bits whenever its wavefronts do not switch to the
 * cooperative tail (rows of even length, e.g. every stencil).
 *
 * Roofline: HBM / Infinity Cache.  Algorithmic bytes: hellspmvDot = the SpMV's + n*sizeof(T) when w != x;
 * axpbyPairDot = 6*n*sizeof(T).
 */
#include "reduce.hip.h"

#include "spgpu/device_scalars.h"
#include "spgpu/ext/device_scalars_mv.h"
#include "spgpu/ext/precond.h"

namespace spgpu {

template <typename T> struct FusedSpmvArgs {
    T* partials;
    T* z;
    const T* y;
    const T* cM;
    const int* rP;
    const int* hackOffsets;
    const int* rS;
    const T* x;
    const T* w;
    T alpha, beta;
    int hackSize, rows, baseIndex;
};

/* Row sums of VEC consecutive rows (first row `row`, all inside one hack when PACKED) in ascending k. */
template <typename T, int VEC, bool PACKED>
__device__ inline void rowSums(const FusedSpmvArgs<T>& a, long long row, bool live, T (&sum)[VEC])
{
    int len[VEC];
    long long slot[VEC];
    int longest = 0;
#pragma unroll
    for (int t = 0; t < VEC; ++t) {
        sum[t] = zeroOf<T>();
        len[t] = 0;
        slot[t] = 0;
    }
    if (live) {
        if constexpr (PACKED) {
            const Pack<int, VEC> l = loadPack<false, int, VEC>(a.rS + row);
            const long long first = (long long)a.hackOffsets[row / a.hackSize] + row % a.hackSize;
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                len[t] = l.v[t];
                slot[t] = first + t;
            }
        } else {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const long long r = row + t;
                len[t] = a.rS[r];
                slot[t] = (long long)a.hackOffsets[r / a.hackSize] + r % a.hackSize;
            }
        }
#pragma unroll
        for (int t = 0; t < VEC; ++t)
            longest = len[t] > longest ? len[t] : longest;
    }
    for (int k = 0; k < longest; ++k) {
        T value[VEC];
        int column[VEC];
        if constexpr (PACKED) {
            const long long s = slot[0] + (long long)k * a.hackSize;
            const Pack<T, VEC> v = loadPack<false, T, VEC>(a.cM + s);
            const Pack<int, VEC> c = loadPack<false, int, VEC>(a.rP + s);
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                value[t] = v.v[t];
                column[t] = c.v[t];
            }
        } else {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const long long s = slot[t] + (long long)k * a.hackSize;
                const bool in = k < len[t];
                value[t] = in ? a.cM[s] : zeroOf<T>();
                column[t] = in ? a.rP[s] : a.baseIndex;
            }
        }
        /* neighbouring rows of a stencil or a band name neighbouring columns: then the VEC values of x are ONE load
         * (wavefront-uniform choice; the same values either way) */
        bool strip = PACKED && VEC > 1;
        if constexpr (PACKED && VEC > 1) {
            bool mine = column[0] - a.baseIndex >= 0;
#pragma unroll
            for (int t = 0; t < VEC; ++t)
                mine = mine && k < len[t] && column[t] == column[0] + t;
            strip = __ballot(!mine && k < longest) == 0ull;
        }
        if (strip) {
            const Pack<T, VEC> xs = loadPackElementAligned<T, VEC>(a.x + (k < longest ? column[0] - a.baseIndex : 0));
#pragma unroll
            for (int t = 0; t < VEC; ++t)
                if (k < len[t])
                    sum[t] = mulAdd(value[t], xs.v[t], sum[t]);
        } else {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const int col = column[t] - a.baseIndex;
                const bool use = k < len[t] && col >= 0;
                const T xv = a.x[use ? col : 0];
                if (use)
                    sum[t] = mulAdd(value[t], xv, sum[t]);
            }
        }
    }
}

template <typename T, int VEC, bool PACKED, bool HAS_BETA>
__global__ __launch_bounds__(kL1Threads) void hellSpmvDotKernel(FusedSpmvArgs<T> a)
{
    __shared__ T lds[kL1Threads / kWave];
    T acc = zeroOf<T>();
    const long long packs = a.rows / VEC;
    constexpr long long TILE = (long long)kL1Threads * kL1Unroll;
    for (long long base = (long long)blockIdx.x * TILE; base < packs; base += (long long)gridDim.x * TILE) {
        T sums[kL1Unroll][VEC];
        Pack<T, VEC> wv[kL1Unroll], yv[kL1Unroll];
        bool live[kL1Unroll];
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            const long long p = base + u * kL1Threads + threadIdx.x;
            live[u] = p < packs;
            if (live[u]) {
                wv[u] = loadPack<false, T, VEC>(a.w + p * VEC);
                if constexpr (HAS_BETA)
                    yv[u] = loadPackElementAligned<T, VEC>(a.y + p * VEC);
            }
        }
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u)
            rowSums<T, VEC, PACKED>(a, (base + u * kL1Threads + threadIdx.x) * VEC, live[u], sums[u]);
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            if (live[u]) {
                Pack<T, VEC> out;
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    out.v[t] = epilogue<HAS_BETA>(a.alpha, sums[u][t], a.beta, HAS_BETA ? yv[u].v[t] : zeroOf<T>());
                    acc = mulAdd(wv[u].v[t], out.v[t], acc);
                }
                storePack<T, VEC>(a.z + (base + u * kL1Threads + threadIdx.x) * VEC, out);
            }
        }
    }
    const long long tail = packs * VEC + (long long)blockIdx.x * kL1Threads + threadIdx.x;
    if (tail < a.rows) {
        T sum[1];
        rowSums<T, 1, false>(a, tail, true, sum);
        const T out = epilogue<HAS_BETA>(a.alpha, sum[0], a.beta, HAS_BETA ? a.y[tail] : zeroOf<T>());
        acc = mulAdd(a.w[tail], out, acc);
        a.z[tail] = out;
    }
    const T total = blockCombine<kDot>(acc, lds);
    if (threadIdx.x == 0)
        a.partials[blockIdx.x] = total;
}

/* The grid of all three calls is that of the dot they replace (level1.hip reduceFirstStage), without its non-temporal kernel. */
template <typename T>
static void hellSpmvDot(spgpuHandle_t handle, T* result, const T* w, T* z, const T* y, T alpha, const T* cM, const int* rP,
                        int hackSize, const int* hackOffsets, const int* rS, int rows, const T* x, T beta, int baseIndex)
{
    hipStream_t s = handle->currentStream;
    FusedSpmvArgs<T> a;
    a.partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    a.z = z;
    a.y = y;
    a.cM = cM;
    a.rP = rP;
    a.hackOffsets = hackOffsets;
    a.rS = rS;
    a.x = x;
    a.w = w ? w : x;
    a.alpha = alpha;
    a.beta = beta;
    a.hackSize = hackSize;
    a.rows = rows;
    a.baseIndex = baseIndex;
    long long blocks = 0;
    if (rows > 0) {
        const L1Grid g = reduceGrid(sizeof(T), rows, 1, 0, a.w, z, false, SPGPU_REDUCE_MAX_BLOCKS); /* the dot's operands are w and z */
        blocks = g.blocks;
        withConstants([&](auto wide, auto packed, auto hasBeta) {
            hipLaunchKernelGGL((hellSpmvDotKernel<T, wide ? wideOf(sizeof(T)) : 1, wide && packed, hasBeta>), dim3((unsigned)blocks),
                               dim3(kL1Threads), 0, s, a);
        }, g.wide, packedRows(sizeof(T), g.wide, hackSize, cM, rP, rS), isNotZero(beta));
    }
    hipLaunchKernelGGL((reduceFinalKernel<T, kDot>), dim3(1), dim3(kWave), 0, s, result, a.partials, (int)blocks);
    spgpuDebugCheck(handle, "hellspmvDotDevice");
}

/* z1 = y1 + a*x1, z2 = y2 - a*x2, partial sums of z2 . z2; a = *alphaNum / *alphaDen.
 * Arithmetic of axpbyDeviceKernel with beta = 1 (level1.hip): fma(a, x, 1*y) and fma(-a, x, 1*y). */
template <typename T, int VEC>
__device__ inline T axpbyPairDotBlock(int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2, const T* x2, T up, T* lds)
{
    const T down = -up, one = T(1);
    T acc = zeroOf<T>();
    const long long packs = n / VEC;
    constexpr long long TILE = (long long)kL1Threads * kL1Unroll;
    for (long long base = (long long)blockIdx.x * TILE; base < packs; base += (long long)gridDim.x * TILE) {
        Pack<T, VEC> a1[kL1Unroll], b1[kL1Unroll], a2[kL1Unroll], b2[kL1Unroll];
        bool live[kL1Unroll];
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            const long long p = base + u * kL1Threads + threadIdx.x;
            live[u] = p < packs;
            if (live[u]) {
                a2[u] = loadPackElementAligned<T, VEC>(x2 + p * VEC);
                b2[u] = loadPackElementAligned<T, VEC>(y2 + p * VEC);
                a1[u] = loadPackElementAligned<T, VEC>(x1 + p * VEC);
                b1[u] = loadPackElementAligned<T, VEC>(y1 + p * VEC);
            }
        }
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            if (live[u]) {
                const long long p = base + u * kL1Threads + threadIdx.x;
                Pack<T, VEC> o1, o2;
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    o2.v[t] = mulAdd(down, a2[u].v[t], one * b2[u].v[t]);
                    o1.v[t] = mulAdd(up, a1[u].v[t], one * b1[u].v[t]);
                    acc = mulAdd(o2.v[t], o2.v[t], acc);
                }
                storePack<T, VEC>(z2 + p * VEC, o2);
                storePackElementAligned<T, VEC>(z1 + p * VEC, o1);
            }
        }
    }
    const long long tail = packs * VEC + (long long)blockIdx.x * kL1Threads + threadIdx.x;
    if (tail < n) {
        const T o2 = mulAdd(down, x2[tail], one * y2[tail]);
        z1[tail] = mulAdd(up, x1[tail], one * y1[tail]);
        z2[tail] = o2;
        acc = mulAdd(o2, o2, acc);
    }
    return blockCombine<kDot>(acc, lds);
}

template <typename T, int VEC>
__global__ __launch_bounds__(kL1Threads) void axpbyPairDotKernel(T* partials, int n, T* z1, const T* y1, const T* x1, T* z2,
                                                                const T* y2, const T* x2, const T* alphaNum,
                                                                const T* alphaDen)
{
    __shared__ T lds[kL1Threads / kWave];
    const T total = axpbyPairDotBlock<T, VEC>(n, z1, y1, x1, z2, y2, x2, quotientAt(alphaNum, alphaDen), lds);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = total;
}

/* The same on the vectors of a pitch multivector (spgpu/ext/device_scalars_mv.h): grid (blocks, vectors) of the first stage of
 * spgpu?mdotDevice(result, n, z2, z2, count, pitch); vector blockIdx.y takes element blockIdx.y of alphaNum / alphaDen. */
template <typename T, int VEC>
__global__ __launch_bounds__(kL1Threads) void axpbyPairDotMvKernel(T* partials, int n, T* z1, const T* y1, const T* x1, T* z2,
                                                                  const T* y2, const T* x2, const T* alphaNum,
                                                                  const T* alphaDen, long long pitch)
{
    __shared__ T lds[kL1Threads / kWave];
    const long long shift = (long long)blockIdx.y * pitch;
    const T up = quotientAt(alphaNum ? alphaNum + blockIdx.y : nullptr, alphaDen ? alphaDen + blockIdx.y : nullptr);
    const T total = axpbyPairDotBlock<T, VEC>(n, z1 + shift, y1 + shift, x1 + shift, z2 + shift, y2 + shift, x2 + shift, up, lds);
    if (threadIdx.x == 0)
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

template <typename T>
static void axpbyPairDot(spgpuHandle_t handle, T* result, int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2,
                         const T* x2, const T* alphaNum, const T* alphaDen)
{
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    long long blocks = 0;
    if (n > 0) {
        const L1Grid g = reduceGrid(sizeof(T), n, 1, 0, z2, z2, false, SPGPU_REDUCE_MAX_BLOCKS); /* both operands of the dot are z2 */
        blocks = g.blocks;
        withConstants([&](auto wide) {
            hipLaunchKernelGGL((axpbyPairDotKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)blocks), dim3(kL1Threads), 0, s,
                               partials, n, z1, y1, x1, z2, y2, x2, alphaNum, alphaDen);
        }, g.wide);
    }
    hipLaunchKernelGGL((reduceFinalKernel<T, kDot>), dim3(1), dim3(kWave), 0, s, result, partials, (int)blocks);
    spgpuDebugCheck(handle, "axpbyPairDotDevice");
}

/* Passes, grid and `wide` of spgpu?mdotDevice on (z2, z2) (level1.hip reduceVectorsToDevice), the first stage replaced. */
template <typename T>
static void axpbyPairDotMv(spgpuHandle_t handle, T* result, int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2,
                           const T* x2, const T* alphaNum, const T* alphaDen, int count, int pitch)
{
    if (count <= 0)
        return;
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    forEachPass(count, kReduceMaxVectorsPerPass, [&](int first, int vectors) {
        const size_t shift = (size_t)first * pitch;
        long long blocks = 0;
        if (n > 0) {
            const L1Grid g = reduceGrid(sizeof(T), n, vectors, pitch, z2 + shift, z2 + shift, false, SPGPU_REDUCE_MAX_BLOCKS);
            blocks = g.blocks;
            withConstants([&](auto wide) {
                hipLaunchKernelGGL((axpbyPairDotMvKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)blocks, (unsigned)vectors),
                                   dim3(kL1Threads), 0, s, partials, n, z1 + shift, y1 + shift, x1 + shift, z2 + shift, y2 + shift,
                                   x2 + shift, alphaNum ? alphaNum + first : nullptr, alphaDen ? alphaDen + first : nullptr,
                                   (long long)pitch);
            }, g.wide);
        }
        hipLaunchKernelGGL((reduceFinalBatchKernel<T, kDot>), dim3((unsigned)vectors), dim3(kWave), 0, s, result + first,
                           partials, (int)blocks);
    });
    spgpuDebugCheck(handle, "maxpbyPairDotDevice");
}

/* ---- the Jacobi step of PCG inside the same passes (include/spgpu/ext/precond.h) ------------------------------------------------
 * z = d o r with the arithmetic of mapKernel<kAxy> at alpha = 1 (level1.hip: 1 * (d * r)), r . z added as the first stage of
 * spgpu?dotDevice(result, n, r, z) adds it.  r and z are the dot's operands and decide VEC; d is an extra stream, read
 * element-aligned wherever it lies. */
template <typename T> __device__ inline T axyOne(T d, T r) { return mul(T(1), mul(d, r)); }

template <typename T, int VEC> __device__ inline T axyDotBlock(int n, T* z, const T* d, const T* r, T* lds)
{
    T acc = zeroOf<T>();
    const long long packs = n / VEC;
    constexpr long long TILE = (long long)kL1Threads * kL1Unroll;
    for (long long base = (long long)blockIdx.x * TILE; base < packs; base += (long long)gridDim.x * TILE) {
        Pack<T, VEC> rv[kL1Unroll], dv[kL1Unroll];
        bool live[kL1Unroll];
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            const long long p = base + u * kL1Threads + threadIdx.x;
            live[u] = p < packs;
            if (live[u]) {
                rv[u] = loadPack<false, T, VEC>(r + p * VEC);
                dv[u] = loadPackElementAligned<T, VEC>(d + p * VEC);
            }
        }
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            if (live[u]) {
                Pack<T, VEC> out;
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    out.v[t] = axyOne(dv[u].v[t], rv[u].v[t]);
                    acc = mulAdd(rv[u].v[t], out.v[t], acc);
                }
                storePack<T, VEC>(z + (base + u * kL1Threads + threadIdx.x) * VEC, out);
            }
        }
    }
    const long long tail = packs * VEC + (long long)blockIdx.x * kL1Threads + threadIdx.x;
    if (tail < n) {
        const T out = axyOne(d[tail], r[tail]);
        acc = mulAdd(r[tail], out, acc);
        z[tail] = out;
    }
    return blockCombine<kDot>(acc, lds);
}

/* grid (blocks, vectors); one vector: pitch 0 */
template <typename T, int VEC>
__global__ __launch_bounds__(kL1Threads) void axyDotKernel(T* partials, int n, T* z, const T* d, const T* r, long long pitch)
{
    __shared__ T lds[kL1Threads / kWave];
    const long long shift = (long long)blockIdx.y * pitch;
    const T total = axyDotBlock<T, VEC>(n, z + shift, d + shift, r + shift, lds);
    if (threadIdx.x == 0)
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

/* axpbyPairDotBlock with w = d o z2 stored and z2 . w added beside z2 . z2, from the z2 the lane holds: one more load stream and one
 * store.  z2 is the operand of both dots and decides VEC, as there; x1, y1, z1, d and w go element-aligned.  Returns the block's
 * z2 . z2 (the additions of axpbyPairDotBlock, in its order) and leaves its z2 . w in *zw.  (A function of its own, not a flag of
 * axpbyPairDotBlock: the kernels of plain CG stay the code they were.) */
template <typename T, int VEC>
__device__ inline T axpbyPairAxyDotBlock(int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2, const T* x2, T* w, const T* d,
                                        T up, T* lds, T* zw)
{
    const T down = -up, one = T(1);
    T acc = zeroOf<T>(), accW = zeroOf<T>();
    const long long packs = n / VEC;
    constexpr long long TILE = (long long)kL1Threads * kL1Unroll;
    for (long long base = (long long)blockIdx.x * TILE; base < packs; base += (long long)gridDim.x * TILE) {
        Pack<T, VEC> a1[kL1Unroll], b1[kL1Unroll], a2[kL1Unroll], b2[kL1Unroll], dv[kL1Unroll];
        bool live[kL1Unroll];
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            const long long p = base + u * kL1Threads + threadIdx.x;
            live[u] = p < packs;
            if (live[u]) {
                a2[u] = loadPackElementAligned<T, VEC>(x2 + p * VEC);
                b2[u] = loadPackElementAligned<T, VEC>(y2 + p * VEC);
                dv[u] = loadPackElementAligned<T, VEC>(d + p * VEC);
                a1[u] = loadPackElementAligned<T, VEC>(x1 + p * VEC);
                b1[u] = loadPackElementAligned<T, VEC>(y1 + p * VEC);
            }
        }
#pragma unroll
        for (int u = 0; u < kL1Unroll; ++u) {
            if (live[u]) {
                const long long p = base + u * kL1Threads + threadIdx.x;
                Pack<T, VEC> o1, o2, ow;
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    o2.v[t] = mulAdd(down, a2[u].v[t], one * b2[u].v[t]);
                    o1.v[t] = mulAdd(up, a1[u].v[t], one * b1[u].v[t]);
                    ow.v[t] = axyOne(dv[u].v[t], o2.v[t]);
                    acc = mulAdd(o2.v[t], o2.v[t], acc);
                    accW = mulAdd(o2.v[t], ow.v[t], accW);
                }
                storePack<T, VEC>(z2 + p * VEC, o2);
                storePackElementAligned<T, VEC>(w + p * VEC, ow);
                storePackElementAligned<T, VEC>(z1 + p * VEC, o1);
            }
        }
    }
    const long long tail = packs * VEC + (long long)blockIdx.x * kL1Threads + threadIdx.x;
    if (tail < n) {
        const T o2 = mulAdd(down, x2[tail], one * y2[tail]);
        const T ow = axyOne(d[tail], o2);
        z1[tail] = mulAdd(up, x1[tail], one * y1[tail]);
        z2[tail] = o2;
        w[tail] = ow;
        acc = mulAdd(o2, o2, acc);
        accW = mulAdd(o2, ow, accW);
    }
    *zw = blockCombine<kDot>(accW, lds + kL1Threads / kWave);
    return blockCombine<kDot>(acc, lds);
}

/* grid (blocks, vectors); one vector: pitch 0.  The partials lie as [2][vectors][blocks]: set 0 is z2 . w, set 1 is z2 . z2. */
template <typename T, int VEC>
__global__ __launch_bounds__(kL1Threads) void axpbyPairAxyDotKernel(T* partials, int n, T* z1, const T* y1, const T* x1, T* z2,
                                                                   const T* y2, const T* x2, T* w, const T* d, const T* alphaNum,
                                                                   const T* alphaDen, long long pitch)
{
    __shared__ T lds[2 * (kL1Threads / kWave)];
    const long long shift = (long long)blockIdx.y * pitch;
    const T up = quotientAt(alphaNum ? alphaNum + blockIdx.y : nullptr, alphaDen ? alphaDen + blockIdx.y : nullptr);
    T zw;
    const T zz = axpbyPairAxyDotBlock<T, VEC>(n, z1 + shift, y1 + shift, x1 + shift, z2 + shift, y2 + shift, x2 + shift, w + shift,
                                             d + shift, up, lds, &zw);
    if (threadIdx.x == 0) {
        const size_t at = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[at] = zw;
        partials[(size_t)gridDim.y * gridDim.x + at] = zz;
    }
}

/* Second stage for the two result sets of a multivector: grid (vectors, 2) wavefronts; wavefront (j, set) combines
 * partials[set][j][0 .. blocks) in the order of finalOrder into result[set * setStride + j]. */
template <typename T>
__global__ __launch_bounds__(kWave) void reduceFinalPairBatchKernel(T* result, const T* partials, int blocks, int setStride)
{
    const T sum = finalCombine<kDot>(partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * blocks, blocks);
    if (threadIdx.x == 0)
        result[(size_t)blockIdx.y * setStride + blockIdx.x] = sum;
}

template <typename T> static void axyDot(spgpuHandle_t handle, T* result, int n, T* z, const T* d, const T* r)
{
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    long long blocks = 0;
    if (n > 0) {
        const L1Grid g = reduceGrid(sizeof(T), n, 1, 0, r, z, false, SPGPU_REDUCE_MAX_BLOCKS); /* the dot's operands are r and z */
        blocks = g.blocks;
        withConstants([&](auto wide) {
            hipLaunchKernelGGL((axyDotKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)blocks), dim3(kL1Threads), 0, s, partials, n,
                               z, d, r, 0ll);
        }, g.wide);
    }
    hipLaunchKernelGGL((reduceFinalKernel<T, kDot>), dim3(1), dim3(kWave), 0, s, result, partials, (int)blocks);
    spgpuDebugCheck(handle, "axyDotDevice");
}

/* Passes, grid and `wide` of spgpu?mdotDevice on (r, z). */
template <typename T> static void axyDotMv(spgpuHandle_t handle, T* result, int n, T* z, const T* d, const T* r, int count, int pitch)
{
    if (count <= 0)
        return;
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    forEachPass(count, kReduceMaxVectorsPerPass, [&](int first, int vectors) {
        const size_t shift = (size_t)first * pitch;
        long long blocks = 0;
        if (n > 0) {
            const L1Grid g = reduceGrid(sizeof(T), n, vectors, pitch, r + shift, z + shift, false, SPGPU_REDUCE_MAX_BLOCKS);
            blocks = g.blocks;
            withConstants([&](auto wide) {
                hipLaunchKernelGGL((axyDotKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)blocks, (unsigned)vectors),
                                   dim3(kL1Threads), 0, s, partials, n, z + shift, d + shift, r + shift, (long long)pitch);
            }, g.wide);
        }
        hipLaunchKernelGGL((reduceFinalBatchKernel<T, kDot>), dim3((unsigned)vectors), dim3(kWave), 0, s, result + first, partials,
                           (int)blocks);
    });
    spgpuDebugCheck(handle, "maxyDotDevice");
}

/* The grid is that of z2 . z2 (axpbyPairDot); both sets of block partials, [2][blocks], fill the scratch exactly where the cap binds
 * (2 x SPGPU_REDUCE_MAX_BLOCKS x 8 bytes = SPGPU_REDUCE_SCRATCH_BYTES), and one launch of two wavefronts combines them. */
template <typename T>
static void axpbyPairAxyDot(spgpuHandle_t handle, T* result, int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2,
                            const T* x2, T* w, const T* d, const T* alphaNum, const T* alphaDen)
{
    static_assert(2 * SPGPU_REDUCE_MAX_BLOCKS * sizeof(T) <= SPGPU_REDUCE_SCRATCH_BYTES, "two sets of partials must fit the scratch");
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    long long blocks = 0;
    if (n > 0) {
        const L1Grid g = reduceGrid(sizeof(T), n, 1, 0, z2, z2, false, SPGPU_REDUCE_MAX_BLOCKS);
        blocks = g.blocks;
        withConstants([&](auto wide) {
            hipLaunchKernelGGL((axpbyPairAxyDotKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)blocks), dim3(kL1Threads), 0, s,
                               partials, n, z1, y1, x1, z2, y2, x2, w, d, alphaNum, alphaDen, 0ll);
        }, g.wide);
    }
    hipLaunchKernelGGL((reduceFinalBatchKernel<T, kDot>), dim3(2), dim3(kWave), 0, s, result, partials, (int)blocks);
    spgpuDebugCheck(handle, "axpbyPairAxyDotDevice");
}

/* Passes, grid and `wide` of spgpu?mdotDevice on (z2, z2), as axpbyPairDotMv: result[count + j] keeps the bits of
 * spgpu?maxpbyPairDotDevice for every count.  A pass of `vectors` vectors leaves 2 * vectors * blocks partials with
 * blocks <= SPGPU_REDUCE_MAX_BLOCKS / vectors; the scratch holds 2 * SPGPU_REDUCE_MAX_BLOCKS of them.  Up to
 * kPairAxyMaxVectorsPerLaunch = SPGPU_REDUCE_MAX_BLOCKS / 2 vectors that is at most 2 * SPGPU_REDUCE_MAX_BLOCKS: one launch.  Beyond,
 * blocks is 1 and the pass runs as two launches of at most half the cap's vectors each -- 2 * 512 * 1 partials --, on the grid and
 * the `wide` of the whole pass (a pass of more than one vector is wide only with a pitch that keeps every vector on the boundary,
 * so the second half's are there too). */
constexpr int kPairAxyMaxVectorsPerLaunch = SPGPU_REDUCE_MAX_BLOCKS / 2;

template <typename T>
static void axpbyPairAxyDotMv(spgpuHandle_t handle, T* result, int n, T* z1, const T* y1, const T* x1, T* z2, const T* y2,
                              const T* x2, T* w, const T* d, const T* alphaNum, const T* alphaDen, int count, int pitch)
{
    if (count <= 0)
        return;
    hipStream_t s = handle->currentStream;
    T* partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    forEachPass(count, kReduceMaxVectorsPerPass, [&](int passFirst, int passVectors) {
        L1Grid g = {false, 0, false};
        if (n > 0)
            g = reduceGrid(sizeof(T), n, passVectors, pitch, z2 + (size_t)passFirst * pitch, z2 + (size_t)passFirst * pitch, false,
                           SPGPU_REDUCE_MAX_BLOCKS);
        forEachPass(passVectors, kPairAxyMaxVectorsPerLaunch, [&](int launchFirst, int vectors) {
            const int first = passFirst + launchFirst;
            const size_t shift = (size_t)first * pitch;
            if (n > 0)
                withConstants([&](auto wide) {
                    hipLaunchKernelGGL((axpbyPairAxyDotKernel<T, wide ? wideOf(sizeof(T)) : 1>), dim3((unsigned)g.blocks, (unsigned)vectors),
                                       dim3(kL1Threads), 0, s, partials, n, z1 + shift, y1 + shift, x1 + shift, z2 + shift, y2 + shift,
                                       x2 + shift, w + shift, d + shift, alphaNum ? alphaNum + first : nullptr,
                                       alphaDen ? alphaDen + first : nullptr, (long long)pitch);
                }, g.wide);
            hipLaunchKernelGGL((reduceFinalPairBatchKernel<T>), dim3((unsigned)vectors, 2), dim3(kWave), 0, s, result + first, partials,
                               (int)g.blocks, count);
        });
    });
    spgpuDebugCheck(handle, "maxpbyPairAxyDotDevice");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

void spgpuShellspmvDotDevice(spgpuHandle_t h, float* result, const float* w, float* z, const float* y, float alpha,
                             const float* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS, int rows,
                             const float* x, float beta, int baseIndex)
{ hellSpmvDot<float>(h, result, w, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rows, x, beta, baseIndex); }

void spgpuDhellspmvDotDevice(spgpuHandle_t h, double* result, const double* w, double* z, const double* y, double alpha,
                             const double* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS, int rows,
                             const double* x, double beta, int baseIndex)
{ hellSpmvDot<double>(h, result, w, z, y, alpha, cM, rP, hackSize, hackOffsets, rS, rows, x, beta, baseIndex); }

void spgpuSaxpbyPairDotDevice(spgpuHandle_t h, float* result, int n, float* z1, const float* y1, const float* x1, float* z2,
                              const float* y2, const float* x2, const float* alphaNum, const float* alphaDen)
{ axpbyPairDot<float>(h, result, n, z1, y1, x1, z2, y2, x2, alphaNum, alphaDen); }

void spgpuDaxpbyPairDotDevice(spgpuHandle_t h, double* result, int n, double* z1, const double* y1, const double* x1,
                              double* z2, const double* y2, const double* x2, const double* alphaNum, const double* alphaDen)
{ axpbyPairDot<double>(h, result, n, z1, y1, x1, z2, y2, x2, alphaNum, alphaDen); }

void spgpuSmaxpbyPairDotDevice(spgpuHandle_t h, float* result, int n, float* z1, const float* y1, const float* x1, float* z2,
                               const float* y2, const float* x2, const float* alphaNum, const float* alphaDen, int count, int pitch)
{ axpbyPairDotMv<float>(h, result, n, z1, y1, x1, z2, y2, x2, alphaNum, alphaDen, count, pitch); }

void spgpuDmaxpbyPairDotDevice(spgpuHandle_t h, double* result, int n, double* z1, const double* y1, const double* x1,
                               double* z2, const double* y2, const double* x2, const double* alphaNum, const double* alphaDen,
                               int count, int pitch)
{ axpbyPairDotMv<double>(h, result, n, z1, y1, x1, z2, y2, x2, alphaNum, alphaDen, count, pitch); }

/* ---- include/spgpu/ext/precond.h ---- */
#define SPGPU_PRECOND_STEPS(L, T)                                                                                         \
    void spgpu##L##axyDotDevice(spgpuHandle_t h, T* result, int n, T* z, const T* d, const T* r)                          \
    { axyDot<T>(h, result, n, z, d, r); }                                                                                 \
    void spgpu##L##maxyDotDevice(spgpuHandle_t h, T* result, int n, T* z, const T* d, const T* r, int count, int pitch)   \
    { axyDotMv<T>(h, result, n, z, d, r, count, pitch); }                                                                 \
    void spgpu##L##axpbyPairAxyDotDevice(spgpuHandle_t h, T* result, int n, T* z1, const T* y1, const T* x1, T* z2,       \
                                         const T* y2, const T* x2, T* w, const T* d, const T* alphaNum, const T* alphaDen) \
    { axpbyPairAxyDot<T>(h, result, n, z1, y1, x1, z2, y2, x2, w, d, alphaNum, alphaDen); }                               \
    void spgpu##L##maxpbyPairAxyDotDevice(spgpuHandle_t h, T* result, int n, T* z1, const T* y1, const T* x1, T* z2,      \
                                          const T* y2, const T* x2, T* w, const T* d, const T* alphaNum,                  \
                                          const T* alphaDen, int count, int pitch)                                        \
    { axpbyPairAxyDotMv<T>(h, result, n, z1, y1, x1, z2, y2, x2, w, d, alphaNum, alphaDen, count, pitch); }

SPGPU_PRECOND_STEPS(S, float)
SPGPU_PRECOND_STEPS(D, double)

} // extern "C"

