/*
 * The SpMV + dot step of a captured CG iteration on HDIA and DIA matrices, for gfx950 (MI355X).
 *
 * C ABI: spgpu{S,D}hdiaspmvDotDevice, spgpu{S,D}diaspmvDotDevice (include/spgpu/ext/hdia_solver.h).  NEW: the reference has no
 * fused calls.  The HELL form is hellSpmvDotKernel (fused_solver.hip); this is the same step for the format stencil matrices are
 * kept in, which has no column indices to stream.
 *
 * The kernel IS the first stage of the dot (reduce.hip.h: same grid, same element -> lane mapping, same order of additions) with
 * the second operand produced on the fly: element i of the second operand = row i of alpha*A*x + beta*y, computed by the lane
 * that owns element i of the dot and stored to z.  The fit is natural: hdiaSpmvKernel (hdia_spmv.hip) gives a lane a strip of
 * 16 B / sizeof(T) consecutive rows and lets it walk all diagonals of the strip's hack itself, without a cross-lane step; the
 * dot gives a lane packs of wideOf(sizeof(T)) consecutive elements -- the same width.  A row's products are added in ascending
 * stored diagonal, as on every path of spgpu?hdiaspmv: z has that call's bits for every matrix, *result the bits
 * spgpu?dotDevice / spgpu?dot would return for the stored z.
 *
 * Three paths (level1_grid.h: reduceGrid decides `wide`, packedStrips `packed`):
 *   packed   a pack lies inside one hack and its coefficients are one 16-byte non-temporal load per diagonal; the VEC values of
 *            x at row0 + offsets[d] are one element-aligned 16-byte load unless a strip of the wavefront crosses an edge of the
 *            matrix (wavefront-uniform ballot), element loads under the `use` mask then: the logic of hdiaSpmvKernel, kStage
 *            diagonals per stage, the coefficients and offsets of a stage requested one stage ahead;
 *   wide     the dot's wide mapping, each of the pack's rows walked on its own (hackSize no multiple of VEC, or dM off its
 *            boundary: rows of one pack may lie in two hacks);
 *   narrow   the element mapping (w or z off a 16-byte boundary).
 * The rows beyond packs * VEC go one per lane.  DIA is the same kernel over one hack of all rows: hackOffsets == NULL,
 * `flatDiags` diagonals, slab stride dMPitch.
 *
 * Roofline: HBM / Infinity Cache.  Algorithmic bytes: the SpMV's + rows * sizeof(T) when w != x.
 */
#include "reduce.hip.h"

#include "spgpu/ext/hdia_solver.h"

namespace spgpu {

template <typename T> struct FusedHdiaArgs {
    T* partials;
    T* z;
    const T* y;
    const T* dM;
    const int* offsets;
    const int* hackOffsets; /* NULL: plain DIA -- one hack holding all rows, `flatDiags` diagonals */
    const T* x;
    const T* w;
    T alpha, beta;
    int hackSize, rows, cols, flatDiags;
};

constexpr int kStage = 4; /* diagonals per stage of the packed path, as hdiaSpmvKernel */

/* Row sums of the VEC consecutive rows from row0 (all below a.rows), products added in ascending stored diagonal.  PACKED: the rows
 * lie in one hack and the call is made by every lane of a wavefront together (`live` false: a lane without rows). */
template <typename T, int VEC, bool PACKED>
__device__ inline void stripSums(const FusedHdiaArgs<T>& a, long long row0, bool live, T (&sum)[VEC])
{
#pragma unroll
    for (int t = 0; t < VEC; ++t)
        sum[t] = zeroOf<T>();
    const T* __restrict__ x = a.x;

    if constexpr (PACKED) {
        int firstDiag = 0, diags = 0;
        long long slab = 0;
        if (live) {
            if (a.hackOffsets) {
                const long long hack = row0 / a.hackSize;
                firstDiag = a.hackOffsets[hack];
                diags = a.hackOffsets[hack + 1] - firstDiag;
                slab = (long long)firstDiag * a.hackSize + (row0 - hack * a.hackSize);
            } else {
                diags = a.flatDiags;
                slab = row0;
            }
        }
        const int waveDiags = waveReduce(diags, MaxOf{}); /* wave-uniform trip count */
        const T* __restrict__ vals = a.dM + slab;
        const int* __restrict__ offs = a.offsets + firstDiag;

        /* coefficients and offsets of a stage travel while the x values of the stage before are fetched and used */
        Pack<T, VEC> v[kStage], vNext[kStage];
        int off[kStage], offNext[kStage];
        auto fetch = [&](int dBase, Pack<T, VEC>* vv, int* oo) {
            const bool whole = __ballot(dBase + kStage > diags) == 0ull; /* a full stage everywhere: its offsets are one load */
            if (whole) {
                const Pack<int, kStage> o4 = loadPackElementAligned<int, kStage>(offs + dBase);
#pragma unroll
                for (int u = 0; u < kStage; ++u) {
                    vv[u] = loadPack<true, T, VEC>(vals + (long long)(dBase + u) * a.hackSize);
                    oo[u] = o4.v[u];
                }
                return;
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                if (dBase + u < diags) {
                    vv[u] = loadPack<true, T, VEC>(vals + (long long)(dBase + u) * a.hackSize);
                    oo[u] = offs[dBase + u];
                } else {
#pragma unroll
                    for (int t = 0; t < VEC; ++t)
                        vv[u].v[t] = zeroOf<T>();
                    oo[u] = 0;
                }
            }
        };
        if (waveDiags > 0)
            fetch(0, v, off);
        for (int dBase = 0; dBase < waveDiags; dBase += kStage) {
            if (dBase + kStage < waveDiags) /* wave-uniform */
                fetch(dBase + kStage, vNext, offNext);
            Pack<T, VEC> xv[kStage];
            bool use[kStage][VEC];
            bool ragged = false; /* a live diagonal whose strip crosses an edge of the matrix */
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                const long long col0 = row0 + off[u];
                const bool dLive = dBase + u < diags;
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    use[u][t] = dLive && col0 + t >= 0 && col0 + t < a.cols;
                ragged |= dLive && !(col0 >= 0 && col0 + VEC <= a.cols);
            }
            if (a.cols >= VEC && __ballot(ragged) == 0ull) { /* wavefront-uniform: the same values either way */
#pragma unroll
                for (int u = 0; u < kStage; ++u)
                    xv[u] = loadPackElementAligned<T, VEC>(x + (dBase + u < diags ? row0 + off[u] : 0));
            } else {
#pragma unroll
                for (int u = 0; u < kStage; ++u)
#pragma unroll
                    for (int t = 0; t < VEC; ++t)
                        xv[u].v[t] = use[u][t] ? x[row0 + off[u] + t] : zeroOf<T>();
            }
#pragma unroll
            for (int u = 0; u < kStage; ++u)
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    sum[t] = pick(use[u][t], mulAdd(v[u].v[t], xv[u].v[t], sum[t]), sum[t]);
#pragma unroll
            for (int u = 0; u < kStage; ++u) {
                v[u] = vNext[u];
                off[u] = offNext[u];
            }
        }
    } else {
        int first[VEC], diags[VEC];
        long long slab[VEC];
        int longest = 0;
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
            first[t] = 0;
            diags[t] = 0;
            slab[t] = 0;
        }
        if (live) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const long long r = row0 + t;
                if (a.hackOffsets) {
                    const long long hack = r / a.hackSize;
                    first[t] = a.hackOffsets[hack];
                    diags[t] = a.hackOffsets[hack + 1] - first[t];
                    slab[t] = (long long)first[t] * a.hackSize + (r - hack * a.hackSize);
                } else {
                    diags[t] = a.flatDiags;
                    slab[t] = r;
                }
                longest = diags[t] > longest ? diags[t] : longest;
            }
        }
        for (int d = 0; d < longest; ++d) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                const bool in = d < diags[t];
                const long long col = row0 + t + (in ? a.offsets[first[t] + d] : 0);
                const bool use = in && col >= 0 && col < a.cols;
                const T value = use ? a.dM[slab[t] + (long long)d * a.hackSize] : zeroOf<T>();
                const T xv = use ? x[col] : zeroOf<T>();
                sum[t] = pick(use, mulAdd(value, xv, sum[t]), sum[t]);
            }
        }
    }
}

template <typename T, int VEC, bool PACKED, bool HAS_BETA>
__global__ __launch_bounds__(kL1Threads) void hdiaSpmvDotKernel(const FusedHdiaArgs<T> a)
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
            stripSums<T, VEC, PACKED>(a, (base + u * kL1Threads + threadIdx.x) * VEC, live[u], sums[u]);
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
        stripSums<T, 1, false>(a, tail, true, sum);
        const T out = epilogue<HAS_BETA>(a.alpha, sum[0], a.beta, HAS_BETA ? a.y[tail] : zeroOf<T>());
        acc = mulAdd(a.w[tail], out, acc);
        a.z[tail] = out;
    }
    const T total = blockCombine<kDot>(acc, lds);
    if (threadIdx.x == 0)
        a.partials[blockIdx.x] = total;
}

/* The grid is that of the dot the call replaces (level1.hip reduceFirstStage), without its non-temporal kernel. */
template <typename T>
static void hdiaSpmvDot(spgpuHandle_t handle, T* result, const T* w, T* z, const T* y, T alpha, const T* dM, const int* offsets,
                        int hackSize, const int* hackOffsets, int rows, int cols, const T* x, T beta, int flatDiags)
{
    hipStream_t s = handle->currentStream;
    FusedHdiaArgs<T> a;
    a.partials = static_cast<T*>(spgpuPrivate(handle)->reduceScratch);
    a.z = z;
    a.y = y;
    a.dM = dM;
    a.offsets = offsets;
    a.hackOffsets = hackOffsets;
    a.x = x;
    a.w = w ? w : x;
    a.alpha = alpha;
    a.beta = beta;
    a.hackSize = hackSize;
    a.rows = rows;
    a.cols = cols;
    a.flatDiags = flatDiags;
    long long blocks = 0;
    if (rows > 0 && hackSize > 0) {
        const L1Grid g = reduceGrid(sizeof(T), rows, 1, 0, a.w, z, false, SPGPU_REDUCE_MAX_BLOCKS); /* the dot's operands are w and z */
        blocks = g.blocks;
        withConstants([&](auto wide, auto packed, auto hasBeta) {
            hipLaunchKernelGGL((hdiaSpmvDotKernel<T, wide ? wideOf(sizeof(T)) : 1, wide && packed, hasBeta>), dim3((unsigned)blocks),
                               dim3(kL1Threads), 0, s, a);
        }, g.wide, packedStrips(sizeof(T), g.wide, hackSize, dM), isNotZero(beta));
    }
    hipLaunchKernelGGL((reduceFinalKernel<T, kDot>), dim3(1), dim3(kWave), 0, s, result, a.partials, (int)blocks);
    spgpuDebugCheck(handle, hackOffsets ? "hdiaspmvDotDevice" : "diaspmvDotDevice");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

#define SPGPU_HDIA_SOLVER_STEPS(L, T)                                                                                            \
    void spgpu##L##hdiaspmvDotDevice(spgpuHandle_t h, T* result, const T* w, T* z, const T* y, T alpha, const T* dM,             \
                                     const int* offsets, int hackSize, const int* hackOffsets, int rows, int cols, const T* x,   \
                                     T beta)                                                                                     \
    { hdiaSpmvDot<T>(h, result, w, z, y, alpha, dM, offsets, hackSize, hackOffsets, rows, cols, x, beta, 0); }                   \
    void spgpu##L##diaspmvDotDevice(spgpuHandle_t h, T* result, const T* w, T* z, const T* y, T alpha, const T* dM,              \
                                    const int* offsets, int dMPitch, int rows, int cols, int diags, const T* x, T beta)          \
    { hdiaSpmvDot<T>(h, result, w, z, y, alpha, dM, offsets, dMPitch, nullptr, rows, cols, x, beta, diags); }

SPGPU_HDIA_SOLVER_STEPS(S, float)
SPGPU_HDIA_SOLVER_STEPS(D, double)

} // extern "C"
