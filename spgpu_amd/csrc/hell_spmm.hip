/*
 * HELL SpMM for gfx950 (MI355X):  Z = alpha*A*X + beta*Y, `count` right-hand
 * sides, interleaved multivectors (include/spgpu/spmm.h) or the reference's
 * pitch layout (include/spgpu/ext/spmm_mv.h).  New operation (the reference has
 * none); A uses the HELL arguments of hell.h:45-59.
 *
 * This file is the dispatch and the C ABI.  The kernels: spmm_rows.hip.h (one
 * row per loader lane), spmm_strip.hip.h (16-byte strips, the default for
 * hackSize % 32 == 0), mv_transpose.hip.h (layout conversion); what they share,
 * and the wavefront design: spmm_common.hip.h.
 *
 * Roofline: HBM.  Algorithmic bytes: the matrix once, nnz*(sizeof(T)+4) +
 * rows*4 + hacks*4, plus count * (cols + rows*(1+[beta!=0])) * sizeof(T).
 */
#include "spmm_strip.hip.h"
#include "mv_transpose.hip.h"

#include "spgpu/spmm.h"
#include "spgpu/ext/spmm_mv.h"

#include <stdio.h>
#include <stdlib.h>

namespace spgpu {

constexpr int kSpmmPass = 16; /* right-hand sides of one pass; more run as passes (the matrix is re-read per pass) */

/* The kernel shapes a pass can run as.  strip2 / strip1: hellSpmmStripKernel<T, 2, VEC> with VEC = 2 / 1 right-hand sides per
 * lane; tiled: hellSpmmKernel<T, 8, 2, 4, true>; kAxB: the plain hellSpmmKernel with teams of A lanes x B right-hand sides. */
enum class SpmmShape { strip2, strip1, tiled, k16, k4x2, k8x1, k4x1 };

/* what the strip kernels' 16-byte loads of whole 32-row half columns need of the matrix */
static bool matrixLoads16(int hackSize, const void* cM, const void* rP)
{
    return hackSize % 32 == 0 && (uintptr_t)cM % 16 == 0 && (uintptr_t)rP % 16 == 0;
}

/* Interleaved layout.  count: right-hand sides of the pass; pairs: two per lane are possible (even count, 2*sizeof(T)-aligned
 * rows of X, Y and Z). */
static SpmmShape spmmShape(int count, bool pairs, bool loads16)
{
    if (count > 8) /* X window in LDS when it fits, 16-byte loads; else tiled, one row per loader lane; else 16 lanes x 1 */
        return pairs && loads16 ? SpmmShape::strip2 : pairs ? SpmmShape::tiled : SpmmShape::k16;
    if (count > 4) /* 5 to 8 right-hand sides: the strip kernel with one per lane (64-byte X rows for fp64; no pairing, so odd
                    * counts and odd leading dimensions too) */
        return loads16 ? SpmmShape::strip1 : pairs ? SpmmShape::k4x2 : SpmmShape::k8x1;
    /* 4: the strip kernel with half of each team idle still wins (banded 0.58 vs 0.63 ms, windowed 1.54 vs
     * 1.72 ms); 1-3: the small-team plain kernel is as fast or faster on scattered columns */
    return count == 4 && loads16 ? SpmmShape::strip1 : SpmmShape::k4x1;
}

/* Pitch layout (spgpu?hellspmmMv): two shapes.  The strip kernel with PITCH where the matrix admits its 16-byte loads -- two
 * vectors per lane for 9..16 of a pass, one for up to 8; a.wideRuns switches its fill and epilogue between 16-byte pieces and
 * single elements -- and the one-row-per-lane kernel for everything else. */
static SpmmShape spmmMvShape(int count, bool loads16)
{
    return !loads16 ? SpmmShape::k16 : count > 8 ? SpmmShape::strip2 : SpmmShape::strip1;
}

/* one workgroup per kSpmmThreads rows (a wavefront per 64), every kernel of the family */
static unsigned spmmBlocks(int rows)
{
    const long long groups = ((long long)rows + kWave - 1) / kWave;
    return (unsigned)((groups + kSpmmThreads / kWave - 1) / (kSpmmThreads / kWave));
}

/* the arguments that are the same in every pass of a call; a pass sets Z, Y, X and count (and wideRuns), a launcher the rest */
template <typename T>
static SpmmArgs<T> spmmCallArgs(T alpha, const T* cM, const int* rP, int hackSize, const int* hackOffsets, const int* rS,
                                const int* rIdx, int rows, T beta, int baseIndex, long long ldX, long long ldYZ)
{
    SpmmArgs<T> a = {};
    a.cM = cM;
    a.rP = rP;
    a.rS = rS;
    a.rIdx = rIdx;
    a.hackOffsets = hackOffsets;
    a.alpha = alpha;
    a.beta = beta;
    a.rows = rows;
    a.baseIndex = baseIndex;
    a.hackSize = hackSize;
    a.ldX = ldX;
    a.ldYZ = ldYZ;
    return a;
}

template <typename T, int TRIP, int VEC, bool PITCH = false> static void launchSpmmStrips(hipStream_t stream, const SpmmArgs<T>& in)
{
    SpmmArgs<T> a = in;
    /* PITCH: the rows the window grows by when its low end is rounded down to a 16-byte piece are kept free */
    a.tileRows = kStripTileBytes / (8 * VEC * (int)sizeof(T)) - (PITCH ? 16 / (int)sizeof(T) - 1 : 0);
    /* whole tile rows of valid bytes: all KP * VEC right-hand sides present, rows of X 16-byte aligned */
    a.directFill = !PITCH && a.count == 8 * VEC && (8 * VEC * sizeof(T)) % 16 == 0 && (uintptr_t)a.X % 16 == 0 &&
                   (a.ldX * (long long)sizeof(T)) % 16 == 0;
    const size_t lds = kStripTileBytes + (kSpmmThreads / kWave) * sizeof(SpmmStage<T>);
    hipLaunchKernelGGL((hellSpmmStripKernel<T, TRIP, VEC, PITCH>), dim3(spmmBlocks(a.rows)), dim3(kSpmmThreads), lds, stream, a);
}

template <typename T, int KP, int VEC, int UNROLL, bool TILED = false, bool PITCH = false>
static void launchSpmm(hipStream_t stream, const SpmmArgs<T>& in)
{
    SpmmArgs<T> a = in;
    a.tileRows = TILED ? kSpmmTileBytes / (KP * VEC * (int)sizeof(T)) : 0;
    const size_t lds = TILED ? kSpmmTileBytes + (kSpmmThreads / kWave) * kSpmmStage * kRecordsPerColumn * sizeof(SpmmRecord<T>) : 0;
    hipLaunchKernelGGL((hellSpmmKernel<T, KP, VEC, UNROLL, TILED, PITCH>), dim3(spmmBlocks(a.rows)), dim3(kSpmmThreads), lds, stream, a);
}

/* Both layouts.  PITCH: right-hand side j at base + j*ldX (X) or j*ldYZ (Y, Z), the multivectors of spgpu/ext/spmm_mv.h; else
 * interleaved, right-hand side j of row r at r*ld + j. */
template <typename T, bool PITCH>
static void hellSpmm(spgpuHandle_t handle, T* Z, const T* Y, T alpha, const T* cM, const int* rP, int hackSize,
                     const int* hackOffsets, const int* rS, const int* rIdx, int rows, const T* X, T beta,
                     int baseIndex, int count, int ldX, int ldYZ)
{
    if (rows <= 0 || count <= 0 || hackSize <= 0)
        return;
    hipStream_t stream = handle->currentStream;
    const bool loads16 = matrixLoads16(hackSize, cM, rP);
    const long long nextX = PITCH ? ldX : 1, nextYZ = PITCH ? ldYZ : 1; /* from one right-hand side to the next */
    SpmmArgs<T> a = spmmCallArgs<T>(alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, beta, baseIndex, ldX, ldYZ);
    for (int first = 0; first < count; first += kSpmmPass) {
        a.Z = Z + first * nextYZ;
        a.Y = Y ? Y + first * nextYZ : nullptr;
        a.X = X + first * nextX;
        a.count = count - first < kSpmmPass ? count - first : kSpmmPass;
        if constexpr (PITCH) {
            a.wideRuns = !rIdx && (uintptr_t)a.X % 16 == 0 && (uintptr_t)a.Z % 16 == 0 && (!a.Y || (uintptr_t)a.Y % 16 == 0) &&
                         ((long long)ldX * sizeof(T)) % 16 == 0 && ((long long)ldYZ * sizeof(T)) % 16 == 0;
            switch (spmmMvShape(a.count, loads16)) {
            case SpmmShape::strip2: launchSpmmStrips<T, 2, 2, true>(stream, a); break;
            case SpmmShape::strip1: launchSpmmStrips<T, 2, 1, true>(stream, a); break;
            case SpmmShape::k16: launchSpmm<T, 16, 1, 2, false, true>(stream, a); break;
            default: break; /* spmmMvShape names no other */
            }
        } else {
            /* two right-hand sides per lane need 2*sizeof(T)-aligned rows of X, Y and Z */
            const size_t pair = 2 * sizeof(T);
            const bool pairsOk = ldX % 2 == 0 && ldYZ % 2 == 0 && (uintptr_t)X % pair == 0 && (uintptr_t)Z % pair == 0 &&
                                 (!Y || (uintptr_t)Y % pair == 0);
            switch (spmmShape(a.count, pairsOk && a.count % 2 == 0, loads16)) {
            case SpmmShape::strip2: launchSpmmStrips<T, 2, 2>(stream, a); break;
            case SpmmShape::strip1: launchSpmmStrips<T, 2, 1>(stream, a); break;
            case SpmmShape::tiled: launchSpmm<T, 8, 2, 4, true>(stream, a); break;
            case SpmmShape::k16: launchSpmm<T, 16, 1, 2>(stream, a); break;
            case SpmmShape::k4x2: launchSpmm<T, 4, 2, 4>(stream, a); break;
            case SpmmShape::k8x1: launchSpmm<T, 8, 1, 2>(stream, a); break;
            case SpmmShape::k4x1: launchSpmm<T, 4, 1, 4>(stream, a); break;
            default: break;
            }
        }
    }
    spgpuDebugCheck(handle, PITCH ? "hellspmmMv" : "hellspmm");
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

void spgpuShellspmm(spgpuHandle_t handle, float* Z, const float* Y, float alpha, const float* cM, const int* rP,
                    int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int avgNnzPerRow, int rows,
                    const float* X, float beta, int baseIndex, int count, int ldX, int ldYZ)
{
    (void)avgNnzPerRow;
    hellSpmm<float, false>(handle, Z, Y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, X, beta, baseIndex, count, ldX, ldYZ);
}

void spgpuDhellspmm(spgpuHandle_t handle, double* Z, const double* Y, double alpha, const double* cM, const int* rP,
                    int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int avgNnzPerRow, int rows,
                    const double* X, double beta, int baseIndex, int count, int ldX, int ldYZ)
{
    (void)avgNnzPerRow;
    hellSpmm<double, false>(handle, Z, Y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, X, beta, baseIndex, count, ldX, ldYZ);
}

void spgpuShellspmmMv(spgpuHandle_t handle, float* Z, const float* Y, float alpha, const float* cM, const int* rP,
                      int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int avgNnzPerRow, int rows,
                      const float* X, float beta, int baseIndex, int count, int pitchX, int pitchYZ)
{
    (void)avgNnzPerRow;
    hellSpmm<float, true>(handle, Z, Y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, X, beta, baseIndex, count, pitchX, pitchYZ);
}

void spgpuDhellspmmMv(spgpuHandle_t handle, double* Z, const double* Y, double alpha, const double* cM, const int* rP,
                      int hackSize, const int* hackOffsets, const int* rS, const int* rIdx, int avgNnzPerRow, int rows,
                      const double* X, double beta, int baseIndex, int count, int pitchX, int pitchYZ)
{
    (void)avgNnzPerRow;
    hellSpmm<double, true>(handle, Z, Y, alpha, cM, rP, hackSize, hackOffsets, rS, rIdx, rows, X, beta, baseIndex, count, pitchX, pitchYZ);
}

void spgpuSmvInterleave(spgpuHandle_t h, float* dst, int ld, const float* src, int pitch, int n, int count)
{ mvTranspose<float, true>(h, dst, ld, src, pitch, n, count); }
void spgpuDmvInterleave(spgpuHandle_t h, double* dst, int ld, const double* src, int pitch, int n, int count)
{ mvTranspose<double, true>(h, dst, ld, src, pitch, n, count); }
void spgpuSmvDeinterleave(spgpuHandle_t h, float* dst, int pitch, const float* src, int ld, int n, int count)
{ mvTranspose<float, false>(h, dst, pitch, src, ld, n, count); }
void spgpuDmvDeinterleave(spgpuHandle_t h, double* dst, int pitch, const double* src, int ld, int n, int count)
{ mvTranspose<double, false>(h, dst, pitch, src, ld, n, count); }

} // extern "C"
