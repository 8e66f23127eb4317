#pragma once
/*
 * What every HELL SpMM kernel is handed and what more than one of them uses: the argument struct, the workgroup and tile
 * constants, the (coefficient, offset) records of the tiled kernel, lane shuffles, the wavefront-local LDS ordering point and the
 * two epilogues.  The kernels: spmm_rows.hip.h (one row per loader lane, hellSpmmKernel) and spmm_strip.hip.h (16-byte strips,
 * hellSpmmStripKernel); the dispatch and the C ABI: hell_spmm.hip.
 *
 * ---- Wavefront design -------------------------------------------------------
 * A wavefront owns 64 consecutive rows.  Two lane roles alternate:
 *
 *  load role   lane l fetches coefficient and column index of (row l, slab
 *              column k): for hackSize 32 the wave reads two whole slab columns
 *              of two hacks -- fully coalesced, every byte of cM/rP is fetched
 *              exactly once, UNROLL columns ahead of their use.
 *  team role   KP lanes form a row team, G = 64/KP teams per wave; lane t of a
 *              team owns VEC consecutive right-hand sides (KP*VEC >= count, for
 *              16 rhs: 8 lanes x 2).  Team g owns rows g*KP .. g*KP+KP-1 of the
 *              group and keeps one running sum per owned row and rhs.  In step
 *              i every team takes the (coef, col) pair that lane g*KP+i loaded
 *              -- a lane shuffle inside the team (ds_bpermute / DPP, no LDS
 *              allocation, no barrier) -- and all its lanes read their slice of
 *              X row `col`: the KP lanes of a team read ONE contiguous 128-byte
 *              line (16 doubles), one wave-wide 16-byte load serves G nonzeros.
 *
 * Per (row, rhs) the products are added in ascending k.  More than 16
 * right-hand sides run as passes of 16 (the matrix is re-read per pass).
 *
 * This describes hellSpmmKernel (any hackSize, any rhs count).  The default for
 * hackSize % 32 == 0 and an even rhs count > 8 is hellSpmmStripKernel of
 * spmm_strip.hip.h: same teams and summation order, but 16-byte loads of whole half-columns,
 * the X window of a workgroup in LDS, and (offset, coefficient) handed from the
 * loader lanes to the teams through LDS instead of lane shuffles.
 */
#include "numeric.hip.h"
#include <type_traits>
#include "spgpu_internal.h"

namespace spgpu {

template <typename T> struct SpmmArgs {
    T* Z;
    const T* Y;
    const T* X;
    const T* cM;
    const int* rP;
    const int* rS;
    const int* rIdx;
    const int* hackOffsets;
    T alpha, beta;
    int rows, baseIndex, hackSize;
    int count;      /* right-hand sides in this pass (<= KP*VEC) */
    int tileRows;   /* tiled kernel: X rows the LDS tile can hold */
    int directFill; /* strip kernel: every 16-byte piece of a tile row is 16 valid, aligned bytes of X (global_load_lds) */
    long long ldX, ldYZ; /* pitch layout (spgpu?hellspmmMv): the pitches of X and of Y / Z */
    int wideRuns;   /* pitch layout: X, Y, Z 16-byte aligned, pitches multiples of 16 bytes, no rIdx: 16-byte runs along the rows */
};

constexpr int kSpmmThreads = 256;
constexpr int kSpmmTileBytes = 43 * 1024; /* X tile; tile + padded record slots = 52 KiB, so three workgroups fit the 160 KiB LDS of a CU */

__device__ inline float laneFrom(float v, int src) { return __shfl(v, src, kWave); }
__device__ inline double laneFrom(double v, int src) { return __shfl(v, src, kWave); }
__device__ inline int laneFrom(int v, int src) { return __shfl(v, src, kWave); }

/* A 16-byte LDS read is served in 16-lane groups over 64 banks (256 B): two teams whose records lie 128 B apart
 * hit the same banks.  One pad record after every 8 shifts the teams of a group onto different banks
 * (SQ_LDS_BANK_CONFLICT was 58 % of the LDS cycles without it). */
constexpr int kSpmmStage = 2; /* slab columns published to LDS and consumed at a time */
constexpr int kRecordPadEvery = 8;
constexpr int kRecordsPerColumn = kWave + kWave / kRecordPadEvery;

/* What a loader lane publishes for its row's entry of one slab column.  `at` is the byte offset of the X row inside
 * the LDS tile, computed once by the loader instead of by each of the KP consumer lanes; negative = no entry. */
template <typename T> struct alignas(16) SpmmRecord {
    T coef;
    int at;
};
/* moved as ONE 16-byte LDS access (the compiler would split a plain struct copy into b64 + b32) */
template <typename T> __device__ inline SpmmRecord<T> loadRecord(const SpmmRecord<T>* p)
{
    const Pack<uint32_t, 4> raw = loadPack<false, uint32_t, 4>(reinterpret_cast<const uint32_t*>(p));
    SpmmRecord<T> out;
    __builtin_memcpy(&out, &raw, sizeof(out));
    return out;
}
template <typename T> __device__ inline void storeRecord(SpmmRecord<T>* p, T coef, int at)
{
    SpmmRecord<T> rec = {};
    rec.coef = coef;
    rec.at = at;
    Pack<uint32_t, 4> raw;
    __builtin_memcpy(&raw, &rec, sizeof(raw));
    storePack<uint32_t, 4>(reinterpret_cast<uint32_t*>(p), raw);
}

__device__ inline void waveSync()
{
    /* a wavefront's LDS operations execute in order; this only pins the compiler's order of the accesses */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* Epilogue shared by both kernels: team g writes rows g*KP .. g*KP+KP-1, lane t the rhs t*VEC .. */
template <typename T, int KP, int VEC>
__device__ inline void spmmStore(const SpmmArgs<T>& a, int lane, long long groupRow0, T (&sum)[KP][VEC])
{
    const int team = lane / KP;
    const int rhs0 = (lane % KP) * VEC;
    if (rhs0 >= a.count)
        return;
    const bool hasBeta = isNotZero(a.beta);
    /* Z += alpha*A*X in place (Y == Z, beta == 1): rows of A without entries keep their Z, unread and unwritten.
     * This is what the "rest" product of a column-split row block is made of (spgpu_amd/sharded.py). */
    const bool inPlaceSum = hasBeta && a.Y == a.Z && a.beta == T(1);
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const long long r = groupRow0 + team * KP + i;
        if (r < a.rows && !(inPlaceSum && a.rS[r] == 0)) {
            const long long outRow = a.rIdx ? a.rIdx[r] : r;
            const long long at = outRow * a.ldYZ + rhs0;
            Pack<T, VEC> out;
            if (hasBeta) {
                const Pack<T, VEC> yv = loadPack<false, T, VEC>(a.Y + at);
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    out.v[e] = epilogue<true>(a.alpha, sum[i][e], a.beta, yv.v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    out.v[e] = epilogue<false>(a.alpha, sum[i][e], a.beta, zeroOf<T>());
            }
            storePack<T, VEC>(a.Z + at, out);
        }
        __builtin_amdgcn_sched_barrier(0); /* one row's addresses and y values live at a time */
    }
}

/* The epilogue in the pitch layout (spgpu/ext/spmm_mv.h): Z[j*ldYZ + row].  A lane holds KP consecutive rows of its VEC vectors,
 * i.e. a run of KP elements along the row axis per vector: with a.wideRuns it goes out as 16-byte pieces (the teams of a
 * wavefront own consecutive runs, so a wavefront covers 64 consecutive rows of each vector), else -- row order, unaligned
 * arguments, the ragged end, rows an in-place sum skips -- element by element.  Same epilogue arithmetic as spmmStore. */
template <typename T, int KP, int VEC>
__device__ inline void spmmStorePitch(const SpmmArgs<T>& a, int lane, long long groupRow0, T (&sum)[KP][VEC])
{
    constexpr int RUN = 16 / (int)sizeof(T);
    static_assert(KP % RUN == 0, "a team's rows are whole 16-byte pieces");
    const long long row0 = groupRow0 + (lane / KP) * KP;
    const int rhs0 = (lane % KP) * VEC;
    const bool hasBeta = isNotZero(a.beta);
    const bool inPlaceSum = hasBeta && a.Y == a.Z && a.beta == T(1);
#pragma unroll
    for (int i0 = 0; i0 < KP; i0 += RUN) {
        const long long r0 = row0 + i0;
        bool whole = a.wideRuns && r0 + RUN <= a.rows;
        if (whole && inPlaceSum) {
#pragma unroll
            for (int i = 0; i < RUN; ++i)
                whole = whole && a.rS[r0 + i] != 0;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if (rhs0 + e >= a.count)
                continue;
            const long long at0 = (long long)(rhs0 + e) * a.ldYZ;
            if (whole) {
                Pack<T, RUN> out;
                if (hasBeta) {
                    const Pack<T, RUN> yv = loadPack<false, T, RUN>(a.Y + at0 + r0);
#pragma unroll
                    for (int i = 0; i < RUN; ++i)
                        out.v[i] = epilogue<true>(a.alpha, sum[i0 + i][e], a.beta, yv.v[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < RUN; ++i)
                        out.v[i] = epilogue<false>(a.alpha, sum[i0 + i][e], a.beta, zeroOf<T>());
                }
                storePack<T, RUN>(a.Z + at0 + r0, out);
            } else {
#pragma unroll
                for (int i = 0; i < RUN; ++i) {
                    const long long r = r0 + i;
                    if (r < a.rows && !(inPlaceSum && a.rS[r] == 0)) {
                        const long long at = at0 + (a.rIdx ? a.rIdx[r] : r);
                        a.Z[at] = hasBeta ? epilogue<true>(a.alpha, sum[i0 + i][e], a.beta, a.Y[at])
                                          : epilogue<false>(a.alpha, sum[i0 + i][e], a.beta, zeroOf<T>());
                    }
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0); /* one piece's addresses and y values live at a time */
    }
}


} // namespace spgpu
