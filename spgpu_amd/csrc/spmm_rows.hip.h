#pragma once
/*
 * The one-row-per-lane HELL SpMM family: spmmAccumulate (the accumulation loop, from global memory or from an LDS tile) and
 * hellSpmmKernel (plain and tiled; any hackSize, any right-hand-side count, both layouts).  The wavefront design is described in
 * spmm_common.hip.h; the strip kernel (spmm_strip.hip.h) falls back on spmmAccumulate when its window does not fit.
 */
#include "spmm_common.hip.h"

namespace spgpu {

/* The accumulation loop shared by both kernels.
 * FROM_LDS == false: X rows are read from global memory (through L1/L2).
 * FROM_LDS == true : X rows come from the workgroup's LDS tile.  LDS reads retire on lgkmcnt, global loads on
 *                    vmcnt, and each counter retires in issue order -- so only in this form can the (coef, col)
 *                    pairs of the NEXT slab columns be requested from HBM at the top of an iteration and stay in
 *                    flight while the current columns are consumed (with global X reads a wait for them would
 *                    also wait for the older prefetch: measured, profiles/r01b_ab_spmm_pipelined.txt). */
template <typename T, int KP, int VEC, int UNROLL, bool FROM_LDS, bool PITCH = false>
__device__ inline void spmmAccumulate(const SpmmArgs<T>& a, int lane, int myLen, int groupLongest,
                                      const T* __restrict__ vals, const int* __restrict__ idxs,
                                      const T* __restrict__ tile, int tileFirst, T (&sum)[KP][VEC],
                                      SpmmRecord<T>* records = nullptr)
{
    constexpr int TILE_LD = KP * VEC;
    /* CHUNK rows of the team at a time: CHUNK X-row reads in flight per lane */
    constexpr int CHUNK = KP < 4 ? KP : 4;
    const int team = lane / KP;
    const int rhs0 = (lane % KP) * VEC;
    const int rhsSafe = rhs0 < a.count ? rhs0 : 0; /* lanes beyond `count` read a valid slice, result discarded */

    auto fetch = [&](int kBase, T* coef, int* col) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kBase + u;
            if (k < myLen) {
                coef[u] = vals[(long long)k * a.hackSize];
                col[u] = idxs[(long long)k * a.hackSize] - a.baseIndex;
            } else {
                coef[u] = zeroOf<T>();
                col[u] = -1; /* no entry */
            }
        }
    };

    T coefMine[UNROLL];
    int colMine[UNROLL];
    if constexpr (FROM_LDS) {
        static_assert(KP == kRecordPadEvery, "record padding assumes one pad slot per team");
        static_assert(UNROLL % kSpmmStage == 0, "a trip is a whole number of stages");
        const unsigned char* const myTile = reinterpret_cast<const unsigned char*>(tile) + rhsSafe * sizeof(T);
        const SpmmRecord<T>* const teamRecords = records + team * (KP + 1);
        SpmmRecord<T>* const myRecord = records + lane + lane / kRecordPadEvery;
        /* ALL_PRESENT: every row of the wavefront has an entry in these slab columns (always, for uniform rows):
         * no per-entry test, 16 fused multiply-adds + 8 address adds per lane and column.  Otherwise absent
         * entries (at < 0) read tile row 0 and their product is discarded. */
        auto consume = [&](auto allPresent) {
            constexpr bool ALL_PRESENT = decltype(allPresent)::value;
            /* all KP rows of the team at once: LDS bounds the occupancy here (3 wavefronts per SIMD), so the
             * registers for KP reads in flight are free */
            constexpr int CHUNK = KP;
#pragma unroll
            for (int u = 0; u < kSpmmStage; ++u) {
#pragma unroll
                for (int i0 = 0; i0 < KP; i0 += CHUNK) {
                    SpmmRecord<T> rec[CHUNK];
                    Pack<T, VEC> xv[CHUNK];
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i) /* one 16-byte LDS read, the same address for the lanes of a team */
                        rec[i] = loadRecord(teamRecords + u * kRecordsPerColumn + i0 + i);
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i) {
                        const int at = ALL_PRESENT ? rec[i].at : (rec[i].at >= 0 ? rec[i].at : 0);
                        xv[i] = loadPack<false, T, VEC>(reinterpret_cast<const T*>(myTile + at));
                    }
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const T next = mulAdd(rec[i].coef, xv[i].v[e], sum[i0 + i][e]);
                            sum[i0 + i][e] = ALL_PRESENT ? next : pick(rec[i].at >= 0, next, sum[i0 + i][e]);
                        }
                    /* keep the scheduler from hoisting every chunk's reads to the top: that costs registers
                     * (occupancy), not latency -- other wavefronts cover it */
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        const int groupShortest = waveMin(myLen);
        T coefNext[UNROLL];
        int colNext[UNROLL];
        fetch(0, coefMine, colMine);
        for (int kBase = 0; kBase < groupLongest; kBase += UNROLL) {
            /* (coef, col) of the next UNROLL columns requested now: 2*UNROLL loads per lane stay in flight (vmcnt)
             * while this trip runs on LDS (lgkmcnt).  With the 3 wavefronts per SIMD the tile leaves room for,
             * this depth is what keeps enough bytes in flight to cover the HBM latency. */
            fetch(kBase + UNROLL, coefNext, colNext);
#pragma unroll
            for (int s0 = 0; s0 < UNROLL; s0 += kSpmmStage) {
                if (kBase + s0 < groupLongest) { /* wavefront-uniform */
                    /* publish kSpmmStage columns to the wavefront's own record slots; a wavefront's LDS operations
                     * execute in order, the barriers only stop the compiler from reordering across them */
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int u = 0; u < kSpmmStage; ++u)
                        storeRecord(myRecord + u * kRecordsPerColumn, coefMine[s0 + u],
                                    colMine[s0 + u] >= 0 ? (colMine[s0 + u] - tileFirst) * (int)(TILE_LD * sizeof(T)) : -1);
                    __builtin_amdgcn_wave_barrier();
                    if (kBase + s0 + kSpmmStage <= groupShortest) /* wavefront-uniform */
                        consume(std::true_type{});
                    else
                        consume(std::false_type{});
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                coefMine[u] = coefNext[u];
                colMine[u] = colNext[u];
            }
        }
    } else {
        /* PITCH (spmm_mv.h): vector j at X + j*ldX, so a lane's VEC right-hand sides of one X row are VEC gathers */
        const T* __restrict__ Xsafe = a.X + (PITCH ? rhsSafe * a.ldX : (long long)rhsSafe);
        for (int kBase = 0; kBase < groupLongest; kBase += UNROLL) {
            fetch(kBase, coefMine, colMine);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
                for (int i0 = 0; i0 < KP; i0 += CHUNK) {
                    T coef[CHUNK];
                    int col[CHUNK];
                    Pack<T, VEC> xv[CHUNK];
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i) {
                        const int src = team * KP + i0 + i;
                        coef[i] = laneFrom(coefMine[u], src);
                        col[i] = laneFrom(colMine[u], src);
                    }
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i) { /* no branch: absent entries read row 0 and are discarded below */
                        if constexpr (PITCH) {
#pragma unroll
                            for (int e = 0; e < VEC; ++e) /* a lane whose last vector is past `count` reads its first again */
                                xv[i].v[e] = Xsafe[(rhsSafe + e < a.count ? e * a.ldX : 0) + (col[i] >= 0 ? col[i] : 0)];
                        } else {
                            xv[i] = loadPack<false, T, VEC>(Xsafe + (long long)(col[i] >= 0 ? col[i] : 0) * a.ldX);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < CHUNK; ++i)
#pragma unroll
                        for (int e = 0; e < VEC; ++e)
                            sum[i0 + i][e] = pick(col[i] >= 0, mulAdd(coef[i], xv[i].v[e], sum[i0 + i][e]), sum[i0 + i][e]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
}

/* TILED == false: plain kernel.  TILED == true: the workgroup first finds the window of X rows its 256 matrix rows
 * touch; if the window fits the LDS tile (banded / FEM-like matrices) it is copied into LDS once, coalesced, and the
 * accumulation reads X from there (LDS: 256 B/clk/CU, vector L1: 64); otherwise it accumulates from global memory. */
template <typename T, int KP, int VEC, int UNROLL, bool TILED, bool PITCH = false>
__global__ __launch_bounds__(kSpmmThreads) void hellSpmmKernel(const SpmmArgs<T> a)
{
    static_assert(!(TILED && PITCH), "the pitch layout's tiled form is the strip kernel");
    extern __shared__ __attribute__((aligned(16))) unsigned char spmmLds[];
    const int lane = threadIdx.x & (kWave - 1);
    const long long group = (long long)blockIdx.x * (kSpmmThreads / kWave) + (threadIdx.x >> 6);
    const long long groupRow0 = group * kWave;
    if constexpr (!TILED) {
        if (groupRow0 >= a.rows)
            return; /* whole wavefront leaves together (the tiled form has workgroup barriers: everyone stays) */
    }

    /* ---- load role: this lane's row ---- */
    const long long myRow = groupRow0 + lane;
    int myLen = 0;
    long long slab = 0;
    if (myRow < a.rows) {
        const unsigned r = (unsigned)myRow, hs = (unsigned)a.hackSize;
        const unsigned hack = r / hs;
        slab = (long long)a.hackOffsets[hack] + (r - hack * hs);
        myLen = a.rS[myRow];
    }
    const int groupLongest = waveMax(myLen);
    const T* __restrict__ vals = a.cM + slab;
    const int* __restrict__ idxs = a.rP + slab;

    T sum[KP][VEC];
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            sum[i][e] = zeroOf<T>();

    if constexpr (TILED) {
        constexpr int TILE_LD = KP * VEC;
        T* const tile = reinterpret_cast<T*>(spmmLds);
        __shared__ int waveLo[kSpmmThreads / kWave], waveHi[kSpmmThreads / kWave];
        /* pass 1: column window of the workgroup (the indices are read again below, out of L2).
         * First a probe on slab column 0 only (one coalesced load): scattered matrices already span more than
         * the tile there and skip the full scan; then 8 independent loads per trip over all columns. */
        auto blockWindow = [&](int& lo, int& hi) {
#pragma unroll
            for (int m = 1; m < kWave; m <<= 1) {
                const int olo = laneXor(lo, m), ohi = laneXor(hi, m);
                lo = olo < lo ? olo : lo;
                hi = ohi > hi ? ohi : hi;
            }
            __syncthreads(); /* previous use of waveLo/waveHi is over */
            if (lane == 0) {
                waveLo[threadIdx.x >> 6] = lo;
                waveHi[threadIdx.x >> 6] = hi;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < kSpmmThreads / kWave; ++w) {
                lo = waveLo[w] < lo ? waveLo[w] : lo;
                hi = waveHi[w] > hi ? waveHi[w] : hi;
            }
        };
        int lo = 0x7fffffff, hi = -1;
        if (myLen > 0) {
            const int c = idxs[0] - a.baseIndex;
            if (c >= 0)
                lo = hi = c;
        }
        blockWindow(lo, hi);
        const bool worthScanning = hi < lo || (long long)hi - lo < a.tileRows; /* workgroup-uniform */
        if (worthScanning) {
            constexpr int SCAN = 16; /* independent loads per trip: the scan is a chain of memory latencies */
            for (int k0 = 1; k0 < myLen; k0 += SCAN) {
                int c[SCAN];
#pragma unroll
                for (int u = 0; u < SCAN; ++u)
                    c[u] = k0 + u < myLen ? idxs[(long long)(k0 + u) * a.hackSize] - a.baseIndex : -1;
#pragma unroll
                for (int u = 0; u < SCAN; ++u) {
                    if (c[u] >= 0) {
                        lo = c[u] < lo ? c[u] : lo;
                        hi = c[u] > hi ? c[u] : hi;
                    }
                }
            }
            blockWindow(lo, hi);
        }
        const bool useTile = worthScanning && hi >= lo && (long long)hi - lo < a.tileRows; /* workgroup-uniform */
        if (useTile) {
            const int window = hi - lo + 1;
            /* KP lanes copy one X row, VEC elements (16 bytes) each; FILL loads per lane in flight */
            constexpr int FILL = 4;
            const int pieces = window * KP;
            for (int i0 = threadIdx.x; i0 < pieces; i0 += FILL * kSpmmThreads) {
                Pack<T, VEC> part[FILL];
#pragma unroll
                for (int f = 0; f < FILL; ++f) {
                    const int i = i0 + f * kSpmmThreads;
                    const int r = i / KP, piece = i % KP;
                    if (i < pieces && piece * VEC < a.count)
                        part[f] = loadPack<false, T, VEC>(a.X + (long long)(lo + r) * a.ldX + piece * VEC);
                }
#pragma unroll
                for (int f = 0; f < FILL; ++f) {
                    const int i = i0 + f * kSpmmThreads;
                    const int r = i / KP, piece = i % KP;
                    if (i < pieces && piece * VEC < a.count)
                        storePack<T, VEC>(tile + r * TILE_LD + piece * VEC, part[f]);
                }
            }
        }
        __syncthreads();
        /* per-wavefront record slots behind the tile */
        SpmmRecord<T>* records = reinterpret_cast<SpmmRecord<T>*>(spmmLds + kSpmmTileBytes) + (threadIdx.x >> 6) * (kSpmmStage * kRecordsPerColumn);
        if (useTile)
            spmmAccumulate<T, KP, VEC, UNROLL, true>(a, lane, myLen, groupLongest, vals, idxs, tile, lo, sum, records);
        else /* window too wide: X through L1/L2, the plain kernel's trip width */
            spmmAccumulate<T, KP, VEC, (UNROLL < 2 ? UNROLL : 2), false>(a, lane, myLen, groupLongest, vals, idxs, tile, 0, sum);
        if (groupRow0 >= a.rows)
            return;
    } else {
        spmmAccumulate<T, KP, VEC, UNROLL, false, PITCH>(a, lane, myLen, groupLongest, vals, idxs, nullptr, 0, sum);
    }
    if constexpr (PITCH)
        spmmStorePitch<T, KP, VEC>(a, lane, groupRow0, sum);
    else
        spmmStore<T, KP, VEC>(a, lane, groupRow0, sum);
}

} // namespace spgpu
