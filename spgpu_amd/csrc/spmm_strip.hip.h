#pragma once
#include "spmm_rows.hip.h"

namespace spgpu {

/* ---------------------------------------------------------------------------------------------------------------
 * Strip-loading tiled kernel: hackSize a multiple of 32, up to 16 right-hand sides as 8 lanes x 2.
 *
 * The LDS tile leaves room for 3 wavefronts per SIMD only, so what bounds the kernel is the number of bytes each
 * wavefront keeps in flight.  One-row-per-lane loads move 4 (index) or 8 (coefficient) bytes per lane; here every
 * load is 16 bytes per lane: a wavefront's 64 rows are two halves of 32 rows, each inside one hack, and
 *   index role        lane l reads rows 4q..4q+3 (q = l%8) of half (l/8)%2 in slab column k0 + l/16: one
 *                     instruction covers 4 slab columns of the 64 rows;
 *   coefficient role  the same with 16/sizeof(T) rows per lane: 2 (double) or 1 (float) instructions per 4 columns.
 * A stage is 4 slab columns.  The loader lanes publish it to the wavefront's own LDS staging area -- the byte
 * offset of the X row inside the tile, computed once, or -1 for "no entry", and the coefficient -- and the teams
 * read their 8 rows' values back with 16-byte LDS reads (same address for the 8 lanes of a team).  A trip is
 * TRIP stages; the loads of the next trip are issued before the current one is consumed and stay in flight while
 * it runs on LDS.  The window scan of the prologue uses the same 16-byte index loads, 8 per lane in flight.
 * Per (row, rhs) the products are still added in ascending k.
 */
constexpr int kStageCols = 4;
constexpr int kStripTileBytes = 40 * 1024; /* + 4 staging areas of 3 KiB (double) = 52 KiB: three workgroups per CU */

template <typename T> struct alignas(16) SpmmStage {
    int at[kStageCols][kWave];
    T coef[kStageCols][kWave];
};

/* amdgpu_waves_per_eu(3): the LDS footprint admits 3 wavefronts per SIMD; tell the register allocator to stay
 * within the matching 168 VGPRs instead of trading occupancy for scheduling freedom */
/* PITCH: the multivectors of spgpu/ext/spmm_mv.h, vector j at base + j*pitch.  The tile keeps its row-major form, so everything
 * between the fill and the epilogue -- records, teams, the band window, the order of the additions -- is the code of
 * spmm_common.hip.h and spmm_rows.hip.h, unchanged; the fill transposes `count` runs of X on the way in, a window too wide for the tile costs one gather per
 * vector, and the epilogue writes runs along the row axis (spmmStorePitch). */
template <typename T, int TRIP, int VEC, bool PITCH = false>
__global__ __launch_bounds__(kSpmmThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void hellSpmmStripKernel(const SpmmArgs<T> a)
{
    constexpr int KP = 8, TILE_LD = KP * VEC; /* VEC right-hand sides per lane: 2 (up to 16 in all) or 1 (up to 8) */
    constexpr int ROW_BYTES = TILE_LD * (int)sizeof(T);
    constexpr int CR = 16 / (int)sizeof(T);                     /* rows per coefficient load */
    constexpr int COEF_LOADS = kStageCols * (int)sizeof(T) / 16; /* per stage */
    constexpr int COLS_PER_COEF_LOAD = kStageCols / COEF_LOADS;
    constexpr int LANES_PER_HALF_COL = 32 / CR;
    constexpr int WAVES = kSpmmThreads / kWave;
    /* Tile layout.  A team reads one whole X row (ROW_BYTES) per instruction, and the LDS serves 256 bytes (64 banks)
     * per pass: rows at a distance of 8 -- what neighbouring teams read in a banded matrix -- would share banks if
     * row r simply sat at r*ROW_BYTES.  Inside each 256-byte line the rows are therefore permuted by r>>3
     * (measured: SQ_LDS_BANK_CONFLICT was 32 % of the LDS cycles without it). */
    constexpr int ROWS_PER_LINE = 256 / ROW_BYTES;
    auto tileOffset = [](int r) { return (r / ROWS_PER_LINE) * 256 + ((r ^ (r >> 3)) & (ROWS_PER_LINE - 1)) * ROW_BYTES; };

    extern __shared__ __attribute__((aligned(16))) unsigned char spmmLds[];
    __shared__ int waveLo[WAVES], waveHi[WAVES], waveLongest[WAVES];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const long long groupRow0 = ((long long)blockIdx.x * WAVES + wave) * kWave;
    T* const tile = reinterpret_cast<T*>(spmmLds);
    SpmmStage<T>* const stage = reinterpret_cast<SpmmStage<T>*>(spmmLds + kStripTileBytes) + wave;
    const unsigned hs = (unsigned)a.hackSize;
    /* The tile fill: X rows first .. first + count - 1 into LDS.  Where whole 16-byte pieces line up (a.directFill, decided by
     * the host) the copy goes straight from global memory into LDS (global_load_lds_dwordx4): no registers, no ds_write, and
     * ALL of a lane's pieces in flight at once -- through registers (5 pieces per lane at a time beside the two trips
     * already in flight) a 288-row window was two dependent round trips.  One wave-wide instruction writes 1 KiB of LDS in
     * lane order from 64 per-lane addresses: lane -> LDS position is fixed, so the lane works out WHICH piece of X lands
     * there (the inverse of tileOffset); only whole wavefronts take it, the ragged end goes through registers. */
    auto fillTile = [&](int first, int count) {
        if constexpr (PITCH) {
            /* `first` is a multiple of RUN here (the window's low end is rounded down below), so with a.wideRuns every piece
             * X[j*ldX + first + RUN*c ..] is 16 aligned bytes.  A lane takes RUN consecutive X rows of ONE vector; the 16 lanes
             * next to it the same rows of the other vectors (64-byte runs per vector and wavefront in global memory, one
             * contiguous tile row per 16 lanes in LDS; the rows of a piece are written in an order rotated by the piece's number,
             * so that the two pieces of a 32-lane LDS pass do not meet in one 256-byte line's banks).  Elements past the
             * window's high end are not read: the last X row a matrix names may be the last element of its vector. */
            constexpr int RUN = 16 / (int)sizeof(T);
            constexpr int FILL = 4;
            unsigned char* const tileBytes = reinterpret_cast<unsigned char*>(tile);
            const int j = threadIdx.x % TILE_LD;
            const bool mine = j < a.count;
            const T* const xj = a.X + (long long)(mine ? j : 0) * a.ldX + first;
            if (a.wideRuns) {
                const int whole = count / RUN;
                for (int c0 = threadIdx.x / TILE_LD; c0 < whole; c0 += FILL * (kSpmmThreads / TILE_LD)) {
                    Pack<T, RUN> part[FILL];
#pragma unroll
                    for (int f = 0; f < FILL; ++f) {
                        const int c = c0 + f * (kSpmmThreads / TILE_LD);
                        if (c < whole && mine)
                            part[f] = loadPack<false, T, RUN>(xj + c * RUN);
                    }
#pragma unroll
                    for (int f = 0; f < FILL; ++f) {
                        const int c = c0 + f * (kSpmmThreads / TILE_LD);
                        if (c < whole && mine) {
#pragma unroll
                            for (int e = 0; e < RUN; ++e) {
                                const int ee = (e + c) % RUN;
                                T v = part[f].v[0];
#pragma unroll
                                for (int q = 1; q < RUN; ++q)
                                    v = ee == q ? part[f].v[q] : v;
                                *reinterpret_cast<T*>(tileBytes + tileOffset(c * RUN + ee) + j * (int)sizeof(T)) = v;
                            }
                        }
                    }
                }
                for (int r = whole * RUN + threadIdx.x / TILE_LD; r < count; r += kSpmmThreads / TILE_LD)
                    if (mine)
                        *reinterpret_cast<T*>(tileBytes + tileOffset(r) + j * (int)sizeof(T)) = xj[r];
            } else {
                for (int r = threadIdx.x / TILE_LD; r < count; r += kSpmmThreads / TILE_LD)
                    if (mine)
                        *reinterpret_cast<T*>(tileBytes + tileOffset(r) + j * (int)sizeof(T)) = xj[r];
            }
            return;
        }
        constexpr int PIECES_PER_ROW = ROW_BYTES >= 16 ? ROW_BYTES / 16 : 1;
        constexpr int PIECE_ELEMS = 16 / (int)sizeof(T);
        if (ROW_BYTES >= 16 && a.directFill) {
            const int lines = (count + ROWS_PER_LINE - 1) / ROWS_PER_LINE;
            const int slots = lines * 16; /* 16-byte slots of LDS, in address order */
            for (int s0 = wave * kWave; s0 < slots; s0 += kSpmmThreads) { /* wavefront-uniform */
                const int slot = s0 + lane;
                const int line = slot >> 4, q = (slot & 15) / PIECES_PER_ROW, piece = slot % PIECES_PER_ROW;
                const int r = line * ROWS_PER_LINE + ((q ^ ((line * ROWS_PER_LINE) >> 3)) & (ROWS_PER_LINE - 1));
                const bool live = slot < slots && r < count;
                const T* from = a.X + (long long)(first + (live ? r : 0)) * a.ldX + piece * PIECE_ELEMS;
                if (__ballot(live) == ~0ull) {
#if defined(__HIP_DEVICE_COMPILE__) /* the host pass of hipcc parses the kernel body too and has no such builtin */
                    __builtin_amdgcn_global_load_lds(from, reinterpret_cast<unsigned char*>(tile) + (size_t)slot * 16, 16, 0, 0);
#endif
                } else if (live) {
                    const Pack<T, PIECE_ELEMS> w = loadPack<false, T, PIECE_ELEMS>(from);
                    storePack<T, PIECE_ELEMS>(reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(tile) + (size_t)slot * 16), w);
                }
            }
            return;
        }
        /* KP lanes copy one X row, VEC elements each; FILL loads per lane in flight */
        constexpr int FILL = 5;
        const int pieces = count * KP;
        for (int i0 = threadIdx.x; i0 < pieces; i0 += FILL * kSpmmThreads) {
            Pack<T, VEC> part[FILL];
#pragma unroll
            for (int f = 0; f < FILL; ++f) {
                const int i = i0 + f * kSpmmThreads;
                const int r = i / KP, piece = i % KP;
                if (i < pieces && piece * VEC < a.count)
                    part[f] = loadPack<false, T, VEC>(a.X + (long long)(first + r) * a.ldX + piece * VEC);
            }
#pragma unroll
            for (int f = 0; f < FILL; ++f) {
                const int i = i0 + f * kSpmmThreads;
                const int r = i / KP, piece = i % KP;
                if (i < pieces && piece * VEC < a.count)
                    storePack<T, VEC>(reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(tile) + tileOffset(r)) + piece * VEC, part[f]);
            }
        }
    };


    /* ---- index role ---- */
    const int iCol = lane >> 4, iHalf = (lane >> 3) & 1, iQ = lane & 7;
    const long long iRow0 = groupRow0 + 32 * iHalf + 4 * iQ;
    int iLen[4] = {0, 0, 0, 0};
    const int* __restrict__ iBase = a.rP;
    if (iRow0 < a.rows) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (iRow0 + j < a.rows)
                iLen[j] = a.rS[iRow0 + j];
        const unsigned hack = (unsigned)iRow0 / hs;
        iBase += (long long)a.hackOffsets[hack] + ((unsigned)iRow0 - hack * hs);
    }
    int iLenMax = iLen[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        iLenMax = iLen[j] > iLenMax ? iLen[j] : iLenMax;
    /* ---- coefficient role ---- */
    const int cCol = lane / (2 * LANES_PER_HALF_COL), cHalf = (lane / LANES_PER_HALF_COL) & 1, cQ = lane % LANES_PER_HALF_COL;
    const long long cRow0 = groupRow0 + 32 * cHalf + CR * cQ;
    int cLenMax = 0;
    const T* __restrict__ cBase = a.cM;
    if (cRow0 < a.rows) {
#pragma unroll
        for (int j = 0; j < CR; ++j)
            if (cRow0 + j < a.rows) {
                const int len = a.rS[cRow0 + j];
                cLenMax = len > cLenMax ? len : cLenMax;
            }
        const unsigned hack = (unsigned)cRow0 / hs;
        cBase += (long long)a.hackOffsets[hack] + ((unsigned)cRow0 - hack * hs);
    }
    const int groupLongest = waveMax(iLenMax);

    /* ---- prologue: the window of X rows the workgroup's 256 matrix rows touch ---- */
    auto blockWindow = [&](int& lo, int& hi) {
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            const int olo = laneXor(lo, m), ohi = laneXor(hi, m);
            lo = olo < lo ? olo : lo;
            hi = ohi > hi ? ohi : hi;
        }
        __syncthreads(); /* previous use of waveLo/waveHi is over */
        if (lane == 0) {
            waveLo[wave] = lo;
            waveHi[wave] = hi;
            waveLongest[wave] = groupLongest;
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            lo = waveLo[w] < lo ? waveLo[w] : lo;
            hi = waveHi[w] > hi ? waveHi[w] : hi;
        }
    };
    auto widen = [&](const Pack<int, 4>& c4, int k, int& lo, int& hi) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c4.v[j] - a.baseIndex;
            if (k < iLen[j] && c >= 0) {
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
            }
        }
    };
    struct Trip {
        Pack<int, 4> idx[TRIP];
        Pack<T, CR> coef[TRIP * COEF_LOADS];
    };
    auto loadTripCoef = [&](int k0, Trip& t) {
#pragma unroll
        for (int s = 0; s < TRIP; ++s) {
#pragma unroll
            for (int j = 0; j < COEF_LOADS; ++j) {
                const int kc = k0 + kStageCols * s + COLS_PER_COEF_LOAD * j + cCol;
                if (kc < cLenMax) {
                    t.coef[s * COEF_LOADS + j] = loadPack<true, T, CR>(cBase + (long long)kc * hs);
                } else {
#pragma unroll
                    for (int e = 0; e < CR; ++e)
                        t.coef[s * COEF_LOADS + j].v[e] = zeroOf<T>();
                }
            }
        }
    };
    constexpr int STEP = kStageCols * TRIP;
    Trip cur, next;
    int lo = 0x7fffffff, hi = -1;
    /* The indices of the first HEAD*4 slab columns are requested at once and stay in registers: the accumulation
     * below takes them from there instead of reading them a second time. */
    constexpr int HEAD = 8;
    Pack<int, 4> head[HEAD];
#pragma unroll
    for (int u = 0; u < HEAD; ++u) {
        const int k = kStageCols * u + iCol;
        if (k < iLenMax)
            head[u] = loadPack<false, int, 4>(iBase + (long long)k * hs);
        else
            head[u] = Pack<int, 4>{{0, 0, 0, 0}};
    }
#pragma unroll
    for (int u = 0; u < HEAD; ++u)
        widen(head[u], kStageCols * u + iCol, lo, hi);
    blockWindow(lo, hi);
    int blockLongest = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w)
        blockLongest = waveLongest[w] > blockLongest ? waveLongest[w] : blockLongest;
    /* scattered matrices already span more than the tile here and skip the rest (workgroup-uniform) */
    const bool fitsSoFar = hi < lo || (long long)hi - lo < a.tileRows;
    if (fitsSoFar && blockLongest > kStageCols * HEAD) {
        constexpr int SCAN = 8; /* 16-byte loads per lane in flight: 32 slab columns per trip */
        for (int k0 = kStageCols * HEAD; k0 < groupLongest; k0 += kStageCols * SCAN) {
            Pack<int, 4> c4[SCAN];
#pragma unroll
            for (int u = 0; u < SCAN; ++u) {
                const int k = k0 + kStageCols * u + iCol;
                if (k < iLenMax)
                    c4[u] = loadPack<false, int, 4>(iBase + (long long)k * hs);
            }
#pragma unroll
            for (int u = 0; u < SCAN; ++u) {
                const int k = k0 + kStageCols * u + iCol;
                if (k < iLenMax)
                    widen(c4[u], k, lo, hi);
            }
        }
        blockWindow(lo, hi);
    }
    const bool useTile = fitsSoFar && hi >= lo && (long long)hi - lo < a.tileRows; /* workgroup-uniform */
    if constexpr (PITCH) /* 16-byte pieces of the vectors start at multiples of 16 bytes; a.tileRows leaves room for it */
        lo = hi >= lo ? lo & ~(16 / (int)sizeof(T) - 1) : lo;

    /* BAND wavefronts.  In a band or stencil matrix in natural order row r + 1 names the columns of row r shifted by one, and a
     * row's entries ascend by one: over the 8 rows of a team and 8 slab columns only 15 different X rows occur, each used up to 8
     * times.  A wavefront all of whose 64 rows have that shape through ALL their columns -- column of (row i, slab column k) =
     * bandBase + k + i, every row exactly groupLongest <= 32 entries long; checked here against the indices of the head, one
     * ballot -- takes a loop of its own below: a team keeps a sliding window of 8 X rows in registers and reads ONE new row per
     * slab column from the tile instead of 8, needs no offsets from the loader lanes (only the coefficients go through LDS), and
     * never looks at an index again (the head's 32 registers are dead in that loop: the window takes their place).  It is the
     * SpMM counterpart of the SpMV's strip x loads.  Same products, added in the same order: ascending k. */
    int bandBase = -1; /* relative to lo; wavefront-uniform */
    if (useTile && groupLongest > 0 && groupLongest <= kStageCols * HEAD && groupLongest % (kStageCols * TRIP) == 0) {
        const int base = __builtin_amdgcn_readfirstlane(head[0].v[0] - a.baseIndex - lo);
        bool off = false;
#pragma unroll
        for (int u = 0; u < HEAD; ++u) {
            const int k = kStageCols * u + iCol;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                off |= k < groupLongest && (iLen[j] != groupLongest || head[u].v[j] - a.baseIndex - lo != base + k + 32 * iHalf + 4 * iQ + j);
        }
        bandBase = __ballot(off) == 0ull && groupRow0 + kWave <= a.rows ? base : -1;
    }

    auto loadTrip = [&](int k0, Trip& t) {
#pragma unroll
        for (int s = 0; s < TRIP; ++s) {
            const int ki = k0 + kStageCols * s + iCol;
            if (k0 + kStageCols * s < kStageCols * HEAD) { /* uniform: still in the registers of the prologue */
                t.idx[s] = head[0];
#pragma unroll
                for (int u = 0; u + 1 < HEAD; ++u)
                    head[u] = head[u + 1];
            } else if (ki < iLenMax) {
                t.idx[s] = loadPack<true, int, 4>(iBase + (long long)ki * hs);
            } else {
                t.idx[s] = Pack<int, 4>{{0, 0, 0, 0}};
            }
#pragma unroll
            for (int j = 0; j < COEF_LOADS; ++j) {
                const int kc = k0 + kStageCols * s + COLS_PER_COEF_LOAD * j + cCol;
                if (kc < cLenMax) {
                    t.coef[s * COEF_LOADS + j] = loadPack<true, T, CR>(cBase + (long long)kc * hs);
                } else {
#pragma unroll
                    for (int e = 0; e < CR; ++e)
                        t.coef[s * COEF_LOADS + j].v[e] = zeroOf<T>();
                }
            }
        }
    };
    auto loadTripIdx = [&](Trip& t) { /* of the first trips: from the registers of the prologue */
        static_assert(2 * TRIP <= HEAD, "the first two trips' indices are in the head");
#pragma unroll
        for (int s = 0; s < TRIP; ++s) {
            t.idx[s] = head[0];
#pragma unroll
            for (int u = 0; u + 1 < HEAD; ++u)
                head[u] = head[u + 1];
        }
    };
    if (useTile) {
        /* the first two trips' coefficients are requested before the tile is filled: one memory round trip for both */
        loadTripCoef(0, cur);
        loadTripCoef(STEP, next);
        loadTripIdx(cur);
        loadTripIdx(next);
        fillTile(lo, hi - lo + 1);
    }
    /* (global_load_lds retires on vmcnt like any load, and the barrier below is what hands the tile to the other wavefronts:
     * the wait is spelled out rather than left to whatever else happens to be waited for here) */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    T sum[KP][VEC];
#pragma unroll
    for (int i = 0; i < KP; ++i)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            sum[i][e] = zeroOf<T>();

    if (bandBase >= 0) {
        static_assert(kStageCols * TRIP == KP, "the window's names come round once per trip");
        const int team = lane / KP;
        const int rhs0 = (lane % KP) * VEC;
        const int rhsSafe = rhs0 < a.count ? rhs0 : 0;
        const unsigned char* const myTile = reinterpret_cast<const unsigned char*>(tile) + rhsSafe * sizeof(T);
        auto tileRow = [&](int r) { return loadPack<false, T, VEC>(reinterpret_cast<const T*>(myTile + tileOffset(r))); };
        /* X rows first + C .. first + C + 7 of slab column C (counted from 0), by rotating name: row first + C + i sits in
         * window[(C + i) % 8]; a trip of 8 columns brings the names round once, so the window carries on from trip to trip */
        int newest = bandBase + KP * team + KP - 1; /* the row that enters with the next slab column */
        Pack<T, VEC> window[KP];
#pragma unroll
        for (int i = 0; i + 1 < KP; ++i)
            window[i] = tileRow(newest - (KP - 1) + i);
        Pack<T, CR> coefNow[TRIP * COEF_LOADS], coefNext[TRIP * COEF_LOADS];
#pragma unroll
        for (int q = 0; q < TRIP * COEF_LOADS; ++q) { /* requested with the tile fill, above */
            coefNow[q] = cur.coef[q];
            coefNext[q] = next.coef[q];
        }
        /* every row of the wavefront is groupLongest long: the bounds of the coefficient loads are wavefront-uniform, and a
         * lane's loads of one trip differ from the previous trip's by a uniform stride */
        const T* coefAt = cBase + ((long long)(2 * STEP) + cCol) * hs; /* this lane's first load of the trip after next */
        const long long tripStride = (long long)STEP * hs, loadStride = (long long)COLS_PER_COEF_LOAD * hs, stageStride = (long long)kStageCols * hs;
        const T* const stageCoefRead = &stage->coef[0][KP * team];
        T* const stageCoefWrite = &stage->coef[cCol][32 * cHalf + CR * cQ];
#pragma clang loop unroll(disable)
        for (int k0 = 0; k0 < groupLongest; k0 += STEP) {
            /* the trip after next: coefficients only, requested BEFORE this trip is consumed (a third set of registers: this
             * loop has them to spare), so that all of a 32-column row's matrix bytes are on their way within the first trip */
            Pack<T, CR> coefAfter[TRIP * COEF_LOADS];
            if (k0 + 2 * STEP < groupLongest) { /* wavefront-uniform */
#pragma unroll
                for (int s = 0; s < TRIP; ++s)
#pragma unroll
                    for (int j = 0; j < COEF_LOADS; ++j)
                        coefAfter[s * COEF_LOADS + j] = loadPack<true, T, CR>(coefAt + s * stageStride + j * loadStride);
            }
            coefAt += tripStride;
#pragma unroll
            for (int s = 0; s < TRIP; ++s) {
                waveSync();
#pragma unroll
                for (int j = 0; j < COEF_LOADS; ++j)
                    storePack<T, CR>(stageCoefWrite + COLS_PER_COEF_LOAD * j * kWave, coefNow[s * COEF_LOADS + j]);
                waveSync();
#pragma unroll
                for (int c = 0; c < kStageCols; ++c) {
                    const int C = kStageCols * s + c; /* compile-time after unrolling */
                    window[(C + KP - 1) % KP] = tileRow(newest);
                    newest += 1;
#pragma unroll
                    for (int i0 = 0; i0 < KP; i0 += 4) {
                        T coef[4];
#pragma unroll
                        for (int j0 = 0; j0 < 4; j0 += CR) {
                            const Pack<T, CR> part = loadPack<false, T, CR>(stageCoefRead + c * kWave + i0 + j0);
#pragma unroll
                            for (int j = 0; j < CR; ++j)
                                coef[j0 + j] = part.v[j];
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int e = 0; e < VEC; ++e)
                                sum[i0 + i][e] = mulAdd(coef[i], window[(C + i0 + i) % KP].v[e], sum[i0 + i][e]);
                        /* The multiply-adds have no place of their own in the order of the block (nothing but the next
                         * iteration needs the sums): left alone, the compiler gathers all 128 of a trip behind all 40 LDS
                         * reads and spills what the reads delivered.  The empty statements tie each chunk's sums down here. */
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int e = 0; e < VEC; ++e)
                                asm volatile("" : "+v"(sum[i0 + i][e]));
                        __builtin_amdgcn_sched_barrier(0); /* keep the reads of later chunks from being hoisted: registers */
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < TRIP * COEF_LOADS; ++q) {
                coefNow[q] = coefNext[q];
                coefNext[q] = coefAfter[q];
            }
        }
    } else if (!useTile) {
        /* window too wide for the tile: one row per lane, X through L1/L2 (the plain kernel's loop) */
        const long long myRow = groupRow0 + lane;
        int myLen = 0;
        long long slab = 0;
        if (myRow < a.rows) {
            const unsigned hack = (unsigned)myRow / hs;
            slab = (long long)a.hackOffsets[hack] + ((unsigned)myRow - hack * hs);
            myLen = a.rS[myRow];
        }
        spmmAccumulate<T, KP, VEC, 2, false, PITCH>(a, lane, myLen, groupLongest, a.cM + slab, a.rP + slab, nullptr, 0, sum);
    } else {
        const int team = lane / KP;
        const int rhs0 = (lane % KP) * VEC;
        const int rhsSafe = rhs0 < a.count ? rhs0 : 0; /* lanes beyond `count` read a valid slice, result discarded */
        const unsigned char* const myTile = reinterpret_cast<const unsigned char*>(tile) + rhsSafe * sizeof(T);

        /* wavefront-uniform: every row of the wavefront has an entry in every column of the trip */
        auto allPresent = [&](const Trip& t, int k0) {
            bool absent = false;
#pragma unroll
            for (int s = 0; s < TRIP; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    absent |= !(k0 + kStageCols * s + iCol < iLen[j] && t.idx[s].v[j] - a.baseIndex >= 0);
            return __ballot(absent) == 0ull;
        };
        auto publish = [&](const Trip& t, int s, int k0) {
            const int ki = k0 + kStageCols * s + iCol;
            Pack<int, 4> at4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = t.idx[s].v[j] - a.baseIndex;
                at4.v[j] = ki < iLen[j] && c >= 0 ? tileOffset(c - lo) : -1;
            }
            storePack<int, 4>(&stage->at[iCol][32 * iHalf + 4 * iQ], at4);
#pragma unroll
            for (int j = 0; j < COEF_LOADS; ++j)
                storePack<T, CR>(&stage->coef[COLS_PER_COEF_LOAD * j + cCol][32 * cHalf + CR * cQ], t.coef[s * COEF_LOADS + j]);
        };
        /* (Tried: the offsets -- and the coefficients -- of the next 4 rows read one step ahead, so that a wavefront does not go
         * through two dependent LDS round trips per 8 fused multiply-adds.  Offsets only: within the noise; both: +12 registers
         * at 168, spills inside this loop, 0.97 ms against 0.65.) */
        auto consume = [&](auto allPresent) {
            constexpr bool ALL_PRESENT = decltype(allPresent)::value;
#pragma unroll
            for (int c = 0; c < kStageCols; ++c) {
#pragma unroll
                for (int i0 = 0; i0 < KP; i0 += 4) { /* 4 rows of the team at a time */
                    T coef[4];
                    Pack<T, VEC> xv[4];
                    const Pack<int, 4> at = loadPack<false, int, 4>(&stage->at[c][KP * team + i0]);
#pragma unroll
                    for (int j0 = 0; j0 < 4; j0 += CR) {
                        const Pack<T, CR> part = loadPack<false, T, CR>(&stage->coef[c][KP * team + i0 + j0]);
#pragma unroll
                        for (int j = 0; j < CR; ++j)
                            coef[j0 + j] = part.v[j];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        xv[i] = loadPack<false, T, VEC>(reinterpret_cast<const T*>(myTile + (ALL_PRESENT || at.v[i] >= 0 ? at.v[i] : 0)));
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int e = 0; e < VEC; ++e) {
                            const T next = mulAdd(coef[i], xv[i].v[e], sum[i0 + i][e]);
                            sum[i0 + i][e] = ALL_PRESENT ? next : pick(at.v[i] >= 0, next, sum[i0 + i][e]);
                        }
                    __builtin_amdgcn_sched_barrier(0); /* keep the reads of later chunks from being hoisted: registers */
                }
            }
        };
        auto runTrip = [&](const Trip& t, int k0, auto mode) {
#pragma unroll
            for (int s = 0; s < TRIP; ++s) {
                if (k0 + kStageCols * s < groupLongest) { /* wavefront-uniform */
                    waveSync();
                    publish(t, s, k0);
                    waveSync();
                    consume(mode);
                }
            }
        };
        /* Two loops rather than a per-stage choice: absent entries only appear in the last columns of ragged rows,
         * and one loop body per mode keeps the 32 running sums in one set of registers. */
        int k0 = 0;
#pragma clang loop unroll(disable)
        while (k0 < groupLongest && allPresent(cur, k0)) {
            runTrip(cur, k0, std::true_type{});
            cur = next;
            k0 += STEP;
            loadTrip(k0 + STEP, next); /* in flight (vmcnt) while the next trip runs on LDS (lgkmcnt) */
        }
#pragma clang loop unroll(disable)
        while (k0 < groupLongest) {
            runTrip(cur, k0, std::false_type{});
            cur = next;
            k0 += STEP;
            loadTrip(k0 + STEP, next);
        }
    }
    if (groupRow0 >= a.rows)
        return;
    if constexpr (PITCH)
        spmmStorePitch<T, KP, VEC>(a, lane, groupRow0, sum);
    else
        spmmStore<T, KP, VEC>(a, lane, groupRow0, sum);
}

} // namespace spgpu
