/*
 * slabSpmvKernel, the ELL / HELL SpMV kernel for rows as they come.  Included by ellpack_spmv.hip (namespace spgpu), which picks its form.
 * ---- Wavefront design ("slab" kernel) ------------------------------------
 * Both formats store a block of 32 consecutive rows as a column-major slab:
 * element (row r, k-th entry) sits at  slabBase + r%32 + k*stride  with
 * stride = hackSize (HELL) or the pitch (ELL).  One 64-lane wavefront owns
 * one such 32-row group (for hackSize == 32: exactly one hack).
 *
 *   RPL   = rows per lane = 16 B / sizeof(T)  (S:4  D:2  C:2  Z:1)
 *   LPC   = 32 / RPL lanes cover one slab column with one 16-B load each
 *   PH    = 64 / LPC = 2*RPL "phases": lane group p handles entries k = p, p+PH, ...
 *
 * A wave-wide load therefore moves PH slab columns at once: 1 KiB of
 * coefficients (global_load_dwordx4 per lane) plus the matching indices,
 * and for hackSize == 32 those PH columns are contiguous in memory, so the
 * wave streams the hack front to back in 1-KiB pieces.  Each lane gathers
 * x for its RPL rows, keeps RPL running sums, and the PH partial sums of a
 * row are combined with log2(PH) lane-xor shuffles (DPP / ds_bpermute; no LDS,
 * no barrier).  Lanes of phase 0 apply alpha/beta and write RPL consecutive z
 * values with one wide store.
 *
 * Summation order of one row: entries k = p (mod PH) are accumulated in
 * ascending k per phase p, then phases are added pairwise (xor tree).  For
 * PH == 2 (double complex) this is exactly the reference's two-threads-per-row
 * order (hell_spmv_base_template.cuh:59-101).
 *
 * The same kernel template with RPL == 1 (element loads) and/or PH == 1 (a
 * lane walks whole rows) takes the cases the wide form cannot: streams that
 * are not 16-byte aligned, odd pitches, hackSize not a multiple of RPL
 * (every lane derives its hack from its own first row, so any hackSize works).
 *
 * Roofline: HBM bandwidth.  Algorithmic bytes per nonzero: sizeof(T) + 4;
 * per row: 4 (rS) + sizeof(T) (z) [+ sizeof(T) for y when beta != 0]
 * [+ 4 for rIdx]; per column: sizeof(T) (x once); per hack: 4.
 */

/* Function-scope LDS: only kernels that call this allocate it (the forms without a tile keep 0 bytes of LDS). */
template <typename E, int N> __device__ inline E* ldsArray()
{
    __shared__ __attribute__((aligned(16))) E buffer[N];
    return buffer;
}

/* The wavefronts that report the form they ran in: about the quarter points of the matrix, nudged off them -- grid
 * problems put their boundary rows (the ones that never qualify) exactly on power-of-two row numbers. */
__device__ inline long long sampleGroup(long long groups, int q)
{
    const long long at = groups * q / 4 + 2 * q + 1;
    return at < groups ? at : groups - 1;
}

/*
 * RPL    rows per lane (1, or 16/sizeof(T) with 16-byte loads)
 * PH     phases: lane groups that split the entries of a row by k mod PH
 *        (PH == 1: a lane walks all entries of its rows, no cross-lane sum)
 * UNROLL slab-column loads issued back to back before the first gather
 * PIPE   the next stage is prefetched while the current one is consumed (every kernel but that of the Lean route, spmv_rules.h)
 * One wavefront owns 64/PH strips = (64/PH)*RPL consecutive rows.
 * STRIPS compiles the strip-load form in (see consume below); the form without it exists as well because the mere
 *        presence of the second loop costs the gather loop ~8 % on scattered matrices (measured; same instruction
 *        counts, so a placement / allocation effect), and the host picks per matrix (launchSlabFamily).
 * PACKED a FROZEN matrix without a row order (spgpu?SpmvFreeze, include/spgpu/tuning.h; frozen_slab.hip.h): the stage loads read
 *        the column indices from the library's 16-bit copy (a.planPacked: offsets from the group's a.packBases[group], slot for
 *        slot as in rP; 0xFFFF = "ask rP") -- 2 bytes per stored entry instead of 4.  Same columns, same order: same bits.  The
 *        rare paths (whole-wave tail rows, the sample wavefronts' span) read rP itself, which the caller's promise keeps valid.
 */
template <typename T, int RPL, int PH, bool IS_HELL, bool NT, int UNROLL, bool PIPE, bool TAIL, bool STRIPS = false,
          int BLOCK = kBlockThreads, int TILE_BYTES = 0, int TAIL_EVERY = 0, bool PACKED = false>
__global__ __launch_bounds__(BLOCK) void slabSpmvKernel(const SlabArgs<T> a)
{
    /* (PACKED, measured: the fp64 kernel needs 140 VGPRs -- 3 wavefronts per SIMD, as the unpacked kernel's 146.  Capped at 128 for a
     * fourth wavefront -- amdgpu_waves_per_eu(4, 4) -- it spills 52-64 bytes per lane into its stage loop: 0.575 -> 0.896 ms; with
     * the stage consumed in two halves (16 instead of 32 registers of x alive) 56-152 bytes still.) */
    static_assert(!PACKED || (TILE_BYTES == 0 && RPL >= 2), "packed indices: the gather and strip forms of 4- and 8-byte elements");
    using ColumnWord = typename std::conditional<PACKED, unsigned short, int>::type;
    constexpr int LPC = kWave / PH;         /* lanes that cover one slab column */
    constexpr int GROUP_ROWS = LPC * RPL;   /* rows owned by the wavefront */
    constexpr int WAVES = BLOCK / kWave;
    constexpr bool XTILE = TILE_BYTES > 0;  /* the workgroup stages the slice of x its rows touch in LDS */
    constexpr int TILE_ELEMS = TILE_BYTES / (int)sizeof(T);

    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane % LPC;   /* which RPL-row strip of the group */
    const int phase = lane / LPC; /* which residue class of k */
    const T* __restrict__ x = a.x;
    auto groupOf = [&]() -> long long { /* the group of rows this wavefront owns */
        const int wave = threadIdx.x >> 6;
        return (long long)blockIdx.x * WAVES + wave;
    };

    /* XTILE: x[tileBase .. tileBase + tileCount) lives in `tile` once the prologue below has run */
    T* tile = nullptr;
    int tileBase = 0;
    unsigned tileCount = 0;
    if constexpr (XTILE) {
        tile = ldsArray<T, TILE_ELEMS>();
        /* Which slice of x?  Every row of the workgroup is sampled at its first and its last entry (the extremes of a
         * row whose columns ascend; any row order is still correct, entries outside the tile are gathered from global
         * memory).  If the span of the workgroup's rows fits the tile it starts at the lowest column, otherwise it is
         * centred on the mean of the rows' middles (a few far-away rows then do not drag it off). */
        ColumnProbe mine{0x7fffffff, -0x7fffffff - 1, 0, 0};
        if (phase == 0) {
            int first[RPL], last[RPL], lenAt[RPL];
            /* (a one-trip loop for the same reason as the one around processGroup below) */
#pragma unroll
            for (int once = 0; once < 1; ++once) {
                const long long r0 = groupOf() * GROUP_ROWS + (long long)sub * RPL;
                long long at = 0;
                if (r0 < a.rows) {
                    if constexpr (IS_HELL) {
                        const unsigned u0 = (unsigned)r0, hs = (unsigned)a.hackSize;
                        at = (long long)a.hackOffsets[u0 / hs] + (u0 % hs);
                    } else {
                        at = r0;
                    }
                }
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    const long long r = r0 + t;
                    lenAt[t] = r < a.rows ? (a.rS ? a.rS[r] : a.maxNnz) : 0;
                    first[t] = lenAt[t] > 0 ? a.rP[at + t] : 0;
                    last[t] = lenAt[t] > 0 ? a.rP[at + t + (long long)(lenAt[t] - 1) * a.idxStride] : 0;
                }
            }
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                if (lenAt[t] > 0) {
                    const int f = first[t] - a.baseIndex, l = last[t] - a.baseIndex;
                    const int low = f < l ? f : l, high = f < l ? l : f;
                    mine.lowest = low < mine.lowest ? low : mine.lowest;
                    mine.highest = high > mine.highest ? high : mine.highest;
                    mine.middles += ((long long)f + l) >> 1;
                    mine.rows += 1;
                }
            }
        }
        mine.lowest = waveMin(mine.lowest);
        mine.highest = waveMax(mine.highest);
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) {
            mine.rows += laneXor(mine.rows, m);
            const int lowHalf = laneXor((int)(unsigned)(mine.middles & 0xffffffffll), m);
            const int highHalf = laneXor((int)(mine.middles >> 32), m);
            mine.middles += ((long long)highHalf << 32) | (unsigned)lowHalf;
        }
        ColumnProbe* seen = ldsArray<ColumnProbe, WAVES>();
        if (lane == 0)
            seen[threadIdx.x >> 6] = mine;
        __syncthreads();
        ColumnProbe all{0x7fffffff, -0x7fffffff - 1, 0, 0};
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const ColumnProbe other = seen[w];
            all.lowest = other.lowest < all.lowest ? other.lowest : all.lowest;
            all.highest = other.highest > all.highest ? other.highest : all.highest;
            all.rows += other.rows;
            all.middles += other.middles;
        }
        if (all.rows > 0 && all.lowest >= 0) {
            const long long span = (long long)all.highest - all.lowest + 1;
            if (span <= TILE_ELEMS) {
                tileBase = all.lowest;
                tileCount = (unsigned)span;
            } else {
                long long start = all.middles / all.rows - TILE_ELEMS / 2;
                start = start < all.lowest ? all.lowest : start;
                start = start + TILE_ELEMS > (long long)all.highest + 1 ? (long long)all.highest + 1 - TILE_ELEMS : start;
                tileBase = (int)start;
                tileCount = TILE_ELEMS;
            }
        }
        /* coalesced copy: 16-byte pieces (global memory takes them at any element address), 4 per lane in flight */
        constexpr int PIECE = 16 / (int)sizeof(T);
        const T* __restrict__ from = x + tileBase;
        const unsigned pieces = tileCount / PIECE;
        for (unsigned p0 = threadIdx.x; p0 < pieces; p0 += 4u * BLOCK) {
            Pack<T, PIECE> w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (p0 + q * BLOCK < pieces)
                    w[q] = loadPackElementAligned<T, PIECE>(from + (size_t)(p0 + q * BLOCK) * PIECE);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (p0 + q * BLOCK < pieces)
                    storePack<T, PIECE>(tile + (size_t)(p0 + q * BLOCK) * PIECE, w[q]);
        }
        if (pieces * PIECE + threadIdx.x < tileCount)
            tile[pieces * PIECE + threadIdx.x] = from[pieces * PIECE + threadIdx.x];
        __syncthreads();
    }

    auto processGroup = [&](const long long group) {
    const long long groupRow0 = group * GROUP_ROWS;
    if (groupRow0 >= a.rows)
        return; /* whole wavefront leaves together (the workgroup's barriers are behind it) */
    const long long row0 = groupRow0 + (long long)sub * RPL;
    const bool stripLive = row0 < a.rows;

    /* First slot of this lane's strip, in elements. */
    long long slab = 0;
    if (stripLive) {
        if constexpr (IS_HELL) {
            const unsigned r0 = (unsigned)row0, hs = (unsigned)a.hackSize;
            const unsigned hack = r0 / hs;
            slab = (long long)a.hackOffsets[hack] + (r0 - hack * hs);
        } else {
            slab = row0;
        }
    }

    int len[RPL];
    int laneLongest = 0;
#pragma unroll
    for (int t = 0; t < RPL; ++t) {
        const long long r = row0 + t;
        len[t] = r < a.rows ? (a.rS ? a.rS[r] : a.maxNnz) : 0;
        laneLongest = len[t] > laneLongest ? len[t] : laneLongest;
    }
    const int groupLongest = waveMax(laneLongest); /* wave-uniform trip count */

    T sum[RPL];
#pragma unroll
    for (int t = 0; t < RPL; ++t)
        sum[t] = zeroOf<T>();

    const T* __restrict__ vals = a.cM + slab;
    const int* __restrict__ idxs = a.rP + slab;
    /* PACKED: the group's 16-bit words count from here (wave-uniform: one scalar load) */
    int packBase = 0;
    if constexpr (PACKED)
        packBase = a.packBases[group];

    /* One stage = UNROLL slab columns per phase: the coefficient/index loads of a stage are
     * issued back to back (fetch), its x gathers and multiply-adds follow (consume).  With
     * PIPE the next stage is fetched right behind the current stage's x loads, so the stream
     * loads of stage s+1 are in flight while the gathers of stage s wait for x. */
    struct Stage {
        Pack<T, RPL> v[UNROLL];
        Pack<ColumnWord, RPL> c[UNROLL];
    };
    auto fetch = [&](int kBase, Stage& s) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kBase + u * PH + phase;
            if (k < laneLongest) {
                s.v[u] = loadPack<NT, T, RPL>(vals + (long long)k * a.valStride);
                if constexpr (PACKED)
                    s.c[u] = loadPack<NT, unsigned short, RPL>(a.planPacked + slab + (long long)k * a.idxStride);
                else
                    s.c[u] = loadPack<NT, int, RPL>(idxs + (long long)k * a.idxStride);
            } else {
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    s.v[u].v[t] = zeroOf<T>();
                    s.c[u].v[t] = PACKED ? (ColumnWord)0xFFFF : (ColumnWord)a.baseIndex;
                }
            }
        }
    };
    /* the 0-based column of a stage's word (PACKED: base + offset; an escape asks rP) */
    auto columnOf = [&](const Stage& s, int u, int t, int k) -> int {
        if constexpr (PACKED) {
            const unsigned word = s.c[u].v[t];
            if (word == 0xFFFFu)
                return k < len[t] ? idxs[t + (long long)k * a.idxStride] - a.baseIndex : 0;
            return packBase + (int)word;
        } else {
            return s.c[u].v[t] - a.baseIndex;
        }
    };
    /* consume(form, kBase, stage, between): the x values of the stage, then `between()`, then the multiply-adds.
     * vmcnt retires in issue order: loads issued BEFORE the x loads are waited for together with them,
     * loads issued AFTER them (in `between`) stay in flight while the x values are consumed.
     *
     * Strip form: in a stencil or band matrix in natural order neighbouring rows name neighbouring columns, so the RPL
     * x values of a strip are consecutive and come with ONE element-aligned 16-byte load instead of RPL gathers.
     * Whether a stage qualifies is a wavefront-uniform test (stageIsStrips; a per-lane choice is folded back into
     * element loads by the compiler), and a wavefront that meets scattered columns once stops testing.  The two
     * forms are separate loops on purpose: joined in one loop body their wait counts have to cover both load
     * patterns and the gathers end up waited for together with the prefetch (windowed pattern 1.38 -> 1.64 ms). */
    auto consume = [&](auto stripsTag, int kBase, const Stage& s, auto&& between) {
        constexpr bool AS_STRIPS = decltype(stripsTag)::value;
        T xv[UNROLL][RPL];
        bool use[UNROLL][RPL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kBase + u * PH + phase;
            if constexpr (AS_STRIPS) {
                /* stageIsStrips: in this slab column the rows of the strip are all present (consecutive columns) or
                 * all past their end */
                const bool present = k < len[0];
                /* an absent strip still issues its load (no divergence in the stage): from the coefficient array, which
                 * holds at least one whole strip whenever a stage runs -- x itself may be shorter than RPL elements */
                const Pack<T, RPL> w = loadPackElementAligned<T, RPL>(present ? x + (PACKED ? packBase + (int)s.c[u].v[0] : (int)s.c[u].v[0] - a.baseIndex) : a.cM);
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    use[u][t] = present;
                    xv[u][t] = w.v[t];
                }
            } else if constexpr (XTILE) {
                /* from the tile where the column lies inside it (LDS reads retire on lgkmcnt: the stream prefetch,
                 * on vmcnt, stays in flight); the branch over the global gathers is wavefront-uniform per slab
                 * column and not taken when the tile covers the workgroup's columns */
                bool outside = false;
                unsigned at[RPL];
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    const int col = s.c[u].v[t] - a.baseIndex;
                    use[u][t] = k < len[t] && col >= 0;
                    at[t] = (unsigned)(col - tileBase);
                    const bool inside = at[t] < tileCount;
                    outside |= use[u][t] && !inside;
                    xv[u][t] = tile[inside ? at[t] : 0u];
                }
                if (__ballot(outside) != 0ull) {
#pragma unroll
                    for (int t = 0; t < RPL; ++t) {
                        if (use[u][t] && at[t] >= tileCount)
                            xv[u][t] = x[s.c[u].v[t] - a.baseIndex];
                    }
                }
            } else {
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    const int col = columnOf(s, u, t, k);
                    use[u][t] = k < len[t] && col >= 0;
                    xv[u][t] = x[use[u][t] ? col : 0];
                }
            }
        }
        between();
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                sum[t] = pick(use[u][t], mulAdd(s.v[u].v[t], xv[u][t], sum[t]), sum[t]);
            }
        }
    };
    auto stageIsStrips = [&](int kBase, const Stage& s) -> bool { /* wavefront-uniform */
        bool scattered = false;
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const int k = kBase + u * PH + phase;
            const bool present = k < len[0];
#pragma unroll
            for (int t = 0; t < RPL; ++t) { /* all rows of the strip present with consecutive columns, or all absent */
                if constexpr (PACKED) /* (an escape -- 0xFFFF: the column is in rP -- is never part of a strip; a word's column is >= 0) */
                    scattered |= (k < len[t]) != present ||
                                 (present && (s.c[u].v[t] == 0xFFFFu || (unsigned)s.c[u].v[t] != (unsigned)s.c[u].v[0] + (unsigned)t));
                else
                    scattered |= (k < len[t]) != present ||
                                 (present && (s.c[u].v[0] - a.baseIndex < 0 || s.c[u].v[t] != s.c[u].v[0] + t));
            }
        }
        return __ballot(scattered) == 0ull;
    };

    /* the sample wavefronts: first to last column over the group's rows (their first and last entries: the extremes of
     * rows whose columns ascend), or "unbounded" if an index lies below the base */
    auto columnSpan = [&]() -> long long { /* call with the whole wavefront */
        int lowest = 0x7fffffff, highest = -1;
        bool below = false;
        if (phase == 0) {
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                if (len[t] > 0) {
                    const int f = idxs[t] - a.baseIndex, l = idxs[t + (long long)(len[t] - 1) * a.idxStride] - a.baseIndex;
                    below |= f < 0 || l < 0;
                    lowest = f < lowest ? f : lowest;
                    lowest = l < lowest ? l : lowest;
                    highest = f > highest ? f : highest;
                    highest = l > highest ? l : highest;
                }
            }
        }
        lowest = waveMin(lowest);
        highest = waveMax(highest);
        if (__ballot(below) != 0ull)
            return 1ll << 40;
        return highest < lowest ? 0ll : (long long)highest - lowest + 1;
    };

    constexpr int STEP = PH * UNROLL;
    /* TAIL: when at most kTailLanes lanes of the wavefront still have entries left, the
     * slab loop would run on with >= 7/8 of its lanes idle (ragged matrices: one long row keeps a whole
     * group looping).  The loop stops there and the few remaining rows are finished one at a time by the
     * WHOLE wavefront: lane l takes entries tailFrom + l, + 64, ...; the 64 partial sums are combined
     * with lane-xor shuffles and added to the owner lane's running sum. */
    int tailFrom = groupLongest;
    /* TAIL_EVERY: the switch is only considered at multiples of that many columns -- a kernel with shorter stages then
     * adds every row in exactly the order of the kernel whose stage is TAIL_EVERY columns (the x-tile form of the fp64
     * kernels has 4-column stages and must give the bits of the 8-column gather / strip kernels it alternates with) */
    constexpr int TAIL_STRIDE = TAIL_EVERY > 0 ? TAIL_EVERY : PH * UNROLL;
    auto switchToTail = [&](int kBase) -> bool {
        if constexpr (TAIL) {
            if (kBase % TAIL_STRIDE == 0 && __popcll(__ballot(kBase < laneLongest)) <= a.tailLanes) {
                tailFrom = kBase;
                return true;
            }
        }
        return false;
    };
    constexpr bool STRIPS_POSSIBLE = STRIPS && RPL > 1;
    int kBase = 0;
    bool done = false; /* tail taken */
    if constexpr (PIPE) {
        Stage cur, nxt;
        fetch(0, cur);
        /* one stage: `form` says how its x values are fetched */
        auto stage = [&](auto form) {
            /* prefetch issued after the current x loads: younger in vmcnt order, stays in flight; lanes past their rows'
             * end fetch nothing */
            consume(form, kBase, cur, [&] { fetch(kBase + STEP, nxt); });
            cur = nxt;
        };
        if constexpr (STRIPS_POSSIBLE) {
            for (; kBase < groupLongest; kBase += STEP) {
                if (switchToTail(kBase)) {
                    done = true;
                    break;
                }
                if (!stageIsStrips(kBase, cur))
                    break; /* scattered columns: the gather loop takes over from this stage */
                stage(std::true_type{});
            }
            /* three sample wavefronts tell the host which form this matrix runs in (launchSlabFamily): 2 strips,
             * 3 columns inside a window an LDS tile holds, 1 scattered */
            if (a.feedback) {
                const long long groups = ((long long)a.rows + GROUP_ROWS - 1) / GROUP_ROWS;
                if (group == sampleGroup(groups, 1) || group == sampleGroup(groups, 2) || group == sampleGroup(groups, 3)) {
                    /* rows that fit one stage: placing and filling an LDS tile costs two round trips more than the row's
                     * one stage of gathers (1 M-row 5-point Laplacian: 25.9 us through the tile, 19.4 as gathers) */
                    const int other = groupLongest > STEP && columnSpan() <= a.tileSpanLimit ? 3 : 1;
                    for (int q = 1; q <= 3; ++q)
                        if (group == sampleGroup(groups, q) && lane == 0)
                            /* at least half of it as strips -- and more than one stage of it: the test costs about a
                             * third of a stage, which a single stage of strips does not earn back (5-point Laplacian,
                             * 16.7 M rows: 258 us with it, 251 us as gathers) */
                            a.feedback[q - 1] = a.feedbackTag | (2 * kBase >= groupLongest && groupLongest > STEP ? 2 : other);
                }
            }
        }
        /* (the gather-only and x-tile forms do not report: a walk over the sample wavefronts' indices compiled into this
         * kernel cost its hot loop 7-8 % on scattered columns although three wavefronts ran it -- 1.40 -> 1.51 ms on the
         * 65 536-wide window pattern, profiles/r03_ab_gather_feedback.txt; formProbeKernel, form_probe.hip.h, looks instead) */
        if (!done) {
            /* kBase is wavefront-uniform; saying so keeps the loop counter (and every k derived from it) scalar */
            for (kBase = __builtin_amdgcn_readfirstlane(kBase); kBase < groupLongest; kBase += STEP) {
                if (switchToTail(kBase))
                    break;
                stage(std::false_type{});
            }
        }
    } else {
        for (; kBase < groupLongest; kBase += STEP) {
            if (switchToTail(kBase))
                break;
            Stage cur;
            fetch(kBase, cur);
            consume(std::false_type{}, kBase, cur, [] {});
        }
    }

    if constexpr (TAIL) {
        /* all PH lanes of a strip share laneLongest, so they enter and leave `pending` together */
        unsigned long long pending = __ballot(tailFrom < laneLongest);
        while (pending) { /* wave-uniform */
            const int owner = (__ffsll((long long)pending) - 1) % LPC; /* the strip's phase-0 lane */
            pending &= ~__ballot(sub == owner);
            const long long ownerSlab = __shfl(slab, owner, kWave);
#pragma unroll
            for (int t = 0; t < RPL; ++t) {
                const int rowLen = __shfl(len[t], owner, kWave);
                if (rowLen <= tailFrom)
                    continue;
                const T* __restrict__ rowVals = a.cM + ownerSlab + t;
                const int* __restrict__ rowIdxs = a.rP + ownerSlab + t;
                T part = zeroOf<T>();
                for (int k0 = tailFrom + lane; k0 < rowLen + (kTailUnroll - 1) * kWave; k0 += kTailUnroll * kWave) {
                    T tv[kTailUnroll];
                    int tc[kTailUnroll];
#pragma unroll
                    for (int u = 0; u < kTailUnroll; ++u) {
                        const int k = k0 + u * kWave;
                        const bool in = k < rowLen;
                        tv[u] = in ? rowVals[(long long)k * a.valStride] : zeroOf<T>();
                        tc[u] = in ? rowIdxs[(long long)k * a.idxStride] - a.baseIndex : -1;
                    }
                    T tx[kTailUnroll];
#pragma unroll
                    for (int u = 0; u < kTailUnroll; ++u)
                        tx[u] = x[tc[u] >= 0 ? tc[u] : 0];
#pragma unroll
                    for (int u = 0; u < kTailUnroll; ++u)
                        part = pick(tc[u] >= 0, mulAdd(tv[u], tx[u], part), part);
                }
#pragma unroll
                for (int m = 1; m < kWave; m <<= 1)
                    part = add(part, laneXor(part, m));
                if (lane == owner)
                    sum[t] = add(sum[t], part);
            }
        }
    }

    /* Combine the PH phase partials of every row. */
#pragma unroll
    for (int m = LPC; m < kWave; m <<= 1) {
#pragma unroll
        for (int t = 0; t < RPL; ++t)
            sum[t] = add(sum[t], laneXor(sum[t], m));
    }

    if (phase != 0 || !stripLive)
        return;

    const bool hasBeta = isNotZero(a.beta);
    if (!a.rIdx && a.wideIO && row0 + RPL <= a.rows) {
        Pack<T, RPL> out;
        if (hasBeta) {
            const Pack<T, RPL> yv = loadPack<false, T, RPL>(a.y + row0);
#pragma unroll
            for (int t = 0; t < RPL; ++t)
                out.v[t] = epilogue<true>(a.alpha, sum[t], a.beta, yv.v[t]);
        } else {
#pragma unroll
            for (int t = 0; t < RPL; ++t)
                out.v[t] = epilogue<false>(a.alpha, sum[t], a.beta, zeroOf<T>());
        }
        storePack<T, RPL>(a.z + row0, out);
    } else {
#pragma unroll
        for (int t = 0; t < RPL; ++t) {
            const long long r = row0 + t;
            if (r < a.rows) {
                const int outRow = a.rIdx ? a.rIdx[r] : (int)r;
                a.z[outRow] = hasBeta ? epilogue<true>(a.alpha, sum[t], a.beta, a.y[outRow])
                                      : epilogue<false>(a.alpha, sum[t], a.beta, zeroOf<T>());
            }
        }
    }
    }; /* processGroup */

    /* One group per wavefront.  The one-trip loop (and groupOf evaluated here again) is kept for the code it compiles to:
     * called straight, processGroup comes out with other registers and another instruction order in every slab kernel --
     * a change of its own, for its own A/B. */
    for (int once = 0; once < 1; ++once)
        processGroup(groupOf());
}
