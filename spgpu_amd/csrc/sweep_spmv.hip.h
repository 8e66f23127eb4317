/* Included by ellpack_spmv.hip (namespace spgpu, after SlabArgs); launched by launchSweep there. */
/*
 * SWEEP form (include/spgpu/tuning.h; the caller's hint, and AUTO's choice for 8-byte elements when the probe finds such a
 * matrix): for matrices whose columns are scattered over all of x but ascend inside a row.  A lane owns PACKS packs of VEC
 * neighbouring rows (32 rows for 4- and 8-byte elements) and carries all of them through the slab columns in step; the grid
 * is small enough to be resident at once and walks the rows with a tile stride.  At any moment the rows in flight are at
 * about the same k, i.e. they gather from about the same quantile of x, and meet in L2: 10 M x 32 scattered, fp64: L2 hits
 * 22 M -> 54 M of 320 M gathers, 5.85 -> 4.5 ms.  No LDS; coefficient and index streams non-temporal.
 *
 * Order of additions.  TAIL = false: a row's products in ascending k (orc_?hellspmv / orc_?ellspmv with one phase), the
 * reference's one-thread-per-row order (hell_spmv_base_template.cuh:104-215).  TAIL = true (the types whose default kernel
 * walks whole rows: 8-byte elements): exactly that kernel's order -- pack u of a wavefront is the 64 * VEC consecutive rows
 * one of its wavefronts owns, the group hands its last rows to the whole wavefront at the slab column at which that
 * kernel would (first multiple of 8 with at most tailLanes lanes still busy; slabSpmvKernel, TAIL), and they are finished
 * the same way: so AUTO may pick this form without changing a bit of z.
 */
template <typename T, int VEC, int PACKS, bool IS_HELL, bool HAS_BETA, bool TAIL>
__global__ __launch_bounds__(kBlockThreads) void sweepSpmvKernel(const SlabArgs<T> a)
{
    const long long packs = ((long long)a.rows + VEC - 1) / VEC;
    constexpr long long TILE = (long long)kBlockThreads * PACKS;
    constexpr int TAIL_STRIDE = 8; /* the stage of the default kernel of the 8-byte types (launchSlabFamily: 1 phase x 8 columns) */
    const int lane = threadIdx.x & (kWave - 1);
    for (long long base = (long long)blockIdx.x * TILE; base < packs; base += (long long)gridDim.x * TILE) {
        T sums[PACKS][VEC];
        int len[PACKS][VEC];
        long long slot[PACKS];
        int tailFrom[PACKS]; /* TAIL: pack u walks the slab columns below tailFrom[u] here (wavefront-uniform) */
        int longest = 0;
        unsigned tails = 0u; /* TAIL: packs whose wavefront has tail rows (wavefront-uniform) */
#pragma unroll
        for (int u = 0; u < PACKS; ++u) {
            const long long row = (base + u * kBlockThreads + threadIdx.x) * VEC;
            slot[u] = 0;
            if (row < a.rows) {
                if constexpr (IS_HELL) {
                    const unsigned r0 = (unsigned)row, hs = (unsigned)a.hackSize;
                    const unsigned hack = r0 / hs;
                    slot[u] = (long long)a.hackOffsets[hack] + (r0 - hack * hs);
                } else {
                    slot[u] = row;
                }
            }
            int packLongest = 0;
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                sums[u][t] = zeroOf<T>();
                len[u][t] = row + t < a.rows ? (a.rS ? a.rS[row + t] : a.maxNnz) : 0;
                packLongest = len[u][t] > packLongest ? len[u][t] : packLongest;
            }
            tailFrom[u] = 0x7fffffff;
            if constexpr (TAIL) {
                const int groupLongest = waveMax(packLongest);
                for (int kBase = 0; kBase < groupLongest; kBase += TAIL_STRIDE) {
                    if (__popcll(__ballot(kBase < packLongest)) <= a.tailLanes) {
                        tailFrom[u] = kBase;
                        tails |= 1u << u;
                        break;
                    }
                }
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    len[u][t] = len[u][t] < tailFrom[u] ? len[u][t] : tailFrom[u];
                packLongest = packLongest < tailFrom[u] ? packLongest : tailFrom[u];
            }
            longest = packLongest > longest ? packLongest : longest;
        }
        for (int k = 0; k < longest; ++k) {
            Pack<T, VEC> v[PACKS];
            Pack<int, VEC> c[PACKS];
#pragma unroll
            for (int u = 0; u < PACKS; ++u) {
                bool any = false;
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    any |= k < len[u][t];
                if (any) {
                    v[u] = loadPack<true, T, VEC>(a.cM + slot[u] + (long long)k * a.valStride);
                    c[u] = loadPack<true, int, VEC>(a.rP + slot[u] + (long long)k * a.idxStride);
                } else {
#pragma unroll
                    for (int t = 0; t < VEC; ++t)
                        c[u].v[t] = a.baseIndex;
                }
            }
#pragma unroll
            for (int u = 0; u < PACKS; ++u) {
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    const int col = c[u].v[t] - a.baseIndex;
                    const bool use = k < len[u][t] && col >= 0;
                    const T xv = a.x[use ? col : 0];
                    if (use)
                        sums[u][t] = mulAdd(v[u].v[t], xv, sums[u][t]);
                }
            }
        }
        if constexpr (TAIL) {
            /* the rows a group handed over: one at a time by the WHOLE wavefront, as slabSpmvKernel's tail does -- lane l takes
             * the entries tailFrom + l, + 64, ..., the 64 partial sums are combined with lane-xor shuffles and added to the
             * owner's running sum */
            if (tails != 0u) { /* wavefront-uniform */
#pragma unroll
                for (int u = 0; u < PACKS; ++u) {
                    if (!(tails & (1u << u)))
                        continue;
                    const long long row = (base + u * kBlockThreads + threadIdx.x) * VEC;
                    int full[VEC], fullLongest = 0; /* the lengths again: len[] was cut at tailFrom */
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        full[t] = row + t < a.rows ? (a.rS ? a.rS[row + t] : a.maxNnz) : 0;
                        fullLongest = full[t] > fullLongest ? full[t] : fullLongest;
                    }
                    const int from = tailFrom[u];
                    unsigned long long pending = __ballot(from < fullLongest);
                    while (pending) { /* wavefront-uniform */
                        const int owner = __ffsll((long long)pending) - 1;
                        pending &= pending - 1;
                        const long long ownerSlot = __shfl(slot[u], owner, kWave);
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            const int rowLen = __shfl(full[t], owner, kWave);
                            if (rowLen <= from)
                                continue;
                            const T* __restrict__ rowVals = a.cM + ownerSlot + t;
                            const int* __restrict__ rowIdxs = a.rP + ownerSlot + t;
                            T part = zeroOf<T>();
                            for (int k0 = from + lane; k0 < rowLen + (kTailUnroll - 1) * kWave; k0 += kTailUnroll * kWave) {
                                T tv[kTailUnroll];
                                int tc[kTailUnroll];
#pragma unroll
                                for (int q = 0; q < kTailUnroll; ++q) {
                                    const int k = k0 + q * kWave;
                                    const bool in = k < rowLen;
                                    tv[q] = in ? rowVals[(long long)k * a.valStride] : zeroOf<T>();
                                    tc[q] = in ? rowIdxs[(long long)k * a.idxStride] - a.baseIndex : -1;
                                }
                                T tx[kTailUnroll];
#pragma unroll
                                for (int q = 0; q < kTailUnroll; ++q)
                                    tx[q] = a.x[tc[q] >= 0 ? tc[q] : 0];
#pragma unroll
                                for (int q = 0; q < kTailUnroll; ++q)
                                    part = pick(tc[q] >= 0, mulAdd(tv[q], tx[q], part), part);
                            }
#pragma unroll
                            for (int m = 1; m < kWave; m <<= 1)
                                part = add(part, laneXor(part, m));
                            if (lane == owner)
                                sums[u][t] = add(sums[u][t], part);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PACKS; ++u) {
            const long long row = (base + u * kBlockThreads + threadIdx.x) * VEC;
            if (a.wideIO && row + VEC <= a.rows) {
                Pack<T, VEC> out, yv;
                if constexpr (HAS_BETA)
                    yv = loadPack<false, T, VEC>(a.y + row);
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    out.v[t] = epilogue<HAS_BETA>(a.alpha, sums[u][t], a.beta, HAS_BETA ? yv.v[t] : zeroOf<T>());
                storePack<T, VEC>(a.z + row, out);
            } else {
#pragma unroll
                for (int t = 0; t < VEC; ++t)
                    if (row + t < a.rows)
                        a.z[row + t] = epilogue<HAS_BETA>(a.alpha, sums[u][t], a.beta, HAS_BETA ? a.y[row + t] : zeroOf<T>());
            }
        }
    }
}
