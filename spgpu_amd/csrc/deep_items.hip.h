/* The kernels behind a deep list (spgpu_internal.h: SpgpuDeepList).  Included by ellpack_spmv.hip (namespace spgpu): launchDeep. */
/*
 * The columns >= deepCap of the sub-groups (32 rows) the queue kernel registered (raggedSpmvKernel, DEEP), in two launches right behind it.
 *
 * deepItemsKernel: a wavefront per item, an item = CHUNK columns of one sub-group.  The wavefront reads the chunk the
 * way the format stores it -- 32/RPL lanes with RPL rows each cover a slab column, PH = 64 / (32/RPL) columns per load
 * instruction -- UNROLL load instructions per stage, the next stage requested behind the current stage's gathers.  The
 * items of one very deep sub-group and of many shallow ones alike spread over the whole chip (measured before, with a
 * workgroup per hashed queue of sub-groups: 87-139 us for 108 MB, the grid waiting for its fullest queue).
 * A chunk sum = its PH phase sums (each over ascending k) combined pairwise; it goes to deepItemSums.
 * x comes from global memory: these are the few long rows, their own columns give them their locality.
 *
 * deepFinishKernel: 32 lanes per entry.  Sum of one row = what the main kernel left in deepPartials, plus the chunk
 * sums in chunk order (orc_?spmv_deep restates exactly this); then the SpMV epilogue and the store through rIdx.  The
 * workgroup that finishes last zeroes the header: every workgroup has read it by then, and the next call finds an
 * empty list (a captured graph can be replayed).
 */
template <typename T, int RPL, bool IS_HELL, int UNROLL, int CHUNK>
__global__ __launch_bounds__(kBlockThreads) void deepItemsKernel(const SlabArgs<T> a)
{
    constexpr int LPC = 32 / RPL;    /* lanes per slab column of 32 rows */
    constexpr int PH = kWave / LPC;  /* columns per wave-wide load */
    constexpr int STEP = PH * UNROLL;
    static_assert(CHUNK % STEP == 0, "a chunk is a whole number of stages");
    constexpr int WAVES = kBlockThreads / kWave;

    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane % LPC, phase = lane / LPC;
    /* Round trip 1: the header and the item's record together (the grid has a wavefront for every item the list can hold, and
     * the record lies inside the array whatever the header says).  Round trip 2: the row lengths and ALL of the item's slab
     * columns -- the addresses come from the record, and a column below the sub-group's depth exists in the arrays whether a
     * given row reaches it or not (what lies there is never used: the test is k < len).  Round trips 3 and 4: the gathers of
     * the two halves.  (Before: header, entry number, entry, lengths and hack offset, first half, gathers, second half, gathers.) */
    const int item = (int)blockIdx.x * WAVES + (int)(threadIdx.x >> 6);
    const int handedOut = a.deepHeader[SPGPU_DEEP_HEAD_ITEMS];
    const int cut = a.deepHeader[SPGPU_DEEP_HEAD_CUT];
    const SpgpuDeepItem mine = item < SPGPU_DEEP_ITEMS ? a.deepItems[item] : SpgpuDeepItem{0, 0u, 0, 0};
    const int fresh = SPGPU_DEEP_ITEMS - cut; /* items below this were written by this call */
    const int items = handedOut < fresh ? handedOut : fresh;
    if (item >= items)
        return;
    {
        const int kFirst = a.deepKeep + mine.chunk * CHUNK;
        const int kEnd = kFirst + CHUNK < mine.depth ? kFirst + CHUNK : mine.depth;
        const long long row0 = (long long)mine.row0 + (long long)sub * RPL;
        long long slab = (long long)mine.base + (long long)sub * RPL;
        if constexpr (IS_HELL) {
            if ((a.hackSize & 31) != 0 && row0 < a.rows) { /* the sub-group may straddle hacks: the lane's own hack (wavefront-uniform test) */
                const unsigned r0 = (unsigned)row0, hs = (unsigned)a.hackSize;
                const unsigned hack = r0 / hs;
                slab = (long long)a.hackOffsets[hack] + (r0 - hack * hs);
            }
        }
        int len[RPL];
#pragma unroll
        for (int t = 0; t < RPL; ++t) {
            const long long r = row0 + t;
            len[t] = r < a.rows ? (a.rS ? a.rS[r] : a.maxNnz) : 0;
        }
        const bool rowsExist = row0 < a.rows; /* a strip beyond the last row: nothing of it is loaded */
        /* how far this lane may load: the item's end -- except where the sub-group straddles hacks (hackSize not a multiple of
         * 32): the lane's own hack may be shallower than the sub-group, so there its own rows' lengths bound the loads (and are
         * waited for first) */
        int loadEnd = kEnd;
        if constexpr (IS_HELL) {
            if ((a.hackSize & 31) != 0) {
                int own = 0;
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    own = len[t] > own ? len[t] : own;
                loadEnd = own < kEnd ? own : kEnd;
            }
        }
        const T* __restrict__ vals = a.cM + slab;
        const int* __restrict__ idxs = a.rP + slab;
        constexpr int STAGES = CHUNK / STEP;
        Pack<T, RPL> v[STAGES][UNROLL];
        Pack<int, RPL> c[STAGES][UNROLL];
#pragma unroll
        for (int s = 0; s < STAGES; ++s) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int k = kFirst + s * STEP + u * PH + phase;
                if (k < loadEnd && rowsExist) {
                    v[s][u] = loadPack<true, T, RPL>(vals + (long long)k * a.valStride);
                    c[s][u] = loadPack<true, int, RPL>(idxs + (long long)k * a.idxStride);
                } else {
#pragma unroll
                    for (int t = 0; t < RPL; ++t) {
                        v[s][u].v[t] = zeroOf<T>();
                        c[s][u].v[t] = a.baseIndex;
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < RPL; ++t)
            len[t] = len[t] < kEnd ? len[t] : kEnd;
        T sum[RPL];
#pragma unroll
        for (int t = 0; t < RPL; ++t)
            sum[t] = zeroOf<T>();
#pragma unroll
        for (int s = 0; s < STAGES; ++s) {
            T xv[UNROLL][RPL];
            bool use[UNROLL][RPL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int k = kFirst + s * STEP + u * PH + phase;
#pragma unroll
                for (int t = 0; t < RPL; ++t) {
                    const int col = c[s][u].v[t] - a.baseIndex;
                    use[u][t] = k < len[t] && col >= 0;
                    xv[u][t] = a.x[use[u][t] ? col : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
                for (int t = 0; t < RPL; ++t)
                    sum[t] = pick(use[u][t], mulAdd(v[s][u].v[t], xv[u][t], sum[t]), sum[t]);
            }
            __builtin_amdgcn_sched_barrier(0); /* one half's gathers at a time */
        }
#pragma unroll
        for (int m = LPC; m < kWave; m <<= 1) {
#pragma unroll
            for (int t = 0; t < RPL; ++t)
                sum[t] = add(sum[t], laneXor(sum[t], m));
        }
        if (phase == 0) {
#pragma unroll
            for (int t = 0; t < RPL; ++t)
                a.deepItemSums[(size_t)item * 32 + (size_t)(sub * RPL + t)] = sum[t];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlockThreads) void deepFinishKernel(const SlabArgs<T> a)
{
    const int registered = a.deepHeader[SPGPU_DEEP_HEAD_ENTRIES];
    const int entries = registered < SPGPU_DEEP_ENTRIES ? registered : SPGPU_DEEP_ENTRIES;
    const bool hasBeta = isNotZero(a.beta);
    const int rowInGroup = threadIdx.x & 31;
    constexpr int PER_BLOCK = kBlockThreads / 32;
    for (int e = (int)blockIdx.x * PER_BLOCK + (int)(threadIdx.x >> 5); e < entries; e += (int)gridDim.x * PER_BLOCK) {
        const SpgpuDeepEntry entry = a.deepEntries[e];
        const long long r = (long long)entry.row0 + rowInGroup;
        if (entry.items <= 0 || r >= a.rows)
            continue;
        T total = a.deepPartials[(size_t)e * 32 + rowInGroup];
        constexpr int BATCH = 8; /* item sums requested together; added in item order */
        for (int c0 = 0; c0 < entry.items; c0 += BATCH) {
            T part[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (c0 + u < entry.items)
                    part[u] = a.deepItemSums[(size_t)(entry.firstItem + c0 + u) * 32 + rowInGroup];
#pragma unroll
            for (int u = 0; u < BATCH; ++u)
                if (c0 + u < entry.items)
                    total = add(total, part[u]);
        }
        const int outRow = a.rIdx ? a.rIdx[r] : (int)r;
        a.z[outRow] = hasBeta ? epilogue<true>(a.alpha, total, a.beta, a.y[outRow])
                              : epilogue<false>(a.alpha, total, a.beta, zeroOf<T>());
    }
    __syncthreads(); /* every wavefront of this workgroup has used the header */
    if (threadIdx.x == 0) {
        const int ticket = atomicAdd(&a.deepHeader[SPGPU_DEEP_HEAD_TICKET], 1);
        if (ticket == (int)gridDim.x - 1) {
            /* a list that overflowed: say so where the host can see it (spgpuDeepListOverflows, include/spgpu/tuning.h) */
            const int handedOut = a.deepHeader[SPGPU_DEEP_HEAD_ITEMS];
            if (a.deepOverflow && (registered > SPGPU_DEEP_ENTRIES || handedOut > SPGPU_DEEP_ITEMS)) {
                a.deepOverflow[1] = registered;
                a.deepOverflow[2] = handedOut;
                atomicAdd_system(&a.deepOverflow[0], 1); /* the streams of a handle share the word: two of them may overflow at once */
            }
            a.deepHeader[SPGPU_DEEP_HEAD_ENTRIES] = 0;
            a.deepHeader[SPGPU_DEEP_HEAD_ITEMS] = 0;
            a.deepHeader[SPGPU_DEEP_HEAD_TICKET] = 0;
            a.deepHeader[SPGPU_DEEP_HEAD_CUT] = 0;
        }
    }
}
