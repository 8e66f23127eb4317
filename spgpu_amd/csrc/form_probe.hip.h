/* What does this matrix look like?  Included by ellpack_spmv.hip (namespace spgpu, after slab_spmv.hip.h: sampleGroup). */
/*
 * What do the columns of this matrix look like?  Three wavefronts (the sample groups of slabSpmvKernel) walk their rows'
 * indices and report what the strip-capable kernel's samples would: 2 = neighbouring rows name consecutive columns (strip x
 * loads), 3 = the columns of a group lie inside a window an LDS tile holds, 1 = scattered.  Launched by AUTO with every
 * fourth call of the forms that do not report themselves, and by spgpu?SpmvForm (include/spgpu/tuning.h) for a caller who
 * wants to hold the answer.  STEP = the columns per stage of the strip-capable kernel of the type (its strip test is per stage).
 */
template <typename T, int RPL, int PH, bool IS_HELL, int STEP>
__global__ __launch_bounds__(kWave) void formProbeKernel(const SlabArgs<T> a)
{
    constexpr int LPC = kWave / PH, GROUP_ROWS = LPC * RPL;
    const long long groups = ((long long)a.rows + GROUP_ROWS - 1) / GROUP_ROWS;
    const long long group = sampleGroup(groups, (int)blockIdx.x + 1);
    const int lane = threadIdx.x;
    const long long row0 = group * GROUP_ROWS + (long long)lane * RPL;
    int len[RPL], longest = 0;
    long long slab = 0;
    const bool live = lane < LPC && row0 < a.rows;
    if (live) {
        if constexpr (IS_HELL) {
            const unsigned r0 = (unsigned)row0, hs = (unsigned)a.hackSize;
            slab = (long long)a.hackOffsets[r0 / hs] + (r0 % hs);
        } else {
            slab = row0;
        }
    }
#pragma unroll
    for (int t = 0; t < RPL; ++t) {
        const long long r = row0 + t;
        len[t] = live && r < a.rows ? (a.rS ? a.rS[r] : a.maxNnz) : 0;
        longest = len[t] > longest ? len[t] : longest;
    }
    const int groupLongest = waveMax(longest);
    /* first column at which this lane's strip is neither "all rows present with consecutive columns" nor "all past their end" */
    int firstBad = 0x7fffffff, lowest = 0x7fffffff, highest = -1;
    bool below = false;
    for (int k = 0; k < longest; ++k) {
        const bool present = k < len[0];
        const int c0 = present ? a.rP[slab + (long long)k * a.idxStride] : 0;
        bool bad = present && c0 - a.baseIndex < 0;
#pragma unroll
        for (int t = 1; t < RPL; ++t) {
            const bool here = k < len[t];
            bad |= here != present || (present && a.rP[slab + t + (long long)k * a.idxStride] != c0 + t);
        }
        if (bad) {
            firstBad = k;
            break;
        }
    }
#pragma unroll
    for (int t = 0; t < RPL; ++t) { /* the span of the group's columns: first and last entry of every row */
        if (len[t] > 0) {
            const int f = a.rP[slab + t] - a.baseIndex, l = a.rP[slab + t + (long long)(len[t] - 1) * a.idxStride] - a.baseIndex;
            below |= f < 0 || l < 0;
            lowest = f < lowest ? f : lowest;
            lowest = l < lowest ? l : lowest;
            highest = f > highest ? f : highest;
            highest = l > highest ? l : highest;
        }
    }
    firstBad = waveMin(firstBad);
    lowest = waveMin(lowest);
    highest = waveMax(highest);
    const long long span = __ballot(below) != 0ull ? (1ll << 40) : (highest < lowest ? 0ll : (long long)highest - lowest + 1);
    const int asStrips = firstBad == 0x7fffffff ? groupLongest : firstBad / STEP * STEP; /* whole stages of strips in front */
    /* 4 = a matrix for the SWEEP form: the columns of the group reach over half of x and more (the matrix is taken to be about
     * square: the API does not say how long x is), ascend inside every sampled row (its first 64 entries), and the rows are about
     * equally long (rows walked in step wait for the longest) */
    bool sweepable = false;
    if constexpr (PH == 1 && sizeof(T) == 8) {
        bool ascends = true;
        int total = 0;
#pragma unroll
        for (int t = 0; t < RPL; ++t) {
            total += len[t];
            const int look = len[t] < 64 ? len[t] : 64;
            int before = -0x7fffffff - 1;
            for (int k = 0; k < look; ++k) {
                const int c = a.rP[slab + t + (long long)k * a.idxStride];
                ascends &= c >= before;
                before = c;
            }
        }
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1)
            total += laneXor(total, m);
        const long long slots = (long long)groupLongest * GROUP_ROWS;
        sweepable = __ballot(!ascends) == 0ull && span < (1ll << 40) && 2 * span >= (long long)a.rows && groupLongest >= 2 * STEP &&
                    2 * slots <= 3 * (long long)total;
    }
    if (lane == 0 && a.feedback)
        a.feedback[blockIdx.x] = a.feedbackTag | ((RPL > 1 && 2 * asStrips >= groupLongest && groupLongest > STEP) ? 2
                                                  : (groupLongest > STEP && span <= a.tileSpanLimit ? 3 : (sweepable ? 4 : 1))); /* one stage of rows: no tile */
}

/*
 * Rows with a row order (rIdx): how far from the diagonal -- in the ORIGINAL numbering, rIdx[row] -- do their columns lie?
 * The queue kernel for ordered rows has two product shapes (ragged_spmv.hip.h, launchRagged): 2 048 rows per workgroup with
 * the results staged in LDS by destination (whole-line stores of z; 48 KiB left for the x tile) wins when the columns of a
 * window of rows fit that tile, 1 024 rows with a 64 KiB tile when they spread further (columns +-2 048 of the row: 2 048
 * rows would need 64 KiB and more).  192 sampled rows answer: 4 = three quarters of them keep within 1 024 of the
 * diagonal, 5 = they do not; 6 = whatever the columns do, the kernel's 2 048-row blocks are the windows of the order.
 * Launched by AUTO when it has no answer for the matrix, and again every 64th call.
 */
template <bool IS_HELL>
__global__ __launch_bounds__(kWave) void orderedProbeKernel(const int* rP, const int* rS, const int* hackOffsets, const int* rIdx, int hackSize,
                                                           long long idxStride, int maxNnz, int rows, int baseIndex, int* answer, int tag)
{
    const int lane = threadIdx.x;
    int near = 0, seen = 0;
    for (int q = 1; q <= 3; ++q) {
        const long long r = (long long)rows * q / 4 + 2 * q + lane;
        if (r >= rows)
            continue;
        const int len = rS ? rS[r] : maxNnz;
        if (len <= 0)
            continue;
        long long slot;
        if constexpr (IS_HELL)
            slot = (long long)hackOffsets[(unsigned)r / (unsigned)hackSize] + (unsigned)r % (unsigned)hackSize;
        else
            slot = r;
        const long long dest = rIdx[r];
        const long long first = (long long)rP[slot] - baseIndex - dest, last = (long long)rP[slot + (long long)(len - 1) * idxStride] - baseIndex - dest;
        const long long reach = (first < 0 ? -first : first) > (last < 0 ? -last : last) ? (first < 0 ? -first : first) : (last < 0 ? -last : last);
        seen += 1;
        near += reach <= 1024 ? 1 : 0;
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        near += laneXor(near, m);
        seen += laneXor(seen, m);
    }
    /* Are the kernel's 2 048-row blocks the windows of the order (spgpuOellOrderAlignedDevice)?  64 rows spread over each of
     * three blocks: the rows of ONE window come from a stretch of the original numbering little longer than the window, the
     * rows of a block that straddles two windows from twice that.  Then the 2 048-row shape serves wide columns too: its tile
     * holds the one window +- 2 048 such a block touches, and the block's results are whole lines of z. */
    int blocksAreWindows = 0, blocksSeen = 0;
    for (int q = 1; q <= 3; ++q) {
        const long long block0 = ((long long)rows * q / 4) / 2048 * 2048;
        if (block0 + 2048 > rows)
            continue;
        const int dest = rIdx[block0 + lane * 32 + (lane & 31)];
        const int low = waveMin(dest), high = waveMax(dest);
        blocksSeen += 1;
        blocksAreWindows += high - low < 2048 + 512 ? 1 : 0;
    }
    if (lane == 0)
        *answer = tag | ((blocksSeen > 0 && blocksAreWindows == blocksSeen) ? 6 : (seen > 0 && 4 * near >= 3 * seen) ? 4 : 5);
}
