/* ---- frozen matrices WITHOUT a row order (spgpu?SpmvFreeze with rIdx == NULL, include/spgpu/tuning.h) ------------------------
 * The ordered matrices' frozen form lives with their plan (planned_spmv.hip).  A matrix that runs in the default kernels --
 * BASELINE configs[1], the headline -- gets the same: a 16-bit copy of its column indices, counted per GROUP of rows (the
 * rows one wavefront of slabSpmvKernel owns: 128 for the 8-byte types, 32 for fp32) from the group's lowest column, 0xFFFF where
 * a column lies 65 535 or more above it (or is negative).  The record sits in the handle's plan table under the arrays'
 * addresses with subs = -groupRows (no analysis, no blocks: `device` holds the groups' bases).  A matrix with more than one
 * escape in a hundred entries is not frozen: its columns are scattered, the gathers bound its SpMV, and every escape costs the
 * rP word the copy was to save. */
template <bool IS_HELL>
__global__ __launch_bounds__(256) void slabPackKernel(const int* __restrict__ rP, const int* __restrict__ rS, const int* __restrict__ hackOffsets,
                                                     int hackSize, long long idxStride, int maxNnz, int rows, int baseIndex, int groupRows,
                                                     int* __restrict__ packBases, unsigned short* __restrict__ packed, unsigned long long* counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long group = (long long)blockIdx.x * (256 / kWave) + (threadIdx.x >> 6); /* a wavefront per group */
    const long long groupRow0 = group * groupRows;
    if (groupRow0 >= rows)
        return;
    constexpr int MOST = 2; /* rows per lane: groups of up to 128 rows */
    long long at[MOST];
    int len[MOST];
    int lowest = 0x7fffffff;
    for (int j = 0; j < MOST; ++j) {
        const long long r = groupRow0 + lane + j * kWave;
        len[j] = (lane + j * kWave < groupRows && r < rows) ? (rS ? rS[r] : maxNnz) : 0;
        at[j] = 0;
        if (len[j] > 0) {
            if constexpr (IS_HELL) {
                const unsigned u = (unsigned)r, hs = (unsigned)hackSize;
                at[j] = (long long)((unsigned)hackOffsets[u / hs] + u % hs);
            } else {
                at[j] = r;
            }
        }
        for (int k = 0; k < len[j]; ++k) {
            const int col = rP[at[j] + (long long)k * idxStride] - baseIndex;
            lowest = (col >= 0 && col < lowest) ? col : lowest;
        }
    }
    lowest = waveMin(lowest);
    const int base = lowest == 0x7fffffff ? 0 : lowest;
    if (lane == 0)
        packBases[group] = base;
    unsigned entries = 0, escapes = 0;
    for (int j = 0; j < MOST; ++j) {
        for (int k = 0; k < len[j]; ++k) {
            const long long slot = at[j] + (long long)k * idxStride;
            const int col = rP[slot] - baseIndex;
            const long long off = (long long)col - base;
            const bool fits = col >= 0 && off < 0xFFFF;
            packed[slot] = fits ? (unsigned short)off : (unsigned short)0xFFFF;
            entries += 1;
            escapes += fits ? 0 : 1;
        }
    }
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        entries += (unsigned)laneXor((int)entries, m);
        escapes += (unsigned)laneXor((int)escapes, m);
    }
    if (lane == 0) {
        atomicAdd(&counts[0], (unsigned long long)entries);
        atomicAdd(&counts[1], (unsigned long long)escapes);
    }
}

__global__ __launch_bounds__(kWave) void slabSlotsKernel(const int* __restrict__ rS, const int* __restrict__ hackOffsets, int hackSize, int rows, unsigned long long* out)
{
    /* HELL does not state its slot count (hell.c:64,75: no trailing total): last hack's offset + hackSize x its longest row */
    const int lastHack = (rows - 1) / hackSize;
    int longest = 0;
    for (long long r = (long long)lastHack * hackSize + threadIdx.x; r < rows; r += kWave)
        longest = rS[r] > longest ? rS[r] : longest;
    longest = waveMax(longest);
    if (threadIdx.x == 0)
        out[0] = (unsigned long long)(unsigned)hackOffsets[lastHack] + (unsigned long long)hackSize * (unsigned)longest;
}

/* spgpu?SpmvFreeze of a matrix without a row order: synchronous; true = frozen (or was already).  `key` (planKey with
 * subs = -rows per group) names every array the copy is made from. */
template <bool IS_HELL>
static bool freezeSlab(spgpuHandle_t handle, hipStream_t stream, const SpgpuSpmvPlan& key)
{
    SpgpuPrivateHandle* h = spgpuPrivate(handle);
    const int groupRows = -key.subs;
    const int* rP = static_cast<const int*>(key.rP);
    const int* rS = static_cast<const int*>(key.rS);
    const int* hackOffsets = static_cast<const int*>(key.hackOffsets);
    spgpuTablesLock(handle);
    SpgpuSpmvPlan* plan = spgpuPlanRecord(handle, &key);
    bool frozen = plan && plan->packed && plan->state == SPGPU_PLAN_READY;
    if (plan && !frozen && plan->state != SPGPU_PLAN_GIVEN_UP) {
        const long long groups = ((long long)key.rows + groupRows - 1) / groupRows;
        const size_t baseBytes = roundUpTo((size_t)groups * sizeof(int), 256);
        void *device = spgpuDeviceAlloc(handle, baseBytes + 256), *packed = nullptr;
        bool ok = device != nullptr;
        unsigned long long* counts = ok ? reinterpret_cast<unsigned long long*>(static_cast<char*>(device) + baseBytes) : nullptr;
        unsigned long long said[2] = {0, 0};
        long long slots = IS_HELL ? 0 : key.idxStride * (long long)key.maxNnz;
        if (ok && IS_HELL) {
            hipLaunchKernelGGL(slabSlotsKernel, dim3(1), dim3(kWave), 0, stream, rS, hackOffsets, key.hackSize, key.rows, counts);
            ok = hipMemcpyAsync(said, counts, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream) == hipSuccess &&
                 hipStreamSynchronize(stream) == hipSuccess;
            slots = (long long)said[0];
        }
        ok = ok && slots > 0;
        const size_t copyBytes = ok ? packedBytes(slots) : 0;
        ok = ok && (packed = spgpuDeviceAlloc(handle, copyBytes)) != nullptr;
        if (ok) {
            if (spgpuTuning()->poisonScratch)
                (void)hipMemsetAsync(packed, 0xA5, copyBytes, stream);
            (void)hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), stream);
            hipLaunchKernelGGL((slabPackKernel<IS_HELL>), dim3((unsigned)((groups + 3) / 4)), dim3(256), 0, stream, rP, rS, hackOffsets, key.hackSize,
                               key.idxStride, key.maxNnz, key.rows, key.baseIndex, groupRows, static_cast<int*>(device), static_cast<unsigned short*>(packed), counts);
            ok = hipMemcpyAsync(said, counts, sizeof(said), hipMemcpyDeviceToHost, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
        }
        if (ok && keepsCopy(said[0], said[1], spgpuTuning()->freezeEscapesPct)) { /* at most one escape in a hundred entries (SPGPU_FREEZE_MAX_ESCAPES_PCT) */
            plan->device = device;
            plan->packed = packed;
            plan->packedBytes = (long long)copyBytes;
            plan->blocks = 0;
            plan->deep = 0;
            plan->uses = 0;
            plan->state = SPGPU_PLAN_READY;
            h->planFreezes += 1;
            frozen = true;
        } else {
            (void)hipGetLastError();
            if (device)
                (void)hipFree(device);
            if (packed)
                (void)hipFree(packed);
        }
    }
    spgpuPlanCountFrozenSlabs(handle);
    spgpuTablesUnlock(handle);
    return frozen;
}

/* The SpMV side: a.planPacked / a.packBases of the matrix' frozen record, if it has one (else they stay NULL).  Inside a stream
 * capture only a held record (spgpuSpmvHold, include/spgpu/ext/graph.h): a graph would carry the copy's address beyond a Thaw. */
template <typename T>
static void findFrozenSlab(spgpuHandle_t handle, hipStream_t stream, SlabArgs<T>& a, int groupRows)
{
    SpgpuPrivateHandle* h = spgpuPrivate(handle);
    a.planPacked = nullptr;
    a.packBases = nullptr;
    if (__atomic_load_n(&h->planFrozenSlabs, __ATOMIC_RELAXED) <= 0)
        return;
    const bool heldOnly = spgpuStreamCapturing(stream);
    const SpgpuSpmvPlan key = planKey(a, nullptr, 0, -groupRows);
    spgpuTablesLock(handle);
    SpgpuSpmvPlan* plan = spgpuPlanFind(handle, &key);
    if (plan && plan->packed && plan->state == SPGPU_PLAN_READY && (!heldOnly || plan->holds > 0)) {
        a.planPacked = static_cast<const unsigned short*>(plan->packed);
        a.packBases = static_cast<const int*>(plan->device);
        plan->uses += 1;
        h->planUses += 1;
    }
    spgpuTablesUnlock(handle);
}
