/*
 * The sparse matrix product C = A * B on CSR arrays for gfx950 (include/spgpu/ext/spgemm_device.h).  New functionality: the
 * analysis lists every product a(i,k) * b(k,j) once, sorts the list and keeps the distinct (i, j); the fills add the products up
 * in the storage order of A's row.
 *
 * THE ANALYSIS is set-up code, on the machinery of the assembly (assemble_device.hip); what the two share lies in
 * csr_shared.hip.h and csr_host.h.  Scratch layout (ints), S = productsCount rounded up to 64:
 *   head    misc[16] | rowProducts[aRows+1] | rowStart[aRows+1] | rowTotals[tiles(aRows+1)+2], rounded up to 64 ints: a function
 *           of aRows alone, which is all spgpuCsrSpgemmProductsDevice touches.  misc[1] bad-input flag, misc[2..3] the number of
 *           products in 64 bits
 *   keysA[2S]     64-bit keys as expanded: (i << colBits) | j, both 0-based.  After the sort the buffer is free, and its first S
 *                 ints hold THE COLUMNS OF C until spgpuCsrSpgemmDevice copies them out: their place depends on aRows alone
 *   keysB[2S]     the keys sorted
 *   entryOf[S]    head flags (1 where a sorted position starts a new key), scanned in place: the entry of C of every product
 *   prodTotals[tiles(S)+2], rounded up to 64 ints | rocPRIM temp
 * Products per row (with the check of A's columns; a bad column counts no product and is skipped everywhere) -> the three-launch
 * scan of convert_scan.hip.h -> expansion, a wavefront per row of A, with the checks of B's columns and of their order -> ONE
 * radix sort of the keys over rowBits + colBits bits (rocPRIM) -> head flags -> the same scan -> a head writes its column ->
 * row starts by binary search in the sorted keys (rowStartKernel) -> cRowPtr[i] = entryOf[rowStart[i]].  The number of products
 * is summed in 64 bits beside the int scan, and no kernel writes a key at or beyond productsCount: a caller's count that is not
 * the matrices', or a scan that wrapped, is reported after the synchronise and has written nothing out of bounds.
 *
 * THE FILLS add in the contract's order, each product rounded and then each sum (exactMulAdd of csr_shared.hip.h: contraction off), and give the same
 * bytes:
 *   plain    (spgemmEntryKernel) one thread per entry u of C: its row by bisection of cRowPtr, then a walk over A's row in storage
 *            order with a bisection of B's row k for column j per step.  No LDS;
 *   staged   (spgemmRowKernel) a wavefront owns one row of C at a time, kSpgWaves wavefronts per workgroup, grid-strided.  A row
 *            of at most kSpgRowCap entries has its columns read coalesced into LDS with a zeroed value slot beside each; then one
 *            ROUND per entry of A's row, in storage order: the lanes stride over B's row k with coalesced loads of column and
 *            value, each bisects the LDS columns for its j and does slot = slot + a * b in LDS.  B's row has no duplicate column,
 *            so the lanes of one round touch distinct slots; between rounds, see spgWaveSync.  After the last round the slots are
 *            written out coalesced.  A longer row is done in the same launch by the plain method, the lanes striding over its
 *            entries.  LDS per workgroup: kSpgWaves * kSpgRowCap * (4 + sizeof(T)) bytes, 40 KB for the 16-byte type.
 * No atomics, one writer per element.
 */
#include "csr_shared.hip.h"
#include "numeric.hip.h"
#include "spgpu_internal.h"

#include "spgpu/ext/spgemm_device.h"

#include <limits.h>
#include <string.h>
#include <rocprim/device/device_radix_sort.hpp>

namespace spgpu {

typedef unsigned long long SpgKey;

constexpr int kSpgThreads = 256;
constexpr int kSpgWaves = kSpgThreads / kWave;
constexpr int kSpgRowCap = 512; /* entries of a row of C that a wavefront keeps in LDS: 4 * 512 * (4 + 16) = 40 KB at most */
constexpr int kSpgFillBlocks = 2048; /* enough workgroups of 256 to fill 256 CUs, where the host does not know C's size */

enum { SPGPU_SPGEMM_FILL_PLAIN = 0, SPGPU_SPGEMM_FILL_STAGED = 1 };
/* The fill the public calls run: the staged one until tools/bench_spgemm.py has been run on an MI355X (the rule: the one that is
 * faster on A * A of a 3-D 7-point pattern if the min-max ranges of the two legs do not overlap, the plain one otherwise). */
constexpr int kSpgDefaultFill = SPGPU_SPGEMM_FILL_STAGED;

struct SpgemmWork {
    int* misc;
    int* rowProducts;
    int* rowStart;
    int* rowTotals;
    SpgKey *keysA, *keysB;
    int* cCols; /* the first ints of keysA */
    int* entryOf;
    int* prodTotals;
    void* temp;
};

static size_t spgHeadInts(int rows)
{
    return alignUpCv((size_t)16 + 2 * ((size_t)rows + 1) + scanBlocks((long long)rows + 1) + 2, 64);
}

static size_t spgTotalsInts(size_t products) { return alignUpCv(scanBlocks((long long)products) + 2, 64); }

static SpgemmWork carveSpgemm(void* work, int rows, size_t products)
{
    SpgemmWork w;
    int* p = static_cast<int*>(work);
    w.misc = p;
    w.rowProducts = p + 16;
    w.rowStart = w.rowProducts + (size_t)rows + 1;
    w.rowTotals = w.rowStart + (size_t)rows + 1;
    p += spgHeadInts(rows);
    const size_t S = alignUpCv(products, 64);
    w.keysA = reinterpret_cast<SpgKey*>(p);
    w.cCols = p;
    p += 2 * S;
    w.keysB = reinterpret_cast<SpgKey*>(p);
    p += 2 * S;
    w.entryOf = p;
    p += S;
    w.prodTotals = p;
    p += spgTotalsInts(products);
    w.temp = p;
    return w;
}

static hipError_t spgSortTempBytes(size_t n, size_t* bytes)
{
    size_t need = 0;
    const hipError_t err = rocprim::radix_sort_keys(nullptr, need, (const SpgKey*)nullptr, (SpgKey*)nullptr, n);
    *bytes = alignUpCv(need, 256);
    return err;
}

/* ---- the analysis ---- */
/* rowProducts[i] = sum over the entries of A's row i of the length of B's row k, held to INT_MAX; the grand total in 64 bits
 * (integer atomics: order-independent).  A column of A outside B's rows raises the flag and counts nothing. */
__global__ __launch_bounds__(kCvThreads) void spgRowProductsKernel(int* rowProducts, int* misc, int aRows, int aCols, const int* aPtr,
                                                                    const int* aIdx, const int* bPtr, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i <= aRows; i += stride) {
        unsigned long long count = 0;
        if (i < aRows) {
            for (int e = aPtr[i] - base; e < aPtr[i + 1] - base; ++e) {
                const unsigned k = (unsigned)aIdx[e] - (unsigned)base;
                if (k >= (unsigned)aCols) {
                    misc[1] = 1;
                    continue;
                }
                const int len = bPtr[k + 1] - bPtr[k];
                count += len > 0 ? (unsigned long long)len : 0;
            }
            if (count)
                atomicAdd(reinterpret_cast<unsigned long long*>(misc + 2), count);
        }
        rowProducts[i] = count > (unsigned long long)INT_MAX ? INT_MAX : (int)count; /* element aRows: 0, the scan's last slot */
    }
}

/* One key per product, a wavefront per row of A: the products of entry e of the row follow those of the entries before it, the
 * lanes stride over B's row.  `first` is the exclusive scan of rowProducts.  Nothing is written at or beyond `products`. */
__global__ __launch_bounds__(kCvThreads) void spgExpandKernel(SpgKey* keys, int* misc, int aRows, int aCols, int bCols, const int* aPtr,
                                                               const int* aIdx, const int* bPtr, const int* bIdx, int base, const int* first,
                                                               int products, int colBits)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long waves = (long long)gridDim.x * (kCvThreads / kWave);
    for (long long i = (long long)blockIdx.x * (kCvThreads / kWave) + (threadIdx.x >> 6); i < aRows; i += waves) {
        long long at = first[i];
        for (int e = aPtr[i] - base; e < aPtr[i + 1] - base; ++e) {
            const unsigned k = (unsigned)aIdx[e] - (unsigned)base;
            if (k >= (unsigned)aCols)
                continue;
            const int b0 = bPtr[k] - base, b1 = bPtr[k + 1] - base;
            for (int q = b0 + lane; q < b1; q += kWave) {
                const unsigned j = (unsigned)bIdx[q] - (unsigned)base;
                bool bad = j >= (unsigned)bCols;
                if (q > b0 && bIdx[q - 1] >= bIdx[q])
                    bad = true; /* the row does not ascend strictly */
                if (bad)
                    misc[1] = 1;
                const long long p = at + (q - b0);
                if (p >= 0 && p < products)
                    keys[p] = ((SpgKey)i << colBits) | (bad ? 0u : j);
            }
            at += b1 > b0 ? b1 - b0 : 0;
        }
    }
}

/* a head at sorted position p is entry entryOf[p] of C: its column is the key's low bits */
__global__ __launch_bounds__(kCvThreads) void spgColumnsKernel(int* cCols, const int* entryOf, const SpgKey* keys, int n, SpgKey colMask, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long p = (long long)blockIdx.x * kCvThreads + threadIdx.x; p < n; p += stride)
        if (p == 0 || keys[p] != keys[p - 1])
            cCols[entryOf[p]] = (int)(keys[p] & colMask) + base;
}

/* rowStart[r] is a head, or n: the entries in front of it are the entries of the rows < r */
__global__ __launch_bounds__(kCvThreads) void spgRowPtrKernel(int* cRowPtr, const int* rowStart, const int* entryOf, int rows, int n,
                                                               const int* unique, int base)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long r = (long long)blockIdx.x * kCvThreads + threadIdx.x; r <= rows; r += stride) {
        const int at = rowStart[r];
        cRowPtr[r] = base + (at < n ? entryOf[at] : *unique);
    }
}

/* ---- the fills ---- */
/* c(i, j) by the plain method: A's row in storage order, B's row k bisected for column j (columns compared in the common base) */
template <typename T>
__device__ inline T spgEntry(int i, int j, const int* aPtr, const int* aIdx, const T* aVal, const int* bPtr, const int* bIdx, const T* bVal,
                             int base)
{
    T sum = zeroOf<T>();
    for (int e = aPtr[i] - base; e < aPtr[i + 1] - base; ++e) {
        const int k = aIdx[e] - base;
        int lo = bPtr[k] - base;
        const int end = bPtr[k + 1] - base;
        int hi = end;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (bIdx[mid] < j)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo < end && bIdx[lo] == j)
            sum = exactMulAdd(sum, aVal[e], bVal[lo]);
    }
    return sum;
}

/* The plain fill: one thread per entry of C.  The number of entries is read from cRowPtr. */
template <typename T>
__global__ __launch_bounds__(kSpgThreads) void spgemmEntryKernel(T* cVal, int aRows, const int* aPtr, const int* aIdx, const T* aVal,
                                                                 const int* bPtr, const int* bIdx, const T* bVal, const int* cPtr,
                                                                 const int* cIdx, int base)
{
    const int entries = cPtr[aRows] - base;
    const long long stride = (long long)gridDim.x * kSpgThreads;
    for (long long u = (long long)blockIdx.x * kSpgThreads + threadIdx.x; u < entries; u += stride) {
        int lo = 0, hi = aRows; /* the last row i with cPtr[i] - base <= u: rows without entries in front of it are passed over */
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cPtr[mid] - base <= u)
                lo = mid;
            else
                hi = mid;
        }
        cVal[u] = spgEntry<T>(lo, cIdx[u], aPtr, aIdx, aVal, bPtr, bIdx, bVal, base);
    }
}

/* Orders the wavefront's LDS accesses in front of it before those behind it.  The hardware needs no instruction for that: a
 * wavefront has ONE instruction stream (a diverged loop runs under an EXEC mask and has reconverged when the next statement
 * starts), and the LDS serves the DS instructions of one wavefront in the order they were issued.  What has to be held is the
 * COMPILER: the wavefront-scope fences forbid it to move an LDS access across this point, and the wave barrier forbids it to
 * schedule instructions across it.  Nothing here relies on the lanes running in lockstep between two such points. */
__device__ inline void spgWaveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* The staged fill (head of the file). */
template <typename T>
__global__ __launch_bounds__(kSpgThreads) void spgemmRowKernel(T* cVal, int aRows, const int* aPtr, const int* aIdx, const T* aVal,
                                                               const int* bPtr, const int* bIdx, const T* bVal, const int* cPtr,
                                                               const int* cIdx, int base)
{
    __shared__ int ldsCols[kSpgWaves][kSpgRowCap];
    __shared__ T ldsVals[kSpgWaves][kSpgRowCap];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int* cols = ldsCols[wave];
    T* vals = ldsVals[wave];
    const long long waves = (long long)gridDim.x * kSpgWaves;
    for (long long row = (long long)blockIdx.x * kSpgWaves + wave; row < aRows; row += waves) {
        const int i = (int)row;
        const int c0 = __builtin_amdgcn_readfirstlane(cPtr[i] - base);
        const int len = __builtin_amdgcn_readfirstlane(cPtr[i + 1] - base) - c0;
        if (len <= 0)
            continue;
        if (len > kSpgRowCap) { /* wavefront-uniform: the row does not fit, its entries go by the plain method */
            for (int t = lane; t < len; t += kWave)
                cVal[c0 + t] = spgEntry<T>(i, cIdx[c0 + t], aPtr, aIdx, aVal, bPtr, bIdx, bVal, base);
            continue;
        }
        for (int t = lane; t < len; t += kWave) {
            cols[t] = cIdx[c0 + t];
            vals[t] = zeroOf<T>();
        }
        spgWaveSync();
        const int a0 = __builtin_amdgcn_readfirstlane(aPtr[i] - base), a1 = __builtin_amdgcn_readfirstlane(aPtr[i + 1] - base);
        for (int e = a0; e < a1; ++e) { /* one round per entry of A's row, in storage order */
            const int k = __builtin_amdgcn_readfirstlane(aIdx[e] - base);
            const T a = aVal[e];
            const int b0 = __builtin_amdgcn_readfirstlane(bPtr[k] - base), b1 = __builtin_amdgcn_readfirstlane(bPtr[k + 1] - base);
            for (int q = b0 + lane; q < b1; q += kWave) {
                const int j = bIdx[q];
                const T b = bVal[q];
                int lo = 0, hi = len;
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (cols[mid] < j)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                if (lo < len && cols[lo] == j) /* always, for the pattern the plan made */
                    vals[lo] = exactMulAdd(vals[lo], a, b);
            }
            spgWaveSync(); /* this round's slot writes before the next round's slot reads: another lane may hold the slot then */
        }
        for (int t = lane; t < len; t += kWave)
            cVal[c0 + t] = vals[t];
        spgWaveSync(); /* the next row zeroes what this one read */
    }
}

/* entries < 0: the host does not know how many entries C has (the values-only call) */
template <typename T>
static void launchSpgemm(hipStream_t s, void* cVal, int entries, int aRows, const int* aPtr, const int* aIdx, const void* aVal, const int* bPtr,
                         const int* bIdx, const void* bVal, const int* cPtr, const int* cIdx, int base, int fill, int maxBlocks)
{
    if (fill == SPGPU_SPGEMM_FILL_PLAIN) {
        long long blocks = entries >= 0 ? ((long long)entries + kSpgThreads - 1) / kSpgThreads : ((long long)aRows + 15) / 16;
        if (entries < 0 && blocks < kSpgFillBlocks)
            blocks = kSpgFillBlocks;
        hipLaunchKernelGGL(spgemmEntryKernel<T>, dim3(cappedGrid(blocks, 1, maxBlocks)), dim3(kSpgThreads), 0, s, static_cast<T*>(cVal), aRows, aPtr,
                           aIdx, static_cast<const T*>(aVal), bPtr, bIdx, static_cast<const T*>(bVal), cPtr, cIdx, base);
        return;
    }
    hipLaunchKernelGGL(spgemmRowKernel<T>, dim3(cappedGrid(aRows, kSpgWaves, maxBlocks)), dim3(kSpgThreads), 0, s, static_cast<T*>(cVal), aRows,
                       aPtr, aIdx, static_cast<const T*>(aVal), bPtr, bIdx, static_cast<const T*>(bVal), cPtr, cIdx, base);
}

/* fill < 0: the one the public calls run.  entries >= 0: the full call, the columns are copied out of `work` into cCols first;
 * entries < 0: values only, the host does not know C's size and cCols is the caller's. */
static spgpuStatus_t spgemm(spgpuHandle_t handle, int* cCols, void* cVal, int entries, int aRows, const int* aPtr, const int* aIdx,
                            const void* aVal, const int* bPtr, const int* bIdx, const void* bVal, const int* cPtr, int base, spgpuType_t type,
                            const void* work, int fill, int maxBlocks)
{
    if (aRows <= 0 || entries == 0)
        return SPGPU_SUCCESS;
    if (fill < 0)
        fill = kSpgDefaultFill;
    if (fill != SPGPU_SPGEMM_FILL_PLAIN && fill != SPGPU_SPGEMM_FILL_STAGED)
        return SPGPU_UNSUPPORTED;
    if (!cCols || (entries > 0 && !work))
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const bool launched = forValueType(type, [&](auto tag) {
        if (entries > 0) {
            const SpgemmWork w = carveSpgemm(const_cast<void*>(work), aRows, 0); /* the columns' place depends on aRows alone */
            (void)hipMemcpyAsync(cCols, w.cCols, (size_t)entries * sizeof(int), hipMemcpyDeviceToDevice, s);
        }
        launchSpgemm<decltype(tag)>(s, cVal, entries, aRows, aPtr, aIdx, aVal, bPtr, bIdx, bVal, cPtr, cCols, base, fill, maxBlocks);
    });
    if (!launched)
        return SPGPU_UNSUPPORTED;
    spgpuDebugCheck(handle, "csr spgemm");
    return SPGPU_SUCCESS;
}

/* the products per row and their 64-bit total, enqueued: what the Products call and the Plan share */
static void countProducts(hipStream_t s, const SpgemmWork& w, int aRows, int aCols, const int* aPtr, const int* aIdx, const int* bPtr, int base)
{
    (void)hipMemsetAsync(w.misc, 0, 16 * sizeof(int), s);
    hipLaunchKernelGGL(spgRowProductsKernel, dim3(gridFor((long long)aRows + 1)), dim3(kCvThreads), 0, s, w.rowProducts, w.misc, aRows, aCols, aPtr,
                       aIdx, bPtr, base);
}

} // namespace spgpu

using namespace spgpu;

extern "C" {

/* Not in the headers: the A/B of tools/bench_spgemm.py and the tests that compare the two fills.  fill: 0 the plain fill, 1 the
 * staged fill, < 0 the public call's choice; maxBlocks > 0 caps the grid (the grid stride on a small matrix). */
spgpuStatus_t spgpuCsrSpgemmDeviceWith(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int aRowsCount,
                                       const int* aRowPtr, const int* aColIndices, const void* aValues, const int* bRowPtr,
                                       const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType,
                                       const void* work, int fill, int maxBlocks);
spgpuStatus_t spgpuCsrSpgemmValuesDeviceWith(spgpuHandle_t handle, void* cValues, int aRowsCount, const int* aRowPtr, const int* aColIndices,
                                             const void* aValues, const int* bRowPtr, const int* bColIndices, const void* bValues,
                                             const int* cRowPtr, const int* cColIndices, int baseIndex, spgpuType_t valuesType, int fill,
                                             int maxBlocks);
int spgpuCsrSpgemmDefaultFill(void);
int spgpuCsrSpgemmRowCap(void); /* the longest row of C that the staged fill keeps in LDS */

int spgpuCsrSpgemmDefaultFill(void) { return kSpgDefaultFill; }
int spgpuCsrSpgemmRowCap(void) { return kSpgRowCap; }

size_t spgpuCsrSpgemmWorkBytes(int aRowsCount, int bColumnsCount, int productsCount)
{
    (void)bColumnsCount; /* the columns cost key bits, not scratch */
    const int rows = aRowsCount > 0 ? aRowsCount : 0;
    const size_t products = productsCount > 0 ? (size_t)productsCount : 0;
    size_t temp = 0;
    if (products > 0 && spgSortTempBytes(products, &temp) != hipSuccess)
        return 0; /* no GPU to ask for rocPRIM's share */
    return (spgHeadInts(rows) + 5 * alignUpCv(products, 64) + spgTotalsInts(products)) * sizeof(int) + temp + 256;
}

spgpuStatus_t spgpuCsrSpgemmProductsDevice(spgpuHandle_t handle, int* productsCount, int aRowsCount, int aColumnsCount, const int* aRowPtr,
                                           const int* aColIndices, const int* bRowPtr, int baseIndex, void* work)
{
    *productsCount = 0;
    if (aRowsCount <= 0)
        return SPGPU_SUCCESS;
    if (!work)
        return SPGPU_UNSUPPORTED;
    hipStream_t s = handle->currentStream;
    const SpgemmWork w = carveSpgemm(work, aRowsCount, 0);
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    countProducts(s, w, aRowsCount, aColumnsCount > 0 ? aColumnsCount : 0, aRowPtr, aColIndices, bRowPtr, baseIndex);
    (void)hipMemcpyAsync(host, w.misc, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "csr spgemm products");
    if (host[1])
        return SPGPU_UNSUPPORTED; /* a column of A names no row of B */
    unsigned long long total;
    memcpy(&total, host + 2, sizeof(total));
    if (total > (unsigned long long)INT_MAX) {
        *productsCount = -1;
        return SPGPU_UNSUPPORTED;
    }
    *productsCount = (int)total;
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrSpgemmPlanDevice(spgpuHandle_t handle, int* cNonZerosCount, int* cRowPtr, int aRowsCount, int aColumnsCount,
                                       int bColumnsCount, const int* aRowPtr, const int* aColIndices, const int* bRowPtr,
                                       const int* bColIndices, int baseIndex, int productsCount, void* work)
{
    *cNonZerosCount = 0;
    if (aRowsCount <= 0)
        return SPGPU_SUCCESS;
    hipStream_t s = handle->currentStream;
    if (productsCount <= 0) {
        hipLaunchKernelGGL(csrSetIntsKernel, dim3(gridFor((long long)aRowsCount + 1)), dim3(kCvThreads), 0, s, cRowPtr, (long long)aRowsCount + 1,
                           baseIndex);
        spgpuDebugCheck(handle, "csr spgemm plan");
        return SPGPU_SUCCESS;
    }
    if (aColumnsCount <= 0 || bColumnsCount <= 0 || !work)
        return SPGPU_UNSUPPORTED;
    const int n = productsCount;
    const SpgemmWork w = carveSpgemm(work, aRowsCount, (size_t)n);
    const int rowBits = bitsFor(aRowsCount), colBits = bitsFor(bColumnsCount);
    const int* unique = w.prodTotals + scanBlocks(n); /* the scan's grand total */
    int* host = static_cast<int*>(spgpuPrivate(handle)->reduceHost);
    size_t bytes = 0;
    if (spgSortTempBytes((size_t)n, &bytes) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    countProducts(s, w, aRowsCount, aColumnsCount, aRowPtr, aColIndices, bRowPtr, baseIndex);
    exclusiveScan(s, w.rowProducts, w.rowProducts, (long long)aRowsCount + 1, 1, w.rowTotals); /* in place, as in the assembly */
    hipLaunchKernelGGL(spgExpandKernel, dim3(gridFor((long long)aRowsCount * kWave)), dim3(kCvThreads), 0, s, w.keysA, w.misc, aRowsCount,
                       aColumnsCount, bColumnsCount, aRowPtr, aColIndices, bRowPtr, bColIndices, baseIndex, (const int*)w.rowProducts, n, colBits);
    /* at least one bit: a 1 x 1 product has keys of no bits at all */
    if (rocprim::radix_sort_keys(w.temp, bytes, (const SpgKey*)w.keysA, w.keysB, (size_t)n, 0u,
                                 (unsigned)(rowBits + colBits > 0 ? rowBits + colBits : 1), s) != hipSuccess)
        return SPGPU_UNSPECIFIED;
    hipLaunchKernelGGL(csrHeadFlagsKernel, dim3(gridFor(n)), dim3(kCvThreads), 0, s, w.entryOf, (const SpgKey*)w.keysB, n);
    exclusiveScan(s, w.entryOf, w.entryOf, (long long)n, 1, w.prodTotals);
    hipLaunchKernelGGL(spgColumnsKernel, dim3(gridFor(n)), dim3(kCvThreads), 0, s, w.cCols, (const int*)w.entryOf, (const SpgKey*)w.keysB, n,
                       (SpgKey)(((SpgKey)1 << colBits) - 1), baseIndex);
    hipLaunchKernelGGL(rowStartKernel<SpgKey>, dim3(gridFor((long long)aRowsCount + 1)), dim3(kCvThreads), 0, s, w.rowStart, aRowsCount,
                       (const SpgKey*)w.keysB, colBits, n);
    hipLaunchKernelGGL(spgRowPtrKernel, dim3(gridFor((long long)aRowsCount + 1)), dim3(kCvThreads), 0, s, cRowPtr, (const int*)w.rowStart,
                       (const int*)w.entryOf, aRowsCount, n, unique, baseIndex);
    (void)hipMemcpyAsync(host, w.misc, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipMemcpyAsync(host + 4, unique, sizeof(int), hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    spgpuDebugCheck(handle, "csr spgemm plan");
    unsigned long long total;
    memcpy(&total, host + 2, sizeof(total));
    if (host[1] || total != (unsigned long long)n)
        return SPGPU_UNSUPPORTED; /* a column outside its matrix, a row of B out of order, or not these matrices' productsCount */
    *cNonZerosCount = host[4];
    return SPGPU_SUCCESS;
}

spgpuStatus_t spgpuCsrSpgemmDeviceWith(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int aRowsCount,
                                       const int* aRowPtr, const int* aColIndices, const void* aValues, const int* bRowPtr,
                                       const int* bColIndices, const void* bValues, const int* cRowPtr, int baseIndex, spgpuType_t valuesType,
                                       const void* work, int fill, int maxBlocks)
{
    if (cNonZerosCount <= 0 || aRowsCount <= 0)
        return SPGPU_SUCCESS;
    return spgemm(handle, cColIndices, cValues, cNonZerosCount, aRowsCount, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices, bValues, cRowPtr,
                  baseIndex, valuesType, work, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrSpgemmValuesDeviceWith(spgpuHandle_t handle, void* cValues, int aRowsCount, const int* aRowPtr, const int* aColIndices,
                                             const void* aValues, const int* bRowPtr, const int* bColIndices, const void* bValues,
                                             const int* cRowPtr, const int* cColIndices, int baseIndex, spgpuType_t valuesType, int fill,
                                             int maxBlocks)
{
    if (aRowsCount <= 0)
        return SPGPU_SUCCESS;
    /* the fills write only cValues: the cast gives them the columns where the full call has its destination */
    return spgemm(handle, const_cast<int*>(cColIndices), cValues, -1, aRowsCount, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices, bValues,
                  cRowPtr, baseIndex, valuesType, nullptr, fill, maxBlocks);
}

spgpuStatus_t spgpuCsrSpgemmDevice(spgpuHandle_t handle, int* cColIndices, void* cValues, int cNonZerosCount, int aRowsCount, const int* aRowPtr,
                                   const int* aColIndices, const void* aValues, const int* bRowPtr, const int* bColIndices, const void* bValues,
                                   const int* cRowPtr, int baseIndex, spgpuType_t valuesType, const void* work)
{
    return spgpuCsrSpgemmDeviceWith(handle, cColIndices, cValues, cNonZerosCount, aRowsCount, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices,
                                    bValues, cRowPtr, baseIndex, valuesType, work, -1, 0);
}

spgpuStatus_t spgpuCsrSpgemmValuesDevice(spgpuHandle_t handle, void* cValues, int aRowsCount, const int* aRowPtr, const int* aColIndices,
                                         const void* aValues, const int* bRowPtr, const int* bColIndices, const void* bValues,
                                         const int* cRowPtr, const int* cColIndices, int baseIndex, spgpuType_t valuesType)
{
    return spgpuCsrSpgemmValuesDeviceWith(handle, cValues, aRowsCount, aRowPtr, aColIndices, aValues, bRowPtr, bColIndices, bValues, cRowPtr,
                                          cColIndices, baseIndex, valuesType, -1, 0);
}

} // extern "C"
