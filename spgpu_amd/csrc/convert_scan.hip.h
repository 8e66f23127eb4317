#pragma once
/*
 * What the device-side constructions share (convert_device.hip: COO -> ELL / HELL / DIA; transpose_device.hip: HELL / ELL ->
 * the HELL arrays of the transpose): the launch width, the row-start search in sorted keys, the row lengths and their maximum,
 * and the three-launch exclusive scan.  Every kernel here has internal linkage, so each translation unit that includes the
 * header carries its own copy of the device code and nothing collides at link time.
 */
#include "numeric.hip.h"

namespace spgpu {

constexpr int kCvThreads = 256;
constexpr int kScanPerThread = 4;
constexpr int kScanTile = kCvThreads * kScanPerThread;

static size_t scanBlocks(long long n) { return (size_t)((n + kScanTile - 1) / kScanTile); }
static size_t alignUpCv(size_t v, size_t a) { return (v + a - 1) / a * a; }

static unsigned gridFor(long long n)
{
    const long long blocks = (n + kCvThreads - 1) / kCvThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 1048576 ? 1048576 : blocks));
}

/* rowStart[r] = first sorted position whose row (keys[p] >> shift) is >= r, r = 0 .. rows */
template <typename KEY>
static __global__ __launch_bounds__(kCvThreads) void rowStartKernel(int* rowStart, int rows, const KEY* keys, int shift, int nnz)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long r = (long long)blockIdx.x * kCvThreads + threadIdx.x; r <= rows; r += stride) {
        int lo = 0, hi = nnz;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((keys[mid] >> shift) < (KEY)r)
                lo = mid + 1;
            else
                hi = mid;
        }
        rowStart[r] = lo;
    }
}

static __global__ __launch_bounds__(kCvThreads) void rowLengthsKernel(int* rowLengths, const int* rowStart, int rows, int nnz, int* misc)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long r = (long long)blockIdx.x * kCvThreads + threadIdx.x; r < rows; r += stride)
        rowLengths[r] = rowStart[r + 1] - rowStart[r];
    if (blockIdx.x == 0 && threadIdx.x == 0 && rowStart[rows] < nnz)
        misc[1] = 1; /* entries outside the matrix: reported to the host, the entries skipped */
}

static __global__ __launch_bounds__(kCvThreads) void maxKernel(const int* values, long long n, int scale, int* misc)
{
    int best = 0;
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < n; i += stride)
        best = values[i] > best ? values[i] : best;
    best = waveMax(best);
    if ((threadIdx.x & (kWave - 1)) == 0 && best > 0)
        atomicMax(&misc[0], best * scale);
}

/* ---- exclusive scan in three launches: tile scans, scan of the tile totals, add-back ---- */
__device__ inline int blockExclusiveScan(int value, int* ldsWaveTotals, int* blockTotal)
{
    /* inclusive scan inside the wavefront with lane shuffles */
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    int incl = value;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int up = __shfl_up(incl, d, kWave);
        if (lane >= d)
            incl += up;
    }
    if (lane == kWave - 1)
        ldsWaveTotals[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kCvThreads / kWave; ++w) {
        if (w < wave)
            before += ldsWaveTotals[w];
        total += ldsWaveTotals[w];
    }
    __syncthreads();
    *blockTotal = total;
    return before + incl - value;
}

/* out[i] = sum_{j<i} in[j]*scale within the tile; tile total to totals[tile].  in == NULL scans totals in place. */
static __global__ __launch_bounds__(kCvThreads) void scanTilesKernel(int* out, const int* in, long long n, int scale, int* totals)
{
    __shared__ int waveTotals[kCvThreads / kWave];
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanPerThread;
    int v[kScanPerThread], mine = 0;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        v[j] = base + j < n ? in[base + j] * scale : 0;
        mine += v[j];
    }
    int total;
    int run = blockExclusiveScan(mine, waveTotals, &total);
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        if (base + j < n)
            out[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0)
        totals[blockIdx.x] = total;
}

/* single workgroup: exclusive scan of `count` tile totals in place, grand total to totals[count] */
static __global__ __launch_bounds__(kCvThreads) void scanTotalsKernel(int* totals, long long count)
{
    __shared__ int waveTotals[kCvThreads / kWave];
    int carry = 0;
    for (long long first = 0; first < count; first += kCvThreads) {
        const long long i = first + threadIdx.x;
        const int v = i < count ? totals[i] : 0;
        int total;
        const int excl = blockExclusiveScan(v, waveTotals, &total);
        if (i < count)
            totals[i] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0)
        totals[count] = carry;
}

static __global__ __launch_bounds__(kCvThreads) void addTotalsKernel(int* out, long long n, const int* totals)
{
    const long long base = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanPerThread;
    const int add = totals[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j)
        if (base + j < n)
            out[base + j] += add;
}

/* out[0..n) = exclusive scan of in[0..n)*scale; the grand total lands in totals[tiles] (device). */
static void exclusiveScan(hipStream_t s, int* out, const int* in, long long n, int scale, int* totals)
{
    const size_t tiles = scanBlocks(n);
    hipLaunchKernelGGL(scanTilesKernel, dim3((unsigned)tiles), dim3(kCvThreads), 0, s, out, in, n, scale, totals);
    hipLaunchKernelGGL(scanTotalsKernel, dim3(1), dim3(kCvThreads), 0, s, totals, (long long)tiles);
    hipLaunchKernelGGL(addTotalsKernel, dim3((unsigned)tiles), dim3(kCvThreads), 0, s, out, n, totals);
}

/* Layout of the head of `work` that spgpuHellPlanDevice and the COO calls use for a matrix of `rows` rows (ints):
 * misc[16] | rowStart[rows+1] | depth[rows] | scanTotals[tiles+2], rounded up to 64 ints. */
static size_t fixedInts(int rows) { return alignUpCv((size_t)16 + 2 * (size_t)rows + 1 + scanBlocks((long long)rows + 1) + 2, 64); }

} // namespace spgpu
