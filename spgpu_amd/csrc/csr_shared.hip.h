#pragma once
/*
 * What the device calls on CSR arrays share on the device (assemble, spgemm, add, trsv, ilu0 and aggregate _device.hip): the
 * arithmetic of their bit-exactness contracts, the lower-bound bisection, and two set-up kernels.  A new call on CSR arrays starts
 * from this header and from csr_host.h.  The kernels have internal linkage, as those of convert_scan.hip.h: each translation unit
 * that includes the header carries its own copy of the device code and nothing collides at link time.
 */
#include "convert_scan.hip.h"
#include "csr_host.h"
#include "spgpu/core.h"

namespace spgpu {

static_assert(kTypeFloat == SPGPU_TYPE_FLOAT && kTypeDouble == SPGPU_TYPE_DOUBLE && kTypeComplexFloat == SPGPU_TYPE_COMPLEX_FLOAT &&
                  kTypeComplexDouble == SPGPU_TYPE_COMPLEX_DOUBLE,
              "forValueType switches on the codes of spgpuType_t");

/* ---- the arithmetic of the contracts ----
 * Every operation is rounded on its own.  hipcc contracts by default: the pragma in each body keeps it from fusing a product into
 * the sum or difference that follows.  The headers of the calls state these expression trees, the tests restate them and compare
 * bytes: a change here changes the results of every call of the family. */
/* s * v, rounded once; complex: four products, a difference and a sum, each rounded */
__device__ inline float exactMul(float s, float v)
{
#pragma clang fp contract(off)
    return s * v;
}
__device__ inline double exactMul(double s, double v)
{
#pragma clang fp contract(off)
    return s * v;
}
template <typename R> __device__ inline Cx<R> exactMul(Cx<R> s, Cx<R> v)
{
#pragma clang fp contract(off)
    const R rr = s.x * v.x, ii = s.y * v.y, ri = s.x * v.y, ir = s.y * v.x;
    const R re = rr - ii, im = ri + ir;
    return Cx<R>{re, im};
}
/* (alpha * a) + (beta * b): the two products rounded, then the sum */
__device__ inline float exactScaledSum(float alpha, float a, float beta, float b)
{
#pragma clang fp contract(off)
    const float p = alpha * a, q = beta * b;
    return p + q;
}
__device__ inline double exactScaledSum(double alpha, double a, double beta, double b)
{
#pragma clang fp contract(off)
    const double p = alpha * a, q = beta * b;
    return p + q;
}
template <typename R> __device__ inline Cx<R> exactScaledSum(Cx<R> alpha, Cx<R> a, Cx<R> beta, Cx<R> b)
{
#pragma clang fp contract(off)
    const Cx<R> p = exactMul(alpha, a), q = exactMul(beta, b);
    const R re = p.x + q.x, im = p.y + q.y;
    return Cx<R>{re, im};
}
/* s + a * b, the product rounded, then the sum */
__device__ inline float exactMulAdd(float s, float a, float b)
{
#pragma clang fp contract(off)
    const float p = a * b;
    return s + p;
}
__device__ inline double exactMulAdd(double s, double a, double b)
{
#pragma clang fp contract(off)
    const double p = a * b;
    return s + p;
}
/* re = ar*br - ai*bi, im = ar*bi + ai*br: four products, a difference and a sum, each rounded, then the two sums */
template <typename R> __device__ inline Cx<R> exactMulAdd(Cx<R> s, Cx<R> a, Cx<R> b)
{
#pragma clang fp contract(off)
    const R rr = a.x * b.x, ii = a.y * b.y, ri = a.x * b.y, ir = a.y * b.x;
    const R re = rr - ii, im = ri + ir;
    return Cx<R>{s.x + re, s.y + im};
}
/* acc - (a * x): the product rounded, then the difference */
__device__ inline float exactSubMul(float acc, float a, float x)
{
#pragma clang fp contract(off)
    const float p = a * x;
    return acc - p;
}
__device__ inline double exactSubMul(double acc, double a, double x)
{
#pragma clang fp contract(off)
    const double p = a * x;
    return acc - p;
}
template <typename R> __device__ inline Cx<R> exactSubMul(Cx<R> acc, Cx<R> a, Cx<R> x)
{
#pragma clang fp contract(off)
    const R rr = a.x * x.x, ii = a.y * x.y, ri = a.x * x.y, ir = a.y * x.x;
    const R re = rr - ii, im = ri + ir;
    const R outRe = acc.x - re, outIm = acc.y - im;
    return Cx<R>{outRe, outIm};
}
/* n / d: one correctly rounded division (hipcc's default for fp32 too: no fast-math flag is passed) */
__device__ inline float exactDiv(float n, float d)
{
#pragma clang fp contract(off)
    return n / d;
}
__device__ inline double exactDiv(double n, double d)
{
#pragma clang fp contract(off)
    return n / d;
}
/* the textbook quotient, every operation rounded separately; den may overflow or underflow (the headers of the calls say so) */
template <typename R> __device__ inline Cx<R> exactDiv(Cx<R> n, Cx<R> d)
{
#pragma clang fp contract(off)
    const R rr = d.x * d.x, ii = d.y * d.y;
    const R den = rr + ii;
    const R a = n.x * d.x, b = n.y * d.y, c = n.y * d.x, e = n.x * d.y;
    const R top = a + b, bottom = c - e;
    const R re = top / den, im = bottom / den;
    return Cx<R>{re, im};
}

/* ---- search ---- */
/* the first position in [lo, hi) of `sorted` (ascending) whose element is not below `value`; hi if there is none.  The bisections
 * that spgemm, ilu0, aggregate and the tile bounds of the sum write out by hand are this loop: folding them in reordered two
 * instructions of their kernels, and they were left as they are (profiles/csr_shared_kernel_diff.txt). */
template <typename E, typename I> __device__ inline I lowerBound(const E* sorted, I lo, I hi, E value)
{
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < value)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* ---- set-up kernels ---- */
static __global__ __launch_bounds__(kCvThreads) void csrSetIntsKernel(int* out, long long n, int value)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long i = (long long)blockIdx.x * kCvThreads + threadIdx.x; i < n; i += stride)
        out[i] = value;
}

/* flags[p] = 1 where sorted position p starts a new key */
static __global__ __launch_bounds__(kCvThreads) void csrHeadFlagsKernel(int* flags, const unsigned long long* keys, int n)
{
    const long long stride = (long long)gridDim.x * kCvThreads;
    for (long long p = (long long)blockIdx.x * kCvThreads + threadIdx.x; p < n; p += stride)
        flags[p] = p == 0 || keys[p] != keys[p - 1];
}

} // namespace spgpu
