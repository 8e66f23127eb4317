#pragma once
/*
 * The host rules that the device calls on CSR arrays share (to_csr, update, convert_csr, assemble, spgemm, add, trsv, ilu0 and
 * aggregate _device.hip): the capped grid, the key bits of a count and the dispatch on the value type.  Plain host C++17, no HIP
 * header: the rules compile and run on their own (tests/csr_host_cases.cpp).
 */
#include "cx.h"

namespace spgpu {

constexpr int kCsrMaxBlocks = 1048576; /* as gridFor of convert_scan.hip.h; every kernel launched by this rule strides */

/* workgroups for `items` items at `perBlock` a workgroup: at least 1, at most maxBlocks (> 0) or kCsrMaxBlocks */
inline unsigned cappedGrid(long long items, int perBlock, int maxBlocks)
{
    const long long cap = maxBlocks > 0 ? (long long)maxBlocks : (long long)kCsrMaxBlocks;
    const long long blocks = (items + perBlock - 1) / perBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

/* smallest b with 2^b >= n (n >= 1) */
inline int bitsFor(long long n)
{
    int b = 0;
    while (((long long)1 << b) < n)
        ++b;
    return b;
}

/* The codes of spgpuType_t (include/spgpu/core.h, which needs HIP; csr_shared.hip.h checks that they are the same). */
enum { kTypeFloat = 1, kTypeDouble = 2, kTypeComplexFloat = 3, kTypeComplexDouble = 4 };

/* f(T{}) for the element type T of a value type's code, and true; any other code: false, f is not called.  The caller writes
 * `using T = decltype(tag)`. */
template <typename F> inline bool forValueType(int type, F&& f)
{
    switch (type) {
    case kTypeFloat:
        f(float{});
        return true;
    case kTypeDouble:
        f(double{});
        return true;
    case kTypeComplexFloat:
        f(cfloat{});
        return true;
    case kTypeComplexDouble:
        f(cdouble{});
        return true;
    default:
        return false;
    }
}

} // namespace spgpu
