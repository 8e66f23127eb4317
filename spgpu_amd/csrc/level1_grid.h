#pragma once
/*
 * Where the Level-1 calls (level1.hip) and the fused solver steps (fused_solver.hip, fused_hdia.hip) choose their launches.  Plain host C++17, no
 * HIP header: the rules compile and run on their own (tests/level1_grid_cases.cpp).
 *
 * Every kernel of the family has one shape: kL1Threads lanes, kL1Unroll accesses in flight per lane -- of 16 bytes (WIDE elements)
 * where every operand allows it, else of one element --, a workgroup takes a tile of kL1Threads * kL1Unroll accesses per trip of a
 * tile-stride loop, grid.y = vector of a pitch multivector.  A call that must repeat the bits of another repeats its grid; so the
 * device-scalar reductions and the fused steps all ask reduceGrid.
 *
 * family (grid function)              one launch / passes     blocks of a vector at most     non-temporal kernel
 *   axpby, maxpby (axpbyGrid)         one launch              singleLaunchCap(count)         wide and narrow
 *   scal, abs, axy, axypbz (mapGrid)  one launch              singleLaunchCap(count)         wide only
 *   dot, nrm2, asum, amax, their m-forms, mdotDevice, mnrm2Device (reduceGrid)
 *                                     passes of `cap` vectors cap / vectors of the pass      wide only
 *   dotDevice, nrm2Device, axpbyPairDot, hellspmvDot (reduceGrid, one vector)
 *                                     one launch              cap                            never (spgpu?dot does: see DESIGN.md 3.9)
 *   hdiaspmvDot, diaspmvDot (fused_hdia.hip; reduceGrid, one vector: on w and z, as hellspmvDot; packedStrips for the coefficients)
 *                                     one launch              cap                            never (no such kernel)
 *   maxpbyPairDot (reduceGrid)        passes of `cap` vectors cap / vectors of the pass      never (no such kernel)
 *   axyDot, axpbyPairAxyDot (reduceGrid, one vector: on r and z, resp. on z2 as axpbyPairDot; d and w never count)
 *                                     one launch              cap                            never (no such kernel)
 *   maxyDot (reduceGrid)              passes of `cap` vectors cap / vectors of the pass      never (no such kernel)
 *   maxpbyPairAxyDot (reduceGrid)     passes of `cap` vectors cap / vectors of the pass      never (no such kernel)
 *                                     two sets of partials, [2][vectors][blocks], in a scratch of 2 * cap: a pass of more than
 *                                     cap / 2 vectors (one workgroup each) runs as two launches of at most cap / 2 vectors on
 *                                     the pass' grid and `wide`, so result[] keeps the bits of mdotDevice for every count
 *   axpbyDevice, maxpbyDevice (axpbyDeviceGrid)
 *                                     passes of kL1MaxBlocks  kL1MaxBlocks / vectors         never (no such kernel)
 * cap = SPGPU_REDUCE_MAX_BLOCKS (spgpu_internal.h), the partials the handle's scratch holds.  A reduction decides `wide` anew for every
 * pass, from the pass' own bases and vector count; maxpbyDevice decides once, from the call's.
 */
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

namespace spgpu {

constexpr int kL1Threads = 256;
constexpr int kL1Unroll = 4;        /* independent 16-byte accesses in flight per lane */
constexpr int kL1MaxBlocks = 16384; /* measured: 2 048 -> 64.7 %, 16 384 -> 71 % of 8 TB/s for axpby (tile-stride loop beyond) */
/* Vectors larger than the 256 MiB Infinity Cache cannot be found there again by the next kernel: stream them with the
 * non-temporal hint (measured, n = 1e8: 70-71 % -> 75.5-77 % of the HBM peak, profiles/r01d_level1_nt.txt).  Smaller ones -- the
 * vectors of a solver iteration -- stay cached. */
constexpr long long kL1StreamedBytes = 256ll << 20;

/* WIDE: elements of a 16-byte access. */
constexpr int wideOf(size_t elemBytes) { return (int)(16 / elemBytes); }

constexpr long long ceilDiv(long long a, long long b) { return (a + b - 1) / b; }

/* NULL lies on every boundary: an operand that is not given asks for nothing. */
inline bool allAligned(size_t bytes, std::initializer_list<const void*> pointers)
{
    for (const void* p : pointers)
        if ((uintptr_t)p % bytes != 0)
            return false;
    return true;
}

/* 16-byte accesses need more than one element in 16 bytes, every operand on a 16-byte boundary and, beyond one vector, a pitch that
 * keeps every vector there. */
inline bool wideAccess(size_t elemBytes, std::initializer_list<const void*> operands, int vectors, int pitch)
{
    return wideOf(elemBytes) > 1 && allAligned(16, operands) && (vectors == 1 || pitch % wideOf(elemBytes) == 0);
}

/* Workgroups of one vector: one per tile, `cap` at most (the tile-stride loop takes the rest). */
inline long long blocks(long long n, bool wide, size_t elemBytes, long long cap)
{
    const long long tiles = ceilDiv(wide ? ceilDiv(n, wideOf(elemBytes)) : n, (long long)kL1Threads * kL1Unroll);
    return tiles > cap ? cap : tiles;
}

/* One launch for `count` vectors, which share kL1MaxBlocks workgroups; at least one each. */
inline long long singleLaunchCap(int count) { return kL1MaxBlocks / (count < kL1MaxBlocks ? count : kL1MaxBlocks); }

/* Passes of at most perPass vectors, which share perPass workgroups (perPass / vectors each): f(first, vectors). */
template <typename F> inline void forEachPass(int count, int perPass, F&& f)
{
    for (long long first = 0; first < count; first += perPass)
        f((int)first, (int)(count - first < perPass ? count - first : perPass));
}

inline bool beyondCache(long long n, size_t elemBytes, int vectors, int streams)
{
    return n * (long long)elemBytes * vectors * streams >= kL1StreamedBytes;
}

struct L1Grid {
    bool wide;        /* 16-byte accesses */
    long long blocks; /* grid.x */
    bool nt;          /* the non-temporal kernel */
};

/* y counts for the alignment only where it is read.  Narrow streams go non-temporal too (exact aliasing of z is fine: a lane reads
 * its elements before it writes them). */
inline L1Grid axpbyGrid(size_t elemBytes, int n, int count, int pitch, const void* z, const void* x, const void* y, bool hasBeta)
{
    const bool wide = wideAccess(elemBytes, {z, x, hasBeta ? y : nullptr}, count, pitch);
    return {wide, blocks(n, wide, elemBytes, singleLaunchCap(count)), beyondCache(n, elemBytes, count, hasBeta ? 3 : 2)};
}

/* operands: the output and the inputs the operation reads (NULL for those it does not); streams: how many those are. */
inline L1Grid mapGrid(size_t elemBytes, int n, int count, int pitch, std::initializer_list<const void*> operands, int streams)
{
    const bool wide = wideAccess(elemBytes, operands, count, pitch);
    return {wide, blocks(n, wide, elemBytes, singleLaunchCap(count)), wide && beyondCache(n, elemBytes, count, streams)};
}

/* First stage of a reduction over the `vectors` vectors of one pass that start at a (and b: dot; NULL otherwise). */
inline L1Grid reduceGrid(size_t elemBytes, int n, int vectors, int pitch, const void* a, const void* b, bool mayStream, long long cap)
{
    const bool wide = wideAccess(elemBytes, {a, b}, vectors, pitch);
    return {wide, blocks(n, wide, elemBytes, cap / vectors), mayStream && wide && beyondCache(n, elemBytes, vectors, b ? 2 : 1)};
}

/* The update with coefficients in device memory, for a pass of `vectors` of the call's `count` vectors.  Which vectors read y is
 * known on the device only: its alignment counts whenever beta and y are given. */
inline L1Grid axpbyDeviceGrid(size_t elemBytes, int n, int count, int vectors, int pitch, const void* z, const void* x, const void* y,
                              bool hasBeta)
{
    const bool wide = wideAccess(elemBytes, {z, x, hasBeta ? y : nullptr}, count, pitch);
    return {wide, blocks(n, wide, elemBytes, kL1MaxBlocks / vectors), false};
}

/* hellspmvDot: VEC consecutive rows share one 16-byte load of lengths, coefficients and columns. */
inline bool packedRows(size_t elemBytes, bool wide, int hackSize, const void* cM, const void* rP, const void* rS)
{
    const int rows = wideOf(elemBytes);
    return wide && hackSize % rows == 0 && allAligned(16, {cM}) && allAligned(4 * rows, {rP, rS});
}

/* hdiaspmvDot, diaspmvDot: the VEC consecutive rows of a pack lie in one hack (DIA: one pitch) and their coefficients on a diagonal
 * are one 16-byte load. */
inline bool packedStrips(size_t elemBytes, bool wide, int hackSizeOrPitch, const void* dM)
{
    return wide && hackSizeOrPitch % wideOf(elemBytes) == 0 && allAligned(16, {dM});
}

/* Run-time choices as compile-time constants: f(std::bool_constant of each choice, in order).  A kernel's argument list is then
 * written once, inside f, for all of its instantiations. */
template <typename F> inline void withConstants(F&& f) { f(); }
template <typename F, typename... Rest> inline void withConstants(F&& f, bool first, Rest... rest)
{
    if (first)
        withConstants([&](auto... others) { f(std::true_type{}, others...); }, rest...);
    else
        withConstants([&](auto... others) { f(std::false_type{}, others...); }, rest...);
}

} // namespace spgpu
