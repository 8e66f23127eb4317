/* Stand-alone driver of spgpu_amd/csrc/level1_grid.h for tests/test_level1_grid.py: the launches each Level-1 / fused family makes,
 * computed by the header the library's call sites use, on operands that exist as addresses only.  Built with
 *   g++ -std=c++17 -fsanitize=undefined -fno-sanitize-recover=all -DSPGPU_REDUCE_MAX_BLOCKS=<spgpu_internal.h's>
 * stdin, one case per line:  family elemBytes n count pitch hasBeta yGiven extra off0 off1 off2 off3 off4
 *   off*: bytes by which operand k lies past a 16-byte boundary, in the family's order:
 *     map out x y z (extra: streams 2 scal/abs, 3 axy, 4 axypbz)     axpby, axpby-device, axpby-device-mv  z x y (yGiven 0: y == NULL)
 *     reduce, reduce-device  a b (extra: 2 dot, 1 otherwise: b == NULL)     pair-dot, pair-dot-mv  z2     spmv-dot  w z cM rP rS (extra: hackSize)
 * stdout: "case <line number>", then one line per launch: first vectors wide blocks nt, and for spmv-dot a sixth field packed.
 * A call that launches no first stage (n <= 0) prints blocks 0 for each of its passes, as the device-result calls see it. */
#include "level1_grid.h"

#include <cstdio>
#include <cstring>

using namespace spgpu;

static const void* at(int operand, long long off, long long shiftBytes = 0)
{
    return (const void*)(((uintptr_t)(operand + 1) << 52) + (uintptr_t)off + (uintptr_t)shiftBytes);
}

static void say(int first, int vectors, const L1Grid& g) { printf("%d %d %d %lld %d\n", first, vectors, g.wide, g.blocks, g.nt); }

int main()
{
    char family[32];
    long long eb, n, count, pitch, hasBeta, yGiven, extra, off[5];
    for (int line = 0; scanf("%31s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", family, &eb, &n, &count, &pitch, &hasBeta,
                             &yGiven, &extra, off, off + 1, off + 2, off + 3, off + 4) == 13; ++line) {
        printf("case %d\n", line);
        const size_t size = (size_t)eb;
        const void* y = yGiven ? at(2, off[2]) : nullptr;
        const L1Grid none = {false, 0, false};
        auto is = [&](const char* name) { return strcmp(family, name) == 0; };
        auto shift = [&](int first) { return (long long)first * pitch * eb; };
        if (is("map")) {
            if (n > 0 && count > 0)
                say(0, (int)count, mapGrid(size, (int)n, (int)count, (int)pitch,
                                           {at(0, off[0]), at(1, off[1]), extra >= 3 ? at(2, off[2]) : nullptr, extra == 4 ? at(3, off[3]) : nullptr},
                                           (int)extra));
        } else if (is("axpby")) {
            if (n > 0 && count > 0)
                say(0, (int)count, axpbyGrid(size, (int)n, (int)count, (int)pitch, at(0, off[0]), at(1, off[1]), y, hasBeta != 0));
        } else if (is("reduce")) {
            forEachPass((int)count, SPGPU_REDUCE_MAX_BLOCKS, [&](int first, int vectors) {
                say(first, vectors, n <= 0 ? none : reduceGrid(size, (int)n, vectors, (int)pitch, at(0, off[0], shift(first)),
                                                                extra == 2 ? at(1, off[1], shift(first)) : nullptr, true, SPGPU_REDUCE_MAX_BLOCKS));
            });
        } else if (is("reduce-device")) {
            say(0, 1, n <= 0 ? none : reduceGrid(size, (int)n, 1, 0, at(0, off[0]), extra == 2 ? at(1, off[1]) : nullptr, false, SPGPU_REDUCE_MAX_BLOCKS));
        } else if (is("axpby-device")) {
            if (n > 0)
                say(0, 1, axpbyDeviceGrid(size, (int)n, 1, 1, 0, at(0, off[0]), at(1, off[1]), y, hasBeta != 0));
        } else if (is("axpby-device-mv")) {
            if (n > 0)
                forEachPass((int)count, kL1MaxBlocks, [&](int first, int vectors) {
                    say(first, vectors, axpbyDeviceGrid(size, (int)n, (int)count, vectors, (int)pitch, at(0, off[0]), at(1, off[1]), y, hasBeta != 0));
                });
        } else if (is("pair-dot")) {
            say(0, 1, n <= 0 ? none : reduceGrid(size, (int)n, 1, 0, at(0, off[0]), at(0, off[0]), false, SPGPU_REDUCE_MAX_BLOCKS));
        } else if (is("pair-dot-mv")) {
            forEachPass((int)count, SPGPU_REDUCE_MAX_BLOCKS, [&](int first, int vectors) {
                const void* z2 = at(0, off[0], shift(first));
                say(first, vectors, n <= 0 ? none : reduceGrid(size, (int)n, vectors, (int)pitch, z2, z2, false, SPGPU_REDUCE_MAX_BLOCKS));
            });
        } else if (is("spmv-dot")) {
            const L1Grid g = n <= 0 ? none : reduceGrid(size, (int)n, 1, 0, at(0, off[0]), at(1, off[1]), false, SPGPU_REDUCE_MAX_BLOCKS);
            printf("0 1 %d %lld %d %d\n", g.wide, g.blocks, g.nt,
                   n > 0 && packedRows(size, g.wide, (int)extra, at(2, off[2]), at(3, off[3]), at(4, off[4])));
        } else {
            fprintf(stderr, "unknown family %s\n", family);
            return 2;
        }
    }
    return 0;
}
