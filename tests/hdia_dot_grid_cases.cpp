/* Stand-alone driver of spgpu_amd/csrc/level1_grid.h for tests/test_hdia_dot_launch_shapes.py: the launch spgpu?hdiaspmvDotDevice /
 * spgpu?diaspmvDotDevice makes (fused_hdia.hip: hdiaSpmvDot), computed by the header the call site uses, on operands that exist as
 * addresses only.  Built with
 *   g++ -std=c++17 -fsanitize=undefined -fno-sanitize-recover=all -DSPGPU_REDUCE_MAX_BLOCKS=<spgpu_internal.h's>
 * stdin, one case per line:  elemBytes rows hackSizeOrPitch offW offZ offDM   (off*: bytes past a 16-byte boundary)
 * stdout, one line per case:  wide blocks nt packed   (rows <= 0 or hackSizeOrPitch <= 0: no first stage, 0 0 0 0). */
#include "level1_grid.h"

#include <cstdio>

using namespace spgpu;

static const void* at(int operand, long long off) { return (const void*)(((uintptr_t)(operand + 1) << 52) + (uintptr_t)off); }

int main()
{
    long long eb, rows, hack, offW, offZ, offDM;
    while (scanf("%lld %lld %lld %lld %lld %lld", &eb, &rows, &hack, &offW, &offZ, &offDM) == 6) {
        if (rows <= 0 || hack <= 0) {
            printf("0 0 0 0\n");
            continue;
        }
        const L1Grid g = reduceGrid((size_t)eb, (int)rows, 1, 0, at(0, offW), at(1, offZ), false, SPGPU_REDUCE_MAX_BLOCKS);
        printf("%d %lld %d %d\n", g.wide, g.blocks, g.nt, packedStrips((size_t)eb, g.wide, (int)hack, at(2, offDM)));
    }
    return 0;
}
