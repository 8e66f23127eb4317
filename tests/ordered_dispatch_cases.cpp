/* Stand-alone driver of spgpu_amd/csrc/ordered_rules.h for tests/test_ordered_dispatch.py: what the ELL / HELL SpMV for rows ordered by
 * length launches and decides, computed by the header the library's ordered path (ellpack_spmv.hip launchOrdered, ragged_spmv.hip.h,
 * planned_spmv.hip, frozen_slab.hip.h) uses.  Built with
 *   g++ -std=c++17 -O1 -Wall -Werror -fsanitize=undefined -fno-sanitize-recover=all
 * stdin: one question per line, a rule's name and its integer arguments; stdout: one line of integers per question.
 *   shape elemBytes tiled shape          -> WAVES TILE_BYTES SUBS ZBYTES  rowsPerWorkgroup stagedShape planSubs mayPack(of planSubs)
 *   pack tiled elemBytes subs            -> mayPack packedKernels
 *   decide knob tiled rowOrder elemBytes probed noDeepList -> probesShape orderedShapeFor plannable(of that shape)
 *   said said calls                      -> orderedShapeSaid reprobe
 *   deep isHell maxNnz deepCap           -> deepKernelsFollow
 *   giveup uses stales                   -> planGivesUp
 *   split elemBytes deepCap asked        -> raggedSplit queueStep raggedMostChunks raggedUnroll(WIDE)
 *   grid rows subs                       -> queueGrid subGroupsOf
 *   plan mainBlocks deep                 -> planDeepBlocks planGrid planDeepStride(of that grid)
 *   layout blocks subGroups recordBytes  -> blockBytes countBytes listBytes total
 *   freeze slots                         -> packedBytes
 *   keeps entries escapes pct            -> keepsCopy
 *   constants                            -> kSubRows kPlanDeepMost kStagedShape kPlanRecordBytes kPlanDeepReachPct kRaggedSplitColumns
 * An unknown name ends the program with status 2. */
#include "ordered_rules.h"

#include <cstdio>
#include <cstring>

using namespace spgpu;

int main()
{
    char name[32];
    while (scanf("%31s", name) == 1) {
        long long v[6] = {0, 0, 0, 0, 0, 0};
        auto take = [&](int n) {
            for (int k = 0; k < n; ++k)
                if (scanf("%lld", v + k) != 1)
                    return false;
            return true;
        };
        auto is = [&](const char* rule, int n) { return strcmp(name, rule) == 0 && take(n); };
        if (is("shape", 3)) {
            const QueueShape s = queueShape((size_t)v[0], v[1] != 0, (int)v[2]);
            const int subs = planSubs((size_t)v[0], v[1] != 0, (int)v[2]);
            printf("%d %d %d %d  %d %d %d %d\n", s.waves, s.tileBytes, s.subs, s.zBytes, rowsPerWorkgroup(s), stagedShape((size_t)v[0], v[1] != 0, (int)v[2]), subs,
                   mayPack(v[1] != 0, (size_t)v[0], subs));
        } else if (is("pack", 3)) {
            printf("%d %d\n", mayPack(v[0] != 0, (size_t)v[1], (int)v[2]), packedKernels(v[0] != 0, (size_t)v[1]));
        } else if (is("decide", 6)) {
            const int shape = orderedShapeFor((int)v[0], v[1] != 0, v[2] != 0, (size_t)v[3], (int)v[4], v[5] != 0);
            printf("%d %d %d\n", probesShape((int)v[0], v[1] != 0, v[2] != 0, (size_t)v[3]), shape, plannable(v[1] != 0, shape));
        } else if (is("said", 2)) {
            printf("%d %d\n", orderedShapeSaid((int)v[0]), reprobe((int)v[0], (int)v[1]));
        } else if (is("deep", 3)) {
            printf("%d\n", deepKernelsFollow(v[0] != 0, (int)v[1], (int)v[2]));
        } else if (is("giveup", 2)) {
            printf("%d\n", planGivesUp((int)v[0], (int)v[1]));
        } else if (is("split", 3)) {
            printf("%d %d %d %d\n", raggedSplit((size_t)v[0], (int)v[1], (int)v[2]), queueStep((size_t)v[0]), raggedMostChunks((size_t)v[0]),
                   raggedUnroll(wideOf((size_t)v[0])));
        } else if (is("grid", 2)) {
            printf("%u %lld\n", queueGrid((int)v[0], (int)v[1]), subGroupsOf((int)v[0]));
        } else if (is("plan", 2)) {
            const unsigned grid = planGrid((int)v[0], (int)v[1]);
            printf("%u %u %d\n", planDeepBlocks((int)v[1]), grid, planDeepStride(grid, planDeepBlocks((int)v[1])));
        } else if (is("layout", 3)) {
            const PlanLayout at = planLayout(v[0], v[1], (size_t)v[2]);
            printf("%zu %zu %zu %zu\n", at.blockBytes, at.countBytes, at.listBytes, at.total);
        } else if (is("freeze", 1)) {
            printf("%zu\n", packedBytes(v[0]));
        } else if (is("keeps", 3)) {
            printf("%d\n", keepsCopy((unsigned long long)v[0], (unsigned long long)v[1], (int)v[2]));
        } else if (is("constants", 0)) {
            printf("%d %d %d %zu %d %d\n", kSubRows, kPlanDeepMost, kStagedShape, kPlanRecordBytes, kPlanDeepReachPct, kRaggedSplitColumns);
        } else {
            return 2;
        }
    }
    return 0;
}
