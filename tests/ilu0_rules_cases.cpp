// Stand-alone program around spgpu_amd/csrc/ilu0_rules.h (tests/test_ilu0_rules.py): one case per input line, either
//   segments solve shape maxBlocks levels w_0 ... w_{levels-1}      (w_l = the rows of level l; cut at the factorisation's own width)
// answered by "case <k>" and one line "firstLevel levels chained grid" per segment, in the order the rule emits them, or
//   shape rows nnz
// answered by "case <k>" and one line with the shape the public call chooses; "known <shape>" is answered by 0 or 1.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ilu0_rules.h"

int main()
{
    std::string line;
    int k = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what))
            continue;
        std::printf("case %d\n", k++);
        if (what == "shape") {
            int rows;
            long long nnz;
            in >> rows >> nnz;
            std::printf("%d\n", spgpu::ilu0Shape(nnz, rows));
        } else if (what == "known") {
            int shape;
            in >> shape;
            std::printf("%d\n", spgpu::ilu0ShapeKnown(shape) ? 1 : 0);
        } else {
            int solve, shape, maxBlocks, levels;
            in >> solve >> shape >> maxBlocks >> levels;
            std::vector<int> levelPtr(1, 0);
            for (int l = 0; l < levels; ++l) {
                int w;
                in >> w;
                levelPtr.push_back(levelPtr.back() + w);
            }
            spgpu::forEachTrsvSegment(levelPtr.data(), levels, solve, spgpu::kIlu0ChainWidth, [&](spgpu::TrsvSegment g) {
                const long long rows = (long long)levelPtr[g.firstLevel + g.levels] - levelPtr[g.firstLevel];
                std::printf("%d %d %d %u\n", g.firstLevel, g.levels, g.chained ? 1 : 0, g.chained ? 1u : spgpu::ilu0Grid(rows, shape, maxBlocks));
            });
        }
    }
    std::printf("constants %d %d %d %d %d %d %d %d\n", spgpu::kIlu0Threads, spgpu::kIlu0ChainWidth, spgpu::SPGPU_ILU0_SHAPE_THREAD,
                spgpu::kIlu0GroupNarrow, spgpu::kIlu0GroupWide, spgpu::kIlu0ThreadMaxMean, spgpu::kIlu0NarrowMaxMean, spgpu::kIlu0MaxGroup);
    return 0;
}
