// Stand-alone program around spgpu_amd/csrc/trsv_rules.h (tests/test_trsv_rules.py): one case per input line,
//   solve width maxBlocks levels w_0 ... w_{levels-1}      (w_l = the rows of level l)
// answered by "case <k>" and one line "firstLevel levels chained grid" per segment, in the order the rule emits them.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "trsv_rules.h"

int main()
{
    std::string line;
    int k = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int solve, width, maxBlocks, levels;
        if (!(in >> solve >> width >> maxBlocks >> levels))
            continue;
        std::vector<int> levelPtr(1, 0);
        for (int l = 0; l < levels; ++l) {
            int w;
            in >> w;
            levelPtr.push_back(levelPtr.back() + w);
        }
        std::printf("case %d\n", k++);
        spgpu::forEachTrsvSegment(levelPtr.data(), levels, solve, width, [&](spgpu::TrsvSegment g) {
            const long long rows = (long long)levelPtr[g.firstLevel + g.levels] - levelPtr[g.firstLevel];
            std::printf("%d %d %d %u\n", g.firstLevel, g.levels, g.chained ? 1 : 0, g.chained ? 1u : spgpu::trsvGrid(rows, maxBlocks));
        });
    }
    std::printf("constants %d %d %d %d\n", spgpu::kTrsvThreads, spgpu::kTrsvChainWidth, spgpu::SPGPU_TRSV_SOLVE_PLAIN,
                spgpu::SPGPU_TRSV_SOLVE_CHAINED);
    return 0;
}
