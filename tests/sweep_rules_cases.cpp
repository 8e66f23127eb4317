// Stand-alone program around spgpu_amd/csrc/sweep_rules.h (tests/test_sweep_rules.py): one case per input line,
//   shape rows nnz                  answered by "case <k>" and one line with the shape the public calls choose;
//   known shape                     answered by 0 or 1;
//   grid rows shape maxBlocks       answered by the workgroups of a grid-strided launch;
//   segments step solve n p0 .. pn  answered by one line "firstColour colours step chained" per segment of the list (step 1:
//                                   colourPtrHost p as it is; step -1: its reversal) and a last line "launches <count>".
// The last line of the output is "constants threads chainWidth chainPasses thread narrow wide maxGroup threadMaxMean narrowMaxMean".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sweep_rules.h"

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
            std::printf("%d\n", spgpu::sweepShape(nnz, rows));
        } else if (what == "known") {
            int shape;
            in >> shape;
            std::printf("%d\n", spgpu::sweepShapeKnown(shape) ? 1 : 0);
        } else if (what == "grid") {
            long long rows;
            int shape, maxBlocks;
            in >> rows >> shape >> maxBlocks;
            std::printf("%u\n", spgpu::sweepGrid(rows, shape, maxBlocks));
        } else {
            int step, solve, n;
            in >> step >> solve >> n;
            std::vector<int> ptr((size_t)n + 1), reversed((size_t)n + 1);
            for (int& p : ptr)
                in >> p;
            spgpu::sweepReversed(reversed.data(), ptr.data(), n);
            const int* list = step > 0 ? ptr.data() : reversed.data();
            spgpu::forEachSweepSegment(list, n, step, solve, [](spgpu::SweepSegment g) {
                std::printf("%d %d %d %d\n", g.firstColour, g.colours, g.step, g.chained ? 1 : 0);
            });
            std::printf("launches %d\n", spgpu::sweepLaunches(list, n, solve));
        }
    }
    std::printf("constants %d %d %d %d %d %d %d %d %d\n", spgpu::kSweepThreads, spgpu::kSweepChainWidth, spgpu::kSweepChainPasses,
                spgpu::SPGPU_SWEEP_SHAPE_THREAD, spgpu::kSweepGroupNarrow, spgpu::kSweepGroupWide, spgpu::kSweepMaxGroup,
                spgpu::kSweepThreadMaxMean, spgpu::kSweepNarrowMaxMean);
    return 0;
}
