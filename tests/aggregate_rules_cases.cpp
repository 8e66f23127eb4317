// Stand-alone program around spgpu_amd/csrc/aggregate_rules.h (tests/test_aggregate_rules.py): one case per input line,
//   shape rows nnz            answered by "case <k>" and one line with the shape the public aggregation chooses;
//   known shape               answered by 0 or 1;
//   grid rows shape maxBlocks answered by the workgroups of a launch.
// The last line of the output is "constants threads thread narrow wide threadMaxMean narrowMaxMean maxGroup".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "aggregate_rules.h"

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
            std::printf("%d\n", spgpu::aggShape(nnz, rows));
        } else if (what == "known") {
            int shape;
            in >> shape;
            std::printf("%d\n", spgpu::aggShapeKnown(shape) ? 1 : 0);
        } else {
            long long rows;
            int shape, maxBlocks;
            in >> rows >> shape >> maxBlocks;
            std::printf("%u\n", spgpu::aggGrid(rows, shape, maxBlocks));
        }
    }
    std::printf("constants %d %d %d %d %d %d %d\n", spgpu::kAggThreads, spgpu::SPGPU_AGG_SHAPE_THREAD, spgpu::kAggGroupNarrow, spgpu::kAggGroupWide,
                spgpu::kAggThreadMaxMean, spgpu::kAggNarrowMaxMean, spgpu::kAggMaxGroup);
    return 0;
}
