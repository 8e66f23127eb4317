// Stand-alone program around spgpu_amd/csrc/colour_rules.h (tests/test_colour_rules.py): one case per input line,
//   shape rows nnz            answered by "case <k>" and one line with the shape the public colouring chooses;
//   known shape               answered by 0 or 1;
//   grid rows shape maxBlocks answered by the workgroups of a launch.
// The last line of the output is "constants threads thread maxGroup permuteShape".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "colour_rules.h"

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
            std::printf("%d\n", spgpu::colourShape(nnz, rows));
        } else if (what == "known") {
            int shape;
            in >> shape;
            std::printf("%d\n", spgpu::colourShapeKnown(shape) ? 1 : 0);
        } else {
            long long rows;
            int shape, maxBlocks;
            in >> rows >> shape >> maxBlocks;
            std::printf("%u\n", spgpu::colourGrid(rows, shape, maxBlocks));
        }
    }
    std::printf("constants %d %d %d %d\n", spgpu::kColourThreads, spgpu::SPGPU_COLOUR_SHAPE_THREAD, spgpu::kColourMaxGroup,
                spgpu::kColourPermuteShape);
    return 0;
}
