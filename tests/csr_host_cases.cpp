// Stand-alone program around spgpu_amd/csrc/csr_host.h (tests/test_csr_host.py): one case per input line,
//   grid items perBlock maxBlocks   ->  "grid <workgroups>"
//   bits n                          ->  "bits <b>"
//   type code                       ->  "type <returned 0|1> <calls of f> <sizeof of the element f got, 0 without a call> <1 if floating>"
// and a last line "constants <kCsrMaxBlocks>".
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <type_traits>

#include "csr_host.h"

template <typename T> struct IsReal : std::is_floating_point<T> {};
template <typename R> struct IsReal<spgpu::Cx<R>> : std::false_type {};

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "grid") {
            long long items;
            int perBlock, maxBlocks;
            in >> items >> perBlock >> maxBlocks;
            std::printf("grid %u\n", spgpu::cappedGrid(items, perBlock, maxBlocks));
        } else if (what == "bits") {
            long long n;
            in >> n;
            std::printf("bits %d\n", spgpu::bitsFor(n));
        } else if (what == "type") {
            int code, calls = 0, real = 0;
            unsigned long size = 0;
            in >> code;
            const bool known = spgpu::forValueType(code, [&](auto tag) {
                using T = decltype(tag);
                ++calls;
                size = sizeof(T);
                real = IsReal<T>::value ? 1 : 0;
            });
            std::printf("type %d %d %lu %d\n", known ? 1 : 0, calls, size, real);
        }
    }
    std::printf("constants %d\n", spgpu::kCsrMaxBlocks);
    return 0;
}
