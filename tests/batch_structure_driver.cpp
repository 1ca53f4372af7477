// Checks the arithmetic of csrc/nbody_batch_structure_math.h (include/nbody_batch_structure.h) on the CPU for
// tests/test_batch_structure_cpu.py.  One command per line on stdin, one line of output each:
//   insert v1 v2 ...  -> the eight-smallest list after inserting the values in that order (%.9g; inf as printf writes it)
//   kth k a0 ... a7   -> structure_kth of that list
//   density r2_k w    -> structure_density of the two floats (%.17g)
//   sorted SEED COUNT -> COUNT random sequences (duplicates, +inf, fewer than eight finite entries among them) inserted and
//                        compared with std::sort, every k compared with the sorted sequence: "ok COUNT" or the first mismatch
//   layout            -> sizes of the two records and the offsets of their fields
//   empty             -> the empty body record and the empty system record
#include "nbody_batch_structure_math.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static const float kInf = std::numeric_limits<float>::infinity();

static void fresh(float (&a)[kStructureMaxNeighbour])
{
    for (float &v : a)
        v = kInf;
}

static int sorted(unsigned seed, int count)
{
    std::mt19937 rng(seed);
    for (int c = 0; c < count; ++c) {
        const int len = (int)(rng() % 40);                   // 0 .. 39 values: fewer than eight among them
        const int palette = 1 + (int)(rng() % 12);           // few distinct values: duplicates
        std::vector<float> seq(len);
        for (float &v : seq) {
            const unsigned r = rng() % 10;
            v = r == 0 ? kInf : r < 5 ? (float)(rng() % palette) * 0.25f + 0.125f : (float)(rng() % 100000) / 1024.0f;
        }
        float a[kStructureMaxNeighbour];
        fresh(a);
        for (float v : seq)
            structure_insert(a, v);
        std::vector<float> want(seq);
        std::sort(want.begin(), want.end());
        want.resize(kStructureMaxNeighbour, kInf);
        for (int t = 0; t < kStructureMaxNeighbour; ++t)
            if (!(a[t] == want[t]) || !(structure_kth(a, t + 1) == want[t])) {
                std::printf("mismatch in sequence %d at %d: %.9g against %.9g, kth %.9g\n", c, t, a[t], want[t], structure_kth(a, t + 1));
                return 1;
            }
    }
    std::printf("ok %d\n", count);
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "insert") {
            float a[kStructureMaxNeighbour];
            fresh(a);
            while (in >> word)
                structure_insert(a, std::strtof(word.c_str(), nullptr));
            for (int t = 0; t < kStructureMaxNeighbour; ++t)
                std::printf("%.9g%c", a[t], t + 1 < kStructureMaxNeighbour ? ' ' : '\n');
        } else if (word == "kth") {
            int k = 0;
            float a[kStructureMaxNeighbour];
            in >> k;
            for (float &v : a) {
                in >> word;
                v = std::strtof(word.c_str(), nullptr);
            }
            std::printf("%.9g\n", structure_kth(a, k));
        } else if (word == "density") {
            std::string r2, w;
            in >> r2 >> w;
            std::printf("%.17g\n", structure_density(std::strtof(r2.c_str(), nullptr), std::strtof(w.c_str(), nullptr)));
        } else if (word == "sorted") {
            unsigned seed = 0;
            int count = 0;
            in >> seed >> count;
            if (sorted(seed, count))
                return 1;
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchStructureBody),
                        offsetof(BatchStructureBody, density), offsetof(BatchStructureBody, radius), offsetof(BatchStructureBody, enclosed),
                        offsetof(BatchStructureBody, neighbour_r2), offsetof(BatchStructureBody, neighbour_weight),
                        offsetof(BatchStructureBody, inside), sizeof(BatchStructureSystem), offsetof(BatchStructureSystem, centre),
                        offsetof(BatchStructureSystem, core_radius), offsetof(BatchStructureSystem, core_density),
                        offsetof(BatchStructureSystem, total_weight), offsetof(BatchStructureSystem, lagrange),
                        offsetof(BatchStructureSystem, estimated));
        } else if (word == "empty") {
            const BatchStructureBody b = structure_empty_body();
            const BatchStructureSystem s = structure_empty_system();
            double sum = s.centre[0] + s.centre[1] + s.centre[2] + s.core_radius + s.core_density + s.total_weight;
            for (double v : s.lagrange)
                sum += v;
            std::printf("%g %g %g %g %g %d %d  %g %d %d\n", b.density, b.radius, b.enclosed, (double)b.neighbour_r2,
                        (double)b.neighbour_weight, b.inside, b.reserved, sum, s.estimated, s.reserved);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
