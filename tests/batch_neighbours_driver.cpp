// Runs whole systems through the arithmetic of csrc/nbody_batch_neighbours_math.h (include/nbody_batch_neighbours.h) on the CPU
// for tests/test_batch_neighbours_cpu.py: the functions batch_neighbours_kernel calls per row, here in sequential loops.
// Commands on stdin:
//   system N K RADIUS -> then N lines "x y z source" (coordinates read as double, narrowed to float; RADIUS a number, or "none").
//                          Prints  bodies sources listed complete mutual reserved mean_nearest mean_kth (%.17g)
//                          per row: "found within", the K indices, the K bits(r2)
//   layout            -> sizes of the two records and the offsets of their fields
//   empty             -> the empty index, the bits of the empty r2, the empty body record, the limit and the no-radius value
#include "nbody_batch_neighbours_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static unsigned float_bits(float f)
{
    unsigned w;
    std::memcpy(&w, &f, sizeof w);
    return w;
}

static void run_system(std::istringstream &in)
{
    int n = 0, k = 0;
    std::string radius;
    in >> n >> k >> radius;
    float b2 = kNeighboursNoRadius2;
    if (radius != "none") {
        const float b = (float)std::strtod(radius.c_str(), nullptr);
        b2 = b * b;  // one fp32 product
    }
    std::vector<float> x((size_t)3 * (size_t)(n > 0 ? n : 1));
    std::vector<int> flag((size_t)(n > 0 ? n : 1));
    int sources = 0;
    for (int i = 0; i < n; ++i) {
        std::string line, w[3];
        int source = 1;
        std::getline(std::cin, line);
        std::istringstream row(line);
        row >> w[0] >> w[1] >> w[2] >> source;
        for (int c = 0; c < 3; ++c)
            x[3 * i + c] = (float)std::strtod(w[c].c_str(), nullptr);
        flag[i] = source ? 1 : 0;
        sources += flag[i];
    }
    std::vector<NeighbourList> list((size_t)(n > 0 ? n : 1));
    std::vector<int> nearest((size_t)(n > 0 ? n : 1)), found((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {  // every row over the columns in ascending j; a column that is no source is skipped
        neighbours_clear(list[i]);
        for (int j = 0; j < n; ++j) {
            if (!flag[j])
                continue;
            neighbours_step(list[i], i, x[3 * i], x[3 * i + 1], x[3 * i + 2], x[3 * j], x[3 * j + 1], x[3 * j + 2], true, j, b2);
        }
        found[i] = neighbours_found(list[i], k);
        nearest[i] = list[i].index[0];
    }
    int listed = 0, complete = 0, mutual = 0;
    double nearest_sum = 0.0, kth_sum = 0.0;
    for (int i = 0; i < n; ++i) {  // ascending i
        listed += found[i] >= 1 ? 1 : 0;
        complete += found[i] == k ? 1 : 0;
        mutual += neighbours_mutual(nearest.data(), i) ? 1 : 0;
        nearest_sum += neighbours_term(found[i] >= 1, list[i].r2[0]);
        kth_sum += neighbours_term(found[i] == k, neighbours_kth(list[i], k));
    }
    std::printf("%d %d %d %d %d %d %.17g %.17g\n", n, sources, listed, complete, mutual, 0, neighbours_mean(nearest_sum, listed),
                neighbours_mean(kth_sum, complete));
    for (int i = 0; i < n; ++i) {
        std::printf("%d %d", found[i], list[i].within);
        for (int t = 0; t < k; ++t)
            std::printf(" %d", list[i].index[t]);
        for (int t = 0; t < k; ++t)
            std::printf(" %u", float_bits(list[i].r2[t]));
        std::printf("\n");
    }
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "system") {
            run_system(in);
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu\n", sizeof(BatchNeighbourSystem),
                        offsetof(BatchNeighbourSystem, bodies), offsetof(BatchNeighbourSystem, sources),
                        offsetof(BatchNeighbourSystem, listed), offsetof(BatchNeighbourSystem, complete),
                        offsetof(BatchNeighbourSystem, mutual), offsetof(BatchNeighbourSystem, reserved),
                        offsetof(BatchNeighbourSystem, mean_nearest), offsetof(BatchNeighbourSystem, mean_kth),
                        sizeof(BatchNeighbourBody), offsetof(BatchNeighbourBody, found), offsetof(BatchNeighbourBody, within));
        } else if (word == "empty") {
            const BatchNeighbourBody b = neighbours_empty_body();
            std::printf("%d %u %d %d %d %g\n", kNeighboursNoIndex, float_bits(neighbours_no_r2()), b.found, b.within, kNeighboursMax,
                        (double)kNeighboursNoRadius2);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
