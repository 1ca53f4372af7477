// Prints the fp64 record csrc/nbody_batch_pairs_elements.h computes for one pair (include/nbody_batch_pairs.h, "The record")
// as text for tests/test_batch_pairs_cpu.py.  One case per line on stdin, one line of output each:
//   xi yi zi vxi vyi vzi xj yj zj vxj vyj vzj mu   (the twelve state words are rounded to fp32, mu is taken in fp64)
//       -> partner mutual energy semi_major_axis eccentricity inclination separation (%.17g; inf and -inf as printf writes them)
//   empty -> the empty record
//   sizeof -> the size of the record in bytes
#include "nbody_batch_pairs_elements.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

using namespace nbody;

static void print(const BatchPairRecord &r)
{
    std::printf("%d %d %.17g %.17g %.17g %.17g %.17g\n", r.partner, r.mutual, r.energy, r.semi_major_axis, r.eccentricity,
                r.inclination, r.separation);
}

int main()
{
    std::string word;
    while (std::cin >> word) {
        if (word == "empty") {
            print(batch_pair_empty());
            continue;
        }
        if (word == "sizeof") {
            std::printf("%zu\n", sizeof(BatchPairRecord));
            continue;
        }
        float s[12];
        s[0] = std::strtof(word.c_str(), nullptr);
        for (int k = 1; k < 12; ++k) {
            std::cin >> word;
            s[k] = std::strtof(word.c_str(), nullptr);
        }
        std::cin >> word;
        const double mu = std::strtod(word.c_str(), nullptr);
        if (!std::cin) {
            std::fprintf(stderr, "a case needs thirteen numbers\n");
            return 1;
        }
        print(batch_pair_record(1, 1, s, s + 3, s + 6, s + 9, mu));
    }
    return 0;
}
