// Checks the arithmetic and the launch plan of csrc/nbody_batch_gravity_math.h (include/nbody_batch_gravity.h) on the CPU for
// tests/test_batch_gravity_cpu.py.  A stand-alone program: it may be built with -fsanitize=address,undefined.  One command per
// line on stdin:
//   field EPS SELF M R  sx sy sz sm (M times)  x y z (R times)
//                     -> R lines "ax ay az phi txx txy txz tyy tyz tzz": every row against the M sources in ascending order
//                        through gravity_pair and GravityRow, as batch_gravity_kernel does it, with the guard when EPS == 0 and,
//                        when SELF != 0, source j == row skipped.  Floats as %.9g, the potential as %.17g.  The rsq is
//                        1 / sqrtf here.
//   plan own N        -> "rpl threads blocks lds": gravity_plan_own(N) and gravity_lds_bytes(N)
//   plan points P     -> "rpl threads blocks": gravity_plan_points(P)
//   cover own N | cover points P
//                     -> "least most beyond": over every block, lane and q of the plan, how often the least and the most served
//                        row in [0, N or P) is reached through gravity_row, and how many rows beyond are
//   layout            -> size of the record, the offsets of its fields, the limit, and the words of the empty record
#include "nbody_batch_gravity_math.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

template <bool GUARD>
static void field(float eps2, bool self, const std::vector<float> &src, const std::vector<float> &rows)
{
    const int m = (int)(src.size() / 4), R = (int)(rows.size() / 3);
    for (int r = 0; r < R; ++r) {
        GravityRow<true> row;
        GravityRow<false> lean;
        for (int j = 0; j < m; ++j) {
            const float *s = &src[4 * (size_t)j];
            row.add(gravity_pair<GUARD, true>(rows[3 * (size_t)r], rows[3 * (size_t)r + 1], rows[3 * (size_t)r + 2], s[0], s[1], s[2], s[3],
                                              eps2, self && j == r));
            lean.add(gravity_pair<GUARD, false>(rows[3 * (size_t)r], rows[3 * (size_t)r + 1], rows[3 * (size_t)r + 2], s[0], s[1], s[2], s[3],
                                                eps2, self && j == r));
        }
        const BatchGravityRecord g = row.record(), h = lean.record();
        if (g.acceleration[0] != h.acceleration[0] || g.acceleration[1] != h.acceleration[1] || g.acceleration[2] != h.acceleration[2] ||
            g.potential != h.potential) {
            std::fprintf(stderr, "the record depends on TIDAL in row %d\n", r);
            std::exit(3);
        }
        float t[kGravityTidalWords];
        row.tidal(t);
        std::printf("%.9g %.9g %.9g %.17g %.9g %.9g %.9g %.9g %.9g %.9g\n", g.acceleration[0], g.acceleration[1], g.acceleration[2],
                    g.potential, t[0], t[1], t[2], t[3], t[4], t[5]);
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
        if (word == "field") {
            std::string eps;
            int self = 0, m = 0, R = 0;
            in >> eps >> self >> m >> R;
            if (!in || m < 0 || R < 0 || m > 1 << 20 || R > 1 << 20) {
                std::fprintf(stderr, "field: bad counts\n");
                return 2;
            }
            std::vector<float> src(4 * (size_t)m), rows(3 * (size_t)R);
            std::string w;
            for (float &u : src) {
                in >> w;
                u = std::strtof(w.c_str(), nullptr);
            }
            for (float &u : rows) {
                in >> w;
                u = std::strtof(w.c_str(), nullptr);
            }
            if (!in) {
                std::fprintf(stderr, "field: too few numbers\n");
                return 2;
            }
            const float e = std::strtof(eps.c_str(), nullptr), eps2 = e * e;
            if (eps2 > 0.f)
                field<false>(eps2, self != 0, src, rows);
            else
                field<true>(eps2, self != 0, src, rows);
        } else if (word == "plan" || word == "cover") {
            std::string mode;
            long long n = 0;
            in >> mode >> n;
            if (!in || n < 1 || n > kGravityMaxPoints || (mode != "own" && mode != "points") || (mode == "own" && n > NBODY_BATCH_MAX_BODIES)) {
                std::fprintf(stderr, "%s: bad arguments\n", word.c_str());
                return 2;
            }
            const GravityPlan p = mode == "own" ? gravity_plan_own((int)n) : gravity_plan_points(n);
            if (word == "plan") {
                if (mode == "own")
                    std::printf("%d %d %d %zu\n", p.rpl, p.threads, p.blocks, gravity_lds_bytes((int)n));
                else
                    std::printf("%d %d %d\n", p.rpl, p.threads, p.blocks);
            } else {
                std::vector<int> hits((size_t)n, 0);
                long long beyond = 0;
                for (int block = 0; block < p.blocks; ++block)
                    for (int q = 0; q < p.rpl; ++q)
                        for (int lane = 0; lane < p.threads; ++lane) {
                            const int r = gravity_row(block, p.rpl, p.threads, q, lane);
                            if (r >= 0 && r < n)
                                ++hits[(size_t)r];
                            else
                                ++beyond;
                        }
                std::printf("%d %d %lld\n", *std::min_element(hits.begin(), hits.end()), *std::max_element(hits.begin(), hits.end()), beyond);
            }
        } else if (word == "layout") {
            const BatchGravityRecord e = gravity_empty_record();
            std::printf("%zu %zu %zu %zu %lld %g %g %g %g %g\n", sizeof(BatchGravityRecord), offsetof(BatchGravityRecord, acceleration),
                        offsetof(BatchGravityRecord, reserved), offsetof(BatchGravityRecord, potential), (long long)kGravityMaxPoints,
                        e.acceleration[0], e.acceleration[1], e.acceleration[2], e.reserved, e.potential);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
