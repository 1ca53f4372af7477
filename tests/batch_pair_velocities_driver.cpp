// Runs whole systems through the arithmetic of csrc/nbody_batch_pair_velocities_math.h (include/nbody_batch_pair_velocities.h)
// on the CPU for tests/test_batch_pair_velocities_cpu.py: the functions batch_pair_velocities_kernel calls, here lane by lane in
// sequential loops, for any workgroup shape and any number of bins per pass.
// Commands on stdin:
//   system N BINS WEIGHT T RPL G -> then one line of BINS + 1 edges, then N lines "x y z m vx vy vz row source", every fp32
//                    word as its 32 bits in decimal.  T threads and RPL rows per lane (N <= T * RPL), G in 1, 2, 4, 8, 32
//                    bins per pass.  Prints  rows sources both bins weight reserved pairs below above unmeasured  and then
//                    one line per bin: count approaching receding and the nine sums, every fp64 word as its 64 bits in
//                    decimal.
//   layout        -> sizes and offsets of the two records
//   limits        -> the limit, the block, the terms, the passes and padded edges of 5 bins at 2 per pass
#include "nbody_batch_pair_velocities_math.h"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static float float_of(unsigned int bits)
{
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
}

static unsigned long long bits_of(double d)
{
    unsigned long long w;
    std::memcpy(&w, &d, sizeof w);
    return w;
}

template <int G>
static void run(int n, int bins, int weight, int T, int rpl, const std::vector<float> &edges, const std::vector<PairVelocityPoint> &body,
                const std::vector<int> &row, const std::vector<int> &source)
{
    // the host's part: the squared edges laid out for the passes, copies of the last edge behind it
    const int padded = pair_velocities_padded_edges(bins, G), passes = pair_velocities_passes(bins, G);
    std::vector<float> e2((size_t)padded);
    for (int t = 0; t < padded; ++t)
        e2[(size_t)t] = correlation_edge2(edges[(size_t)(t <= bins ? t : bins)]);
    // the image's flags
    std::vector<int> flags((size_t)(n > 0 ? n : 1));
    int rows = 0, sources = 0, both = 0;
    for (int i = 0; i < n; ++i) {
        flags[(size_t)i] = pair_velocities_flags(row[(size_t)i] != 0, source[(size_t)i] != 0, pair_velocities_body_measured(body[(size_t)i]));
        rows += row[(size_t)i];
        sources += source[(size_t)i];
        both += row[(size_t)i] && source[(size_t)i] ? 1 : 0;
    }
    const int blocks = pair_velocities_blocks(n), waves = T / kPairVelocitiesBlock;
    constexpr int SUMS = G * kPairVelocitiesTerms;
    std::vector<BatchPairVelocitiesBin> out((size_t)bins);
    PairVelocitySystemCounts seen;
    pair_velocities_clear(seen);
    const float first = e2[0], last = e2[(size_t)bins];
    std::vector<double> partials((size_t)waves * SUMS);  // of one round: [wave][G][9]
    std::vector<PairVelocityCounts<G>> c((size_t)T);     // the integers of a lane run on over its rows
    for (int pass = 0; pass < passes; ++pass) {
        const float *mine2 = e2.data() + (size_t)pass * G;
        for (PairVelocityCounts<G> &lane : c)
            pair_velocities_clear(lane);
        double total[SUMS];
        for (double &t : total)
            t = 0.0;
        for (int q0 = 0; q0 < n; q0 += T) {  // a round
            partials.assign(partials.size(), -1.0);  // a partial never written would show
            for (int wave = 0; wave < waves; ++wave) {
                const int r0 = q0 + wave * kPairVelocitiesBlock;
                if (r0 >= n)
                    continue;
                static double sums[G][kPairVelocitiesTerms][kPairVelocitiesBlock];
                for (int lane = 0; lane < kPairVelocitiesBlock; ++lane) {
                    const int r = r0 + lane;
                    PairVelocityPoint mine{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    int f = 0;
                    if (r < n) {
                        mine = body[(size_t)r];
                        f = flags[(size_t)r];
                    }
                    const bool is_row = (f & kPairVelocitiesRow) != 0, row_measured = (f & kPairVelocitiesMeasured) != 0;
                    PairVelocitySums<G> a;
                    pair_velocities_clear(a);
                    for (int j = 0; j < n; ++j) {
                        const int fj = flags[(size_t)j];
                        if ((fj & kPairVelocitiesSource) == 0)
                            continue;
                        const float r2 = pair_velocities_step<G>(a, c[(size_t)(wave * kPairVelocitiesBlock + lane)],
                                                                 correlation_examined(is_row, true, r, j),
                                                                 row_measured && (fj & kPairVelocitiesMeasured) != 0, mine, body[(size_t)j],
                                                                 mine2, weight);
                        if (pass == 0)
                            pair_velocities_system_step(seen, r2, first, last);
                    }
                    for (int g = 0; g < G; ++g)
                        for (int k = 0; k < kPairVelocitiesTerms; ++k)
                            sums[g][k][lane] = a.w[g][k];
                }
                for (int g = 0; g < G; ++g)
                    for (int k = 0; k < kPairVelocitiesTerms; ++k)
                        partials[(size_t)wave * SUMS + g * kPairVelocitiesTerms + k] = pair_velocities_tree(sums[g][k]);
            }
            const int left = blocks - q0 / kPairVelocitiesBlock;
            for (int sum = 0; sum < SUMS; ++sum)
                total[sum] = pair_velocities_total(total[sum], partials.data() + sum, SUMS, left < waves ? left : waves);
        }
        unsigned int totals[kPairVelocitiesIntegers * G];
        for (unsigned int &t : totals)
            t = 0;
        for (const PairVelocityCounts<G> &lane : c)
            for (int g = 0; g < G; ++g) {
                totals[g] += lane.count[g];
                totals[G + g] += lane.approaching[g];
                totals[2 * G + g] += lane.receding[g];
            }
        for (int g = 0; g < G; ++g) {
            const int t = pass * G + g;
            if (t >= bins)
                continue;
            for (int word = 0; word < kPairVelocitiesIntegers; ++word)
                pair_velocities_store(&out[(size_t)t], word, totals[word * G + g]);
            for (int k = 0; k < kPairVelocitiesTerms; ++k)
                pair_velocities_store(&out[(size_t)t], kPairVelocitiesIntegers + k, total[g * kPairVelocitiesTerms + k]);
        }
    }
    const BatchPairVelocitiesSystem s = pair_velocities_system(rows, sources, both, bins, weight, seen);
    std::printf("%d %d %d %d %d %d %lld %lld %lld %lld\n", s.rows, s.sources, s.both, s.bins, s.weight, s.reserved, s.pairs, s.below, s.above,
                s.unmeasured);
    for (int t = 0; t < bins; ++t) {
        const BatchPairVelocitiesBin &b = out[(size_t)t];
        std::printf("%lld %lld %lld %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", b.count, b.approaching, b.receding, bits_of(b.weight),
                    bits_of(b.r1), bits_of(b.r2), bits_of(b.rv), bits_of(b.vr1), bits_of(b.vr2), bits_of(b.vt2), bits_of(b.v1), bits_of(b.v2));
    }
}

static int run_system(std::istringstream &in)
{
    int n = 0, bins = 0, weight = 0, T = 0, rpl = 0, g = 0;
    in >> n >> bins >> weight >> T >> rpl >> g;
    if (n < 0 || bins < 1 || bins > kPairVelocitiesMaxBins || T < kPairVelocitiesBlock || T % kPairVelocitiesBlock || rpl < 1 || n > T * rpl) {
        std::fprintf(stderr, "system: bad N, BINS, T or RPL\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream edge_line(line);
    std::vector<float> edges((size_t)bins + 1);
    for (float &e : edges) {
        unsigned int w = 0;
        edge_line >> w;
        e = float_of(w);
    }
    std::vector<PairVelocityPoint> body((size_t)(n > 0 ? n : 1));
    std::vector<int> row((size_t)(n > 0 ? n : 1)), source((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        unsigned int w[7] = {0, 0, 0, 0, 0, 0, 0};
        for (unsigned int &x : w)
            words >> x;
        body[(size_t)i] = PairVelocityPoint{float_of(w[0]), float_of(w[1]), float_of(w[2]), float_of(w[3]), float_of(w[4]), float_of(w[5]),
                                            float_of(w[6])};
        int r = 1, s = 1;
        words >> r >> s;
        row[(size_t)i] = r ? 1 : 0;
        source[(size_t)i] = s ? 1 : 0;
    }
    switch (g) {
    case 1: run<1>(n, bins, weight, T, rpl, edges, body, row, source); break;
    case 2: run<2>(n, bins, weight, T, rpl, edges, body, row, source); break;
    case 4: run<4>(n, bins, weight, T, rpl, edges, body, row, source); break;
    case 8: run<8>(n, bins, weight, T, rpl, edges, body, row, source); break;
    case 32: run<32>(n, bins, weight, T, rpl, edges, body, row, source); break;
    default: std::fprintf(stderr, "system: G must be 1, 2, 4, 8 or 32\n"); return 2;
    }
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
        if (word == "system") {
            if (const int status = run_system(in))
                return status;
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchPairVelocitiesBin), offsetof(BatchPairVelocitiesBin, count),
                        offsetof(BatchPairVelocitiesBin, approaching), offsetof(BatchPairVelocitiesBin, receding),
                        offsetof(BatchPairVelocitiesBin, weight), offsetof(BatchPairVelocitiesBin, r1), offsetof(BatchPairVelocitiesBin, r2),
                        offsetof(BatchPairVelocitiesBin, rv), offsetof(BatchPairVelocitiesBin, vr1), offsetof(BatchPairVelocitiesBin, vr2),
                        offsetof(BatchPairVelocitiesBin, vt2), offsetof(BatchPairVelocitiesBin, v1), offsetof(BatchPairVelocitiesBin, v2));
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchPairVelocitiesSystem), offsetof(BatchPairVelocitiesSystem, rows),
                        offsetof(BatchPairVelocitiesSystem, sources), offsetof(BatchPairVelocitiesSystem, both),
                        offsetof(BatchPairVelocitiesSystem, bins), offsetof(BatchPairVelocitiesSystem, weight),
                        offsetof(BatchPairVelocitiesSystem, reserved), offsetof(BatchPairVelocitiesSystem, pairs),
                        offsetof(BatchPairVelocitiesSystem, below), offsetof(BatchPairVelocitiesSystem, above),
                        offsetof(BatchPairVelocitiesSystem, unmeasured));
        } else if (word == "limits") {
            std::printf("%d %d %d %d %d %d\n", kPairVelocitiesMaxBins, kPairVelocitiesBlock, kPairVelocitiesTerms, kPairVelocitiesPassBins,
                        pair_velocities_passes(5, 2), pair_velocities_padded_edges(5, 2));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
