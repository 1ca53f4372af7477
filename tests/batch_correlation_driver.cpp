// Runs whole systems through the arithmetic of csrc/nbody_batch_correlation_math.h (include/nbody_batch_correlation.h) on the CPU
// for tests/test_batch_correlation_cpu.py: the functions batch_correlation_kernel calls, here in sequential loops.
// Commands on stdin:
//   system N BINS -> then one line of BINS + 1 edges, then N lines "x y z row source" (numbers read as double, narrowed to
//                    float).  Prints  rows sources both bins pairs below above unmeasured  and then one line of BINS counts.
//                    Like the kernel it runs the instantiation of correlation_padded_bins(BINS), its edges padded with copies
//                    of the last.
//   layout        -> size of the record and the offsets of its fields
//   limits        -> the limit, the padded bins of 1, 8, 9, 16, 17 and 32, and the bits of correlation_edge2 of the largest
//                    finite float
#include "nbody_batch_correlation_math.h"

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

static float read_float(std::istream &in)
{
    std::string w;
    in >> w;
    return (float)std::strtod(w.c_str(), nullptr);
}

template <int BINS>
static void count_system(int n, int bins, const std::vector<float> &edges, const std::vector<float> &x, const std::vector<int> &row,
                         const std::vector<int> &source)
{
    constexpr int EDGES = BINS + 1;
    float e2[EDGES];
    for (int t = 0; t < EDGES; ++t)
        e2[t] = correlation_edge2(edges[(size_t)(t < bins + 1 ? t : bins)]);  // one fp32 product; copies of the last edge behind it
    int rows = 0, sources = 0, both = 0;
    for (int i = 0; i < n; ++i) {
        rows += row[i];
        sources += source[i];
        both += row[i] && source[i] ? 1 : 0;
    }
    CorrelationCounters<EDGES> c;
    correlation_clear(c);
    for (int i = 0; i < n; ++i) {  // every row over the columns in ascending j; a column that is no source is skipped
        for (int j = 0; j < n; ++j) {
            if (!source[j])
                continue;
            correlation_step(c, correlation_examined(row[i] != 0, true, i, j), x[3 * i], x[3 * i + 1], x[3 * i + 2], x[3 * j],
                             x[3 * j + 1], x[3 * j + 2], e2, CorrelationAddOne{});
        }
    }
    const BatchCorrelationSystem s = correlation_record(rows, sources, both, bins, c.within, c.measured);
    std::printf("%d %d %d %d %lld %lld %lld %lld\n", s.rows, s.sources, s.both, s.bins, s.pairs, s.below, s.above, s.unmeasured);
    for (int t = 0; t < bins; ++t)
        std::printf("%s%u", t ? " " : "", correlation_bin(c.within[t], c.within[t + 1]));
    std::printf("\n");
}

static int run_system(std::istringstream &in)
{
    int n = 0, bins = 0;
    in >> n >> bins;
    if (n < 0 || bins < 1 || bins > kCorrelationMaxBins) {
        std::fprintf(stderr, "system: bad N or BINS\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream edge_line(line);
    std::vector<float> edges((size_t)bins + 1);
    for (float &e : edges)
        e = read_float(edge_line);
    std::vector<float> x((size_t)3 * (size_t)(n > 0 ? n : 1));
    std::vector<int> row((size_t)(n > 0 ? n : 1)), source((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream body(line);
        for (int c = 0; c < 3; ++c)
            x[3 * i + c] = read_float(body);
        int r = 1, s = 1;
        body >> r >> s;
        row[i] = r ? 1 : 0;
        source[i] = s ? 1 : 0;
    }
    switch (correlation_padded_bins(bins)) {
    case 8: count_system<8>(n, bins, edges, x, row, source); break;
    case 16: count_system<16>(n, bins, edges, x, row, source); break;
    default: count_system<kCorrelationMaxBins>(n, bins, edges, x, row, source); break;
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
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchCorrelationSystem), offsetof(BatchCorrelationSystem, rows),
                        offsetof(BatchCorrelationSystem, sources), offsetof(BatchCorrelationSystem, both),
                        offsetof(BatchCorrelationSystem, bins), offsetof(BatchCorrelationSystem, pairs),
                        offsetof(BatchCorrelationSystem, below), offsetof(BatchCorrelationSystem, above),
                        offsetof(BatchCorrelationSystem, unmeasured));
        } else if (word == "limits") {
            std::printf("%d %d %d %d %d %d %d %u %d %d %d\n", kCorrelationMaxBins, correlation_padded_bins(1), correlation_padded_bins(8),
                        correlation_padded_bins(9), correlation_padded_bins(16), correlation_padded_bins(17),
                        correlation_padded_bins(32), float_bits(correlation_edge2(__FLT_MAX__)), (int)correlation_edge_valid(-0.5f),
                        (int)correlation_edge_valid(__builtin_nanf("")), (int)correlation_edge_valid(__builtin_inff()));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
