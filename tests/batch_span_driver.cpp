// Runs whole systems through the arithmetic of csrc/nbody_batch_span_math.h (include/nbody_batch_span.h) on the CPU for
// tests/test_batch_span_cpu.py: the functions batch_span_kernel calls per row, here in sequential loops with every read of a
// step before its writes.  Commands on stdin:
//   system N SEPARATIONS -> then N lines "x y z selected" (coordinates read as double, narrowed to float).  Prints
//                             edges selected rounds reserved total_length longest mean_separation (%.17g)
//                             per edge slot below `edges`: "i j bits(r2)"
//                             the N degrees
//                             the N nearest
//   sort N               -> then one line of N keys (decimal).  Prints them as the network leaves them, padded to a power of two
//                           with all-ones keys and sorted: the first N slots.
//   layout               -> sizes of the three records and the offsets of their fields
//   empty                -> the empty edge, body and system records, and the constants
#include "nbody_batch_span_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static float word_as_float(int w)
{
    float f;
    std::memcpy(&f, &w, sizeof f);
    return f;
}

static int float_as_word(float f)
{
    int w;
    std::memcpy(&w, &f, sizeof w);
    return w;
}

// The network of batch_span_kernel on `keys`, whose size is a power of two: every pass's exchanges in any order.
static void sort_keys(std::vector<SpanKey> &keys)
{
    const int length = (int)keys.size();
    for (int k = 2; k <= length; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1)
            for (int t = length / 2 - 1; t >= 0; --t)  // descending: the exchanges of a pass do not depend on each other
                span_exchange(keys.data(), t, k, j);
}

static void run_system(std::istringstream &in)
{
    int n = 0, separations = 0;
    in >> n >> separations;
    std::vector<int> words((size_t)kGroupsWords * (size_t)(n > 0 ? n : 1));  // the image {x, y, z, component}
    int selected = 0;
    for (int i = 0; i < n; ++i) {
        std::string line, w[3];
        int sel = 1;
        std::getline(std::cin, line);
        std::istringstream row(line);
        row >> w[0] >> w[1] >> w[2] >> sel;
        for (int c = 0; c < 3; ++c)
            words[kGroupsWords * i + c] = float_as_word((float)std::strtod(w[c].c_str(), nullptr));
        words[groups_label_at(i)] = sel ? i : kSpanNoComponent;
        selected += sel ? 1 : 0;
    }
    const auto X = [&](int i, int c) { return word_as_float(words[kGroupsWords * i + c]); };
    const auto L = [&](int i) { return words[groups_label_at(i)]; };
    // The separations: rows in ascending i, columns in ascending j.
    double separation = 0.0;
    if (separations && selected > 1) {
        for (int i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int j = 0; j < n; ++j)
                sum += span_separation(L(j) != kSpanNoComponent && j != i, groups_r2(X(i, 0), X(i, 1), X(i, 2), X(j, 0), X(j, 1), X(j, 2)));
            separation += L(i) != kSpanNoComponent ? sum : 0.0;
        }
    }
    int left = selected, rounds = 0;
    std::vector<SpanKey> key(n > 0 ? n : 1), rec(n > 0 ? n : 1, kSpanNoKey);
    std::vector<int> nearest(n, -1), under(n), next(n);
    while (left > 1 && rounds < kSpanMaxRounds) {
        ++rounds;
        for (int i = 0; i < n; ++i)
            key[i] = kSpanNoKey;
        for (int i = 0; i < n; ++i) {  // every row, then its component's minimum: reads of the image alone
            if (L(i) == kSpanNoComponent)
                continue;
            SpanBest best;
            for (int j = 0; j < n; ++j)
                span_step(best, L(i), X(i, 0), X(i, 1), X(i, 2), X(j, 0), X(j, 1), X(j, 2), L(j), j);
            if (rounds == 1)
                nearest[i] = best.j;
            const SpanKey k = span_row_key(best, i);
            if (k < key[L(i)])
                key[L(i)] = k;
        }
        for (int r = 0; r < n; ++r) {  // the roots decide: reads alone
            under[r] = kSpanNoComponent;
            if (L(r) != r || key[r] == kSpanNoKey)
                continue;
            const SpanKey k = key[r];
            const int o = span_other(r, L(span_key_i(k)), L(span_key_j(k)));
            if (span_hooks(k, key[o], r, o)) {
                under[r] = o;
                rec[r] = k;
            }
        }
        for (int r = 0; r < n; ++r) {  // Hook
            if (under[r] != kSpanNoComponent) {
                words[groups_label_at(r)] = under[r];
                --left;
            }
        }
        for (;;) {  // Compress: every row reads, then every row writes
            bool moved = false;
            for (int i = 0; i < n; ++i) {
                next[i] = L(i);
                if (L(i) == kSpanNoComponent)
                    continue;
                next[i] = span_compress(words.data(), L(i));
                moved = moved || next[i] != L(i);
            }
            for (int i = 0; i < n; ++i)
                words[groups_label_at(i)] = next[i];
            if (!moved)
                break;
        }
    }
    const int recorded = selected - left;
    std::vector<SpanKey> sorted((size_t)span_sort_length(n), kSpanNoKey);
    for (int r = 0; r < n; ++r)
        sorted[r] = rec[r];
    sort_keys(sorted);
    std::vector<int> degree(n, 0);
    double total = 0.0, longest = 0.0;
    for (int e = 0; e < recorded; ++e) {
        const BatchSpanEdge edge = span_edge(sorted[e]);
        ++degree[edge.i];
        ++degree[edge.j];
        longest = span_length(edge.r2);
        total += longest;
    }
    std::printf("%d %d %d %d %.17g %.17g %.17g\n", recorded, selected, rounds, 0, total, longest,
                span_mean_separation(separation, selected));
    for (int e = 0; e < recorded; ++e) {
        const BatchSpanEdge edge = span_edge(sorted[e]);
        std::printf("%d %d %u\n", edge.i, edge.j, span_bits(edge.r2));
    }
    for (int i = 0; i < n; ++i)
        std::printf("%d ", degree[i]);
    std::printf("\n");
    for (int i = 0; i < n; ++i)
        std::printf("%d ", L(i) != kSpanNoComponent ? nearest[i] : span_empty_body().nearest);
    std::printf("\n");
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
        } else if (word == "sort") {
            int n = 0;
            in >> n;
            std::getline(std::cin, line);
            std::istringstream row(line);
            std::vector<SpanKey> keys((size_t)span_sort_length(n), kSpanNoKey);
            for (int i = 0; i < n; ++i)
                row >> keys[i];
            sort_keys(keys);
            for (int i = 0; i < n; ++i)
                std::printf("%llu ", keys[i]);
            std::printf("\n");
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu  %zu %zu %zu\n", sizeof(BatchSpanSystem),
                        offsetof(BatchSpanSystem, edges), offsetof(BatchSpanSystem, selected), offsetof(BatchSpanSystem, rounds),
                        offsetof(BatchSpanSystem, reserved), offsetof(BatchSpanSystem, total_length),
                        offsetof(BatchSpanSystem, longest), offsetof(BatchSpanSystem, mean_separation), sizeof(BatchSpanEdge),
                        offsetof(BatchSpanEdge, i), offsetof(BatchSpanEdge, j), offsetof(BatchSpanEdge, r2),
                        offsetof(BatchSpanEdge, reserved), sizeof(BatchSpanBody), offsetof(BatchSpanBody, degree),
                        offsetof(BatchSpanBody, nearest));
        } else if (word == "empty") {
            const BatchSpanEdge e = span_empty_edge();
            const BatchSpanBody b = span_empty_body();
            const BatchSpanSystem s = span_empty_system();
            std::printf("%d %d %g %d  %d %d  %d %d %d %d %g  %d %d %llu\n", e.i, e.j, e.r2, e.reserved, b.degree, b.nearest, s.edges,
                        s.selected, s.rounds, s.reserved, s.total_length + s.longest + s.mean_separation, kSpanMaxRounds,
                        kSpanIndexBits, kSpanNoKey);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
