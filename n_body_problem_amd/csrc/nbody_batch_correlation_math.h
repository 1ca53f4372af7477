// nbody_batch_correlation_math.h -- the arithmetic of nbody_batch_correlation (include/nbody_batch_correlation.h) that needs no
// GPU: the record, the limit and the edge counts the kernel is instantiated for, the squared edge, the examined-pair
// predicate, the step of one row over one column on an array of cumulative counters, and the differencing of the cumulative
// counters into below, counts[], above and unmeasured.  Plain C++17 without HIP, like nbody_batch_neighbours_math.h, and like
// it on top of nbody_batch_groups_math.h, whose r2 chain and `friends` predicate it reuses: batch_correlation_kernel
// (nbody_batch_analysis.hip) calls these with the columns in LDS, and a stand-alone driver
// (tests/batch_correlation_driver.cpp) runs whole systems through the same functions in sequential loops on the CPU, where
// tests/test_batch_correlation_cpu.py compares them with numpy.  Internal; the public surface is
// include/nbody_batch_correlation.h.
#pragma once

#include "nbody_batch_groups_math.h"

namespace nbody {

constexpr int kCorrelationMaxBins = 32;  // NBODY_BATCH_CORRELATION_MAX_BINS

// nbody_batch_correlation_system's layout (nbody_batch_analysis.hip asserts it): 48 bytes.
struct BatchCorrelationSystem {
    int rows, sources, both, bins;
    long long pairs, below, above, unmeasured;
};

// The kernel is instantiated for 8, 16 and 32 bins; a call runs the next one up, its edges padded with copies of the last.
// A padded cumulative counter equals the last real one and is not read.
NBODY_HD inline int correlation_padded_bins(int bins) { return bins <= 8 ? 8 : (bins <= 16 ? 16 : kCorrelationMaxBins); }

// An edge is a number that is not negative: false for NaN, for an infinity and for anything below zero.
NBODY_HD inline bool correlation_edge_valid(float e) { return e >= 0.f && e < __builtin_inff(); }

// e2 of one edge: one fp32 product, groups()' and neighbours()' own.  A product that overflows becomes the largest finite
// value: every measured r2 is within it, and an unmeasured one is within nothing.
NBODY_HD inline float correlation_edge2(float e)
{
    const float e2 = e * e;
    return e2 < __builtin_inff() ? e2 : __FLT_MAX__;
}

// ---- One column of one row -------------------------------------------------------------------------------------------------
// The ordered pair (i, j) is examined iff i is a row, j is a source and they are two bodies.
NBODY_HD inline bool correlation_distinct(int i, int j) { return j != i; }
NBODY_HD inline bool correlation_examined(bool row, bool source, int i, int j) { return row && source && correlation_distinct(i, j); }

// Measured: r2 < +inf, false for +inf and for NaN, stated as "within the largest finite value" -- the same set of numbers, and
// the comparison of the edges: an ordered <= against a finite value.
NBODY_HD inline bool correlation_measured(float r2) { return groups_friends(r2, __FLT_MAX__); }

// The cumulative counters of one system, or of a part of its pairs: within[t], the examined pairs within edge t, for the
// EDGES = bins + 1 edges, and the measured ones.  Integers, so parts add up in any order.
template <int EDGES, class Word = unsigned int>
struct CorrelationCounters {
    Word within[EDGES];
    Word measured;
};

template <int EDGES, class Word>
NBODY_HD inline void correlation_clear(CorrelationCounters<EDGES, Word> &c)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t < EDGES; ++t)
        c.within[t] = 0;
    c.measured = 0;
}

// Row i at {xi, yi, zi} meets column j at {xj, yj, zj}: within[t] += examined && friends(r2, e2[t]), and the measured counter.
// e2 holds EDGES squared edges, ascending.  t never leaves the unrolled loop, so the counters stay where they are.
// add(word, examined, flag) is how a counter takes a pair: `word += examined && flag` for the counter of one row (a sequential
// loop, or a lane of the device); a counter that a wave shares takes the number of its lanes whose flag is set, and has
// add.seen(examined, r2) hide the r2 of a pair that is not examined behind a NaN, which is within nothing and not measured.
template <int EDGES, class Word, class Add>
NBODY_HD inline void correlation_step(CorrelationCounters<EDGES, Word> &c, bool examined, float xi, float yi, float zi, float xj,
                                      float yj, float zj, const float *e2, Add add)
{
    const float r2 = add.seen(examined, groups_r2(xi, yi, zi, xj, yj, zj));
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t < EDGES; ++t)
        add(c.within[t], examined, groups_friends(r2, e2[t]));
    add(c.measured, examined, correlation_measured(r2));
}

// The counter of one row takes a pair.
struct CorrelationAddOne {
    NBODY_HD float seen(bool, float r2) const { return r2; }
    template <class Word>
    NBODY_HD void operator()(Word &word, bool examined, bool flag) const { word += examined && flag ? 1 : 0; }
};

// ---- Differencing ----------------------------------------------------------------------------------------------------------
// The cumulative counters ascend with t (e2 does), and within[t] <= measured <= pairs (every e2 is finite).
NBODY_HD inline long long correlation_pairs(int rows, int sources, int both) { return (long long)rows * (long long)sources - (long long)both; }
NBODY_HD inline long long correlation_below(unsigned int within0) { return (long long)within0; }
NBODY_HD inline unsigned int correlation_bin(unsigned int within_lower, unsigned int within_upper) { return within_upper - within_lower; }
NBODY_HD inline long long correlation_above(unsigned int measured, unsigned int within_last) { return (long long)measured - (long long)within_last; }
NBODY_HD inline long long correlation_unmeasured(long long pairs, unsigned int measured) { return pairs - (long long)measured; }

// The record of one system from its totals: within holds bins + 1 cumulative counts.
NBODY_HD inline BatchCorrelationSystem correlation_record(int rows, int sources, int both, int bins, const unsigned int *within,
                                                          unsigned int measured)
{
    const long long pairs = correlation_pairs(rows, sources, both);
    return BatchCorrelationSystem{rows,  sources, both, bins, pairs, correlation_below(within[0]), correlation_above(measured, within[bins]),
                                  correlation_unmeasured(pairs, measured)};
}

}  // namespace nbody
