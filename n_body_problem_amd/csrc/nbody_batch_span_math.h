// nbody_batch_span_math.h -- the arithmetic of nbody_batch_span (include/nbody_batch_span.h) that needs no GPU: the three
// records and their empty values, the 64-bit key of an edge and its fields, the step of one row over one column, the decision
// of one component given its own minimum and the other's, one Compress pass, the compare-exchange of the sort, and the length
// and separation terms.  Plain C++17 without HIP, like nbody_batch_groups_math.h, whose r2 and image layout it reuses:
// batch_span_kernel (nbody_batch_analysis.hip) calls these per row with the image in LDS, and a stand-alone driver
// (tests/batch_span_driver.cpp) runs whole systems through the same functions in sequential loops on the CPU, where
// tests/test_batch_span_cpu.py compares them with Prim's algorithm.  Internal; the public surface is
// include/nbody_batch_span.h.
#pragma once

#include "nbody_batch_groups_math.h"

namespace nbody {

constexpr int kSpanMaxRounds = 13;  // NBODY_BATCH_SPAN_MAX_ROUNDS

// nbody_batch_span_system's layout (nbody_batch_analysis.hip asserts it): 40 bytes.
struct BatchSpanSystem {
    int edges, selected, rounds, reserved;
    double total_length, longest, mean_separation;
};

// nbody_batch_span_edge's layout (nbody_batch_analysis.hip asserts it): 16 bytes.
struct BatchSpanEdge {
    int i, j;
    float r2;
    int reserved;
};

// nbody_batch_span_body's layout (nbody_batch_analysis.hip asserts it): 8 bytes.
struct BatchSpanBody {
    int degree, nearest;
};

// Slots from `edges` on; unselected bodies, slots from the count on and lone selected bodies; a system without selected bodies.
NBODY_HD inline BatchSpanEdge span_empty_edge() { return BatchSpanEdge{-1, -1, 0.f, 0}; }
NBODY_HD inline BatchSpanBody span_empty_body() { return BatchSpanBody{0, -1}; }
NBODY_HD inline BatchSpanSystem span_empty_system() { return BatchSpanSystem{0, 0, 0, 0, 0.0, 0.0, 0.0}; }

// ---- The image: {x, y, z, component} per body, the layout of the groups image (kGroupsWords, groups_label_at).  A body that
// is no column -- unselected -- carries a component that no row has.
constexpr int kSpanNoComponent = -1;

// ---- The key ---------------------------------------------------------------------------------------------------------------
// K = (bits(r2) << 24) | (i << 12) | j for the edge between i < j.  Indices stay below 2^12 (4096 bodies at most), the bits of
// r2 fill 32, so K stays below 2^56 and the all-ones word is above every key: it stands for "no edge" and pads the sort.
typedef unsigned long long SpanKey;
constexpr int kSpanIndexBits = 12;
constexpr SpanKey kSpanNoKey = ~0ull;
constexpr unsigned kSpanNoBits = ~0u;  // above the bits of every r2 a row has seen: a row's best before its first column

NBODY_HD inline unsigned span_bits(float r2) { return __builtin_bit_cast(unsigned, r2); }
NBODY_HD inline float span_bits_r2(unsigned bits) { return __builtin_bit_cast(float, bits); }

NBODY_HD inline SpanKey span_key(unsigned r2_bits, int a, int b)
{
    const int i = a < b ? a : b, j = a < b ? b : a;
    return ((SpanKey)r2_bits << (2 * kSpanIndexBits)) | ((SpanKey)i << kSpanIndexBits) | (SpanKey)j;
}
NBODY_HD inline int span_key_i(SpanKey k) { return (int)(k >> kSpanIndexBits) & ((1 << kSpanIndexBits) - 1); }
NBODY_HD inline int span_key_j(SpanKey k) { return (int)k & ((1 << kSpanIndexBits) - 1); }
NBODY_HD inline unsigned span_key_bits(SpanKey k) { return (unsigned)(k >> (2 * kSpanIndexBits)); }

// ---- One column of one row ------------------------------------------------------------------------------------------------
// Row i of component ci keeps the lowest (bits(r2), j) among the columns of another component, under a strict <: the columns
// come in ascending j, and for a fixed row the lower j is the lower key at equal length whichever side of i it lies on, so no
// key is formed here.  The bits are compared as integers: r2 is never negative, so they order as the values do, and a NaN is
// just a long edge.  The row's own column has the row's component and passes.
struct SpanBest {
    unsigned bits = kSpanNoBits;
    int j = -1;
};

NBODY_HD inline void span_step(SpanBest &best, int ci, float xi, float yi, float zi, float xj, float yj, float zj, int cj, int j)
{
    const unsigned bits = span_bits(groups_r2(xi, yi, zi, xj, yj, zj));
    const bool better = cj != ci && cj != kSpanNoComponent && bits < best.bits;
    best.bits = better ? bits : best.bits;
    best.j = better ? j : best.j;
}

// The key of what row i found; kSpanNoKey where it found nothing (no other component has a body).
NBODY_HD inline SpanKey span_row_key(const SpanBest &best, int i) { return best.j < 0 ? kSpanNoKey : span_key(best.bits, i, best.j); }

// ---- One component -----------------------------------------------------------------------------------------------------------
// The component at the other end of c's minimum, from the components of the edge's two ends: one of them is c.
NBODY_HD inline int span_other(int c, int component_i, int component_j) { return component_i == c ? component_j : component_i; }

// Component c, whose minimum `mine` leads to component o with minimum `other`: whether c records the edge and hooks under o.
// Two components that chose the same edge would hook under each other; the higher one does.
NBODY_HD inline bool span_hooks(SpanKey mine, SpanKey other, int c, int o) { return mine != kSpanNoKey && (other != mine || c > o); }

// One pass of Compress for a row whose label is `label`: the pass of groups(), two steps up from the label.  A pass that moves
// nothing has found roots everywhere.  The caller writes the result after every row has read.
NBODY_HD inline int span_compress(const int *words, int label) { return groups_compress(words, label); }

// ---- The sort ----------------------------------------------------------------------------------------------------------------
// A bitonic network over `length` keys, a power of two: passes (k, j) for k = 2, 4, ... length and j = k / 2, k / 4, ... 1; pass
// (k, j) holds length / 2 compare-exchanges t, independent of each other, between slots lo and lo | j, ascending where
// (lo & k) == 0.
NBODY_HD inline int span_sort_length(int n)
{
    int p = 1;
    while (p < n)
        p <<= 1;
    return p;
}
NBODY_HD inline int span_sort_low(int t, int j) { return ((t & ~(j - 1)) << 1) | (t & (j - 1)); }
NBODY_HD inline void span_exchange(SpanKey *keys, int t, int k, int j)
{
    const int lo = span_sort_low(t, j), hi = lo | j;
    const SpanKey a = keys[lo], b = keys[hi];
    const bool swap = ((lo & k) == 0) == (a > b);  // ascending and out of order, or descending and in order (keys are distinct)
    keys[lo] = swap ? b : a;
    keys[hi] = swap ? a : b;
}

// ---- The terms ---------------------------------------------------------------------------------------------------------------
// The length of an edge: the correctly rounded fp64 square root of its fp32 r2.
NBODY_HD inline double span_length(float r2) { return __builtin_sqrt((double)r2); }

// A column's share of row i's separation sum: the correctly rounded fp32 square root, widened.  A column that does not count
// adds +0.0, which leaves the bits of a sum that is never -0.0 as they are.
NBODY_HD inline double span_separation(bool counts, float r2) { return counts ? (double)__builtin_sqrtf(r2) : 0.0; }

// sum over selected (selected - 1): one division; 0 below two bodies.
NBODY_HD inline double span_mean_separation(double sum, int selected)
{
    return selected < 2 ? 0.0 : sum / ((double)selected * (double)(selected - 1));
}

NBODY_HD inline BatchSpanEdge span_edge(SpanKey k)
{
    return k == kSpanNoKey ? span_empty_edge() : BatchSpanEdge{span_key_i(k), span_key_j(k), span_bits_r2(span_key_bits(k)), 0};
}

}  // namespace nbody
