// nbody_batch_neighbours_math.h -- the arithmetic of nbody_batch_neighbours (include/nbody_batch_neighbours.h) that needs no
// GPU: the two records and the empty values, the limit, the candidate predicate, the step of one row over one column (the
// sorted list of the eight nearest candidates with their indices, and the count within the radius), the reading of a list,
// the `mutual` decision and the two means.  Plain C++17 without HIP, like nbody_batch_span_math.h, and like it on top of
// nbody_batch_groups_math.h, whose r2 chain and `friends` predicate it reuses: batch_neighbours_kernel
// (nbody_batch_analysis.hip) calls these per row with the columns in LDS, and a stand-alone driver
// (tests/batch_neighbours_driver.cpp) runs whole systems through the same functions in sequential loops on the CPU, where
// tests/test_batch_neighbours_cpu.py compares them with a stable sort.  Internal; the public surface is
// include/nbody_batch_neighbours.h.
#pragma once

#include "nbody_batch_groups_math.h"

namespace nbody {

constexpr int kNeighboursMax = 8;  // NBODY_BATCH_NEIGHBOURS_MAX

// nbody_batch_neighbour_system's layout (nbody_batch_analysis.hip asserts it): 40 bytes.
struct BatchNeighbourSystem {
    int bodies, sources, listed, complete, mutual, reserved;
    double mean_nearest, mean_kth;
};

// nbody_batch_neighbour_body's layout (nbody_batch_analysis.hip asserts it): 8 bytes.
struct BatchNeighbourBody {
    int found, within;
};

// Slots of a list from `found` on, and every slot of a row from the count on; such a row's record.
constexpr int kNeighboursNoIndex = -1;
NBODY_HD inline float neighbours_no_r2() { return __builtin_inff(); }
NBODY_HD inline BatchNeighbourBody neighbours_empty_body() { return BatchNeighbourBody{0, 0}; }

// The squared radius of a call without radii: below every r2 (which is never negative), so that nothing is within it.
constexpr float kNeighboursNoRadius2 = -1.f;

// ---- One column of one row -------------------------------------------------------------------------------------------------
// Column j is a candidate of row i iff it is another body, a source, and at a distance that is a number: r2 < +inf is false
// for +inf and for NaN.  A coincident body (r2 == 0) is a candidate.
NBODY_HD inline bool neighbours_candidate(int i, int j, bool source, float r2) { return j != i && source && r2 < neighbours_no_r2(); }

// The row's state while the columns pass: the eight nearest candidates so far in ascending (r2, j), +inf and -1 where there
// is none yet, and the candidates within the radius.
struct NeighbourList {
    float r2[kNeighboursMax];
    int index[kNeighboursMax];
    int within;
};

NBODY_HD inline void neighbours_clear(NeighbourList &l)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t < kNeighboursMax; ++t) {
        l.r2[t] = neighbours_no_r2();
        l.index[t] = kNeighboursNoIndex;
    }
    l.within = 0;
}

// (c, j) goes in front of the first slot it is strictly below, and the slots from there on move up one; the last falls out.
// The columns come in ascending j, so an equal r2 already in the list has the lower index and stays in front: the order is
// (r2, j) with no key.  below[t] = c < r2[t] is false up to the place and true from it on (the list is ascending), so slot t
// takes its lower neighbour where below[t - 1], c where below[t] alone, and stays otherwise.  Walked from the top down, each
// slot reads its neighbour before that one changes.  Eight compares and two selects per word: no branch and no index, so
// the list stays in registers.  c = +inf (what is no candidate) is below nothing and leaves the list as it is; so does NaN.
NBODY_HD inline void neighbours_insert(NeighbourList &l, float c, int j)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = kNeighboursMax - 1; t > 0; --t) {
        const bool moves = c < l.r2[t - 1], here = c < l.r2[t];
        l.r2[t] = moves ? l.r2[t - 1] : (here ? c : l.r2[t]);
        l.index[t] = moves ? l.index[t - 1] : (here ? j : l.index[t]);
    }
    const bool first = c < l.r2[0];
    l.r2[0] = first ? c : l.r2[0];
    l.index[0] = first ? j : l.index[0];
}

// Row i at {xi, yi, zi} meets column j at {xj, yj, zj}; b2 is the squared radius (kNeighboursNoRadius2 without one).  The
// column is counted where it is within the radius, and what neighbours_insert is to take comes back: r2, or +inf for what is
// no candidate -- one select, so that it needs no branch.
NBODY_HD inline float neighbours_measure(NeighbourList &l, int i, float xi, float yi, float zi, float xj, float yj, float zj,
                                         bool source, int j, float b2)
{
    const float r2 = groups_r2(xi, yi, zi, xj, yj, zj);
    const bool candidate = neighbours_candidate(i, j, source, r2);
    l.within += candidate && groups_friends(r2, b2) ? 1 : 0;
    return candidate ? r2 : neighbours_no_r2();
}

// Whether neighbours_insert would change the list: c is below its last slot.  Where it is not, the insertion may be skipped.
NBODY_HD inline bool neighbours_wanted(const NeighbourList &l, float c) { return c < l.r2[kNeighboursMax - 1]; }

// One column of one row, whole: the kernel runs the three parts with a vote of the wave between the second and the third.
NBODY_HD inline void neighbours_step(NeighbourList &l, int i, float xi, float yi, float zi, float xj, float yj, float zj, bool source,
                                     int j, float b2)
{
    const float c = neighbours_measure(l, i, xi, yi, zi, xj, yj, zj, source, j, b2);
    if (neighbours_wanted(l, c))
        neighbours_insert(l, c, j);
}

// ---- Reading a list --------------------------------------------------------------------------------------------------------
// found = min(k, candidates): the slots below k that hold one.  Counted, not indexed.
NBODY_HD inline int neighbours_found(const NeighbourList &l, int k)
{
    int found = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t < kNeighboursMax; ++t)
        found += t < k && l.index[t] != kNeighboursNoIndex ? 1 : 0;
    return found;
}

// r2 of slot k - 1, 1 <= k <= 8: the list is ascending, so it is the largest of the first k, taken slot by slot as in
// structure_kth (an index into the list would send it to scratch memory).  +inf where the row is not complete.
NBODY_HD inline float neighbours_kth(const NeighbourList &l, int k)
{
    float r = l.r2[0];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 1; t < kNeighboursMax; ++t)
        r = t < k ? (l.r2[t] > r ? l.r2[t] : r) : r;
    return r;
}

// ---- The system record -----------------------------------------------------------------------------------------------------
// Row i, whose nearest candidate is nearest[i] (-1 without one), is mutual iff it has one and that one's nearest is i.  A j
// whose nearest is i >= 0 has found(j) >= 1.
NBODY_HD inline bool neighbours_mutual(const int *nearest, int i)
{
    const int j = nearest[i];
    return j != kNeighboursNoIndex && nearest[j] == i;
}

// A row's term of a mean: the correctly rounded fp64 square root of its fp32 r2 where the row counts, +0.0 where it does not,
// which leaves the bits of a sum that is never -0.0 as they are.
NBODY_HD inline double neighbours_term(bool counts, float r2) { return counts ? __builtin_sqrt((double)r2) : 0.0; }

// sum over rows: one division; 0 without rows.
NBODY_HD inline double neighbours_mean(double sum, int rows) { return rows > 0 ? sum / (double)rows : 0.0; }

}  // namespace nbody
