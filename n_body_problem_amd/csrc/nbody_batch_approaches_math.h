// nbody_batch_approaches_math.h -- the arithmetic of nbody_batch_approaches (include/nbody_batch_approaches.h) that needs no
// GPU: the three records, the rv chain beside the r2 and v2 chains (both groups_r2), the measured predicate, the separation at
// the horizon, the phase of a pair, the step of one row over one column (degree, upper, now and the phase counts of the pairs
// above the row), the fill step with its capacity clamp, the pad entry and the body and system records.  Plain C++17 without
// HIP, on top of nbody_batch_contacts_math.h, whose thresholds, examined and above predicates, units, placement and stored it
// reuses as they are.  batch_approaches_kernel (nbody_batch_analysis.hip) calls these with the columns in LDS, and a
// stand-alone driver (tests/batch_approaches_driver.cpp) runs whole systems through the same functions, lane by lane for any
// workgroup shape, on the CPU, where tests/test_batch_approaches_cpu.py compares them with numpy.  Internal; the public
// surface is include/nbody_batch_approaches.h.
#pragma once

#include "nbody_batch_contacts_math.h"

namespace nbody {

constexpr long long kApproachesMaxEntries = 1ll << 27;  // n_systems x capacity, at most: the bytes of kContactsMaxEntries
constexpr int kApproachNone = -1, kApproachNow = 0, kApproachPassage = 1, kApproachEnd = 2;
constexpr int kApproachPhases = 3;

// nbody_batch_approach_system's layout (nbody_batch_analysis.hip asserts it): 48 bytes.
struct BatchApproachSystem {
    int bodies, approaching, max_degree, reserved;
    long long pairs, stored;
    int now, passing, ending, reserved2;
};

// nbody_batch_approach_body's layout (nbody_batch_analysis.hip asserts it): 16 bytes.
struct BatchApproachBody {
    int degree, upper, first, now;
};

// nbody_batch_approach's layout (nbody_batch_analysis.hip asserts it): 24 bytes.
struct BatchApproach {
    int i, j;
    float r2, rv, v2;
    int phase;
};

// ---- The chains -------------------------------------------------------------------------------------------------------------
// H: finite and >= 0, a threshold's own rule.
NBODY_HD inline bool approaches_horizon_valid(float h) { return correlation_edge_valid(h); }

// One body of a pair: where it is and how it moves.
struct ApproachPoint {
    float x, y, z, vx, vy, vz;
};

// rv = d . w in the order of groups_r2: d and w change sign together under i <-> j, so every product is the same bits.
NBODY_HD inline float approaches_rv(const ApproachPoint &i, const ApproachPoint &j)
{
    const float dx = j.x - i.x, dy = j.y - i.y, dz = j.z - i.z;
    const float wx = j.vx - i.vx, wy = j.vy - i.vy, wz = j.vz - i.vz;
    return __builtin_fmaf(dz, wz, __builtin_fmaf(dy, wy, dx * wx));
}

// m2: the r2 chain over e = fmaf(w, H, d), the separation at the horizon.  e changes sign under i <-> j, m2 does not.
NBODY_HD inline float approaches_m2(const ApproachPoint &i, const ApproachPoint &j, float h)
{
    const float dx = j.x - i.x, dy = j.y - i.y, dz = j.z - i.z;
    const float wx = j.vx - i.vx, wy = j.vy - i.vy, wz = j.vz - i.vz;
    const float ex = __builtin_fmaf(wx, h, dx), ey = __builtin_fmaf(wy, h, dy), ez = __builtin_fmaf(wz, h, dz);
    return __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
}

// The three words of a pair that the list keeps.
struct ApproachWords {
    float r2, rv, v2;
};
NBODY_HD inline ApproachWords approaches_words(const ApproachPoint &i, const ApproachPoint &j)
{
    return ApproachWords{groups_r2(i.x, i.y, i.z, j.x, j.y, j.z), approaches_rv(i, j), groups_r2(i.vx, i.vy, i.vz, j.vx, j.vy, j.vz)};
}

// Measured: all three finite (false for +inf and for NaN).
NBODY_HD inline bool approaches_measured(const ApproachWords &p)
{
    return correlation_measured(p.r2) && correlation_measured(p.v2) && correlation_measured(__builtin_fabsf(p.rv));
}

// ---- The phase ----------------------------------------------------------------------------------------------------------------
// The pair is decided at the horizon: measured, out of reach now, closing, and its closest point at or beyond H (one product).
// Only such a pair needs m2.
NBODY_HD inline bool approaches_ends(const ApproachWords &p, float t2, float h)
{
    return approaches_measured(p) && !groups_friends(p.r2, t2) && p.rv < 0.f && -p.rv >= p.v2 * h;
}

// -1, 0, 1 or 2, in the header's order.  m2 is read only where approaches_ends holds.  No division; a product that overflows
// is compared as computed; a NaN t2 is within nothing.
NBODY_HD inline int approaches_phase(const ApproachWords &p, float t2, float h, float m2)
{
    if (!approaches_measured(p))
        return kApproachNone;
    if (groups_friends(p.r2, t2))
        return kApproachNow;
    if (!(p.rv < 0.f))
        return kApproachNone;
    if (-p.rv >= p.v2 * h)
        return correlation_measured(m2) && groups_friends(m2, t2) ? kApproachEnd : kApproachNone;
    const float g = p.r2 - t2, lhs = g * p.v2, rhs = p.rv * p.rv;
    return lhs <= rhs ? kApproachPassage : kApproachNone;
}

// ---- One column of one row ----------------------------------------------------------------------------------------------------
// What row i keeps over its walk: its approaches, those with j > i, and those of phase 0.
struct ApproachRow {
    int degree = 0, upper = 0, now = 0;
};

// phases[k]: the lane's pairs of phase k among those above its rows -- every unordered pair once.
NBODY_HD inline void approaches_step(ApproachRow &row, int (&phases)[kApproachPhases], bool examined, int i, int j, int phase)
{
    const bool approach = examined && phase != kApproachNone;
    const bool above = approach && contacts_above(i, j);
    row.degree += approach ? 1 : 0;
    row.upper += above ? 1 : 0;
    row.now += approach && phase == kApproachNow ? 1 : 0;
    phases[kApproachNow] += above && phase == kApproachNow ? 1 : 0;
    phases[kApproachPassage] += above && phase == kApproachPassage ? 1 : 0;
    phases[kApproachEnd] += above && phase == kApproachEnd ? 1 : 0;
}

// ---- Fill -----------------------------------------------------------------------------------------------------------------------
// Row i meets column j again, t of its entries behind it: an approach with j > i goes to first + t while that is below the
// capacity.  list is the system's part of the list.
NBODY_HD inline void approaches_fill(BatchApproach *list, long long capacity, int first, int &t, bool examined, int i, int j,
                                     const ApproachWords &p, int phase)
{
    if (examined && contacts_above(i, j) && phase != kApproachNone) {
        const long long at = (long long)first + (long long)t;
        if (at < capacity)
            list[at] = BatchApproach{i, j, p.r2, p.rv, p.v2, phase};
        ++t;
    }
}
// A row has something to write: entries, and a start below the capacity.
NBODY_HD inline bool approaches_row_fills(int first, int upper, long long capacity) { return contacts_row_fills(first, upper, capacity); }

NBODY_HD inline BatchApproach approaches_pad() { return BatchApproach{-1, -1, __builtin_inff(), 0.f, 0.f, kApproachNone}; }

// ---- Records --------------------------------------------------------------------------------------------------------------------
NBODY_HD inline BatchApproachBody approaches_body(const ApproachRow &row, int first) { return BatchApproachBody{row.degree, row.upper, first, row.now}; }

NBODY_HD inline BatchApproachSystem approaches_system(int bodies, int approaching, int max_degree, long long pairs, long long capacity, int now,
                                                      int passing, int ending)
{
    return BatchApproachSystem{bodies, approaching, max_degree, 0, pairs, contacts_stored(pairs, capacity), now, passing, ending, 0};
}

}  // namespace nbody
