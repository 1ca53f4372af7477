// nbody_batch_contacts_math.h -- the arithmetic of nbody_batch_contacts (include/nbody_batch_contacts.h) that needs no GPU: the
// three records, the two thresholds and the contact predicate, the step of one row over one column (degree, upper, nearest),
// the 64-bit key of the closest contact and its unpacking, the placement of the rows' entries from the running sum of their
// upper counts, the fill step with its capacity clamp, the pad entry and the system record.  Plain C++17 without HIP, like
// nbody_batch_correlation_math.h, and like it on top of nbody_batch_groups_math.h, whose r2 chain and `friends` predicate it
// reuses; the squared radius is correlation_edge2 and the key is nbody_batch_span_math.h's.  batch_contacts_kernel
// (nbody_batch_analysis.hip) calls these with the columns in LDS, and a stand-alone driver (tests/batch_contacts_driver.cpp)
// runs whole systems through the same functions, lane by lane for any workgroup shape, on the CPU, where
// tests/test_batch_contacts_cpu.py compares them with numpy.  Internal; the public surface is include/nbody_batch_contacts.h.
#pragma once

#include "nbody_batch_correlation_math.h"
#include "nbody_batch_groups_math.h"
#include "nbody_batch_span_math.h"

namespace nbody {

constexpr long long kContactsMaxEntries = 1ll << 28;  // n_systems x capacity, at most
constexpr int kContactsWave = 64;                     // the lanes of a wave: the unit of the placement scan

// nbody_batch_contact_system's layout (nbody_batch_analysis.hip asserts it): 48 bytes.
struct BatchContactSystem {
    int bodies, touching, max_degree, reserved;
    long long pairs, stored;
    int closest_i, closest_j;
    float closest_r2;
    int reserved2;
};

// nbody_batch_contact_body's layout (nbody_batch_analysis.hip asserts it): 16 bytes.
struct BatchContactBody {
    int degree, upper, first, nearest;
};

// nbody_batch_contact's layout (nbody_batch_analysis.hip asserts it): 12 bytes.
struct BatchContact {
    int i, j;
    float r2;
};

// ---- Thresholds and the predicate -------------------------------------------------------------------------------------------
// Radius mode: t2 = b2, the one fp32 product of groups(), neighbours() and correlation(); one that overflows is FLT_MAX.
NBODY_HD inline float contacts_radius_t2(float radius) { return correlation_edge2(radius); }

// Radii mode: S = R_i + R_j is one fp32 add, t2 = S * S one fp32 product: nbody_batch_radii.h's fmaf(S, S, eps^2) at eps = 0.
// A body that does not take part carries a NaN for its radius: S, t2 and every compare against t2 are then NaN and false.
NBODY_HD inline float contacts_radii_t2(float ri, float rj)
{
    const float s = ri + rj;
    return s * s;
}
NBODY_HD inline float contacts_no_radius() { return __builtin_nanf(""); }

// Contact iff measured (r2 <= FLT_MAX: false for +inf and for NaN) and within the threshold (r2 <= t2: false for a NaN t2).
NBODY_HD inline bool contacts_touch(float r2, float t2) { return correlation_measured(r2) && groups_friends(r2, t2); }

// ---- One column of one row ----------------------------------------------------------------------------------------------------
// What row i keeps over its walk: its contacts, those with j > i, and the partner of smallest (bits(r2), j) under a strict <.
// The columns come in ascending j, so a tie stays with the lower index.  r2 of a contact is measured and never negative, so
// its bits order as its value does.
struct ContactRow {
    int degree = 0, upper = 0;
    unsigned bits = kSpanNoBits;
    int nearest = -1;
};

// examined: row i and column j both take part and are two bodies.
NBODY_HD inline bool contacts_examined(bool row, bool column, int i, int j) { return row && column && j != i; }
NBODY_HD inline bool contacts_above(int i, int j) { return j > i; }

NBODY_HD inline void contacts_step(ContactRow &row, bool examined, int i, int j, float r2, float t2)
{
    const bool touch = examined && contacts_touch(r2, t2);
    const unsigned bits = span_bits(r2);
    const bool better = touch && bits < row.bits;
    row.degree += touch ? 1 : 0;
    row.upper += touch && contacts_above(i, j) ? 1 : 0;
    row.bits = better ? bits : row.bits;
    row.nearest = better ? j : row.nearest;
}

// ---- The closest contact --------------------------------------------------------------------------------------------------------
// The key of what row i found: the r2 bits, then the lower index, then the higher (span_key).  The smallest key over the rows
// is the smallest (r2, i, j) over the contacts with i < j: the row at the lower end of that contact holds exactly it, and every
// other row's key is the key of some contact.  Integers: the minimum may be taken in any order.
NBODY_HD inline SpanKey contacts_row_key(const ContactRow &row, int i) { return row.nearest < 0 ? kSpanNoKey : span_key(row.bits, i, row.nearest); }
NBODY_HD inline int contacts_key_i(SpanKey k) { return k == kSpanNoKey ? -1 : span_key_i(k); }
NBODY_HD inline int contacts_key_j(SpanKey k) { return k == kSpanNoKey ? -1 : span_key_j(k); }
NBODY_HD inline float contacts_key_r2(SpanKey k) { return k == kSpanNoKey ? __builtin_inff() : span_bits_r2(span_key_bits(k)); }

// ---- Placement ----------------------------------------------------------------------------------------------------------------
// Row r = q * T + tid of a workgroup of T lanes belongs to unit u = q * (T / 64) + wave: the units in ascending u hold the rows
// in ascending r, 64 to a unit.  totals[u] is the sum of `upper` over unit u.  A row's entries start at the sum of the units
// below its own plus the `upper` of the lower rows of its own unit.
NBODY_HD inline int contacts_unit(int q, int waves, int wave) { return q * waves + wave; }
NBODY_HD inline int contacts_units_below(const int *totals, int unit)
{
    int sum = 0;
    for (int u = 0; u < unit; ++u)
        sum += totals[u];
    return sum;
}
// One row from the running sum: where it starts, and the sum it leaves behind.  Not clamped.
NBODY_HD inline int contacts_place(int &running, int upper)
{
    const int first = running;
    running += upper;
    return first;
}
NBODY_HD inline long long contacts_stored(long long pairs, long long capacity) { return pairs < capacity ? pairs : capacity; }

// ---- Fill -----------------------------------------------------------------------------------------------------------------------
// Row i meets column j again, t of its entries behind it: a contact with j > i goes to first + t while that is below the
// capacity.  list is the system's part of the list.
NBODY_HD inline void contacts_fill(BatchContact *list, long long capacity, int first, int &t, bool examined, int i, int j, float r2,
                                   float t2)
{
    if (examined && contacts_above(i, j) && contacts_touch(r2, t2)) {
        const long long at = (long long)first + (long long)t;
        if (at < capacity)
            list[at] = BatchContact{i, j, r2};
        ++t;
    }
}
// A row has something to write: entries, and a start below the capacity.
NBODY_HD inline bool contacts_row_fills(int first, int upper, long long capacity) { return upper > 0 && (long long)first < capacity; }

NBODY_HD inline BatchContact contacts_pad() { return BatchContact{-1, -1, __builtin_inff()}; }

// ---- Records --------------------------------------------------------------------------------------------------------------------
NBODY_HD inline BatchContactBody contacts_body(const ContactRow &row, int first) { return BatchContactBody{row.degree, row.upper, first, row.nearest}; }

NBODY_HD inline BatchContactSystem contacts_system(int bodies, int touching, int max_degree, long long pairs, long long capacity, SpanKey closest)
{
    return BatchContactSystem{bodies, touching, max_degree, 0, pairs, contacts_stored(pairs, capacity), contacts_key_i(closest),
                              contacts_key_j(closest), contacts_key_r2(closest), 0};
}

}  // namespace nbody
