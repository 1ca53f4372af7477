/* nbody_batch_approaches.h -- the approach lists of batched ensembles: for every system every unordered pair of bodies whose
 * separation, with both bodies moved on straight lines at their current velocities, is within a radius, or within the sum of
 * their own two radii, at some time in [0, horizon], as a list of (i, j, r2, rv, v2, phase), with per body the number of its
 * approaches and their place in the list, and per system their number by phase.  Which encounters are coming before the next
 * output, which pairs to watch when choosing dt_max and the horizon of the next nbody_batch_evolve_on, the "line" collision
 * search beside the "direct" one of nbody_batch_contacts: that one lists the pairs within reach now, this one those that will be.
 * It is read from one snapshot.  The result is a set of integers plus the bits of three fp32 chains.
 * Included by nbody.h (inside its extern "C") after nbody_batch_contacts.h; additive to ABI version 5, no new status.
 *
 * Bodies, subset, thresholds.  Exactly those of nbody_batch_contacts.h.  Body i of system s takes part iff
 *   i < min(counts[s], max_bodies) and subset is NULL or subset[s * max_bodies + i] != 0; this is geometry, whatever the
 *   massive counts are, and the state is read as it stands.  Exactly one of radius and radii is non-NULL.
 *   Radius mode: t2 = correlation_edge2(radius[s]): one fp32 product on the host, one that overflows taken as the largest finite
 *     fp32 value.  Radii mode: S = R_i + R_j is one fp32 add and t2 = S * S one fp32 product; the caller passes the radii.
 * Horizon.  horizon is a host pointer to n_systems fp32 values H, each finite and >= 0.
 * Chains.  For row i and column j, d = x_j - x_i and w = v_j - v_i per component, as fp32 subtractions.  Three chains of the
 *   shape of groups_r2, every fmaf one fused operation, nothing else contracted:
 *     r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx));  v2 = fmaf(wz, wz, fmaf(wy, wy, wx wx));  rv = fmaf(dz, wz, fmaf(dy, wy, dx wx)).
 *   All three are bit-symmetric under i <-> j: d and w change sign together, and no product does.  (A component that is zero
 *   is +0 either way round, so an rv that is zero may be +0 one way and -0 the other; no decision reads the sign of a zero,
 *   and the list takes rv from i to j.)
 * Measured.  A pair is measured iff r2 <= FLT_MAX, v2 <= FLT_MAX and fabsf(rv) <= FLT_MAX: false for an infinite or NaN
 *   coordinate or velocity component of either body.  A pair that is not measured is no approach, in reach now or not.
 * Phase.  Decided in this order, with no division anywhere:
 *   0 `now`: r2 <= t2.  This is the predicate of nbody_batch_contacts.
 *   Otherwise the pair must be closing: rv < 0.  If it is not, it is no approach.
 *   2 `end`: with vh = v2 * H (one product), the pair is in this phase when -rv >= vh: the closest point of the two lines lies
 *     at or beyond the horizon, so the separation falls over all of [0, H] and is smallest at H.  e = fmaf(w, H, d) per
 *     component, and m2 is the r2 chain over e.  It is an approach iff m2 <= FLT_MAX and m2 <= t2.  e is bit-antisymmetric
 *     and m2 bit-symmetric under i <-> j.
 *   1 `passage`: otherwise; then v2 > 0 follows.  g = r2 - t2, lhs = g * v2, rhs = rv * rv, one operation each.  It is an
 *     approach iff lhs <= rhs: that is r2 - rv^2 / v2 <= t2, cross-multiplied by v2 > 0.
 *   Products that overflow are compared as computed: a vh of +inf sends the pair to phase 1, where an lhs of +inf is within an
 *   rhs of +inf and of nothing else.  A NaN t2 (a body that takes no part) is within no phase.
 *   Consequences.  With H == 0, or with all velocities equal (and finite), the approaches are exactly the contacts: at H == 0
 *   a closing pair is in phase 2 with e == d and m2 == r2 > t2, and with w == 0 no pair is closing.  Adding one velocity to
 *   every body changes nothing where it leaves the differences w the same bits, as it does wherever they are exact.
 * Approaches.  The unordered pair {i, j}, i != j, both taking part, is an approach iff it is measured and has a phase.  Every
 *   word of the decision is bit-symmetric, so (i, j) and (j, i) agree.
 * List.  A system's approaches are listed as (i, j, r2, rv, v2, phase) with i < j, d and w taken from i to j, ascending in i and
 *   then in j: the order is total.  capacity, stored, truncation, the pads and first follow nbody_batch_contacts.h: capacity is
 *   the number of entries kept per system, >= 0, the same for all systems; entry k of system s is at s * capacity + k;
 *   stored = min(pairs, capacity); the first `stored` approaches in that order are kept, and entries from `stored` on hold
 *   {-1, -1, +inf, 0, 0, -1}.  pairs is exact whatever the capacity, and a call with capacity == 0 (and list_out NULL) only
 *   counts.
 * Records.
 *   nbody_batch_approach is {int i; int j; float r2; float rv; float v2; int phase;}, 24 bytes.
 *   Per body, nbody_batch_approach_body, 16 bytes: degree (offset 0) the approaches of i; upper (4) those with j > i; first (8)
 *     the exclusive sum of upper over the lower rows, not clamped: row i's entries are [first, first + upper) cut at stored;
 *     now (12) its approaches of phase 0, which is its degree in nbody_batch_contacts.  Slots from the count on, and unselected
 *     bodies, hold {0, 0, first, 0}: first is the running sum there too.
 *   Per system, nbody_batch_approach_system, 48 bytes: bodies (offset 0) those taking part; approaching (4) those with
 *     degree >= 1; max_degree (8); reserved (12) 0; pairs (16, long long); stored (24, long long); now (32), passing (36) and
 *     ending (40) the unordered pairs of phase 0, 1 and 2; reserved2 (44) 0.
 *   The identities  now + passing + ending == pairs  and  sum(degree) == 2 * pairs == 2 * sum(upper)  hold exactly.
 *   systems_out is a host pointer to n_systems records.  bodies_out is a host pointer to n_systems x max_bodies records, or
 *   NULL; list_out one to n_systems x capacity entries, NULL iff capacity == 0.  NULL skips that copy; the system records are
 *   the same bits either way.
 * No time or distance is computed on the device.  From an entry's words, in fp64: phase 0 is at time 0 with miss distance
 *   sqrt(r2); phase 1 at time -rv / v2 with miss distance sqrt(max(0, r2 - rv^2 / v2)); phase 2 at time H with miss distance
 *   sqrt(r2 + 2 rv H + v2 H^2).
 * Bit invariance.  A system's records and list depend on its state, its subset, its radius or radii and its horizon alone: no
 *   schedule, slot, n_systems, max_bodies or capacity changes a bit of them.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more, and freed in nbody_batch_destroy.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, horizon or systems_out; a horizon that is negative, NaN or infinite (the message names the system); both of
 *   radius and radii given, or neither; a per-system radius that is negative, NaN or infinite (the message names the system);
 *   a per-body radius below its system's count that is negative or not finite (the message names the system and the slot);
 *   capacity < 0; capacity > 0 with list_out NULL, or capacity == 0 with list_out non-NULL; n_systems * capacity > 2^27
 *   (NBODY_BATCH_APPROACHES_MAX_ENTRIES, the bytes of the contacts limit).  All are refused before any device work, and nothing
 *   is written to the outputs.
 * Out of scope: curved paths (accelerations), pairs across systems, softening, sorting by time on the device, device-side
 *   outputs, and changing the state. */
#ifndef NBODY_AMD_BATCH_APPROACHES_H
#define NBODY_AMD_BATCH_APPROACHES_H

#define NBODY_BATCH_APPROACHES_MAX_ENTRIES (1LL << 27)

#define NBODY_BATCH_APPROACH_NOW 0      /* within the threshold at time 0 */
#define NBODY_BATCH_APPROACH_PASSAGE 1  /* closest inside (0, H), and within the threshold there */
#define NBODY_BATCH_APPROACH_END 2      /* still closing at H, and within the threshold there */

typedef struct nbody_batch_approach_system {
    int bodies;        /* offset  0: the bodies taking part */
    int approaching;   /* offset  4: those with degree >= 1 */
    int max_degree;    /* offset  8: the largest degree */
    int reserved;      /* offset 12: 0 */
    long long pairs;   /* offset 16: the approaches, exact whatever the capacity */
    long long stored;  /* offset 24: min(pairs, capacity) */
    int now;           /* offset 32: the pairs of phase 0 */
    int passing;       /* offset 36: the pairs of phase 1 */
    int ending;        /* offset 40: the pairs of phase 2 */
    int reserved2;     /* offset 44: 0 */
} nbody_batch_approach_system;  /* 48 bytes */

typedef struct nbody_batch_approach_body {
    int degree;  /* offset  0: the approaches of this body */
    int upper;   /* offset  4: those with a higher index */
    int first;   /* offset  8: the exclusive sum of upper over the lower rows */
    int now;     /* offset 12: those of phase 0 */
} nbody_batch_approach_body;  /* 16 bytes */

typedef struct nbody_batch_approach {
    int i;
    int j;
    float r2;   /* |d|^2 now */
    float rv;   /* d . w */
    float v2;   /* |w|^2 */
    int phase;  /* 0, 1 or 2; -1 in a pad */
} nbody_batch_approach;  /* 24 bytes */

typedef char nbody_batch_approach_system_is_48_bytes[sizeof(nbody_batch_approach_system) == 48 ? 1 : -1];
typedef char nbody_batch_approach_body_is_16_bytes[sizeof(nbody_batch_approach_body) == 16 ? 1 : -1];
typedef char nbody_batch_approach_is_24_bytes[sizeof(nbody_batch_approach) == 24 ? 1 : -1];

int nbody_batch_approaches(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities,
                           const float *horizon,         /* n_systems values */
                           const float *radius,          /* n_systems values, or NULL */
                           const float *radii,           /* n_systems x max_bodies values, or NULL */
                           const unsigned char *subset,  /* n_systems x max_bodies bytes, or NULL */
                           long long capacity,           /* list entries kept per system, >= 0 */
                           nbody_batch_approach_system *systems_out,
                           nbody_batch_approach_body *bodies_out,   /* or NULL */
                           nbody_batch_approach *list_out);         /* n_systems x capacity, or NULL; required NULL iff capacity == 0 */

#endif /* NBODY_AMD_BATCH_APPROACHES_H */
