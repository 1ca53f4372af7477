/* nbody_batch_contacts.h -- the contact lists of batched ensembles: for every system every unordered pair of bodies that lie
 * within a radius of each other, or within the sum of their own two radii, as a list of (i, j, r2), with per body the number
 * of its contacts and their place in the list, and per system their number and the closest of them.  Which planetesimals
 * overlap now, every encounter inside an impact parameter, the edges of a contact network, all neighbours inside a sphere
 * however many there are: nbody_batch_neighbours counts the bodies within a radius but lists eight, nbody_batch_correlation
 * returns totals, nbody_batch_groups the connected components without their edges, and nbody_batch_evolve_on names one
 * touching pair per stop.  This is the first batch result of variable length.  The result is a set of integers plus the bits
 * of r2.
 * Included by nbody.h (inside its extern "C") after nbody_batch_correlation.h; additive to ABI version 5, no new status.
 *
 * Bodies.  subset is a host pointer to n_systems x max_bodies bytes, like sources of nbody_batch_neighbours, or NULL.  Body i
 *   of system s takes part iff i < min(counts[s], max_bodies) and subset is NULL or subset[s * max_bodies + i] != 0.  Only
 *   bodies below the count take part, whatever the massive counts (nbody_batch_massive.h) are: this is geometry, as in
 *   nbody_batch_neighbours.h.  Removed tracers and merged bodies are seen as the state holds them.
 * Distance.  r2 is groups_r2, the fp32 chain of nbody_batch_groups.h, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 *   There is no softening.  A pair is measured iff r2 <= FLT_MAX: false for +inf and for NaN (a NaN or infinite coordinate).
 * Threshold.  Exactly one of radius and radii is non-NULL.
 *   Radius mode: radius is a host pointer to n_systems values, each finite and >= 0.  t2 = b2 = radius[s] * radius[s] is one
 *     fp32 product on the host, the product nbody_batch_groups, nbody_batch_neighbours and nbody_batch_correlation form; a
 *     product that overflows is taken as the largest finite fp32 value (correlation_edge2's rule).  The predicate is
 *     groups_friends: r2 <= t2.
 *   Radii mode: radii is a host pointer to n_systems x max_bodies values, laid out like the positions, each finite and >= 0
 *     below its system's count.  S = R_i + R_j is one fp32 add and t2 = S * S one fp32 product: nbody_batch_radii.h's
 *     fmaf(S, S, eps^2) at eps = 0.  Contact iff measured and r2 <= t2.  A coincident pair with zero radii is a contact, as
 *     there.  The caller passes the radii: they are not the handle's (nbody_batch_radii_read gives those).
 * Contacts.  The unordered pair {i, j}, i != j, both taking part, is a contact iff it is measured and within its threshold.
 *   r2 is bit-symmetric, and so is S, so (i, j) and (j, i) agree.
 * List.  A system's contacts are listed as (i, j, r2) with i < j, ascending in i and then in j: the order is total, so the
 *   list is a set of integers plus the r2 bits, and it does not depend on schedule, slot, n_systems or max_bodies.  capacity
 *   is the number of list entries kept per system, >= 0, the same for all systems; entry k of system s is at
 *   s * capacity + k.  stored = min(pairs, capacity): the first `stored` contacts in that order are kept, and entries from
 *   `stored` on hold {-1, -1, +inf}.  pairs is exact whatever the capacity: a caller who sees stored < pairs calls again with
 *   more, and a call with capacity == 0 (and list_out NULL) only counts.
 * Records.
 *   Per body, nbody_batch_contact_body, 16 bytes: degree (offset 0) the contacts of i; upper (4) those with j > i; first (8)
 *     the exclusive sum of upper over the lower rows, not clamped: row i's entries are [first, first + upper) cut at stored;
 *     nearest (12) the contact partner of smallest r2, ties to the lower index, -1 without a contact.  Slots from the count
 *     on, and unselected bodies, hold {0, 0, first, -1}: first is the running sum there too.
 *   Per system, nbody_batch_contact_system, 48 bytes: bodies (offset 0) those taking part; touching (4) those with
 *     degree >= 1; max_degree (8); reserved (12) 0; pairs (16); stored (24); closest_i (32), closest_j (36) and closest_r2
 *     (40) the contact of smallest r2, i < j, ties to the smallest i and then the smallest j (nbody_batch_radii.h's "Pair"
 *     rule), -1, -1 and +inf without a contact; reserved2 (44) 0.
 *   nbody_batch_contact is {int i; int j; float r2;}, 12 bytes.
 *   The identity  sum(degree) == 2 * pairs == 2 * sum(upper)  holds exactly.
 *   systems_out is a host pointer to n_systems records.  bodies_out is a host pointer to n_systems x max_bodies records, or
 *   NULL; list_out one to n_systems x capacity entries, NULL iff capacity == 0.  NULL skips that copy; the system records are
 *   the same bits either way.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more, and freed in nbody_batch_destroy.
 * Bit invariance.  A system's records and list depend on its state, its subset and its radius or radii alone: the same bits
 *   in any slot, n_systems and max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm or
 *   systems_out; both of radius and radii given, or neither; a per-system radius that is negative, NaN or infinite (the
 *   message names the system); a per-body radius below its system's count that is negative or not finite (the message names
 *   the system and the slot); capacity < 0; capacity > 0 with list_out NULL, or capacity == 0 with list_out non-NULL;
 *   n_systems * capacity > 2^28 (NBODY_BATCH_CONTACTS_MAX_ENTRIES).  All are refused before any device work, and nothing is
 *   written to the outputs.
 * Out of scope: pairs across systems, softened or periodic distances, velocity criteria (approaching pairs, impact
 *   parameters), device-side outputs, per-system capacities, a list sorted by distance, and changing the state. */
#ifndef NBODY_AMD_BATCH_CONTACTS_H
#define NBODY_AMD_BATCH_CONTACTS_H

#define NBODY_BATCH_CONTACTS_MAX_ENTRIES (1LL << 28)

typedef struct nbody_batch_contact_system {
    int bodies;        /* offset  0: the bodies taking part */
    int touching;      /* offset  4: those with degree >= 1 */
    int max_degree;    /* offset  8: the largest degree */
    int reserved;      /* offset 12: 0 */
    long long pairs;   /* offset 16: the contacts, exact whatever the capacity */
    long long stored;  /* offset 24: min(pairs, capacity) */
    int closest_i;     /* offset 32: the contact of smallest r2, i < j; -1 without a contact */
    int closest_j;     /* offset 36 */
    float closest_r2;  /* offset 40: +inf without a contact */
    int reserved2;     /* offset 44: 0 */
} nbody_batch_contact_system;  /* 48 bytes */

typedef struct nbody_batch_contact_body {
    int degree;   /* offset  0: the contacts of this body */
    int upper;    /* offset  4: those with a higher index */
    int first;    /* offset  8: the exclusive sum of upper over the lower rows */
    int nearest;  /* offset 12: the contact partner of smallest r2, ties to the lower index; -1 without a contact */
} nbody_batch_contact_body;  /* 16 bytes */

typedef struct nbody_batch_contact {
    int i;
    int j;
    float r2;
} nbody_batch_contact;  /* 12 bytes */

typedef char nbody_batch_contact_system_is_48_bytes[sizeof(nbody_batch_contact_system) == 48 ? 1 : -1];
typedef char nbody_batch_contact_system_pairs_at_16[(sizeof(int) == 4 && sizeof(long long) == 8) ? 1 : -1];
typedef char nbody_batch_contact_body_is_16_bytes[sizeof(nbody_batch_contact_body) == 16 ? 1 : -1];
typedef char nbody_batch_contact_is_12_bytes[sizeof(nbody_batch_contact) == 12 ? 1 : -1];

int nbody_batch_contacts(nbody_batch *b, const float *d_positions_xyzm,
                         const float *radius,          /* n_systems values, or NULL */
                         const float *radii,           /* n_systems x max_bodies values, or NULL */
                         const unsigned char *subset,  /* n_systems x max_bodies bytes, or NULL */
                         long long capacity,           /* list entries kept per system, >= 0 */
                         nbody_batch_contact_system *systems_out,
                         nbody_batch_contact_body *bodies_out,   /* or NULL */
                         nbody_batch_contact *list_out);         /* n_systems x capacity, or NULL; required NULL iff capacity == 0 */

#endif /* NBODY_AMD_BATCH_CONTACTS_H */
