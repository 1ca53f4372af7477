/* nbody_batch_structure.h -- the cluster structure of batched ensembles: every body's neighbour density, and per system the
 * density centre, the core radius and density, and Lagrangian radii about the centre, found on the device by a sibling of
 * the force kernels.  These are the Casertano & Hut (1985) quantities an N-body code prints at every output time: where the
 * cluster is, how concentrated it is, how it expands or collapses.  nbody_batch_pairs.h leaves neighbour lists out of scope;
 * this is the sibling that does the neighbour work.
 * Included by nbody.h (inside its extern "C") after nbody_batch_pairs.h; additive to ABI version 5, no new status.
 *
 * The bodies are all j < counts[s] of system s, whatever the massive counts (nbody_batch_massive.h) are: test particles
 *   are bodies here, rows and columns alike.  Removed tracers (nbody_batch_fate.h) and merged bodies (nbody_batch_merge.h)
 *   are seen as the state holds them, as in nbody_batch_pairs: frozen tracers are ordinary bodies, the counts are the live ones.
 * The weight w_j.  NBODY_BATCH_WEIGHT_MASS (0): the mass word.  NBODY_BATCH_WEIGHT_NUMBER (1): every body weighs 1, so that
 *   test particles with zero mass words have a structure too.
 * The neighbour search runs in fp32, the columns in ascending j, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 *   A pair is a neighbour pair only where r2 > 0: that single test drops the self pair, coincident bodies and NaN.
 *   r2_k(i) is the k-th smallest r2 of row i's neighbour pairs, 1 <= k <= NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR (8); it is
 *   +inf where the row has fewer than k.  The k-th smallest of a set does not depend on the order it is found in, so this
 *   number is a function of the state alone.
 * Neighbour weight and density (the unbiased estimator: the k-th neighbour and the body itself are left out).
 *   inside(i) is the number of pairs with 0 < r2 < r2_k(i); neighbour_weight(i) is the fp32 sum, in ascending j, of w_j over
 *   those pairs.  Exact ties with the k-th distance are not inside, so inside may be below k - 1.  Where r2_k is +inf every
 *   neighbour pair of the row is inside.
 *     density(i) = neighbour_weight / (4 pi / 3 r^3) with r = sqrt((double)r2_k), computed in fp64;
 *     4 pi / 3 = 4.1887902047863909846.  density is 0 where r2_k is +inf.
 * System quantities, fp64 from the fp32 state and the densities rho_i:
 *     estimated    = the number of bodies with finite r2_k
 *     centre       = sum rho_i x_i / sum rho_i
 *     core_radius  = sqrt(sum rho_i^2 |x_i - centre|^2 / sum rho_i^2)
 *     core_density = sum rho_i^2 / sum rho_i
 *     total_weight = sum w_i, the fp32 weights summed in fp64
 *   Where sum rho = 0 (for example n <= k): centre is the centre of weight sum w x / sum w, and core radius and core density
 *   are 0.  Where total_weight is also 0: everything is 0 -- centre, core radius, core density, total weight and every
 *   Lagrangian radius; estimated stays the count it is.
 * Radii about the centre, fp64:
 *     s_i = dx^2 + dy^2 + dz^2 with dx = (double)x_i - centre_x, and so on;  radius(i) = sqrt(s_i);
 *     enclosed(i) = sum_j w_j [s_j <= s_i], summed in fp64.
 *   fp32 weights of up to 4096 bodies sum exactly in fp64 whenever they span less than a factor 2^17 (24 bits of each, 17 of
 *   span and 12 of count are the 53 of a double), so enclosed and total_weight then do not depend on the summation order.
 * Lagrangian radii.  The caller gives up to NBODY_BATCH_STRUCTURE_FRACTIONS (8) fractions f in (0, 1].  lagrange[q] is the
 *   smallest radius(i) with enclosed(i) >= f_q total_weight (one fp64 product); where no body qualifies it is the largest
 *   radius.  Unused slots are 0; a system without bodies has 0 throughout.
 * Records.  systems_out is a host pointer to n_systems records.  bodies_out is a host pointer to n_systems x max_bodies
 *   records laid out like the positions, or NULL: NULL skips the per-body copy, so a caller who wants the 120 bytes per system
 *   does not pay 40 bytes per body; the system records are the same bits either way.  Slots from the count on read the empty
 *   body record: all zero, inside 0.
 * The call reads the caller's buffer as nbody_batch_pairs does, on the handle's stream after the queued work, and waits for
 *   it: synchronous.  It forgets nothing: the cached accelerations, jerks, levels, stops, fates and logs are untouched, so a
 *   nbody_batch_evolve_on after it is bit for bit the nbody_batch_evolve_on without it.  The device buffers belong to the
 *   handle; they are allocated on first use and freed in nbody_batch_destroy.
 * A body's neighbour_r2, inside, neighbour_weight and density are functions of its system's state alone: the slot,
 *   n_systems and max_bodies change no bit.  The system record is the same bits in every slot and n_systems at one
 *   max_bodies; across max_bodies its sums are taken in another order and agree to round-off.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle, d_positions_xyzm or
 *   systems_out; k outside 1 ... 8; weight not 0 or 1; n_fractions outside 0 ... 8; n_fractions > 0 with fractions NULL; a
 *   fraction outside (0, 1] (NaN included).  All are refused before any device work.
 * Out of scope: subsets of bodies, softened or velocity-dependent estimators, k > 8, the neighbours' indices, and
 *   recentring the state. */
#ifndef NBODY_AMD_BATCH_STRUCTURE_H
#define NBODY_AMD_BATCH_STRUCTURE_H

#define NBODY_BATCH_WEIGHT_MASS 0
#define NBODY_BATCH_WEIGHT_NUMBER 1
#define NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR 8
#define NBODY_BATCH_STRUCTURE_FRACTIONS 8

typedef struct nbody_batch_structure_body {
    double density;         /* neighbour_weight / (4 pi / 3 r^3), r = sqrt(neighbour_r2) */
    double radius;          /* |x_i - centre| */
    double enclosed;        /* the weight within radius, the body itself included */
    float neighbour_r2;     /* r2_k: the squared distance to the k-th neighbour, +inf without one */
    float neighbour_weight; /* the weight strictly inside it */
    int inside;             /* the number of bodies strictly inside it */
    int reserved;
} nbody_batch_structure_body; /* 40 bytes */

typedef struct nbody_batch_structure_system {
    double centre[3];
    double core_radius, core_density, total_weight;
    double lagrange[8];
    int estimated;          /* bodies with a finite neighbour_r2 */
    int reserved;
} nbody_batch_structure_system; /* 120 bytes */

int nbody_batch_structure(nbody_batch *b, const float *d_positions_xyzm, int k, int weight, const double *fractions,
                          int n_fractions, nbody_batch_structure_system *systems_out, nbody_batch_structure_body *bodies_out);

#endif /* NBODY_AMD_BATCH_STRUCTURE_H */
