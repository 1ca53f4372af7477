/* nbody_batch_groups.h -- the groups of batched ensembles: friends-of-friends clumps at a linking length.  Two bodies closer
 * than the linking length b are friends; a group is a connected set of friends (Davis et al. 1985, the FoF of every halo
 * finder).  nbody_batch_structure gives one centre per system, nbody_batch_members one bound set and nbody_batch_hierarchy
 * nested pairs; this is the sibling that says into how many pieces a system has fallen, which bodies are together, and where
 * each piece is and how it moves.  The group of a body is the lowest index among the bodies connected to it, so the result is
 * a set of integers that does not depend on the schedule that found it.
 * Included by nbody.h (inside its extern "C") after nbody_batch_gravity.h; additive to ABI version 5, no new status.
 *
 * Bodies.  The rows are all i < counts[s] of system s, whatever the massive counts (nbody_batch_massive.h) are: this is
 *   geometry, as in nbody_batch_structure.h, and test particles link like every other body.  Removed tracers
 *   (nbody_batch_fate.h) and merged bodies (nbody_batch_merge.h) are seen as the state holds them.
 * Link.  Bodies i != j are friends iff r2 <= b2, in fp32, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx));  b2 = b[s] b[s], one fp32 product formed on the
 *     host.
 *   There is no softening.  r2 is bit-symmetric in i and j, so the relation is symmetric.  A NaN coordinate links to nothing:
 *   the comparison is false.  b[s] == 0 links only coincident bodies.
 * Labels.  L_i starts as i.  Sweeps t = 1, 2, ... follow, each made of three steps with all reads before any write:
 *   Link.  c_i = min L_j over the friends of i.  The label of row i is lowered by the sweep iff c_i < L_i.
 *   Hook.  If c_i < L_i: L[L_i] = min(L[L_i], c_i) and L_i = c_i.  L_i is a root here (L[L_i] == L_i), because the previous
 *     sweep compressed; where i is its own root the two writes are the one min.  Min commutes, so the outcome does not depend
 *     on the order in which the rows hook.
 *   Compress.  L_i <- L[L_i] for all rows at once, repeated until a pass changes nothing: every label is a root again.
 *   End.  Stop after sweep t if its Link step lowered no label: converged = 1.  Stop after sweep t if t == max_sweeps:
 *   converged = 0.  A label never rises and L_i <= i throughout, so the labels cannot cycle.  sweeps is the number of sweeps
 *   run, the last one that lowered nothing included; it is a function of the state alone: every step above is.  When
 *   converged, L_i is the lowest index of i's group.  When not, L_i is a root below or at i in i's group, and the records
 *   describe the sets of equal labels.  The hook makes long chains converge in a handful of sweeps (a chain of 4096 bodies in
 *   random index order: 8 to 10, against more than a thousand without it); NBODY_BATCH_GROUPS_MAX_SWEEPS (64) keeps a launch
 *   bounded whatever the state is.
 * Weights.  NBODY_BATCH_WEIGHT_MASS (0, nbody_batch_structure.h): w_j is the mass word for j < m, where
 *   m = min(massive[s], counts[s]) with massive counts set, otherwise m = counts[s]; w_j = 0 for a test particle, whose mass
 *   word is read by nothing here.  NBODY_BATCH_WEIGHT_NUMBER (1): w_j = 1 for every body, so that groups of test particles
 *   have a centre too.
 * Records.  All sums are fp64 from the fp32 state, over a group's members in ascending index: weight = sum (double)w_j,
 *   sum (double)w_j (double)x_j and sum (double)w_j (double)v_j.  Each product is exact (24 x 24 bits), so the sums are the
 *   same bits wherever they are formed.  Nothing is summed across lanes.
 *   Per body, nbody_batch_group_body: group is the final L_i and size the number of members of its group; -1 and 0 from the
 *     count on.
 *   Per slot, nbody_batch_group_record: filled at slot r where L_r == r, the root of a group: weight, centre = sum w x / weight
 *     and velocity = sum w v / weight (one fp64 division each; 0 where the weight is 0), count (all members) and sources (the
 *     members j < m).  Every other slot, and every slot from the count on, is the all-zero record.
 *   Per system, nbody_batch_group_system: groups is the number of groups with count >= min_members, grouped the bodies in
 *     those groups, singles the groups of one body, largest the root of the group with the most members (ties to the lower
 *     root; -1 for a system without bodies) and largest_count its count; sweeps and converged as above; reserved is 0.  A
 *     system without bodies is all zero with largest = -1, sweeps = 0 and converged = 1.
 *   systems_out is a host pointer to n_systems records.  groups_out and bodies_out are host pointers to n_systems x max_bodies
 *   records laid out like the positions, or NULL: NULL skips that copy; the system records are the same bits either way.
 *   linking_lengths is a host pointer to n_systems floats.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use and
 *   freed in nbody_batch_destroy.
 * Bit invariance.  A system's group, size, sweeps and group records depend on its state, its linking length and its massive
 *   count alone: the same bits in any slot, n_systems and max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, linking_lengths or systems_out; a negative or non-finite linking length; min_members < 1; an unknown weight;
 *   max_sweeps outside 1 ... 64.  All are refused before any device work.
 * Out of scope: linking in velocity (6-D FoF), unbinding of the groups (compose with nbody_batch_members and its initial
 *   set), periodic boxes, groups across systems, second moments, and changing the state. */
#ifndef NBODY_AMD_BATCH_GROUPS_H
#define NBODY_AMD_BATCH_GROUPS_H

#define NBODY_BATCH_GROUPS_MAX_SWEEPS 64

typedef struct nbody_batch_group_body {
    int group;   /* the final label L_i: the lowest index of the body's group when converged; -1 from the count on */
    int size;    /* the members of its group; 0 from the count on */
} nbody_batch_group_body;    /* 8 bytes */

typedef struct nbody_batch_group_record {
    double weight;        /* sum of w_j over the members */
    double centre[3];     /* sum w x / weight; 0 where the weight is 0 */
    double velocity[3];   /* sum w v / weight; 0 where the weight is 0 */
    int count;            /* all members */
    int sources;          /* the members j < m */
} nbody_batch_group_record;  /* 64 bytes; filled at the root's slot, all zero elsewhere */

typedef struct nbody_batch_group_system {
    int groups;          /* groups with count >= min_members */
    int grouped;         /* the bodies in those groups */
    int singles;         /* groups of one body */
    int largest;         /* root of the group with the most members, ties to the lower root; -1 without bodies */
    int largest_count;   /* its count */
    int sweeps;          /* sweeps run */
    int converged;       /* 1 if the last sweep's Link step lowered no label */
    int reserved;        /* 0 */
} nbody_batch_group_system;  /* 32 bytes */

int nbody_batch_groups(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities, const float *linking_lengths,
                       int min_members, int weight, int max_sweeps, nbody_batch_group_system *systems_out,
                       nbody_batch_group_record *groups_out, nbody_batch_group_body *bodies_out);

#endif /* NBODY_AMD_BATCH_GROUPS_H */
