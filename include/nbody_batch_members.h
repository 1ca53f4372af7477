/* nbody_batch_members.h -- the bound members of batched ensembles: every body's potential and energy in the rest frame of
 * the bodies that still belong to its system, found by iterative unbinding on the device, and per system the bound mass, its
 * centre and velocity, and the kinetic and potential energy of what is left.  This is the "bound mass" every cluster code and
 * halo finder reports (SUBFIND, AHF, ROCKSTAR): compute every body's energy in the frame of the current member set, drop the
 * bodies with energy >= 0, repeat with the potential and frame of the survivors until nothing changes.  nbody_batch_energy
 * gives one total per system and nbody_batch_pairs looks at two-body energies; this is the sibling with a per-body potential.
 * Included by nbody.h (inside its extern "C") after nbody_batch_structure.h; additive to ABI version 5, no new status.
 *
 * Bodies.  The rows are all i < counts[s] of system s.  The sources are the bodies j < m: with massive counts set
 *   (nbody_batch_massive.h) m = min(massive[s], counts[s]), otherwise m = counts[s].  A test particle is a row but never a
 *   source: it can be a member, and its mass word is read by nothing here.  Removed tracers (nbody_batch_fate.h) and merged
 *   bodies (nbody_batch_merge.h) are seen as the state holds them, as in nbody_batch_pairs and nbody_batch_structure.
 * Start.  member_0(i) = 1 for every row; if initial is given, member_0(i) = initial[s * max_bodies + i] != 0.  initial is a
 *   host pointer to n_systems x max_bodies bytes laid out like the positions, or NULL.
 * Iteration t = 1, 2, ... over the member set of t - 1:
 *   Frame.  M = sum (double)m_j over member sources; V = sum m_j v_j / M, in fp64 from the fp32 state.  The sum order is
 *     fixed: the lanes of a wave, then the waves in ascending order.  If M == 0, V = 0.
 *   Potential.  phi_i = - sum_j term_ij over member sources j != i in ascending j.  Each term is fp32, formed exactly as
 *     nbody_batch_energy forms its own, every fmaf one fused operation, nothing else contracted:
 *       d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps2)));  inv = rsq(r2), where at eps = 0
 *       an r2 below 2^-84 (coincident bodies) gives inv = 0;  term = m_j inv.
 *     The terms are accumulated in fp64.  A non-member source enters as a source of mass 0: its term is +0 and leaves the
 *     sum's bits unchanged.
 *   Energy.  e_i = |v_i - V|^2 / 2 + phi_i in fp64: d = (double)v_i - V per component, e = 0.5 (dx dx + dy dy + dz dz) + phi.
 *   Decision.  member_t(i) = member_{t-1}(i) && e_i < 0.  The comparison is strict: a lone body has e = 0 and is not a bound
 *     system.  A NaN energy is not negative either.  Bodies only ever leave the set.
 *   End.  Stop after iteration t if it removed nobody or left no member: converged = 1.  Stop after iteration t if
 *     t == max_iterations: converged = 0.
 * Records.  potential and energy are the last iteration's, written for every row i < counts[s], members or not.  removed_at
 *   is the iteration that dropped the body; 0 for a member and for a body not in initial.  After the loop one more O(n)
 *   reduction gives bound_mass, centre, velocity, members and sources of the final set; centre and velocity are 0 where
 *   bound_mass is 0.  kinetic and potential of the system are summed over the final member sources with the last iteration's
 *   V and phi: exact for the final set when converged.  Slots from the count on read the empty record, all zero.  A system
 *   without bodies is all zero, with iterations = 0 and converged = 1.
 *   systems_out is a host pointer to n_systems records.  bodies_out is a host pointer to n_systems x max_bodies records laid
 *   out like the positions, or NULL: NULL skips the 24 bytes per body; the system records are the same bits either way.
 * Softening.  nbody_batch_energy's rule: finite, 0 or >= NBODY_MIN_SOFTENING.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use and
 *   freed in nbody_batch_destroy.
 * Bit invariance.  potential depends on the system's state and initial alone: the same bits in any slot, n_systems and
 *   max_bodies.  energy and the system sums are the same bits at one max_bodies; across max_bodies the frame's sums are taken
 *   in another order and agree to round-off.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities or systems_out; max_iterations outside 1 ... 64; a bad softening.  All are refused before any device work.
 *   The cap of NBODY_BATCH_MEMBERS_MAX_ITERATIONS (64) keeps a launch bounded whatever the state is.
 * Out of scope: the external field and tidal radii (the criterion is the self-gravity of the set alone), re-admitting a body
 *   once removed, a centre other than the centre of mass, more than one bound group per system, and changing the state. */
#ifndef NBODY_AMD_BATCH_MEMBERS_H
#define NBODY_AMD_BATCH_MEMBERS_H

#define NBODY_BATCH_MEMBERS_MAX_ITERATIONS 64

typedef struct nbody_batch_member_body {
    double potential;   /* phi_i of the last iteration evaluated (G = 1), <= 0 */
    double energy;      /* |v_i - V|^2 / 2 + phi_i of the last iteration evaluated */
    int member;         /* 1: in the final member set */
    int removed_at;     /* the iteration that removed it; 0 for a member and for a body not in `initial` */
} nbody_batch_member_body;   /* 24 bytes */

typedef struct nbody_batch_member_system {
    double bound_mass;          /* sum of the mass words of the final member sources */
    double centre[3];           /* their centre of mass */
    double velocity[3];         /* their centre-of-mass velocity */
    double kinetic, potential;  /* over the final member sources: sum m |v - V|^2 / 2 and sum m phi / 2, last evaluation's V and phi */
    int members, sources;       /* final members (test particles included); final member sources */
    int iterations, converged;  /* iterations evaluated; 1 if the last one removed nothing or left no member */
} nbody_batch_member_system; /* 88 bytes */

int nbody_batch_members(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities, float softening,
                        int max_iterations, const unsigned char *initial,
                        nbody_batch_member_system *systems_out, nbody_batch_member_body *bodies_out);

#endif /* NBODY_AMD_BATCH_MEMBERS_H */
