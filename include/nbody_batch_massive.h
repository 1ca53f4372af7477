/* nbody_batch_massive.h -- test particles for batched ensembles: bodies that feel the massive bodies of their system and
 * exert no force themselves (planetesimals, ring particles, a swarm of probes around a binary).
 * Included by nbody.h (inside its extern "C") after nbody_batch_radii.h; additive to ABI version 5, no new status.
 *
 * Massive counts.  One number massive[s] per system, n_systems values in [0, max_bodies].  The first
 *   m_s = min(massive[s], counts[s]) bodies of system s are massive; the bodies after them, up to counts[s], are test
 *   particles.  The handle owns the values: nbody_batch_massive_set takes them (NULL switches the feature off, which is
 *   the default) and nbody_batch_massive_read returns them as they were set (NBODY_ERR_STATE with a message when off).
 *   A NULL handle or a value outside [0, max_bodies] is refused with NBODY_ERR_INVALID and a message that names the
 *   function, the system and the value, before any device work; a refused call changes nothing.
 *   nbody_batch_massive_set forgets what nbody_batch_set_counts forgets -- the cached accelerations and jerks, the evolve
 *   level, the stops, and an interrupted nbody_batch_evolve_on call -- with NULL too.  The values belong to the handle:
 *   nbody_batch_set_counts, new states and nbody_batch_invalidate_forces leave them alone, and a count that falls below
 *   massive[s] makes every body of the system massive.
 * Test particles are rows like any other: they are predicted, corrected, kicked and drifted, and they count in the
 *   time-step criterion of nbody_batch_evolve_on (the first-step rule and Aarseth's criterion take the maximum level over
 *   every body of the system).  They are never columns: no body, massive or not, receives a force or jerk contribution
 *   from them.  Row i sums the columns j = 0 .. m_s - 1 in ascending order in the one fp32 chain nbody.h describes, the
 *   self pair included for i < m_s.
 * Mass words.  positions[s, i, 3] of a test particle is read by no force kernel and is preserved bit for bit, as are the
 *   velocities' fourth words.  nbody_batch_energy and nbody_batch_momentum keep reading the mass words of every body: with
 *   the test particles' mass words zero they give the energy and momentum of the massive bodies; with other values the
 *   test particles enter both sums as if they had that mass, which no integrator step agrees with.
 * Equivalence.  With the feature on, a run equals bit for bit the run with the feature off and the test particles' mass
 *   words zero, wherever that run is finite: a zero-mass column adds fma(d, +0, a), which leaves a as it is.  Where it is
 *   not -- with eps = 0 two test particles that pass close to each other overflow the jerk term of a zero-mass column
 *   (inf 0 = NaN) -- the feature stays finite: the pair is never formed.
 * m_s = 0.  Every acceleration and jerk is exactly +0 and the bodies move on straight lines.  In nbody_batch_evolve_on
 *   both the first-step rule and the criterion then have a zero denominator, which nbody_batch_evolve.h defines as +inf:
 *   the level is 0.
 * Off (the default, or after NULL) every entry point launches exactly the kernels it launches without this header: no
 *   bit and no launch changes.  On, nbody_batch_step_n_* for all three integrators and nbody_batch_evolve_on run siblings
 *   of their kernels whose column loop ends at m_s; the workgroup shape and the LDS layout are the same.  Everything
 *   nbody_batch_evolve.h promises holds unchanged: the exact tick axis, independence of
 *   nbody_batch_evolve_launch_steps, evolve(a) followed by evolve(b) is evolve(a + b), resumption after max_steps, and
 *   results that are functions of the system alone -- not of its slot, B, max_bodies or the other systems.
 * Out of scope here: stopping conditions, mergers and per-body radii together with massive counts.  By default
 *   nbody_batch_evolve_on is refused with NBODY_ERR_INVALID and a message while massive counts are set and a collision
 *   radius, an escape radius or radii are (a collision action other than the default acts only with one of those).  The
 *   reason: the collision test of the evaluation (nbody_batch_stop.h) counts on the row's own column being among the columns
 *   it walks -- two columns within the threshold mean a neighbour -- and a test-particle row has no column of its own.
 *   nbody_batch_fate.h lifts the refusal for those who opt in (nbody_batch_fate_set, NBODY_BATCH_TRACERS_REMOVE): a
 *   test-particle row is judged by one column within the threshold, a test particle that hits a massive body or escapes is
 *   removed with a fate, and the system carries on; mergers together with massive counts stay refused.
 *   nbody_batch_step_n_* ignores the conditions, as it does without massive counts.  Also out of scope: test particles that
 *   are not the last bodies of their system, and a force of the test particles on each other. */
#ifndef NBODY_AMD_BATCH_MASSIVE_H
#define NBODY_AMD_BATCH_MASSIVE_H

int nbody_batch_massive_set(nbody_batch *b, const int64_t *host_massive);
int nbody_batch_massive_read(nbody_batch *b, int64_t *host_massive);

#endif /* NBODY_AMD_BATCH_MASSIVE_H */
