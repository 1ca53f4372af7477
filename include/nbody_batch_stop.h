/* nbody_batch_stop.h -- stopping conditions for Hermite batches: nbody_batch_evolve_on ends a system's run when two of its
 * bodies come within a collision radius or a body leaves an escape radius, and reports when, and which bodies.  Included by
 * nbody.h (inside its extern "C") after nbody_batch_evolve.h; additive to ABI version 5, no new status.
 *
 * Collision, collision_radius R_c > 0 (0: off).  Examined at every acceleration-and-jerk evaluation: the one of each step,
 *   at the predicted positions, and the initial one at the current positions when the caches are empty.  For body i, m_i is
 *   the minimum over j != i of the evaluation's own fp32 r2 = d.d + eps^2 (its FMA chain, nbody.h).  The system stops when
 *   min_i m_i <= thr, thr = fmaf(R_c, R_c, eps^2) in fp32, formed once on the host.  The self pair never counts; a
 *   coincident pair (d = 0, i != j) does, with eps = 0 too (the value compared is the one before the zero-distance guard).
 * Escape, escape_radius R_e > 0 (0: off).  Examined on the corrected positions after every step, and on the current
 *   positions at the initial evaluation.  Body i has escaped when fmaf(z, z, fmaf(y, y, x x)) > R_e R_e, all fp32.  The
 *   distance is from the coordinate ORIGIN: the caller centres its systems (no centre of mass is formed).
 * Stopping.  The step in which a condition is found is completed as usual -- corrector, caches, level, tick -- and the
 *   system then leaves the loop with its tick where it is, before the target.  reason is a bit mask: NBODY_BATCH_STOP_COLLISION
 *   (1) | NBODY_BATCH_STOP_ESCAPE (2).  nbody_batch_evolve_on returns NBODY_OK: a stop is a result, not an error.  Running
 *   out of max_steps keeps its NBODY_ERR_STATE, and counts unfinished systems only, never stopped ones.
 * Report per system (nbody_batch_stop_read; for a system that has not stopped every value is 0):
 *   reason; tick of the stop, in the units of the nbody_batch_evolve_on call that found it; the colliding pair (i, j), i < j:
 *   the pair of smallest r2 at the evaluation that found it, ties to the smallest i, then the smallest j; its separation,
 *   sqrtf of the fp32 chain fmaf(dz, dz, fmaf(dy, dy, dx dx)) without eps, at the positions of that evaluation; the escaping
 *   body: the smallest index that satisfies the test.  A stop for one reason only has -1 for the other's indices (pair or
 *   escaper) and separation 0.
 * After a stop the system is frozen: later nbody_batch_evolve_on calls leave its state, caches and report alone and give
 *   steps 0, ticks 0 for it in nbody_batch_evolve_stats.  The stop is forgotten with the caches (new counts, another
 *   softening, other buffers, another integrator, nbody_batch_invalidate_forces), by nbody_batch_step_n_* and by a new
 *   nbody_batch_stop_set; nbody_batch_stop_set also forgets the caches, so that the next nbody_batch_evolve_on starts with
 *   an evaluation, which examines the conditions.  Merging the colliding bodies and carrying the run on is the collision
 *   action MERGE of nbody_batch_merge.h, per-body radii in place of R_c are nbody_batch_radii.h.  A centre-of-mass escape
 *   test is out of scope.
 * No conditions set (the default, NULL, or both radii 0): nbody_batch_evolve_on is what it is without this header, bit
 *   for bit, the same kernels.  Conditions that never trigger change no bit of any state.  Reports and stopped states are
 *   functions of the system alone: not of its slot, B, max_bodies, the other systems or nbody_batch_evolve_launch_steps.
 * nbody_batch_stop_set: negative or non-finite radii are refused with NBODY_ERR_INVALID before any device work; an
 *   integrator other than NBODY_INTEGRATOR_HERMITE is refused by the nbody_batch_evolve_on that follows.
 * nbody_batch_stop_read: arrays of n_systems values, NULL arrays are skipped; synchronous.  nbody_batch_stop_count: how many
 *   systems have stopped. */
#ifndef NBODY_AMD_BATCH_STOP_H
#define NBODY_AMD_BATCH_STOP_H

#define NBODY_BATCH_STOP_COLLISION 1
#define NBODY_BATCH_STOP_ESCAPE 2

typedef struct nbody_batch_stop_config {
    float collision_radius; /* R_c; 0: off */
    float escape_radius;    /* R_e, from the coordinate origin; 0: off */
} nbody_batch_stop_config;

int nbody_batch_stop_set(nbody_batch *b, const nbody_batch_stop_config *cfg);
int nbody_batch_stop_read(nbody_batch *b, int *reason, int64_t *tick, int *pair_i, int *pair_j, float *separation, int *escaper);
int nbody_batch_stop_count(nbody_batch *b, int64_t *stopped);

#endif /* NBODY_AMD_BATCH_STOP_H */
