/* nbody_batch_radii.h -- per-body collision radii for Hermite batches: with radii set, two bodies collide when they come
 * within the sum of their own radii, not within one collision_radius shared by the batch, and a merged body grows.
 * Included by nbody.h (inside its extern "C") after nbody_batch_merge.h; additive to ABI version 5, no new status.
 *
 * Radii.  One fp32 radius R >= 0 per slot, n_systems x max_bodies floats laid out like the positions (system s at
 *   s * max_bodies).  The handle owns a device copy: nbody_batch_radii_set uploads it (NULL switches radii off) and
 *   nbody_batch_radii_read downloads it as the library left it (synchronous; NBODY_ERR_STATE with a message when no radii
 *   are set).  A negative or non-finite radius in a slot below that system's count is refused with NBODY_ERR_INVALID and a
 *   message naming the system and the slot, before any device work; slots beyond the count are copied verbatim and never
 *   examined.  nbody_batch_radii_set forgets stops, the merge log and the caches, exactly as nbody_batch_stop_set does.
 *   Radii are a property of the slots: new states, new counts and nbody_batch_invalidate_forces leave them alone, and a
 *   caller who loads new bodies after mergers sets radii again.  The values are checked against the counts of the moment
 *   only: a caller who raises a count sets radii again, or has given the slots it brings in valid radii beforehand.
 * Detection.  With radii set the pair (i, j), i != j, collides when the evaluation's own fp32 r2 = d.d + eps^2 (its FMA
 *   chain, the value before the zero-distance guard) satisfies r2 <= fmaf(S, S, eps^2) with S = R_i + R_j, one fp32 add.
 *   It is examined at every evaluation, where nbody_batch_stop.h's rule is: each step's at the predicted positions, the
 *   initial one, and the restart after a merger.  A coincident pair with zero radii collides, with eps = 0 too.
 *   Radii replace collision_radius: with radii set collisions are watched whether or not a collision radius is, and an
 *   nbody_batch_evolve_on call with radii set and collision_radius > 0 is refused with NBODY_ERR_INVALID ("radii and
 *   collision_radius are both set").  escape_radius and on_collision keep their meaning; MERGE acts while
 *   collision_radius > 0 or radii are set.  An integrator other than NBODY_INTEGRATOR_HERMITE is refused by the
 *   nbody_batch_evolve_on that follows, as for stops.  nbody_batch_step_n_* ignores radii, as it ignores stops.
 * Pair.  Among the pairs that satisfy their own threshold at the evaluation that found the collision, the pair of smallest
 *   r2, i < j, ties to the smallest i, then the smallest j: the stop report's key and minimum with a threshold per pair.
 *   It need not be the closest pair of the system: a closer pair of small bodies that do not touch is passed over.  The
 *   separation of the report and the merge event keep their definitions.
 * Merger (action MERGE).  Everything in nbody_batch_merge.h holds, and:
 *   radius    the survivor's becomes cbrt(R_i R_i R_i + R_j R_j R_j): volumes add.  Formed in fp64 from the fp32 operands
 *             and rounded once to fp32;
 *   slots     the radii of slots j and n - 1 swap with their bodies, so the absorbed body's radius lies with its last state
 *             in the first slot beyond the count;
 *   restart   the restart evaluation examines collisions with the new radii: a body that has grown can swallow a neighbour
 *             at the same tick.
 *   nbody_batch_merge_event stays as it is; the radii are read with nbody_batch_radii_read.
 * Without radii every entry point is what it is without this header, bit for bit, through the same kernels.  Radii that
 *   never trigger change no bit of any state.  States, counts, radii, reports and logs are functions of the system alone:
 *   not of its slot, B, max_bodies, the other systems or nbody_batch_evolve_launch_steps; evolve(a) followed by evolve(b) is
 *   evolve(a + b) bit for bit.
 * Out of scope: other mass-radius laws, fragmentation, radii in nbody_batch_step_n_*, a radius column in the merge log. */
#ifndef NBODY_AMD_BATCH_RADII_H
#define NBODY_AMD_BATCH_RADII_H

int nbody_batch_radii_set(nbody_batch *b, const float *host_radii);
int nbody_batch_radii_read(nbody_batch *b, float *host_radii);

#endif /* NBODY_AMD_BATCH_RADII_H */
