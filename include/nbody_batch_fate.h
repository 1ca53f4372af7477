/* nbody_batch_fate.h -- tracer fates for Hermite batches: test particles (nbody_batch_massive.h) together with the stopping
 * conditions (nbody_batch_stop.h) and per-body radii (nbody_batch_radii.h).  A test particle that touches a massive body or
 * leaves the escape radius is removed from its system -- frozen where it is, with a fate: why, when, which massive body, how
 * close, how fast -- and the system carries on inside the same launch.  Which planetesimals fell onto which planet, which
 * were ejected, which are still in orbit.  Included by nbody.h (inside its extern "C") after nbody_batch_massive.h; additive
 * to ABI version 5, no new status.
 *
 * Opting in.  nbody_batch_fate_set takes cfg->action: NBODY_BATCH_TRACERS_REFUSE (0, the default; NULL selects it too) or
 *   NBODY_BATCH_TRACERS_REMOVE (1).  Any other value, or a NULL handle, is refused with NBODY_ERR_INVALID and a message
 *   before any device work; a refused call changes nothing.  With REFUSE every entry point does exactly what it does without
 *   this header: the same refusals with the same messages, the same kernels, no bit and no launch changed.
 *   nbody_batch_fate_set forgets what nbody_batch_stop_set forgets: the stops, the fates and the cached accelerations and
 *   jerks.  The first REMOVE allocates the fate arrays, which the handle owns.
 * When it acts.  REMOVE acts in nbody_batch_evolve_on while massive counts are set and at least one of a collision radius,
 *   radii or an escape radius is.  The collision action MERGE together with massive counts stays refused (NBODY_ERR_INVALID
 *   with a message that says so) while a collision radius or radii are set; a collision radius and radii together stay
 *   refused as nbody_batch_radii.h says.  Without massive counts REMOVE changes nothing: the same kernels, the same bits.
 *   With massive counts and no condition nbody_batch_evolve_on is nbody_batch_massive.h's.  nbody_batch_step_n_* ignores
 *   the conditions, as it does without this header.
 * Collision.  Examined at every acceleration-and-jerk evaluation, as in nbody_batch_stop.h: each step's at the predicted
 *   positions, the initial one at the current positions.  The value compared is the evaluation's own fp32
 *   r2 = d.d + eps^2 (its FMA chain, nbody.h), before the zero-distance guard; the threshold is fmaf(R_c, R_c, eps^2), or with
 *   radii fmaf(S, S, eps^2), S = R_i + R_j (a test particle's radius counts).  Only pairs the evaluation forms are judged,
 *   with m the system's massive count: massive-massive, i, j < m, i != j; tracer-massive, i >= m, j < m.  Two tracers
 *   never collide: the pair is never formed, so coincident tracers stay finite with eps = 0 too.  One kernel serves both kinds
 *   of radius: a shared R_c rides as the radius R_c / 2 of every body, whose fp32 sum is R_c exactly.
 * Escape.  Examined on the corrected positions after every step, and on the current ones at the initial evaluation:
 *   fmaf(z, z, fmaf(y, y, x x)) > R_e R_e, all fp32, from the coordinate origin.
 * A massive-massive collision or a massive escaper stops the system exactly as nbody_batch_stop.h says, and
 *   nbody_batch_stop_read reports it: the pair is the closest touching pair among the massive bodies (with radii, among the
 *   pairs within their own threshold), the escaper the smallest massive index; both name massive bodies only.  Tracers found
 *   in that same step still receive their fates.  The stopped system is frozen, tracers included.
 * A tracer that hits or escapes.  The step in which it is found is completed for it -- corrector and state write.  From
 *   then on it is dead: its position, velocity, mass word and w stay bit for bit through later steps and later
 *   nbody_batch_evolve_on calls; it is not predicted, corrected, examined or counted in the time-step criterion.  It does not
 *   vote in the step that found it.  Found at the initial evaluation, it does not vote in the first-step rule and its state
 *   is untouched.  A tracer that meets both conditions in one step has fate HIT.  Body counts do not change and nothing moves
 *   between slots; the live bodies of the system go on to the target tick.  Removing a tracer changes no bit of any other
 *   body beyond its missing vote: it was a column for nobody.
 * Fate report per body.  nbody_batch_fate_read fills arrays of n_systems * max_bodies values, laid out like the positions;
 *   NULL arrays are skipped; synchronous.  fate: NBODY_BATCH_FATE_ALIVE 0, NBODY_BATCH_FATE_HIT 1, NBODY_BATCH_FATE_ESCAPED 2.
 *   tick: defined as the tick of a stop is in nbody_batch_stop.h -- after the step that found it, the start tick at the
 *   initial evaluation, in the units of the nbody_batch_evolve_on call that found it.  target: the massive body hit, the
 *   one of smallest r2 among those within the threshold at that evaluation, ties to the smallest index; -1 for an escape.
 *   separation: sqrtf of the fp32 chain fmaf(dz, dz, fmaf(dy, dy, dx dx)) without eps, at that evaluation's positions.
 *   relative_speed: the same chain on the velocity difference of that evaluation.  Both are 0 for an escape.  Massive
 *   bodies, live tracers and slots beyond a system's count read 0, 0, -1, 0, 0.  nbody_batch_fate_count gives per-system
 *   totals (n_systems values each; NULL arrays are skipped).  With REFUSE both return NBODY_ERR_STATE with a message.
 * Forgetting.  The fates are zeroed exactly where the stops are forgotten: with the caches (new counts, another softening,
 *   other buffers, another integrator, nbody_batch_invalidate_forces), by nbody_batch_step_n_*, nbody_batch_stop_set,
 *   nbody_batch_merge_set, nbody_batch_radii_set, nbody_batch_massive_set and nbody_batch_fate_set.  The tracers are alive
 *   again after that, and are examined anew by the next call's initial evaluation.  evolve(a) followed by evolve(b) is
 *   evolve(a + b), states and fates included; the tick of a fate the second call finds counts from that call's start.
 * Invariances.  Fates and states are functions of the system alone: not of its slot, B, max_bodies, the other systems or
 *   nbody_batch_evolve_launch_steps.  Conditions that never trigger change no bit of the run nbody_batch_massive.h describes.
 * Diagnostics.  nbody_batch_energy and nbody_batch_momentum keep reading every body, dead tracers included.
 * Out of scope: stopping a system at the first tracer event; merging a tracer's mass word into the body it hits; mergers
 *   among massive bodies while massive counts are set; compacting dead tracers out of the rows -- a dead row still rides
 *   through the column loop and its result is discarded, so removal saves no time; a centre-of-mass escape test. */
#ifndef NBODY_AMD_BATCH_FATE_H
#define NBODY_AMD_BATCH_FATE_H

#define NBODY_BATCH_TRACERS_REFUSE 0
#define NBODY_BATCH_TRACERS_REMOVE 1

#define NBODY_BATCH_FATE_ALIVE 0
#define NBODY_BATCH_FATE_HIT 1
#define NBODY_BATCH_FATE_ESCAPED 2

typedef struct nbody_batch_fate_config {
    int action; /* NBODY_BATCH_TRACERS_REFUSE or NBODY_BATCH_TRACERS_REMOVE */
} nbody_batch_fate_config;

int nbody_batch_fate_set(nbody_batch *b, const nbody_batch_fate_config *cfg);
int nbody_batch_fate_read(nbody_batch *b, int *fate, int64_t *tick, int *target, float *separation, float *relative_speed);
int nbody_batch_fate_count(nbody_batch *b, int64_t *hit, int64_t *escaped);

#endif /* NBODY_AMD_BATCH_FATE_H */
