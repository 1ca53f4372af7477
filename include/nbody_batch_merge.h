/* nbody_batch_merge.h -- mergers for Hermite batches: with the collision action MERGE, nbody_batch_evolve_on does not end the
 * run of a system whose bodies collide (nbody_batch_stop.h) but merges the colliding pair and carries the run on with the
 * merged body.  Included by nbody.h (inside its extern "C") after nbody_batch_stop.h; additive to ABI version 5, no new status.
 *
 * Action.  on_collision belongs to the stopping conditions: NBODY_BATCH_ON_COLLISION_STOP (0, the default) is
 *   nbody_batch_stop.h's behaviour; NBODY_BATCH_ON_COLLISION_MERGE (1) merges.  It acts only while collision_radius > 0.
 * Detection is nbody_batch_stop.h's rule, unchanged: r2 + eps^2 <= fmaf(R_c, R_c, eps^2) on the evaluation's own fp32 r2, at
 *   every evaluation, the initial one included.  The step in which a collision is found is completed as usual: corrector,
 *   caches, level, tick, step count.
 * The pair is the one the stop report would name: the pair of smallest r2 at the evaluation that found the collision,
 *   i < j, ties to the smallest i, then the smallest j.  One pair is merged per finding.
 * Merger, on the corrected state (on the current state when the initial evaluation found the collision):
 *   mass      m = m_i + m_j, formed in fp32;
 *   x, v      per component in fp64 from the fp32 operands, fma(m_j, u_j, m_i u_i) / (m_i + m_j), the sum of the masses
 *             formed in fp64 and the result rounded once to fp32; the arithmetic mean (u_i + u_j) / 2 when m_i + m_j == 0;
 *   survivor  keeps slot i and body i's vel.w;
 *   slots     bodies j and n - 1 swap slots, all four words of position and velocity (nothing moves when j == n - 1), and
 *             the count drops by one: the absorbed body's state before the merger lies in the first slot beyond the count.
 *             After k mergers of a system that began with n0 bodies, slots n0 - k .. n0 - 1 hold the absorbed bodies, the
 *             most recent first.  w travels with its body: a caller that stores ids in w keeps track of identities.
 * Restart.  After a merger the accelerations and jerks are evaluated afresh at the current state.  This evaluation is like
 *   the initial one: it is not a step, and it examines both conditions, collisions among the current positions and escapers
 *   among them.  The level comes from the first-step rule (eta_start |a| / |j|, the level L* of nbody_batch_evolve.h) but is
 *   never coarser than the tick allows: L = min(levels, max(L*, L_tick)), L_tick the smallest level whose step
 *   2^(levels - L) divides the system's tick, so that interval boundaries stay hit exactly; L* > levels counts as clamped.
 *   Another collision found there is merged at once (a clump resolves as a chain of mergers at one tick).  An escaper found
 *   there stops the system with reason NBODY_BATCH_STOP_ESCAPE and the indices after the merger.  A step that finds a
 *   collision and an escaper merges first; the escape is then judged by the restart evaluation alone.
 *   Under MERGE the collision bit is never set in reason.  An escape found in a step without a collision stops the system
 *   as without this header.  A system merged down to one body coasts to the target (a = j = 0, the request is +inf).
 * Counts.  The device counts change; nbody_batch_evolve_on refreshes the handle's host copy before it returns, also when it
 *   returns NBODY_ERR_STATE for max_steps, and nbody_batch_get_counts reads it.  Later nbody_batch_step_n_*, _energy,
 *   _momentum and _evolve_on calls see the new counts.  The library's own change of a count does not forget the caches: the
 *   restart has refilled them.
 * Log per system: the number of mergers, and the first log_capacity of them as events (later mergers are performed and
 *   counted, not logged): the tick, in the units of the nbody_batch_evolve_on call that found it; the survivor's index; the
 *   absorbed body's index before the swap; the body count before the merger; the separation, by the stop report's
 *   definition, at the evaluation that found it; the relative speed sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex ex))), e = v_j - v_i
 *   in fp32, at the state merged; the two masses before.  The log accumulates across nbody_batch_evolve_on calls and is
 *   forgotten exactly where stops are forgotten.
 * nbody_batch_merge_set: NULL switches merging off (the action STOP).  It forgets stops, the log and the caches, as
 *   nbody_batch_stop_set does; an unknown action or a log_capacity outside [0, NBODY_BATCH_MAX_BODIES - 1] is refused with
 *   NBODY_ERR_INVALID before any device work.
 * nbody_batch_merge_read: n_merges has n_systems values, events n_systems x log_capacity (system s at events + s
 *   log_capacity; entries from its merger count on are zero); NULL arrays are skipped; synchronous.
 * With the action STOP, or MERGE and collision_radius == 0, nbody_batch_evolve_on is what it is without this header, bit for
 *   bit, the same kernels.  With MERGE and a radius that never triggers no bit of any state differs from the plain call.
 *   States, counts and logs are functions of the system alone: not of its slot, B, max_bodies, the other systems or
 *   nbody_batch_evolve_launch_steps; evolve(a) followed by evolve(b) is evolve(a + b) bit for bit, mergers included.
 * Per-body radii, and the merged body's, are nbody_batch_radii.h.  Out of scope: fragmentation or any outcome other than
 *   perfect merging, mergers in nbody_batch_step_n_*. */
#ifndef NBODY_AMD_BATCH_MERGE_H
#define NBODY_AMD_BATCH_MERGE_H

#define NBODY_BATCH_ON_COLLISION_STOP 0
#define NBODY_BATCH_ON_COLLISION_MERGE 1

typedef struct nbody_batch_merge_config {
    int on_collision; /* NBODY_BATCH_ON_COLLISION_* */
    int log_capacity; /* events kept per system, [0, NBODY_BATCH_MAX_BODIES - 1] */
} nbody_batch_merge_config;

typedef struct nbody_batch_merge_event {
    int64_t tick;
    int survivor;     /* i */
    int absorbed;     /* j, before the swap */
    int count_before; /* bodies before the merger */
    float separation;
    float relative_speed;
    float mass_survivor; /* m_i and m_j before */
    float mass_absorbed;
    int reserved;
} nbody_batch_merge_event;

int nbody_batch_merge_set(nbody_batch *b, const nbody_batch_merge_config *cfg);
int nbody_batch_merge_read(nbody_batch *b, int64_t *n_merges, nbody_batch_merge_event *events);
int nbody_batch_get_counts(nbody_batch *b, int64_t *counts);

#endif /* NBODY_AMD_BATCH_MERGE_H */
