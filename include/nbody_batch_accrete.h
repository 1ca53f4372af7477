/* nbody_batch_accrete.h -- accreting tracers for Hermite batches: with the hit action ACCRETE a test particle that hits a
 * massive body (nbody_batch_fate.h) gives its mass word to that body, which grows, and the system is evaluated afresh and
 * carries on.  How the planets grow from the disc.  Included by nbody.h (inside its extern "C") after nbody_batch_fate.h;
 * additive to ABI version 5, no new status.
 *
 * Opting in.  nbody_batch_accrete_set takes cfg->on_hit: NBODY_BATCH_ON_HIT_REMOVE (0, the default; NULL selects it too) or
 *   NBODY_BATCH_ON_HIT_ACCRETE (1).  Any other value, or a NULL handle, is refused with NBODY_ERR_INVALID and a message
 *   ("unknown hit action") before any device work; a refused call changes nothing.  nbody_batch_accrete_set forgets what
 *   nbody_batch_stop_set forgets.  The first ACCRETE allocates the report arrays, which the handle owns.  With REMOVE every
 *   entry point is what it is without this header: the same kernels, the same bits, the same refusals and messages.  The
 *   tracer actions stay nbody_batch_fate.h's two: this is a setting of its own.
 * When it acts.  In nbody_batch_evolve_on, and only where fates act and collisions are watched: massive counts set, the
 *   tracer action REMOVE, and a collision radius or radii.  With an escape radius alone, or without massive counts, ACCRETE
 *   changes nothing: the same kernel, the same bits.  The collision action MERGE together with massive counts stays refused
 *   as nbody_batch_fate.h says, and every other refusal is unchanged.
 * Accretion follows an evaluation -- a step's, the initial one, a restart's -- that gave at least one tracer the fate HIT and
 *   did not stop the system.  The step is completed as nbody_batch_fate.h says, corrector and state write, for the tracer
 *   too, and its fate is recorded as there.  Then the tracers hit at that evaluation are processed in ascending index i, each
 *   seeing the state as the one before left it.  m_i is the tracer's mass word.  m_i == 0 (either sign): nothing happens,
 *   the tracer is REMOVE's bit for bit.  Otherwise a merger onto t, the fate's target, on the corrected state (on the current
 *   state at the initial and the restart evaluations), by nbody_batch_merge.h's arithmetic with t the survivor and the
 *   tracer the absorbed body:
 *   mass      m_t + m_i, formed in fp32;
 *   x, v      per component in fp64 from the fp32 operands, fma(m_i, u_i, m_t u_t) / (m_t + m_i), the sum of the masses formed
 *             in fp64 and the result rounded once to fp32; the arithmetic mean (u_t + u_i) / 2 when m_t + m_i == 0;
 *   t         keeps its slot and its vel.w;
 *   radius    with radii set R_t becomes cbrt(R_t^3 + R_i^3), nbody_batch_radii.h's rule: fp64, rounded once.  With a shared
 *             collision radius nothing grows;
 *   tracer    stays in its slot; position, velocity and w stay as the completed step wrote them; its mass word becomes
 *             +0.0f; given[i] = m_i, and the system's accretions go up by one.
 *   Counts and massive counts do not change and nothing moves between slots, so the target of a fate stays meaningful.
 *   Mass words are not validated: a non-finite one propagates by the arithmetic above.
 * Restart.  When at least one mass moved, the accelerations and jerks are evaluated afresh at the current state for every
 *   live row (dead rows ride and their results are dropped), as the "Restart" paragraph of nbody_batch_merge.h says: not a
 *   step.  This evaluation examines collisions and escapes as the initial one does, with the new radii.  A tracer found
 *   there receives its fate with the current tick and, when it hit, is accreted at once, followed by another restart: a
 *   grown planet can swallow a neighbour at the same tick.  A collision among the massive bodies or a massive escaper found
 *   there stops the system as at the initial evaluation.  The level is L = min(levels, max(L*, L_tick)), L* from the
 *   first-step rule over the live rows only, L_tick the smallest level whose step divides the tick; L* > levels counts as
 *   clamped.  When no mass moved nothing else happens: the run is REMOVE's bit for bit.
 * A step that stops the system (a collision among the massive bodies, a massive escaper) accretes nothing: its tracers
 *   receive their fates as nbody_batch_fate.h says, given stays 0, no mass word changes, and the system is frozen as that
 *   step left it.
 * Report.  nbody_batch_accrete_read fills given, n_systems * max_bodies values laid out like the positions -- the mass each
 *   tracer gave, 0 elsewhere -- and accretions, n_systems values; NULL arrays are skipped; synchronous.  With REMOVE it
 *   returns NBODY_ERR_STATE with a message.  Both arrays are zeroed exactly where the fates are zeroed.  Mass that has moved
 *   stays moved, because the state is the caller's: a tracer that is forgotten and so alive again has a zero mass word.
 * Invariances, as for fates.  States, fates, given and accretions are functions of the system alone: not of its slot, B,
 *   max_bodies, the other systems or nbody_batch_evolve_launch_steps; evolve(a) followed by evolve(b) is evolve(a + b) bit
 *   for bit.  nbody_batch_energy and nbody_batch_momentum keep reading every body; since the mass word moved, the total mass
 *   is preserved up to the fp32 rounding of each sum.
 * Out of scope: mergers among massive bodies while massive counts are set; accretion in nbody_batch_step_n_*; stopping a
 *   system at the first accretion; fragmentation; a log of accretion events beyond the fates and given. */
#ifndef NBODY_AMD_BATCH_ACCRETE_H
#define NBODY_AMD_BATCH_ACCRETE_H

#define NBODY_BATCH_ON_HIT_REMOVE 0
#define NBODY_BATCH_ON_HIT_ACCRETE 1

typedef struct nbody_batch_accrete_config {
    int on_hit; /* NBODY_BATCH_ON_HIT_REMOVE or NBODY_BATCH_ON_HIT_ACCRETE */
} nbody_batch_accrete_config;

int nbody_batch_accrete_set(nbody_batch *b, const nbody_batch_accrete_config *cfg);
int nbody_batch_accrete_read(nbody_batch *b, float *given, int64_t *accretions);

#endif /* NBODY_AMD_BATCH_ACCRETE_H */
