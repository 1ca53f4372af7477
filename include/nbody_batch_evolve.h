/* nbody_batch_evolve.h -- adaptive shared time steps for Hermite batches: evolve every system of a nbody_batch to a common
 * time, each system on its own step.  Included by nbody.h (inside its extern "C"); additive to ABI version 5, no new status.
 *
 * Each system carries ONE step, shared by its bodies (block steps per system; individual per-body steps stay out of
 * scope), and advances independently of the others to the common end time.
 * Time axis: a call advances every system by n_intervals x dt_max.  A system's step is h = dt_max 2^-L with its level L in
 *   [0, levels], levels <= NBODY_BATCH_EVOLVE_MAX_LEVELS; h is formed in fp64 from the fp32 dt_max, so it is exact.  Time is
 *   an integer tick count per system in units of dt_max 2^-levels (a step at level L is 2^(levels - L) ticks), never a float
 *   sum: every system lands on the end time exactly, and between calls it sits on a multiple of dt_max.
 * Step: one step is exactly NBODY_INTEGRATOR_HERMITE's predict-evaluate-correct step (nbody.h) with that h: the same
 *   arithmetic and summation order, so levels = 0 is nbody_batch_step_n_on(n_intervals, dt_max) bit for bit.
 * Criterion: after the corrector each body forms, in fp64 from the fp32 a0, j0 (start of the step just taken) and a1, j1
 *   (its end), per component
 *     a2_0 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2 ;  a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3 ;  a2_1 = a2_0 + h a3
 *   and Aarseth's  dt_i^2 = eta (|a1| |a2_1| + |j1|^2) / (|j1| |a3| + |a2_1|^2),  a zero denominator counting as +inf
 *   (|a1| |a2_1| = sqrt(|a1|^2 |a2_1|^2), likewise |j1| |a3|).  Squares are compared: no root of dt_i^2 is taken, and
 *   nothing is divided -- a step of square h^2 is too long for a body when h^2 x denominator > numerator.  The system's
 *   request is the minimum over its bodies; the level rule below is monotone in it, so the kernel takes the largest level
 *   any body asks for, an integer maximum -- exact and independent of order like the minimum, so the batch's bit-for-bit
 *   invariances (slot, B, max_bodies, neighbours) hold for evolve as for step_n.
 *   The criterion reads differences of fp32 accelerations divided by h^2 and h^3: for systems of a thousand bodies and
 *   more and a dt_max far below their dynamical step, the fp32 summation error of the accelerations shows in it as
 *   structure and the systems take more (shorter) steps than an fp64 evaluation would ask for; accuracy does not suffer.
 * Level rule: L* = the smallest level with (dt_max 2^-L*)^2 <= request, at most `levels`; a step still longer than the
 *   request at L* = levels counts as clamped.  L* > L: refine to L* at once.  L* < L: coarsen by ONE level, and only when
 *   the system's tick is a multiple of the coarser step (the block-step commensurability rule: interval boundaries are
 *   always hit).
 * First step: without a level (below) the step comes from dt_i = eta_start |a| / |j| of the evaluation at the current
 *   state (|j| = 0: +inf), minimised over the bodies, by the same L* rule.
 * Persistence: the per-system level lives in the handle beside the acceleration and jerk caches and is forgotten with
 *   them (new counts, another softening, other buffers, another integrator, nbody_batch_invalidate_forces); a
 *   nbody_batch_step_n_* call, another dt_max or another `levels` forget the level alone.  So evolve(a) then evolve(b)
 *   is evolve(a + b) bit for bit.  While a call that ran out of steps waits to be resumed (below), Hermite
 *   nbody_batch_step_n_* is refused with NBODY_ERR_STATE.
 * Kernel: batch_hermite_adaptive_kernel, one workgroup per system, NBODY_INTEGRATOR_HERMITE's layout and LDS plus a few
 *   words for the waves' levels (a wave-wide vote per level, then a maximum over the waves' words; no barrier is added).
 *   Registers hold the accelerations and jerks; positions and velocities stay in the state arrays between the steps, read
 *   by the predictor and the corrector and written back by the corrector, the same fp32 bits.  A workgroup loops until
 *   its system reaches the target tick or a per-launch step budget (nbody_batch_evolve_launch_steps, default 128, at
 *   most 4096) is spent; the host relaunches while any system is unfinished.
 *   The state crosses launches as the same fp32 bits and integers: the budget changes no bit.
 * max_steps bounds every system's steps per call (<= 0: NBODY_BATCH_EVOLVE_DEFAULT_MAX_STEPS), so no launch is unbounded.
 *   If a system runs out: NBODY_ERR_STATE, the message names the first unfinished system and how many are unfinished; the
 *   state is consistent at the ticks nbody_batch_evolve_stats reports, and the next nbody_batch_evolve_on with the same
 *   dt_max and levels resumes: its n_intervals counts from the start of the interrupted call (the same n_intervals
 *   completes it, bit for bit what one unbounded call gives).  Forgetting the caches drops the interrupted call.
 * Refused before any device work (NBODY_ERR_INVALID with a message): NULL arguments, an integrator other than
 *   NBODY_INTEGRATOR_HERMITE, n_intervals < 0 or n_intervals x 2^levels >= 2^62, dt_max, eta or eta_start not finite or
 *   not positive, levels outside [0, 20], the softening rule of nbody_step.
 * nbody_batch_evolve_on returns with the work complete.  nbody_batch_evolve_stats: n_systems values each for the last
 *   call (NULL arrays are skipped): steps taken, lowest and highest level stepped at (0 and 0 when no step was taken),
 *   clamped steps, and the tick reached (the target n_intervals x 2^levels when finished; systems of count 0 report it too). */
#ifndef NBODY_AMD_BATCH_EVOLVE_H
#define NBODY_AMD_BATCH_EVOLVE_H

#define NBODY_BATCH_EVOLVE_MAX_LEVELS 20
#define NBODY_BATCH_EVOLVE_DEFAULT_MAX_STEPS 1048576

typedef struct nbody_batch_evolve_config {
    float dt_max;    /* the interval, and the longest step */
    int levels;      /* shortest step dt_max 2^-levels */
    float eta;       /* accuracy parameter of the criterion (0.01 .. 0.02 is customary) */
    float eta_start; /* of the first step */
    float softening;
    int max_steps;   /* per system and call; <= 0: the default */
} nbody_batch_evolve_config;

int nbody_batch_evolve_on(nbody_batch *b, float *d_positions_xyzm, float *d_velocities_xyzw, int64_t n_intervals,
                          const nbody_batch_evolve_config *cfg);
int nbody_batch_evolve_stats(nbody_batch *b, int64_t *steps, int *min_level, int *max_level, int64_t *clamped, int64_t *ticks);
int nbody_batch_evolve_launch_steps(nbody_batch *b, int steps_per_launch); /* in [1, 4096]; results do not depend on it */

#endif /* NBODY_AMD_BATCH_EVOLVE_H */
