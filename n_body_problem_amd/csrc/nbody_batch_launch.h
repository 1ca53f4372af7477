// nbody_batch_launch.h -- what crosses between the integrators' kernels (nbody_batch.hip) and the host code behind their C ABI
// (nbody_batch_capi.hip): what the launches of a call share, the structs the kernels take by value, and the three entry points.
// The launchers of the single families stay private to nbody_batch.hip.  Internal: nothing here crosses the C ABI.
#pragma once

#include "nbody_batch_handle.h"

#pragma GCC visibility push(hidden)

namespace nbody {

// What the launches of a call share: the choice, the systems, the stream, the caller's state and the handle's arrays (those a
// family does not read may be null).
struct BatchLaunch {
    BatchChoice choice;
    int n_systems, max_bodies;
    hipStream_t stream;
    float4 *pos, *vel, *acc, *jerk;
    int *counts;
    const int *massive;
    BatchEvolveState *state;
    int *counters;
    BatchStopReport *report;
    const BatchFieldTerm *field;  // nbody_batch_field.h: [n_systems][4], null while no field is set
};

// ---- kernel arguments, by value: members, order and types are the kernels' ---------------------------------------------------

struct BatchEvolveArgs {
    // dt_max and what every step needs of it, formed once on the host in fp64: a level only scales them by a power of two,
    // which is exact, so h / 3, 1 / h^2 ... are the values the division would give for h = dt_max 2^-L
    double dt, dt_half, dt_third, dt_sixth, dt_six;  // dt_max, dt_max / 2, dt_max / 3, dt_max / 6, 6 dt_max
    double dt2, inv_dt2, inv_dt3;                     // dt_max^2, 1 / dt_max^2, 1 / dt_max^3
    double eta, eta_start2;  // eta_start^2
    long long target, max_steps;
    float eps2;
    int levels, budget;  // steps per launch at most
    int have_acc, have_level;
    int new_call;    // first launch of a call: the call's counters start at 0
    int reset_tick;  // ... and the tick too (not when the call resumes one that ran out of steps)
};

// Stopping conditions (include/nbody_batch_stop.h) as the kernels take them, formed once on the host in fp32.
struct BatchStopArgs {
    float thr;  // a pair collides when its r^2 + eps^2 <= thr = fma(R_c, R_c, eps^2); -1: never
    float re2;  // a body has escaped when |x|^2 > re2 = R_e R_e; +inf: never
};

// Per launch: the systems' merger counts and logs (events: [n_systems][capacity], nullptr for capacity 0).
struct BatchMergeArgs {
    int *merges;
    nbody_batch_merge_event *events;
    int capacity;
};

// Per launch: the radii ([n_systems][max_bodies], laid out like the positions) and the collision action, workgroup-uniform.
struct BatchRadiiArgs {
    float *radii;
    int merge;  // NBODY_BATCH_ON_COLLISION_MERGE: merge the pair and carry on; otherwise stop and report
};

// Per launch.  One kernel serves both kinds of radius: a shared R_c rides as the radius R_c / 2 of every body, whose fp32 sum
// is R_c exactly, so the threshold is fmaf(R_c, R_c, eps^2) as nbody_batch_stop.h states it.  The fates (BatchFate,
// nbody_batch_handle.h) are laid out like the positions; all zero: alive.
struct BatchFateArgs {
    float *radii;        // [n_systems][max_bodies], or nullptr: every body has the radius half_rc (written by accretion only)
    float half_rc;
    int collide;         // a collision radius or radii are set (otherwise the column loop's masks are dropped)
    BatchFate *fates;    // one pointer: the kernel's scalar registers are all taken
};

// Per launch: the mass each tracer gave ([n_systems][max_bodies], laid out like the positions) and the systems' accretions.
struct BatchAccreteArgs {
    float *given;
    int *accretions;
};

// What one nbody_batch_evolve_on call hands its kernel; p's have_acc, have_level, new_call and reset_tick change per launch.
struct BatchEvolveLaunch {
    BatchEvolveArgs p;
    BatchStopArgs sa;
    BatchMergeArgs ma;
    BatchRadiiArgs ra;
    BatchFateArgs fa;
    BatchAccreteArgs aa;
};

// ---- the entry points (nbody_batch.hip) --------------------------------------------------------------------------------------

// One launch of nbody_batch_evolve_on by the chosen family.
hipError_t launch_batch_evolve(const BatchLaunch &l, const BatchEvolveLaunch &a);

// One launch of nbody_batch_step_n_async by the chosen family: `run` steps of every system.  Kick-drift keeps no accelerations.
hipError_t launch_batch_steps(const BatchLaunch &l, bool kdk, int run, float dt, float eps2, bool acc_valid);

// nbody_batch_field_potential's launch: Phi(x_i) of every slot from the components as set ([n_systems][n_components]) into phi.
hipError_t launch_batch_field_potential(const float4 *pos, const int *counts, const nbody_batch_field_component *comps,
                                        int n_components, int n_systems, int max_bodies, double *phi, hipStream_t stream);

}  // namespace nbody

#pragma GCC visibility pop
