// nbody_batch_handle.h -- the handle of a batched ensemble (include/nbody.h, nbody_batch_*), as the three sources behind it see
// it: nbody_batch.hip (the integrators' kernels and launchers), nbody_batch_capi.hip (the host code behind the integrators' C
// ABI: their settings and records) and nbody_batch_analysis.hip (the kernels that read a state and write only records of their
// own, and their calls).  Internal: nothing here crosses the C ABI.
//
// Ownership: every device array is a DeviceArray (nbody_device_owned.h), which frees itself.  What the integrators keep lives in
// the handle, allocated by nbody_batch_create, a setter or the first evolve, and freed when nbody_batch_destroy deletes it.  What the analysis
// calls keep lives in one BatchAnalysis behind `analysis`, created by the first analysis call and freed by
// batch_analysis_destroy; no integrator reads it and no analysis call writes anything else.
#pragma once

#include "../../include/nbody.h"
#include "nbody_batch_choice.h"
#include "nbody_device_owned.h"

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>

// Internal to the library: the names below are not exported, so its dynamic symbols stay those of the C ABI.
#pragma GCC visibility push(hidden)

namespace nbody {

// Steps per launch at most: a long k is cut into launches of this many steps.  The state goes through HBM between them as
// the same fp32 bits (the KDK accelerations through the handle's cache), so the cut changes nothing.
constexpr int kBatchStepsPerLaunch = 128;

// nbody_batch_energy, nbody_batch_momentum: per system {kinetic, potential, px, py, pz, mass}
constexpr int kDiagValues = 6;

// The batch kernels are instantiated for <RPL, GUARD>: rows per lane and the eps = 0 guard (nbody_batch_choice.h chooses
// them, and which family runs).  with_shape is the one place that turns the two numbers into template arguments:
// f(integral_constant<int, RPL>, bool_constant<GUARD>).
template <class F>
hipError_t with_shape(int rpl, bool guard, F &&f)
{
    switch (rpl * 2 + (guard ? 1 : 0)) {
    case 2: return f(std::integral_constant<int, 1>{}, std::bool_constant<false>{});
    case 3: return f(std::integral_constant<int, 1>{}, std::bool_constant<true>{});
    case 4: return f(std::integral_constant<int, 2>{}, std::bool_constant<false>{});
    case 5: return f(std::integral_constant<int, 2>{}, std::bool_constant<true>{});
    case 8: return f(std::integral_constant<int, 4>{}, std::bool_constant<false>{});
    default: return f(std::integral_constant<int, 4>{}, std::bool_constant<true>{});
    }
}

// Per system, in HBM between launches and calls of nbody_batch_evolve_on (the adaptive Hermite families of nbody_batch.hip).
// steps, clamped, min_level and max_level are those of the current call.
struct BatchEvolveState {
    long long tick;  // in units of dt_max 2^-levels, from the start of the call
    long long steps, clamped;
    int level, min_level, max_level, pad;
};
constexpr int kEvolveNoLevel = 1 << 30;
// A system that has not stepped in this call, at tick 0.
constexpr BatchEvolveState kEvolveStateFresh{0, 0, 0, 0, kEvolveNoLevel, -1, 0};

// Per system, beside BatchEvolveState: what a stopping condition found (include/nbody_batch_stop.h).  All zero: the system
// has not stopped.  A system whose reason is set is frozen: later launches leave it alone.
struct BatchStopReport {
    long long tick;  // of the stop, in the units of the call that found it
    int reason;      // kStopCollision | kStopEscape
    int pair_i, pair_j, escaper;  // -1: not that reason
    float separation;
    int pad;
};
constexpr BatchStopReport kNotStopped{0, 0, 0, 0, 0, 0.f, 0};

// Per slot: what became of a test particle (include/nbody_batch_fate.h).  All zero: alive.
struct BatchFate {
    long long tick;
    int fate;  // kFateHit, kFateEscaped; 0: alive
    int target;
    float separation, speed;
};

// One component of the external field as the kernels take it, formed by nbody_batch_field_set on the host in fp32 (the header's
// "once per nbody_batch_field_set"): PLUMMER {M, b b, -}, LOG_HALO {v0 v0, rc rc, 1 / (q q)}, MIYAMOTO_NAGAI {M, a, b b}.
struct BatchFieldTerm {
    int kind;
    float c0, c1, c2;
};

struct BatchAnalysis;  // nbody_batch_analysis.hip

// Frees what the analysis calls keep; nothing to do while none was made.  nbody_batch_destroy calls it with the device set and
// the stream idle.
void batch_analysis_destroy(nbody_batch *b);

// The message of a failed call, kept in the handle or, without one, per thread for nbody_batch_last_error(NULL); returns status.
int bfail(nbody_batch *b, int status, const std::string &msg);

}  // namespace nbody

#pragma GCC visibility pop

#define BATCH_TRY(b, call)                                                                                 \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return nbody::bfail((b), e_ == hipErrorOutOfMemory ? NBODY_ERR_ALLOC : NBODY_ERR_DEVICE,       \
                                std::string(#call) + ": " + hipGetErrorString(e_));                        \
    } while (0)

struct nbody_batch {
    int device = 0;
    int64_t n_systems = 0, max_bodies = 0;
    std::vector<int> counts;      // host copy of the per-system body counts
    nbody::DeviceArray<int> counts_dev;  // [n_systems]
    // what picks the kernels (nbody_batch_choice.h): the integrator, whether massive counts and radii are set, the stopping
    // conditions, the collision action and the tracer action, each written by its setter
    nbody::BatchConfig config;
    nbody::DeviceArray<float4> acc;   // KDK, Hermite: [n_systems][max_bodies] accelerations at the current state (slots < n_b)
    nbody::DeviceArray<float4> jerk;  // Hermite: [n_systems][max_bodies] jerks at the current state, allocated on first use
    bool acc_valid = false;
    int acc_integrator = -1;      // the integrator that filled the cache
    const void *acc_pos = nullptr, *acc_vel = nullptr;  // the buffers and softening the cache belongs to
    float acc_softening = 0.f;
    // nbody_batch_evolve_on: the per-system level and tick beside the caches, valid only while acc_valid
    nbody::DeviceArray<nbody::BatchEvolveState> evolve_state;  // [n_systems]
    nbody::DeviceArray<int> evolve_counters;          // {unfinished, unfinished and out of steps} of the last launch
    std::vector<nbody::BatchEvolveState> evolve_host; // the last call's, for nbody_batch_evolve_stats
    int64_t evolve_target = 0;
    bool level_valid = false;                  // the levels belong to level_dt_max and level_levels
    float level_dt_max = 0.f;
    int level_levels = 0;
    bool evolve_pending = false;               // the last call ran out of steps: systems sit at different ticks
    int evolve_launch_steps = nbody::kBatchStepsPerLaunch;
    // nbody_batch_stop_set: the per-system reports beside evolve_state
    nbody::DeviceArray<nbody::BatchStopReport> stop_report;  // [n_systems], allocated by the first evolve with conditions
    bool stop_forgotten = true;                // the reports count as all zero: cleared before the next launch reads them
    // nbody_batch_merge_set: the per-system merger counts and logs beside the reports (forgotten with them)
    int merge_capacity = 0;
    nbody::DeviceArray<int> merge_count;                    // [n_systems], allocated by the first evolve that merges
    nbody::DeviceArray<nbody_batch_merge_event> merge_log;  // [n_systems][merge_capacity]
    // nbody_batch_radii_set: one radius per slot, laid out like the positions; a property of the slots, which only
    // nbody_batch_radii_set and the mergers change
    nbody::DeviceArray<float> radii;  // [n_systems][max_bodies], allocated by the first nbody_batch_radii_set
    // nbody_batch_massive_set: per system the number of leading bodies that exert forces; a property of the handle, which only
    // nbody_batch_massive_set changes
    std::vector<int> massive;     // host copy, [n_systems] while config.massive_set
    nbody::DeviceArray<int> massive_dev;  // [n_systems], allocated by the first nbody_batch_massive_set
    // nbody_batch_fate_set: the per-body fates beside the reports (forgotten with them), laid out like the positions and
    // allocated by the first REMOVE
    nbody::DeviceArray<nbody::BatchFate> fates;  // [n_systems][max_bodies]
    // nbody_batch_accrete_set: what the tracers gave, beside the fates (forgotten with them) and allocated by the first ACCRETE
    nbody::DeviceArray<float> given;     // [n_systems][max_bodies]
    nbody::DeviceArray<int> accretions;  // [n_systems]
    // nbody_batch_field_set: the external field's components; a property of the handle, which only nbody_batch_field_set changes
    std::vector<nbody_batch_field_component> field;  // host copy as set, [n_systems][field_components] while config.field_set
    int field_components = 0;
    nbody::DeviceArray<nbody::BatchFieldTerm> field_dev;  // [n_systems][4] as the kernels take them, allocated by the first set
    nbody::DeviceArray<nbody_batch_field_component> field_raw_dev;  // [n_systems][4] as set, for nbody_batch_field_potential
    // nbody_batch_energy, nbody_batch_momentum: allocated by nbody_batch_create, so that a diagnostic never allocates
    nbody::DeviceArray<double> diag_dev;  // [n_systems][kDiagValues]
    std::vector<double> diag_host;
    // nbody_batch_pairs ... nbody_batch_span: the records of the last calls; they belong to no cache and nothing forgets them
    nbody::BatchAnalysis *analysis = nullptr;  // created by the first analysis call
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream or the caller's (nbody_batch_set_stream)
    std::string err;
};

#pragma GCC visibility push(hidden)

namespace nbody {

// `count` elements of a device array to the caller's host array, behind the launches on the handle's stream; no `host`, no copy.
template <class T>
hipError_t copy_out(const nbody_batch *b, void *host, const DeviceArray<T> &array, size_t count)
{
    return host ? hipMemcpyAsync(host, array.ptr, sizeof(T) * count, hipMemcpyDeviceToHost, b->stream) : hipSuccess;
}

}  // namespace nbody

#pragma GCC visibility pop
