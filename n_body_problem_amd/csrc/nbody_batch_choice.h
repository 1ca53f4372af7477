// nbody_batch_choice.h -- which kernel family a batch handle runs, with what launch shape, and which combinations of settings
// nbody_batch_evolve_on refuses: pure functions of the handle's settings.  Plain C++17 without HIP, like
// nbody_launch_choice.h: nbody_batch.hip launches what these functions choose and reports what they refuse, and a CPU test
// (tests/test_batch_choice_cpu.py) checks every choice without a GPU.  Internal; the public surface is include/nbody.h.
#pragma once
#include "../../include/nbody.h"

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace nbody {

// Workgroup shape for a capacity: rows per lane and threads.  Small systems keep a whole wave busy (one or two rows per
// lane); from 129 bodies on four rows per lane feed on every broadcast LDS read, 64 threads per 256 bodies (4096 bodies:
// 1024 threads, 16 waves).
struct BatchShape {
    int rpl, threads;
};
inline BatchShape batch_shape(int max_bodies)
{
    if (max_bodies <= 64)
        return {1, 64};
    if (max_bodies <= 128)
        return {2, 64};
    return {4, (max_bodies + 255) / 256 * 64};
}

// What the choice depends on: the handle's settings, each written by its setter (nbody_batch_set_integrator, _massive_set,
// _radii_set, _stop_set, _merge_set, _fate_set, _accrete_set, _field_set).
struct BatchConfig {
    int integrator = NBODY_INTEGRATOR_KICK_DRIFT;
    bool massive_set = false, radii_set = false;
    float collision_radius = 0.f, escape_radius = 0.f;  // nbody_batch_stop_set; both 0: off
    int collision_action = NBODY_BATCH_ON_COLLISION_STOP;
    int tracer_action = NBODY_BATCH_TRACERS_REFUSE;
    int hit_action = NBODY_BATCH_ON_HIT_REMOVE;
    bool field_set = false;  // nbody_batch_field_set: an external field (nbody_batch_field.h)
};

// What the settings amount to for nbody_batch_evolve_on and for the calls that read what it kept.
struct BatchMode {
    bool collisions;  // collisions are watched: by a collision radius or by radii
    bool stopping;    // stop reports are kept: collisions or an escape radius
    bool merging;     // a collision merges the pair: merger counts and logs are kept
    bool fates;       // tracer fates are kept: massive counts with REMOVE and a condition
    bool accreting;   // a tracer that hits gives its mass word to its target: fates, collisions watched and ACCRETE
};
inline BatchMode batch_mode(const BatchConfig &c)
{
    BatchMode m;
    m.collisions = c.collision_radius > 0.f || c.radii_set;
    m.stopping = m.collisions || c.escape_radius > 0.f;
    m.merging = c.collision_action == NBODY_BATCH_ON_COLLISION_MERGE && m.collisions;
    m.fates = c.massive_set && c.tracer_action == NBODY_BATCH_TRACERS_REMOVE && m.stopping;
    m.accreting = m.fates && m.collisions && c.hit_action == NBODY_BATCH_ON_HIT_ACCRETE;
    return m;
}

// The kernel families of nbody_batch.hip, each instantiated for <rows per lane, guard> (the two step families for KDK too).
enum class BatchKernel { step, step_massive, hermite, hermite_massive, adaptive, stop, merge, radii, adaptive_massive, fate };

// What nbody_batch_evolve_on refuses, in the order it looks.
enum class BatchRefusal {
    none,
    not_hermite,
    radii_and_collision_radius,
    merge_with_massive,
    massive_with_conditions,
    field_with_conditions,  // nbody_batch_field.h: nbody_batch_evolve_on, after the four above
    field_with_step_n       // nbody_batch_field.h: nbody_batch_step_n_*
};

inline int batch_refusal_status(BatchRefusal r) { return r == BatchRefusal::none ? NBODY_OK : NBODY_ERR_INVALID; }

inline const char *batch_refusal_message(BatchRefusal r)
{
    switch (r) {
    case BatchRefusal::not_hermite:
        return "nbody_batch_evolve: adaptive steps need NBODY_INTEGRATOR_HERMITE "
               "(nbody_batch_set_integrator): the criterion uses its accelerations and jerks";
    case BatchRefusal::radii_and_collision_radius:
        return "nbody_batch_evolve: radii and collision_radius are both set (nbody_batch_radii.h: radii "
               "replace the collision radius)";
    case BatchRefusal::merge_with_massive:
        return "nbody_batch_evolve: the collision action MERGE together with massive counts "
               "(nbody_batch_fate.h: mergers among massive bodies while massive counts are set are "
               "not supported); nbody_batch_merge_set(b, NULL) or nbody_batch_massive_set(b, NULL)";
    case BatchRefusal::massive_with_conditions:
        return "nbody_batch_evolve: massive counts are set together with a stopping condition or radii "
               "(nbody_batch_massive.h: not supported, the collision test counts on a row's own column); "
               "nbody_batch_massive_set(b, NULL) or switch the conditions off";
    case BatchRefusal::field_with_conditions:
        return "nbody_batch_evolve: an external field is set together with a collision radius, an escape radius, "
               "radii, the collision action MERGE or the tracer action REMOVE (nbody_batch_field.h: the condition, "
               "fate and accrete kernels take no field); nbody_batch_field_set(b, NULL, 0) or switch the conditions off";
    case BatchRefusal::field_with_step_n:
        return "nbody_batch_step_n: an external field is set (nbody_batch_field.h: fixed steps with a field are "
               "nbody_batch_evolve_on with levels = 0, NBODY_INTEGRATOR_HERMITE); nbody_batch_field_set(b, NULL, 0) "
               "switches the field off";
    default: return "";
    }
}

// One launch: the family, its instantiation <rpl, guard>, the workgroup and its dynamic LDS.  refusal != none: nothing runs.
struct BatchChoice {
    BatchKernel kernel;
    int rpl, threads;
    bool guard;  // eps = 0: the self pair and coincident bodies are dropped by a test, not by the softening
    size_t lds;
    BatchRefusal refusal;
    // The Hermite families pass the default 64 KiB of dynamic LDS from 2049 bodies on and raise their limit before every
    // launch; the two step families stay below it.
    bool raises_lds_limit() const { return kernel != BatchKernel::step && kernel != BatchKernel::step_massive; }
    // nbody_batch_accrete.h: the fate family's accreting sibling (the same shape and LDS); no family of its own
    bool accrete = false;
    // nbody_batch_field.h: the adaptive families' sibling that adds the external field (the same shape and LDS); no family
    // of its own
    bool field = false;
};

constexpr size_t kBatchBytesPerBody = 16;  // one float4

inline BatchChoice batch_choice(BatchKernel kernel, int max_bodies, float softening)
{
    const BatchShape sh = batch_shape(max_bodies);
    const float eps2 = softening * softening;
    BatchChoice c{kernel, sh.rpl, sh.threads, !(eps2 > 0.f), kBatchBytesPerBody * (size_t)max_bodies, BatchRefusal::none, false};
    if (c.raises_lds_limit())  // the predicted positions and velocities of the system's bodies
        c.lds *= 2;
    return c;
}

// nbody_batch_step_n_async: fixed steps know no conditions; they refuse an external field (nbody_batch_field.h) and nothing
// else.
inline BatchChoice batch_step_choice(const BatchConfig &cfg, int max_bodies, float softening)
{
    const bool hermite = cfg.integrator == NBODY_INTEGRATOR_HERMITE;
    // test particles (nbody_batch_massive.h): the siblings whose column loop ends early
    const BatchKernel k = hermite ? (cfg.massive_set ? BatchKernel::hermite_massive : BatchKernel::hermite)
                                  : (cfg.massive_set ? BatchKernel::step_massive : BatchKernel::step);
    BatchChoice c = batch_choice(k, max_bodies, softening);
    if (cfg.field_set)
        c.refusal = BatchRefusal::field_with_step_n;
    return c;
}

// nbody_batch_evolve_on.  Massive counts never meet the plain condition kernels: with conditions they are the fate kernel's
// (REMOVE) or refused (REFUSE), and MERGE is refused with them either way.  The hit action ACCRETE picks the fate family's
// accreting sibling where collisions are watched, and changes nothing else.  An external field (nbody_batch_field.h) runs with
// the two families without conditions, through their sibling with the field, and is refused with everything that watches a
// condition -- looked at after the older refusals, so that every answer without a field stays what it was.
inline BatchChoice batch_evolve_choice(const BatchConfig &cfg, int max_bodies, float softening)
{
    const BatchMode m = batch_mode(cfg);
    BatchRefusal r = BatchRefusal::none;
    if (cfg.integrator != NBODY_INTEGRATOR_HERMITE)
        r = BatchRefusal::not_hermite;
    else if (cfg.radii_set && cfg.collision_radius > 0.f)
        r = BatchRefusal::radii_and_collision_radius;
    else if (m.fates && m.merging)
        r = BatchRefusal::merge_with_massive;
    else if (!m.fates && cfg.massive_set && m.stopping)
        r = BatchRefusal::massive_with_conditions;
    else if (cfg.field_set && m.stopping)  // MERGE and REMOVE act only where a condition is watched
        r = BatchRefusal::field_with_conditions;
    BatchKernel k;
    if (m.fates)  // nbody_batch_fate.h: massive counts together with the conditions, through a kernel of their own
        k = BatchKernel::fate;
    else if (cfg.radii_set)  // nbody_batch_radii.h: collisions without a collision radius, stopping or merging
        k = BatchKernel::radii;
    else if (cfg.massive_set)
        k = BatchKernel::adaptive_massive;
    else if (m.merging)
        k = BatchKernel::merge;
    else
        k = m.stopping ? BatchKernel::stop : BatchKernel::adaptive;
    BatchChoice c = batch_choice(k, max_bodies, softening);
    c.refusal = r;
    c.accrete = k == BatchKernel::fate && m.accreting;
    c.field = cfg.field_set;
    return c;
}

// nbody_step's rule: finite, and 0 or at least NBODY_MIN_SOFTENING
inline bool batch_softening_ok(float softening)
{
    return std::isfinite(softening) && softening >= 0.f && !(softening > 0.f && softening < NBODY_MIN_SOFTENING);
}

// One component of nbody_batch_field_set (nbody_batch_field.h) against its domain: what is wrong with it, for the message that
// names the function, the system, the component and the value (NBODY_ERR_INVALID), or nullptr.
inline const char *batch_field_component_error(int kind, const float *p)
{
    const auto bad = [](float u) { return !std::isfinite(u) || u < 0.f; };  // not a finite number >= 0
    switch (kind) {
    case NBODY_BATCH_FIELD_NONE: return nullptr;  // skipped: its parameters are not read
    case NBODY_BATCH_FIELD_PLUMMER:
        if (bad(p[0]))
            return "PLUMMER: the mass p[0] must be finite and >= 0";
        if (bad(p[1]) || (p[1] > 0.f && p[1] < NBODY_MIN_SOFTENING))
            return "PLUMMER: the scale b = p[1] must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9)";
        return nullptr;
    case NBODY_BATCH_FIELD_LOG_HALO:
        if (bad(p[0]))
            return "LOG_HALO: the velocity v0 = p[0] must be finite and >= 0";
        if (bad(p[1]) || !(p[1] > 0.f))
            return "LOG_HALO: the core radius rc = p[1] must be finite and > 0";
        if (bad(p[2]) || !(p[2] > 0.f))
            return "LOG_HALO: the flattening q = p[2] must be finite and > 0";
        return nullptr;
    case NBODY_BATCH_FIELD_MIYAMOTO_NAGAI:
        if (bad(p[0]))
            return "MIYAMOTO_NAGAI: the mass p[0] must be finite and >= 0";
        if (bad(p[1]))
            return "MIYAMOTO_NAGAI: the scale length a = p[1] must be finite and >= 0";
        if (bad(p[2]) || !(p[2] > 0.f))
            return "MIYAMOTO_NAGAI: the scale height b = p[2] must be finite and > 0";
        return nullptr;
    default: return "unknown kind (NONE = 0, PLUMMER = 1, LOG_HALO = 2, MIYAMOTO_NAGAI = 3)";
    }
}

// The numeric arguments of nbody_batch_evolve_on: the message to report (NBODY_ERR_INVALID), or nullptr.
inline const char *batch_evolve_args_error(int levels, int64_t n_intervals, float dt_max, float eta, float eta_start, float softening)
{
    if (levels < 0 || levels > NBODY_BATCH_EVOLVE_MAX_LEVELS)
        return "nbody_batch_evolve: levels outside [0, NBODY_BATCH_EVOLVE_MAX_LEVELS = 20]";
    if (n_intervals < 0 || n_intervals >= ((int64_t)1 << (62 - levels)))
        return "nbody_batch_evolve: n_intervals < 0 or n_intervals x 2^levels >= 2^62";
    if (!std::isfinite(dt_max) || !(dt_max > 0.f))
        return "nbody_batch_evolve: dt_max must be finite and positive";
    if (!std::isfinite(eta) || !(eta > 0.f) || !std::isfinite(eta_start) || !(eta_start > 0.f))
        return "nbody_batch_evolve: eta and eta_start must be finite and positive";
    if (!batch_softening_ok(softening))
        return "nbody_batch_evolve: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9): "
               "0 < softening < 1e-9 would overflow fp32 (eps^-3 x mass of the self pair)";
    return nullptr;
}

}  // namespace nbody
