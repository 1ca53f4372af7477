// nbody_batch_capi.hip -- the host code behind the integrators' C ABI of a batched ensemble (include/nbody.h, nbody_batch_create
// ... nbody_batch_get_counts): argument checks, the handle's settings and caches, its arrays and the copies back.  Host code
// only: the kernels and their launchers are in nbody_batch.hip, reached through nbody_batch_launch.h; the analysis calls are in
// nbody_batch_analysis.hip; the handle is nbody_batch_handle.h.
#include "nbody_batch_launch.h"
#include "nbody_batch_radii_check.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

using namespace nbody;

static thread_local std::string g_batch_create_error;

int nbody::bfail(nbody_batch *b, int status, const std::string &msg)
{
    if (b)
        b->err = msg;
    else
        g_batch_create_error = msg;
    return status;
}

// The caches are forgotten, and with them the levels (nbody_batch_evolve_on sees to those) and the stops.
static void forget_caches(nbody_batch *b)
{
    b->acc_valid = false;
    b->stop_forgotten = true;
}

// nbody_batch_evolve_on's buffers: the caches and the per-system state, and what the mode keeps beside them -- merger counts and
// logs, stop reports, fates, accretions -- allocated on first use and zeroed where the stops count as forgotten.
static int evolve_prepare_buffers(nbody_batch *b, const BatchMode &mode)
{
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, b->acc.ensure(slots));
    BATCH_TRY(b, b->jerk.ensure(slots));
    if (!b->evolve_state.ptr) {
        BATCH_TRY(b, b->evolve_state.ensure(B));
        BATCH_TRY(b, hipMemsetAsync(b->evolve_state.ptr, 0, sizeof(BatchEvolveState) * B, b->stream));
    }
    BATCH_TRY(b, b->evolve_counters.ensure(2));
    if (mode.merging) {  // nbody_batch_merge.h: counts and logs that start from zero where the reports do
        if (!b->merge_count.ptr) {
            BATCH_TRY(b, b->merge_count.ensure(B));
            b->stop_forgotten = true;
        }
        if (b->merge_capacity > 0 && !b->merge_log.ptr) {
            BATCH_TRY(b, b->merge_log.ensure(B * (size_t)b->merge_capacity));
            b->stop_forgotten = true;
        }
        if (b->stop_forgotten)
            BATCH_TRY(b, hipMemsetAsync(b->merge_count.ptr, 0, sizeof(int) * B, b->stream));
    }
    if (mode.stopping) {  // nbody_batch_stop.h: reports that start from zero
        if (!b->stop_report.ptr) {
            BATCH_TRY(b, b->stop_report.ensure(B));
            b->stop_forgotten = true;
        }
        if (b->stop_forgotten)
            BATCH_TRY(b, hipMemsetAsync(b->stop_report.ptr, 0, sizeof(BatchStopReport) * B, b->stream));
        if (b->stop_forgotten && mode.fates)  // nbody_batch_fate.h: the fates are forgotten where the stops are
            BATCH_TRY(b, hipMemsetAsync(b->fates.ptr, 0, sizeof(BatchFate) * slots, b->stream));
        if (b->stop_forgotten && mode.accreting) {  // nbody_batch_accrete.h: zeroed exactly where the fates are
            BATCH_TRY(b, hipMemsetAsync(b->given.ptr, 0, sizeof(float) * slots, b->stream));
            BATCH_TRY(b, hipMemsetAsync(b->accretions.ptr, 0, sizeof(int) * B, b->stream));
        }
        b->stop_forgotten = false;
    }
    return NBODY_OK;
}

// The arguments from the handle's settings and the call's (after evolve_prepare_buffers: they carry its pointers).
static BatchEvolveLaunch evolve_launch_args(const nbody_batch *b, const BatchMode &mode, const nbody_batch_evolve_config *cfg,
                                            int64_t target, int64_t max_steps)
{
    const BatchConfig &c = b->config;
    BatchEvolveLaunch a;
    BatchEvolveArgs &p = a.p;
    p.dt = (double)cfg->dt_max;
    p.dt_half = 0.5 * p.dt;
    p.dt_six = 6.0 * p.dt;
    p.dt_third = p.dt / 3.0;
    p.dt_sixth = p.dt / 6.0;
    p.dt2 = p.dt * p.dt;
    p.inv_dt2 = 1.0 / (p.dt * p.dt);
    p.inv_dt3 = 1.0 / (p.dt * p.dt * p.dt);
    p.eta = (double)cfg->eta;
    p.eta_start2 = (double)cfg->eta_start * (double)cfg->eta_start;
    p.target = target;
    p.max_steps = max_steps;
    p.eps2 = cfg->softening * cfg->softening;
    p.levels = cfg->levels;
    p.budget = b->evolve_launch_steps;
    // stopping conditions (nbody_batch_stop.h): the thresholds in fp32; radii (nbody_batch_radii.h) watch collisions without one
    a.sa = BatchStopArgs{-1.f, __builtin_inff()};
    if (c.collision_radius > 0.f)
        a.sa.thr = std::fmaf(c.collision_radius, c.collision_radius, cfg->softening * cfg->softening);
    if (c.escape_radius > 0.f)
        a.sa.re2 = c.escape_radius * c.escape_radius;
    a.ma = BatchMergeArgs{b->merge_count.ptr, b->merge_log.ptr, b->merge_capacity};
    a.ra = BatchRadiiArgs{b->radii.ptr, mode.merging ? 1 : 0};
    a.fa = BatchFateArgs{c.radii_set ? b->radii.ptr : nullptr, 0.5f * c.collision_radius, mode.collisions ? 1 : 0, b->fates.ptr};
    a.aa = BatchAccreteArgs{b->given.ptr, b->accretions.ptr};
    return a;
}

// What every launch of a call on these buffers shares.
static BatchLaunch batch_launch(const nbody_batch *b, const BatchChoice &choice, float *d_pos, float *d_vel)
{
    return BatchLaunch{choice, (int)b->n_systems, (int)b->max_bodies, b->stream, reinterpret_cast<float4 *>(d_pos),
                       reinterpret_cast<float4 *>(d_vel), b->acc.ptr, b->jerk.ptr, b->counts_dev.ptr, b->massive_dev.ptr,
                       b->evolve_state.ptr, b->evolve_counters.ptr, b->stop_report.ptr, b->field_dev.ptr};
}

// Whether the caches (accelerations, jerks, levels) belong to these buffers, this softening and the handle's integrator: KDK's
// accelerations come without jerks, so a cache is used only by the integrator that filled it.
static bool caches_belong_to(const nbody_batch *b, const float *d_pos, const float *d_vel, float softening)
{
    return b->acc_pos == d_pos && b->acc_vel == d_vel && b->acc_softening == softening && b->acc_integrator == b->config.integrator;
}

// After a launch: the caches hold the state of these buffers.
static void caches_filled_for(nbody_batch *b, const float *d_pos, const float *d_vel, float softening)
{
    b->acc_integrator = b->config.integrator;
    b->acc_valid = true;
    b->acc_pos = d_pos;
    b->acc_vel = d_vel;
    b->acc_softening = softening;
}

extern "C" {

int nbody_batch_create(nbody_batch **out, int device, int64_t n_systems, int64_t max_bodies)
{
    if (!out)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_create: out is NULL");
    *out = nullptr;
    if (n_systems <= 0 || n_systems > ((int64_t)1 << 30))
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_create: n_systems out of range [1, 2^30]");
    if (max_bodies <= 0 || max_bodies > NBODY_BATCH_MAX_BODIES)
        return bfail(nullptr, NBODY_ERR_INVALID,
                     "nbody_batch_create: max_bodies out of range [1, NBODY_BATCH_MAX_BODIES = 4096] (larger systems: nbody_create)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return bfail(nullptr, NBODY_ERR_NO_DEVICE,
                     std::string("nbody_batch_create: no HIP device (") + hipGetErrorString(e) + "); this library has no CPU path");
    if (device < 0 || device >= ndev)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_create: device index out of range");
    BATCH_TRY(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    BATCH_TRY(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bfail(nullptr, NBODY_ERR_NO_DEVICE,
                     std::string("nbody_batch_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    nbody_batch *b = new (std::nothrow) nbody_batch;
    if (!b)
        return bfail(nullptr, NBODY_ERR_ALLOC, "nbody_batch_create: host allocation failed");
    b->device = device;
    b->n_systems = n_systems;
    b->max_bodies = max_bodies;
    b->counts.assign((size_t)n_systems, (int)max_bodies);
    b->diag_host.resize((size_t)n_systems * kDiagValues);
    hipError_t he = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
    if (he == hipSuccess)
        he = b->counts_dev.ensure((size_t)n_systems);
    if (he == hipSuccess)
        he = b->diag_dev.ensure(b->diag_host.size());
    if (he == hipSuccess)
        he = hipMemcpy(b->counts_dev.ptr, b->counts.data(), sizeof(int) * (size_t)n_systems, hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        const int rc = bfail(nullptr, he == hipErrorOutOfMemory ? NBODY_ERR_ALLOC : NBODY_ERR_DEVICE,
                             std::string("nbody_batch_create: ") + hipGetErrorString(he));
        nbody_batch_destroy(b);
        return rc;
    }
    b->stream = b->own_stream;
    *out = b;
    return NBODY_OK;
}

int nbody_batch_destroy(nbody_batch *b)
{
    if (!b)
        return NBODY_OK;
    (void)hipSetDevice(b->device);
    if (b->stream)
        (void)hipStreamSynchronize(b->stream);
    if (b->own_stream && b->own_stream != b->stream)
        (void)hipStreamSynchronize(b->own_stream);
    batch_analysis_destroy(b);  // nbody_batch_analysis.hip: what the analysis calls keep
    if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
    delete b;  // the handle's arrays free themselves, with the device set and both streams idle
    return NBODY_OK;
}

const char *nbody_batch_last_error(const nbody_batch *b) { return b ? b->err.c_str() : g_batch_create_error.c_str(); }

int nbody_batch_set_counts(nbody_batch *b, const int64_t *host_counts)
{
    if (!b || !host_counts)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_set_counts: NULL argument");
    for (int64_t s = 0; s < b->n_systems; ++s)
        if (host_counts[s] < 0 || host_counts[s] > b->max_bodies)
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_set_counts: count of system " + std::to_string(s) + " (" +
                                                   std::to_string(host_counts[s]) + ") outside [0, max_bodies = " +
                                                   std::to_string(b->max_bodies) + "]");
    for (int64_t s = 0; s < b->n_systems; ++s)
        b->counts[(size_t)s] = (int)host_counts[s];
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, hipMemcpyAsync(b->counts_dev.ptr, b->counts.data(), sizeof(int) * b->counts.size(), hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));  // the host copy may change with the next call
    forget_caches(b);
    return NBODY_OK;
}

int nbody_batch_set_integrator(nbody_batch *b, int integrator)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_set_integrator: batch is NULL");
    if (integrator != NBODY_INTEGRATOR_KICK_DRIFT && integrator != NBODY_INTEGRATOR_KDK && integrator != NBODY_INTEGRATOR_HERMITE)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_set_integrator: unknown integrator (KICK_DRIFT = 0, KDK = 1, HERMITE = 2)");
    if (integrator != b->config.integrator)
        forget_caches(b);
    b->config.integrator = integrator;
    return NBODY_OK;
}

int nbody_batch_invalidate_forces(nbody_batch *b)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_invalidate_forces: batch is NULL");
    forget_caches(b);
    return NBODY_OK;
}

int nbody_batch_set_stream(nbody_batch *b, void *hip_stream)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_set_stream: batch is NULL");
    b->stream = (hipStream_t)hip_stream;  // verbatim: NULL is the HIP default stream
    return NBODY_OK;
}

int nbody_batch_step_n_async(nbody_batch *b, float *d_pos, float *d_vel, int k, float dt, float softening)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_step_n: batch is NULL");
    if (!d_pos || !d_vel)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_step_n: NULL buffer");
    if (k < 0)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_step_n: k < 0");
    if (!std::isfinite(dt))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_step_n: dt must be finite");
    if (!batch_softening_ok(softening))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_step_n: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9): "
                                           "0 < softening < 1e-9 would overflow fp32 (eps^-3 x mass of the self pair)");
    const BatchChoice choice = batch_step_choice(b->config, (int)b->max_bodies, softening);
    if (choice.refusal != BatchRefusal::none)  // nbody_batch_field.h: no fixed-step kernel takes a field
        return bfail(b, batch_refusal_status(choice.refusal), batch_refusal_message(choice.refusal));
    if (k == 0)
        return NBODY_OK;
    if (b->evolve_pending && b->acc_valid && b->config.integrator == NBODY_INTEGRATOR_HERMITE)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_step_n: the last nbody_batch_evolve_on ran out of steps and its systems sit at "
                                         "different times: complete it, or nbody_batch_invalidate_forces to drop it");
    b->level_valid = false;  // fixed steps leave the levels behind, and the stops
    b->stop_forgotten = true;
    BATCH_TRY(b, hipSetDevice(b->device));
    const bool kdk = b->config.integrator == NBODY_INTEGRATOR_KDK, hermite = b->config.integrator == NBODY_INTEGRATOR_HERMITE;
    const size_t slots = (size_t)b->n_systems * (size_t)b->max_bodies;
    if (kdk || hermite) {
        BATCH_TRY(b, b->acc.ensure(slots));
        if (hermite)
            BATCH_TRY(b, b->jerk.ensure(slots));
        if (!caches_belong_to(b, d_pos, d_vel, softening))
            b->acc_valid = false;
    }
    const BatchLaunch launch = batch_launch(b, choice, d_pos, d_vel);
    const float eps2 = softening * softening;
    for (int done = 0; done < k; done += kBatchStepsPerLaunch) {
        const int run = std::min(kBatchStepsPerLaunch, k - done);
        BATCH_TRY(b, launch_batch_steps(launch, kdk, run, dt, eps2, b->acc_valid));
        if (kdk || hermite)
            caches_filled_for(b, d_pos, d_vel, softening);
    }
    return NBODY_OK;
}

int nbody_batch_sync(nbody_batch *b)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_sync: batch is NULL");
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    BATCH_TRY(b, hipGetLastError());
    return NBODY_OK;
}

int nbody_batch_step_n_on(nbody_batch *b, float *d_pos, float *d_vel, int k, float dt, float softening)
{
    const int rc = nbody_batch_step_n_async(b, d_pos, d_vel, k, dt, softening);
    return rc != NBODY_OK ? rc : nbody_batch_sync(b);
}

int nbody_batch_evolve_launch_steps(nbody_batch *b, int steps_per_launch)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_evolve_launch_steps: batch is NULL");
    if (steps_per_launch < 1 || steps_per_launch > 4096)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_evolve_launch_steps: steps_per_launch outside [1, 4096]");
    b->evolve_launch_steps = steps_per_launch;
    return NBODY_OK;
}

int nbody_batch_evolve_on(nbody_batch *b, float *d_pos, float *d_vel, int64_t n_intervals, const nbody_batch_evolve_config *cfg)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_evolve: batch is NULL");
    if (!d_pos || !d_vel || !cfg)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_evolve: NULL argument");
    const BatchMode mode = batch_mode(b->config);
    const BatchChoice choice = batch_evolve_choice(b->config, (int)b->max_bodies, cfg->softening);
    if (choice.refusal != BatchRefusal::none)
        return bfail(b, batch_refusal_status(choice.refusal), batch_refusal_message(choice.refusal));
    if (const char *msg = batch_evolve_args_error(cfg->levels, n_intervals, cfg->dt_max, cfg->eta, cfg->eta_start, cfg->softening))
        return bfail(b, NBODY_ERR_INVALID, msg);
    const int64_t max_steps = cfg->max_steps > 0 ? cfg->max_steps : NBODY_BATCH_EVOLVE_DEFAULT_MAX_STEPS;
    const int64_t target = n_intervals << cfg->levels;
    if (!caches_belong_to(b, d_pos, d_vel, cfg->softening))
        b->acc_valid = false;
    if (!b->acc_valid) {
        b->level_valid = b->evolve_pending = false;
        b->stop_forgotten = true;
    }
    const bool same_axis = b->level_valid && b->level_dt_max == cfg->dt_max && b->level_levels == cfg->levels;
    const bool resume = b->evolve_pending;
    if (resume) {
        if (!same_axis)
            return bfail(b, NBODY_ERR_STATE, "nbody_batch_evolve: the last call ran out of steps; complete it with the same dt_max and "
                                             "levels, or nbody_batch_invalidate_forces to drop it");
        for (int64_t s = 0; s < b->n_systems; ++s)
            if (b->counts[(size_t)s] > 0 && b->evolve_host[(size_t)s].tick > target)
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_evolve: n_intervals ends before the time system " + std::to_string(s) +
                                                       " reached in the call this one resumes");
    }
    const size_t B = (size_t)b->n_systems;
    if (b->evolve_host.size() != B)
        b->evolve_host.assign(B, kEvolveStateFresh);
    if (!resume)
        std::fill(b->evolve_host.begin(), b->evolve_host.end(), kEvolveStateFresh);
    b->evolve_target = target;
    if (target == 0)
        return NBODY_OK;
    BATCH_TRY(b, hipSetDevice(b->device));
    if (const int rc = evolve_prepare_buffers(b, mode); rc != NBODY_OK)
        return rc;
    const BatchLaunch launch = batch_launch(b, choice, d_pos, d_vel);
    BatchEvolveLaunch args = evolve_launch_args(b, mode, cfg, target, max_steps);
    BatchEvolveArgs &p = args.p;
    int counters[2] = {0, 0};
    for (bool first = true;; first = false) {
        p.have_acc = b->acc_valid ? 1 : 0;
        p.have_level = !first || same_axis ? 1 : 0;
        p.new_call = first ? 1 : 0;
        p.reset_tick = first && !resume ? 1 : 0;
        BATCH_TRY(b, hipMemsetAsync(b->evolve_counters.ptr, 0, sizeof(counters), b->stream));
        BATCH_TRY(b, launch_batch_evolve(launch, args));
        caches_filled_for(b, d_pos, d_vel, cfg->softening);
        b->level_valid = true;
        b->level_dt_max = cfg->dt_max;
        b->level_levels = cfg->levels;
        b->evolve_pending = true;  // until every system is seen at the target
        BATCH_TRY(b, hipMemcpyAsync(counters, b->evolve_counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, b->stream));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
        if (counters[0] == 0 || counters[0] == counters[1])
            break;
    }
    if (mode.merging)  // the kernel's own changes of the counts; the caches stay: the restarts have refilled them
        BATCH_TRY(b, hipMemcpyAsync(b->counts.data(), b->counts_dev.ptr, sizeof(int) * B, hipMemcpyDeviceToHost, b->stream));
    BATCH_TRY(b, copy_out(b, b->evolve_host.data(), b->evolve_state, B));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    for (size_t s = 0; s < B; ++s)
        if (b->counts[s] <= 0) {  // an empty system: no steps, at the target
            b->evolve_host[s] = kEvolveStateFresh;
            b->evolve_host[s].tick = target;
        }
    if (counters[0] == 0) {
        b->evolve_pending = false;
        return NBODY_OK;
    }
    std::vector<BatchStopReport> stopped(mode.stopping ? B : 0);  // a stopped system sits before the target too, finished
    if (mode.stopping) {
        BATCH_TRY(b, copy_out(b, stopped.data(), b->stop_report, B));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
    }
    size_t first_unfinished = 0;
    while (first_unfinished < B && (b->evolve_host[first_unfinished].tick >= target || (mode.stopping && stopped[first_unfinished].reason)))
        ++first_unfinished;
    return bfail(b, NBODY_ERR_STATE, "nbody_batch_evolve: system " + std::to_string(first_unfinished) + " is unfinished after max_steps = " +
                                         std::to_string(max_steps) + " steps (tick " +
                                         std::to_string(first_unfinished < B ? b->evolve_host[first_unfinished].tick : 0) + " of " +
                                         std::to_string(target) + "); " + std::to_string(counters[0]) + " of " + std::to_string(B) +
                                         " systems are unfinished; the same call again continues from here");
}

int nbody_batch_evolve_stats(nbody_batch *b, int64_t *steps, int *min_level, int *max_level, int64_t *clamped, int64_t *ticks)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_evolve_stats: batch is NULL");
    if (b->evolve_host.size() != (size_t)b->n_systems)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_evolve_stats: no nbody_batch_evolve_on call yet");
    for (size_t s = 0; s < b->evolve_host.size(); ++s) {
        const BatchEvolveState &st = b->evolve_host[s];
        if (steps) steps[s] = st.steps;
        if (min_level) min_level[s] = st.steps > 0 ? st.min_level : 0;
        if (max_level) max_level[s] = st.steps > 0 ? st.max_level : 0;
        if (clamped) clamped[s] = st.clamped;
        if (ticks) ticks[s] = st.tick;
    }
    return NBODY_OK;
}

int nbody_batch_stop_set(nbody_batch *b, const nbody_batch_stop_config *cfg)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_stop_set: batch is NULL");
    const float rc = cfg ? cfg->collision_radius : 0.f, re = cfg ? cfg->escape_radius : 0.f;
    if (!std::isfinite(rc) || rc < 0.f || !std::isfinite(re) || re < 0.f)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_stop_set: collision_radius and escape_radius must be finite and >= 0 (0: off)");
    b->config.collision_radius = rc;
    b->config.escape_radius = re;
    forget_caches(b);  // the next nbody_batch_evolve_on starts with an evaluation, which examines the conditions
    return NBODY_OK;
}

int nbody_batch_stop_read(nbody_batch *b, int *reason, int64_t *tick, int *pair_i, int *pair_j, float *separation, int *escaper)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_stop_read: batch is NULL");
    const size_t B = (size_t)b->n_systems;
    std::vector<BatchStopReport> rep(B, kNotStopped);
    if (batch_mode(b->config).stopping && b->stop_report.ptr && !b->stop_forgotten) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, copy_out(b, rep.data(), b->stop_report, B));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
    }
    for (size_t s = 0; s < B; ++s) {
        const BatchStopReport r = b->counts[s] > 0 ? rep[s] : kNotStopped;
        if (reason) reason[s] = r.reason;
        if (tick) tick[s] = r.tick;
        if (pair_i) pair_i[s] = r.pair_i;
        if (pair_j) pair_j[s] = r.pair_j;
        if (separation) separation[s] = r.separation;
        if (escaper) escaper[s] = r.escaper;
    }
    return NBODY_OK;
}

int nbody_batch_stop_count(nbody_batch *b, int64_t *stopped)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_stop_count: batch is NULL");
    if (!stopped)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_stop_count: NULL argument");
    std::vector<int> reason((size_t)b->n_systems);
    const int rc = nbody_batch_stop_read(b, reason.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != NBODY_OK)
        return rc;
    *stopped = 0;
    for (int r : reason)
        *stopped += r != 0;
    return NBODY_OK;
}

int nbody_batch_merge_set(nbody_batch *b, const nbody_batch_merge_config *cfg)
{
    const int action = cfg ? cfg->on_collision : NBODY_BATCH_ON_COLLISION_STOP, capacity = cfg ? cfg->log_capacity : 0;
    if (action != NBODY_BATCH_ON_COLLISION_STOP && action != NBODY_BATCH_ON_COLLISION_MERGE)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_merge_set: unknown collision action (STOP = 0, MERGE = 1)");
    if (capacity < 0 || capacity > NBODY_BATCH_MAX_BODIES - 1)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_merge_set: log_capacity outside [0, NBODY_BATCH_MAX_BODIES - 1 = 4095]");
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_merge_set: batch is NULL");
    if (capacity != b->merge_capacity && b->merge_log.ptr) {  // allocated anew by the next evolve that merges
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
        b->merge_log.release();
    }
    b->config.collision_action = action;
    b->merge_capacity = capacity;
    forget_caches(b);  // as nbody_batch_stop_set: the next nbody_batch_evolve_on starts with an evaluation
    return NBODY_OK;
}

int nbody_batch_merge_read(nbody_batch *b, int64_t *n_merges, nbody_batch_merge_event *events)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_merge_read: batch is NULL");
    const size_t B = (size_t)b->n_systems, cap = (size_t)b->merge_capacity;
    std::vector<int> count(B, 0);
    const bool kept = batch_mode(b->config).merging && b->merge_count.ptr && !b->stop_forgotten;
    if (events)
        std::memset(events, 0, sizeof(nbody_batch_merge_event) * B * cap);
    if (kept) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, copy_out(b, count.data(), b->merge_count, B));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
        if (events && cap > 0 && b->merge_log.ptr) {
            std::vector<nbody_batch_merge_event> log(B * cap);
            BATCH_TRY(b, copy_out(b, log.data(), b->merge_log, B * cap));
            BATCH_TRY(b, hipStreamSynchronize(b->stream));
            for (size_t s = 0; s < B; ++s)  // entries beyond a system's count were never written
                for (size_t e = 0; e < cap && e < (size_t)count[s]; ++e)
                    events[s * cap + e] = log[s * cap + e];
        }
    }
    if (n_merges)
        for (size_t s = 0; s < B; ++s)
            n_merges[s] = count[s];
    return NBODY_OK;
}

int nbody_batch_radii_set(nbody_batch *b, const float *host_radii)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_radii_set: batch is NULL");
    if (host_radii) {
        std::string msg;
        if (!batch_radii_ok(host_radii, b->counts.data(), b->n_systems, b->max_bodies, &msg))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radii_set: " + msg);
        const size_t slots = (size_t)b->n_systems * (size_t)b->max_bodies;
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, b->radii.ensure(slots));
        BATCH_TRY(b, hipMemcpyAsync(b->radii.ptr, host_radii, sizeof(float) * slots, hipMemcpyHostToDevice, b->stream));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));  // the caller's array may change with the next call
    }
    b->config.radii_set = host_radii != nullptr;
    forget_caches(b);  // as nbody_batch_stop_set: the next nbody_batch_evolve_on starts with an evaluation
    return NBODY_OK;
}

int nbody_batch_radii_read(nbody_batch *b, float *host_radii)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_radii_read: batch is NULL");
    if (!host_radii)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radii_read: NULL argument");
    if (!b->config.radii_set)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_radii_read: no radii are set (nbody_batch_radii_set)");
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, copy_out(b, host_radii, b->radii, (size_t)b->n_systems * (size_t)b->max_bodies));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_massive_set(nbody_batch *b, const int64_t *host_massive)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_massive_set: batch is NULL");
    if (host_massive) {
        for (int64_t s = 0; s < b->n_systems; ++s)
            if (host_massive[s] < 0 || host_massive[s] > b->max_bodies)
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_massive_set: massive count of system " + std::to_string(s) + " (" +
                                                       std::to_string(host_massive[s]) + ") outside [0, max_bodies = " +
                                                       std::to_string(b->max_bodies) + "]");
        b->massive.resize((size_t)b->n_systems);
        for (int64_t s = 0; s < b->n_systems; ++s)
            b->massive[(size_t)s] = (int)host_massive[s];
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, b->massive_dev.ensure(b->massive.size()));
        BATCH_TRY(b, hipMemcpyAsync(b->massive_dev.ptr, b->massive.data(), sizeof(int) * b->massive.size(), hipMemcpyHostToDevice, b->stream));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));  // the host copy may change with the next call
    }
    b->config.massive_set = host_massive != nullptr;
    forget_caches(b);  // as nbody_batch_set_counts: the cached accelerations and jerks belong to the old columns
    return NBODY_OK;
}

int nbody_batch_massive_read(nbody_batch *b, int64_t *host_massive)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_massive_read: batch is NULL");
    if (!host_massive)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_massive_read: NULL argument");
    if (!b->config.massive_set)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_massive_read: no massive counts are set (nbody_batch_massive_set)");
    for (size_t s = 0; s < (size_t)b->n_systems; ++s)
        host_massive[s] = b->massive[s];
    return NBODY_OK;
}

int nbody_batch_fate_set(nbody_batch *b, const nbody_batch_fate_config *cfg)
{
    const int action = cfg ? cfg->action : NBODY_BATCH_TRACERS_REFUSE;
    if (action != NBODY_BATCH_TRACERS_REFUSE && action != NBODY_BATCH_TRACERS_REMOVE)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_fate_set: unknown tracer action (REFUSE = 0, REMOVE = 1)");
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_fate_set: batch is NULL");
    if (action == NBODY_BATCH_TRACERS_REMOVE && !b->fates.ptr) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, b->fates.ensure((size_t)b->n_systems * (size_t)b->max_bodies));
    }
    b->config.tracer_action = action;
    forget_caches(b);  // as nbody_batch_stop_set: the next nbody_batch_evolve_on starts with an evaluation
    return NBODY_OK;
}

// Whether the fate arrays hold what the last nbody_batch_evolve_on calls found (otherwise every body reads alive).  Asked under
// the tracer action REMOVE only: nbody_batch_fate_read refuses REFUSE first.
static bool fates_kept(const nbody_batch *b)
{
    return batch_mode(b->config).fates && b->fates.ptr && !b->stop_forgotten;
}

int nbody_batch_fate_read(nbody_batch *b, int *fate, int64_t *tick, int *target, float *separation, float *relative_speed)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_fate_read: batch is NULL");
    if (b->config.tracer_action != NBODY_BATCH_TRACERS_REMOVE)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_fate_read: the tracer action is REFUSE (nbody_batch_fate_set): no fates are kept");
    const size_t B = (size_t)b->n_systems, cap = (size_t)b->max_bodies, slots = B * cap;
    std::vector<BatchFate> f(slots, BatchFate{0, 0, 0, 0.f, 0.f});
    if (fates_kept(b)) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, copy_out(b, f.data(), b->fates, slots));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
    }
    for (size_t s = 0; s < B; ++s)
        for (size_t i = 0; i < cap; ++i) {
            const size_t k = s * cap + i;
            const bool gone = (int64_t)i < (int64_t)b->counts[s] && f[k].fate != 0;  // alive, massive or beyond the count: 0, 0, -1, 0, 0
            if (fate) fate[k] = gone ? f[k].fate : NBODY_BATCH_FATE_ALIVE;
            if (tick) tick[k] = gone ? f[k].tick : 0;
            if (target) target[k] = gone ? f[k].target : -1;
            if (separation) separation[k] = gone ? f[k].separation : 0.f;
            if (relative_speed) relative_speed[k] = gone ? f[k].speed : 0.f;
        }
    return NBODY_OK;
}

int nbody_batch_fate_count(nbody_batch *b, int64_t *hit, int64_t *escaped)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_fate_count: batch is NULL");
    if (b->config.tracer_action != NBODY_BATCH_TRACERS_REMOVE)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_fate_count: the tracer action is REFUSE (nbody_batch_fate_set): no fates are kept");
    std::vector<int> fate((size_t)b->n_systems * (size_t)b->max_bodies);
    const int rc = nbody_batch_fate_read(b, fate.data(), nullptr, nullptr, nullptr, nullptr);
    if (rc != NBODY_OK)
        return rc;
    for (size_t s = 0; s < (size_t)b->n_systems; ++s) {
        int64_t h = 0, e = 0;
        for (size_t i = 0; i < (size_t)b->max_bodies; ++i) {
            h += fate[s * (size_t)b->max_bodies + i] == NBODY_BATCH_FATE_HIT;
            e += fate[s * (size_t)b->max_bodies + i] == NBODY_BATCH_FATE_ESCAPED;
        }
        if (hit) hit[s] = h;
        if (escaped) escaped[s] = e;
    }
    return NBODY_OK;
}

int nbody_batch_accrete_set(nbody_batch *b, const nbody_batch_accrete_config *cfg)
{
    const int on_hit = cfg ? cfg->on_hit : NBODY_BATCH_ON_HIT_REMOVE;
    if (on_hit != NBODY_BATCH_ON_HIT_REMOVE && on_hit != NBODY_BATCH_ON_HIT_ACCRETE)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_accrete_set: unknown hit action (REMOVE = 0, ACCRETE = 1)");
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_accrete_set: batch is NULL (refused as an unknown hit action is)");
    if (on_hit == NBODY_BATCH_ON_HIT_ACCRETE && (!b->given.ptr || !b->accretions.ptr)) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, b->given.ensure((size_t)b->n_systems * (size_t)b->max_bodies));
        BATCH_TRY(b, b->accretions.ensure((size_t)b->n_systems));
    }
    b->config.hit_action = on_hit;
    forget_caches(b);  // as nbody_batch_stop_set: the next nbody_batch_evolve_on starts with an evaluation
    return NBODY_OK;
}

int nbody_batch_accrete_read(nbody_batch *b, float *given, int64_t *accretions)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_accrete_read: batch is NULL");
    if (b->config.hit_action != NBODY_BATCH_ON_HIT_ACCRETE)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_accrete_read: the hit action is REMOVE (nbody_batch_accrete_set): no accretions are kept");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    // kept: the arrays hold what the last nbody_batch_evolve_on calls found; otherwise nobody gave anything
    const bool kept = batch_mode(b->config).accreting && b->given.ptr && b->accretions.ptr && !b->stop_forgotten;
    std::vector<int> count(B, 0);
    if (given)
        std::fill(given, given + slots, 0.f);
    if (kept) {
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, copy_out(b, given, b->given, slots));
        BATCH_TRY(b, copy_out(b, count.data(), b->accretions, B));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));
    }
    if (accretions)
        for (size_t s = 0; s < B; ++s)
            accretions[s] = count[s];
    return NBODY_OK;
}

// What the kernels take of one component (BatchFieldTerm): the squares and 1 / (q q) in fp32, formed here once.
static BatchFieldTerm field_term(const nbody_batch_field_component &u)
{
    switch (u.kind) {
    case NBODY_BATCH_FIELD_PLUMMER: return BatchFieldTerm{u.kind, u.p[0], u.p[1] * u.p[1], 0.f};
    case NBODY_BATCH_FIELD_LOG_HALO: return BatchFieldTerm{u.kind, u.p[0] * u.p[0], u.p[1] * u.p[1], 1.f / (u.p[2] * u.p[2])};
    case NBODY_BATCH_FIELD_MIYAMOTO_NAGAI: return BatchFieldTerm{u.kind, u.p[0], u.p[1], u.p[2] * u.p[2]};
    default: return BatchFieldTerm{NBODY_BATCH_FIELD_NONE, 0.f, 0.f, 0.f};
    }
}

int nbody_batch_field_set(nbody_batch *b, const nbody_batch_field_component *host, int n_components)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_field_set: batch is NULL");
    if (host) {
        if (n_components < 1 || n_components > NBODY_BATCH_FIELD_MAX_COMPONENTS)
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_field_set: n_components (" + std::to_string(n_components) +
                                                   ") outside [1, NBODY_BATCH_FIELD_MAX_COMPONENTS = 4]");
        const size_t B = (size_t)b->n_systems, C = (size_t)n_components;
        for (size_t s = 0; s < B; ++s)
            for (size_t c = 0; c < C; ++c) {
                const nbody_batch_field_component &u = host[s * C + c];
                if (const char *msg = batch_field_component_error(u.kind, u.p))
                    return bfail(b, NBODY_ERR_INVALID, "nbody_batch_field_set: system " + std::to_string(s) + ", component " +
                                                           std::to_string(c) + " (kind " + std::to_string(u.kind) + ", p = " +
                                                           std::to_string(u.p[0]) + ", " + std::to_string(u.p[1]) + ", " +
                                                           std::to_string(u.p[2]) + "): " + msg);
            }
        // padded to four components per system with NONE, for the kernels and for the potential
        std::vector<BatchFieldTerm> terms(B * NBODY_BATCH_FIELD_MAX_COMPONENTS, BatchFieldTerm{NBODY_BATCH_FIELD_NONE, 0.f, 0.f, 0.f});
        std::vector<nbody_batch_field_component> raw(B * NBODY_BATCH_FIELD_MAX_COMPONENTS,
                                                     nbody_batch_field_component{NBODY_BATCH_FIELD_NONE, {0.f, 0.f, 0.f}});
        for (size_t s = 0; s < B; ++s)
            for (size_t c = 0; c < C; ++c) {
                terms[s * NBODY_BATCH_FIELD_MAX_COMPONENTS + c] = field_term(host[s * C + c]);
                raw[s * NBODY_BATCH_FIELD_MAX_COMPONENTS + c] = host[s * C + c];
            }
        BATCH_TRY(b, hipSetDevice(b->device));
        BATCH_TRY(b, b->field_dev.ensure(terms.size()));
        BATCH_TRY(b, b->field_raw_dev.ensure(raw.size()));
        BATCH_TRY(b, hipMemcpyAsync(b->field_dev.ptr, terms.data(), sizeof(BatchFieldTerm) * terms.size(), hipMemcpyHostToDevice, b->stream));
        BATCH_TRY(b, hipMemcpyAsync(b->field_raw_dev.ptr, raw.data(), sizeof(nbody_batch_field_component) * raw.size(),
                                    hipMemcpyHostToDevice, b->stream));
        BATCH_TRY(b, hipStreamSynchronize(b->stream));  // the host copies end with this call
        b->field.assign(host, host + B * C);
        b->field_components = n_components;
    }
    b->config.field_set = host != nullptr;
    forget_caches(b);  // as nbody_batch_massive_set: the cached accelerations and jerks belong to the old field
    return NBODY_OK;
}

int nbody_batch_field_read(nbody_batch *b, nbody_batch_field_component *host, int *n_components)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_field_read: batch is NULL");
    if (!host || !n_components)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_field_read: NULL argument");
    if (!b->config.field_set)
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_field_read: no field is set (nbody_batch_field_set)");
    std::copy(b->field.begin(), b->field.end(), host);
    *n_components = b->field_components;
    return NBODY_OK;
}

int nbody_batch_field_potential(nbody_batch *b, const float *d_pos, double *host_phi)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_field_potential: batch is NULL");
    if (!d_pos || !host_phi)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_field_potential: NULL argument");
    const size_t slots = (size_t)b->n_systems * (size_t)b->max_bodies;
    std::fill(host_phi, host_phi + slots, 0.0);
    if (!b->config.field_set)
        return NBODY_OK;
    if (b->n_systems > 65535)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_field_potential: more than 65535 systems");
    BATCH_TRY(b, hipSetDevice(b->device));
    DeviceArray<double> phi;  // freed on every way out, after the wait for the copy where there is one
    BATCH_TRY(b, phi.ensure(slots));
    BATCH_TRY(b, launch_batch_field_potential(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr, b->field_raw_dev.ptr,
                                              NBODY_BATCH_FIELD_MAX_COMPONENTS, (int)b->n_systems, (int)b->max_bodies, phi.ptr,
                                              b->stream));
    BATCH_TRY(b, copy_out(b, host_phi, phi, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_get_counts(nbody_batch *b, int64_t *counts)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_get_counts: batch is NULL");
    if (!counts)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_get_counts: NULL argument");
    for (size_t s = 0; s < (size_t)b->n_systems; ++s)
        counts[s] = b->counts[s];
    return NBODY_OK;
}

}  // extern "C"