// nbody.hpp -- header-only C++ convenience layer over the C ABI of nbody.h.
//
// Keeps the names of the reference's host interface for this path (main_project/kernel.cu):
//   initialize(numBodies)            :130-161      -> nbody::System::initialize / constructor
//   setParticlesPosition(real*)      :163-177      -> System::setParticlesPosition
//   setParticlesVelocity(real*)      :179-188      -> System::setParticlesVelocity
//   the per-frame bracket            :1225-1242    -> System::step(dt, softening)
// so that the reference's main loop reads the same after the swap.  Errors become
// std::runtime_error carrying the library's message; the C ABI itself never throws.
#pragma once
#include "nbody.h"

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace nbody {

constexpr float kTimeTick = 0.008f;            // TIME_TICK, kernel.cu:63
constexpr float kSofteningVersion3 = 1.0e-2f;  // effective eps of cal_single_acclerate_without_mass_new, :665-692
constexpr float kSofteningVersion1 = 1.0e-3f;  // sqrt(EPSILON) of cal_single_acclerate, :808-824

class System {
public:
    System() = default;
    explicit System(std::int64_t numBodies, int device = 0) { initialize(numBodies, device); }
    System(const System &) = delete;
    System &operator=(const System &) = delete;
    ~System() { nbody_destroy(ctx_); }

    void initialize(std::int64_t numBodies, int device = 0)
    {
        nbody_destroy(ctx_);
        ctx_ = nullptr;
        check(nbody_create(&ctx_, device, numBodies), "nbody_create");
        n_ = numBodies;
    }
    // initialize(numBodies) with the faster force mode for this body count already selected (nbody_create_auto): the
    // pair-once kernels from NBODY_PAIR_ONCE_MIN_BODIES bodies on (round 4: at every size), the one-sided ones below.
    void initializeAuto(std::int64_t numBodies, int device = 0)
    {
        nbody_destroy(ctx_);
        ctx_ = nullptr;
        check(nbody_create_auto(&ctx_, device, numBodies), "nbody_create_auto");
        n_ = numBodies;
    }
    bool pairOnce() const { return nbody_force_mode(ctx_) == NBODY_FORCE_SYMMETRIC; }
    // One rank of a sharded run: rows [rowLo, rowLo+rowCount) against all numBodies columns.
    void initializeShard(std::int64_t numBodies, std::int64_t rowLo, std::int64_t rowCount, std::int64_t splitLen = 0,
                         int device = 0)
    {
        nbody_destroy(ctx_);
        ctx_ = nullptr;
        check(nbody_create_shard(&ctx_, device, numBodies, rowLo, rowCount, splitLen), "nbody_create_shard");
        n_ = numBodies;
    }

    void setParticlesPosition(const float *xyzm) { check(nbody_set_positions(ctx_, xyzm), "nbody_set_positions"); }
    void setParticlesVelocity(const float *xyzw) { check(nbody_set_velocities(ctx_, xyzw), "nbody_set_velocities"); }
    void download(float *xyzm, float *xyzw) { check(nbody_download(ctx_, xyzm, xyzw), "nbody_download"); }

    // The mapped-pointer analogue of cudaGraphicsResourceGetMappedPointer (kernel.cu:1226).
    float *positionsDevice() { return nbody_positions_device(ctx_); }
    float *velocitiesDevice() { return nbody_velocities_device(ctx_); }

    // One synchronous step on the owned buffers (the reference synchronises after each kernel, :1232,1236).
    void step(float dt = kTimeTick, float softening = kSofteningVersion3)
    {
        check(nbody_step(ctx_, positionsDevice(), velocitiesDevice(), nullptr, dt, softening), "nbody_step");
    }
    // step(positions, velocities, masses, dt, softening) on caller-owned device buffers.
    void step(float *dPositions, float *dVelocities, const float *dMasses, float dt, float softening)
    {
        check(nbody_step(ctx_, dPositions, dVelocities, dMasses, dt, softening), "nbody_step");
    }
    void stepN(int k, float dt, float softening) { check(nbody_step_n(ctx_, k, dt, softening), "nbody_step_n"); }
    // false: the reference's kick-drift (kernel.cu:777-801); true: velocity Verlet with cached accelerations
    void setKickDriftKick(bool on)
    {
        check(nbody_set_integrator(ctx_, on ? NBODY_INTEGRATOR_KDK : NBODY_INTEGRATOR_KICK_DRIFT), "nbody_set_integrator");
    }
    // experimental pair-once force kernel (context created with splitLen = nbody_pair_once_split_len(numBodies))
    void setPairOnce(bool on)
    {
        check(nbody_set_force_mode(ctx_, on ? NBODY_FORCE_SYMMETRIC : NBODY_FORCE_ONE_SIDED), "nbody_set_force_mode");
    }

    // per-particle softening lengths of all numBodies bodies (host floats, e.g. velocities[4i+3] of the reference's
    // loaders, kernel.cu:223); nullptr switches it off.  eps_ij^2 = softening^2 + eps_i^2 + eps_j^2.
    void setParticleSoftening(const float *hostEps)
    {
        check(nbody_upload_particle_softening(ctx_, hostEps), "nbody_upload_particle_softening");
    }

    struct Energy { double kinetic, potential, total; };
    Energy energy(float softening)
    {
        double e[3];
        check(nbody_energy(ctx_, positionsDevice(), velocitiesDevice(), softening, e), "nbody_energy");
        return {e[0], e[1], e[2]};
    }
    std::vector<double> momentum()
    {
        std::vector<double> p(4);
        check(nbody_momentum(ctx_, positionsDevice(), velocitiesDevice(), p.data()), "nbody_momentum");
        return p;
    }

    void timing(bool on) { check(nbody_timing_enable(ctx_, on ? 1 : 0), "nbody_timing_enable"); }
    struct Timing { double forceMs, updateMs; std::int64_t forceLaunches, updateLaunches; };
    Timing readTiming()
    {
        Timing t{};
        check(nbody_timing_read(ctx_, &t.forceMs, &t.forceLaunches, &t.updateMs, &t.updateLaunches), "nbody_timing_read");
        return t;
    }

    std::int64_t numBodies() const { return n_; }
    nbody_ctx *handle() { return ctx_; }

private:
    void check(int status, const char *what)
    {
        if (status != NBODY_OK)
            throw std::runtime_error(std::string(what) + ": " + nbody_last_error(ctx_) + " (" +
                                     nbody_status_string(status) + ")");
    }
    nbody_ctx *ctx_ = nullptr;
    std::int64_t n_ = 0;
};

// The same host interface for a body set whose rows are sharded over several GPUs of one node, driven from this one
// host thread (nbody_multi_create: one RCCL communicator per device, the exchange inside the library).
class MultiSystem {
public:
    MultiSystem() = default;
    MultiSystem(const MultiSystem &) = delete;
    MultiSystem &operator=(const MultiSystem &) = delete;
    ~MultiSystem() { nbody_multi_destroy(m_); }

    // initialize(numBodies) on the given devices; pairOnce / kickDriftKick / ring / peerCopy select the variants
    void initialize(std::int64_t numBodies, const std::vector<int> &devices, bool pairOnce = false, bool kickDriftKick = false,
                    bool ring = false, bool peerCopy = false, std::int64_t splitLen = 0, bool mortonOrder = false,
                    bool autoMode = false)
    {
        nbody_multi_destroy(m_);
        m_ = nullptr;
        nbody_multi_config cfg{};
        cfg.n_bodies = numBodies;
        cfg.split_len = splitLen;
        cfg.force_mode = autoMode ? NBODY_FORCE_AUTO : pairOnce ? NBODY_FORCE_SYMMETRIC : NBODY_FORCE_ONE_SIDED;
        cfg.integrator = kickDriftKick ? NBODY_INTEGRATOR_KDK : NBODY_INTEGRATOR_KICK_DRIFT;
        cfg.exchange = ring ? NBODY_EXCHANGE_RING : NBODY_EXCHANGE_ALLGATHER;
        cfg.transport = peerCopy ? NBODY_TRANSPORT_PEER_COPY : NBODY_TRANSPORT_RCCL;
        cfg.body_order = mortonOrder ? NBODY_ORDER_MORTON : NBODY_ORDER_GIVEN;  // stored along a Morton curve, downloads undo it
        check(nbody_multi_create(&m_, &cfg, devices.data(), (int)devices.size()), "nbody_multi_create");
        n_ = numBodies;
    }
    // One rank per process (mpirun / torchrun --no-python / a job script): rank 0 calls uniqueId() and hands the bytes to the
    // other ranks by any channel; every rank then calls initializeRank with them.  From setState on all calls are collective.
    static std::vector<unsigned char> uniqueId()
    {
        std::vector<unsigned char> id(NBODY_UNIQUE_ID_BYTES);
        if (nbody_multi_unique_id(id.data()) != NBODY_OK)
            throw std::runtime_error(std::string("nbody_multi_unique_id: ") + nbody_multi_last_error(nullptr));
        return id;
    }
    void initializeRank(std::int64_t numBodies, int device, int rank, int worldSize, const std::vector<unsigned char> &id,
                        bool pairOnce = false, bool kickDriftKick = false, bool ring = false, std::int64_t splitLen = 0,
                        bool mortonOrder = false, bool autoMode = false)
    {
        if (id.size() != NBODY_UNIQUE_ID_BYTES)
            throw std::runtime_error("MultiSystem::initializeRank: the unique id has NBODY_UNIQUE_ID_BYTES bytes");
        nbody_multi_destroy(m_);
        m_ = nullptr;
        nbody_multi_config cfg{};
        cfg.n_bodies = numBodies;
        cfg.split_len = splitLen;
        cfg.force_mode = autoMode ? NBODY_FORCE_AUTO : pairOnce ? NBODY_FORCE_SYMMETRIC : NBODY_FORCE_ONE_SIDED;
        cfg.integrator = kickDriftKick ? NBODY_INTEGRATOR_KDK : NBODY_INTEGRATOR_KICK_DRIFT;
        cfg.exchange = ring ? NBODY_EXCHANGE_RING : NBODY_EXCHANGE_ALLGATHER;
        cfg.transport = NBODY_TRANSPORT_RCCL;
        cfg.body_order = mortonOrder ? NBODY_ORDER_MORTON : NBODY_ORDER_GIVEN;
        check(nbody_multi_create_rank(&m_, &cfg, device, rank, worldSize, id.data()), "nbody_multi_create_rank");
        n_ = numBodies;
    }
    void setState(const float *xyzm, const float *xyzw) { check(nbody_multi_set_state(m_, xyzm, xyzw), "nbody_multi_set_state"); }
    // the reference's two setters, independent copies (kernel.cu:163-188)
    void setParticlesPosition(const float *xyzm) { check(nbody_multi_set_positions(m_, xyzm), "nbody_multi_set_positions"); }
    void setParticlesVelocity(const float *xyzw) { check(nbody_multi_set_velocities(m_, xyzw), "nbody_multi_set_velocities"); }
    void setParticleSoftening(const float *hostEps)
    {
        check(nbody_multi_set_particle_softening(m_, hostEps), "nbody_multi_set_particle_softening");
    }
    void download(float *xyzm, float *xyzw) { check(nbody_multi_download(m_, xyzm, xyzw), "nbody_multi_download"); }
    void reorder() { check(nbody_multi_reorder(m_), "nbody_multi_reorder"); }  // mortonOrder: a new curve through the current positions
    void setReorderPeriod(std::int64_t steps) { check(nbody_multi_set_reorder_period(m_, steps), "nbody_multi_set_reorder_period"); }
    void step(float dt = kTimeTick, float softening = kSofteningVersion3) { check(nbody_multi_step(m_, dt, softening), "nbody_multi_step"); }
    void stepN(int k, float dt, float softening) { check(nbody_multi_step_n(m_, k, dt, softening), "nbody_multi_step_n"); }
    System::Energy energy(float softening)
    {
        double e[3];
        check(nbody_multi_energy(m_, softening, e), "nbody_multi_energy");
        return {e[0], e[1], e[2]};
    }
    std::vector<double> momentum()
    {
        std::vector<double> p(4);
        check(nbody_multi_momentum(m_, p.data()), "nbody_multi_momentum");
        return p;
    }
    bool replicasIdentical()
    {
        std::uint64_t c[2];
        check(nbody_multi_replica_checksums(m_, c), "nbody_multi_replica_checksums");
        return c[0] == c[1];
    }
    // kernels of the shard contexts and the exchanges (nbody_multi_timing_*: HIP events on the streams they run on)
    void timing(bool on) { check(nbody_multi_timing_enable(m_, on ? 1 : 0), "nbody_multi_timing_enable"); }
    // Totals of one local rank since the last read (sums of event-pair durations, ms): where its steps went.
    struct RankTiming {
        std::int64_t steps;
        double hostEnqueueMs, forceMs, updateMs, auxMs, posExchangeCommMs, posExchangeWaitMs, columnSumExchangeMs, reorderMs;
        std::int64_t forceLaunches, updateLaunches, reorders;
    };
    RankTiming readRankTiming(int localIndex)
    {
        double v[16];
        check(nbody_multi_timing_read(m_, localIndex, v), "nbody_multi_timing_read");
        return {(std::int64_t)v[0], v[1], v[2], v[4], v[6], v[8], v[10], v[12], v[14],
                (std::int64_t)v[3], (std::int64_t)v[5], (std::int64_t)v[15]};
    }
    // local rank 0's kernels, in the shape of System::readTiming
    System::Timing readTiming()
    {
        const RankTiming r = readRankTiming(0);
        return {r.forceMs, r.updateMs, r.forceLaunches, r.updateLaunches};
    }
    std::vector<std::int64_t> info()
    {
        std::vector<std::int64_t> v(8);
        check(nbody_multi_info(m_, v.data()), "nbody_multi_info");
        return v;
    }
    std::int64_t numBodies() const { return n_; }
    nbody_multi *handle() { return m_; }

private:
    void check(int status, const char *what)
    {
        if (status != NBODY_OK)
            throw std::runtime_error(std::string(what) + ": " + nbody_multi_last_error(m_) + " (" + nbody_status_string(status) + ")");
    }
    nbody_multi *m_ = nullptr;
    std::int64_t n_ = 0;
};

// B independent systems of up to maxBodies (<= NBODY_BATCH_MAX_BODIES) bodies stepped together (nbody_batch_*): the state
// lives in caller-owned device arrays of B x maxBodies float4, system s at [s * maxBodies, s * maxBodies + counts[s]).
class Batch {
public:
    Batch() = default;
    Batch(std::int64_t numSystems, std::int64_t maxBodies, int device = 0) { create(numSystems, maxBodies, device); }
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    ~Batch() { nbody_batch_destroy(b_); }

    void create(std::int64_t numSystems, std::int64_t maxBodies, int device = 0)
    {
        nbody_batch_destroy(b_);
        b_ = nullptr;
        check(nbody_batch_create(&b_, device, numSystems, maxBodies), "nbody_batch_create");
        systems_ = numSystems;
        maxBodies_ = maxBodies;
    }
    void setCounts(const std::vector<std::int64_t> &counts)
    {
        if ((std::int64_t)counts.size() != systems_)
            throw std::runtime_error("Batch::setCounts: one count per system");
        check(nbody_batch_set_counts(b_, counts.data()), "nbody_batch_set_counts");
    }
    void kickDriftKick(bool on)
    {
        check(nbody_batch_set_integrator(b_, on ? NBODY_INTEGRATOR_KDK : NBODY_INTEGRATOR_KICK_DRIFT), "nbody_batch_set_integrator");
    }
    // NBODY_INTEGRATOR_KICK_DRIFT, NBODY_INTEGRATOR_KDK or NBODY_INTEGRATOR_HERMITE (the batch's fourth-order scheme)
    void setIntegrator(int integrator) { check(nbody_batch_set_integrator(b_, integrator), "nbody_batch_set_integrator"); }
    void invalidateForces() { check(nbody_batch_invalidate_forces(b_), "nbody_batch_invalidate_forces"); }
    void setStream(void *hipStream) { check(nbody_batch_set_stream(b_, hipStream), "nbody_batch_set_stream"); }
    // k steps on the device arrays; returns with the work complete (stepNAsync: enqueued only, sync() waits)
    void stepN(float *dPositions, float *dVelocities, int k, float dt = kTimeTick, float softening = kSofteningVersion3)
    {
        check(nbody_batch_step_n_on(b_, dPositions, dVelocities, k, dt, softening), "nbody_batch_step_n_on");
    }
    void stepNAsync(float *dPositions, float *dVelocities, int k, float dt = kTimeTick, float softening = kSofteningVersion3)
    {
        check(nbody_batch_step_n_async(b_, dPositions, dVelocities, k, dt, softening), "nbody_batch_step_n_async");
    }
    void sync() { check(nbody_batch_sync(b_), "nbody_batch_sync"); }
    // Adaptive shared steps (NBODY_INTEGRATOR_HERMITE only, nbody_batch_evolve.h): every system advances by
    // nIntervals x cfg.dt_max on its own step; returns with the work complete.  Throws when a system runs out of
    // cfg.max_steps: evolveStats() then tells where each system stands, and the same call again continues.
    struct EvolveStats {
        std::vector<std::int64_t> steps, clamped, ticks;
        std::vector<int> minLevel, maxLevel;
    };
    void evolve(float *dPositions, float *dVelocities, std::int64_t nIntervals, const nbody_batch_evolve_config &cfg)
    {
        check(nbody_batch_evolve_on(b_, dPositions, dVelocities, nIntervals, &cfg), "nbody_batch_evolve_on");
    }
    EvolveStats evolveStats()
    {
        EvolveStats s;
        const size_t n = (size_t)systems_;
        s.steps.resize(n), s.clamped.resize(n), s.ticks.resize(n), s.minLevel.resize(n), s.maxLevel.resize(n);
        check(nbody_batch_evolve_stats(b_, s.steps.data(), s.minLevel.data(), s.maxLevel.data(), s.clamped.data(), s.ticks.data()),
              "nbody_batch_evolve_stats");
        return s;
    }
    // Stopping conditions of evolve (nbody_batch_stop.h): a system's run ends after the step in which two bodies come
    // within collisionRadius or a body is farther than escapeRadius from the origin (0: off).  stops(): per system the
    // reason (bit 1 collision, bit 2 escape; 0: not stopped), the tick, the colliding pair i < j, its separation, the escaper.
    struct Stops {
        std::vector<int> reason, pairI, pairJ, escaper;
        std::vector<std::int64_t> ticks;
        std::vector<float> separation;
    };
    void setStopConditions(float collisionRadius, float escapeRadius)
    {
        const nbody_batch_stop_config cfg = {collisionRadius, escapeRadius};
        check(nbody_batch_stop_set(b_, &cfg), "nbody_batch_stop_set");
    }
    Stops stops()
    {
        Stops s;
        const size_t n = (size_t)systems_;
        s.reason.resize(n), s.pairI.resize(n), s.pairJ.resize(n), s.escaper.resize(n), s.ticks.resize(n), s.separation.resize(n);
        check(nbody_batch_stop_read(b_, s.reason.data(), s.ticks.data(), s.pairI.data(), s.pairJ.data(), s.separation.data(),
                                    s.escaper.data()),
              "nbody_batch_stop_read");
        return s;
    }
    // Collision action of evolve (nbody_batch_merge.h): with merge the colliding pair becomes one body in the survivor's
    // slot, the count drops and the run goes on.  mergers(): per system the number of mergers and its first logCapacity
    // events (events[s * logCapacity + e]); counts(): the body counts as evolve left them.
    struct Mergers {
        std::vector<std::int64_t> count;
        std::vector<nbody_batch_merge_event> events;
        int logCapacity = 0;
    };
    void setCollisionAction(bool merge, int logCapacity = 8)
    {
        const nbody_batch_merge_config cfg = {merge ? NBODY_BATCH_ON_COLLISION_MERGE : NBODY_BATCH_ON_COLLISION_STOP, logCapacity};
        check(nbody_batch_merge_set(b_, &cfg), "nbody_batch_merge_set");
        logCapacity_ = logCapacity;
    }
    Mergers mergers()
    {
        Mergers m;
        m.logCapacity = logCapacity_;
        m.count.resize((size_t)systems_);
        m.events.resize((size_t)systems_ * (size_t)logCapacity_);
        check(nbody_batch_merge_read(b_, m.count.data(), m.events.empty() ? nullptr : m.events.data()), "nbody_batch_merge_read");
        return m;
    }
    std::vector<std::int64_t> counts()
    {
        std::vector<std::int64_t> c((size_t)systems_);
        check(nbody_batch_get_counts(b_, c.data()), "nbody_batch_get_counts");
        return c;
    }
    // Per-body collision radii of evolve (nbody_batch_radii.h): numSystems x maxBodies values laid out like the positions;
    // two bodies collide within the sum of their radii, and a merged body's radius is cbrt(R_i^3 + R_j^3).  An empty
    // vector switches radii off.  radii(): the radii as the library left them (throws when none are set).
    void setRadii(const std::vector<float> &radii)
    {
        if (!radii.empty() && (std::int64_t)radii.size() != systems_ * maxBodies_)
            throw std::runtime_error("Batch::setRadii: numSystems x maxBodies radii, or none");
        check(nbody_batch_radii_set(b_, radii.empty() ? nullptr : radii.data()), "nbody_batch_radii_set");
    }
    std::vector<float> radii()
    {
        std::vector<float> r((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_radii_read(b_, r.data()), "nbody_batch_radii_read");
        return r;
    }
    // Test particles (nbody_batch_massive.h): numSystems values; the first min(massive[s], counts[s]) bodies of system s
    // are massive, the bodies after them feel those and exert no force (every integrator, and evolve without stopping
    // conditions or radii).  An empty vector switches the feature off.  massiveCounts(): the values as set (throws when off).
    void setMassiveCounts(const std::vector<std::int64_t> &massive)
    {
        if (!massive.empty() && (std::int64_t)massive.size() != systems_)
            throw std::runtime_error("Batch::setMassiveCounts: numSystems massive counts, or none");
        check(nbody_batch_massive_set(b_, massive.empty() ? nullptr : massive.data()), "nbody_batch_massive_set");
    }
    std::vector<std::int64_t> massiveCounts()
    {
        std::vector<std::int64_t> m((size_t)systems_);
        check(nbody_batch_massive_read(b_, m.data()), "nbody_batch_massive_read");
        return m;
    }
    // Tracer fates (nbody_batch_fate.h): with remove, evolve accepts massive counts together with stopping conditions or
    // radii; a test particle that hits a massive body or escapes is frozen with a fate and its system carries on.  fates():
    // per body (fate[s * maxBodies + i], ...) and per system (hit[s], escaped[s]); throws while the action is refuse.
    struct Fates {
        std::vector<int> fate, target;
        std::vector<std::int64_t> ticks, hit, escaped;
        std::vector<float> separation, relativeSpeed;
    };
    void setTracerAction(bool remove)
    {
        const nbody_batch_fate_config cfg = {remove ? NBODY_BATCH_TRACERS_REMOVE : NBODY_BATCH_TRACERS_REFUSE};
        check(nbody_batch_fate_set(b_, &cfg), "nbody_batch_fate_set");
    }
    Fates fates()
    {
        Fates f;
        const size_t n = (size_t)systems_ * (size_t)maxBodies_;
        f.fate.resize(n), f.target.resize(n), f.ticks.resize(n), f.separation.resize(n), f.relativeSpeed.resize(n);
        f.hit.resize((size_t)systems_), f.escaped.resize((size_t)systems_);
        check(nbody_batch_fate_read(b_, f.fate.data(), f.ticks.data(), f.target.data(), f.separation.data(), f.relativeSpeed.data()),
              "nbody_batch_fate_read");
        check(nbody_batch_fate_count(b_, f.hit.data(), f.escaped.data()), "nbody_batch_fate_count");
        return f;
    }
    // Accreting tracers (nbody_batch_accrete.h): with accrete, a test particle that hits a massive body gives it its mass
    // word -- the body grows, the tracer's mass word becomes 0 -- and the system is evaluated afresh and carries on.
    // accretions(): given[s * maxBodies + i], the mass tracer i gave, and count[s]; throws while the action is remove.
    struct Accretions {
        std::vector<float> given;
        std::vector<std::int64_t> count;
    };
    void setHitAction(bool accrete)
    {
        const nbody_batch_accrete_config cfg = {accrete ? NBODY_BATCH_ON_HIT_ACCRETE : NBODY_BATCH_ON_HIT_REMOVE};
        check(nbody_batch_accrete_set(b_, &cfg), "nbody_batch_accrete_set");
    }
    Accretions accretions()
    {
        Accretions a;
        a.given.resize((size_t)systems_ * (size_t)maxBodies_);
        a.count.resize((size_t)systems_);
        check(nbody_batch_accrete_read(b_, a.given.data(), a.count.data()), "nbody_batch_accrete_read");
        return a;
    }
    // External field of evolve (nbody_batch_field.h): numSystems x nComponents components (nComponents in [1, 4]),
    // components[s * nComponents + c], a static Plummer, logarithmic-halo or Miyamoto-Nagai background centred on the origin
    // that every body feels next to the pair forces.  An empty vector switches the field off.  field(): the components as
    // set (throws when off); fieldPotential(): numSystems x maxBodies values of the field's potential at the positions, fp64.
    void setField(const std::vector<nbody_batch_field_component> &components, int nComponents)
    {
        if (!components.empty() && (nComponents < 1 || (std::int64_t)components.size() != systems_ * nComponents))
            throw std::runtime_error("Batch::setField: numSystems x nComponents components, or none");
        check(nbody_batch_field_set(b_, components.empty() ? nullptr : components.data(), nComponents), "nbody_batch_field_set");
    }
    std::vector<nbody_batch_field_component> field()
    {
        std::vector<nbody_batch_field_component> c((size_t)systems_ * NBODY_BATCH_FIELD_MAX_COMPONENTS);
        int n = 0;
        check(nbody_batch_field_read(b_, c.data(), &n), "nbody_batch_field_read");
        c.resize((size_t)systems_ * (size_t)n);
        return c;
    }
    std::vector<double> fieldPotential(const float *dPositions)
    {
        std::vector<double> phi((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_field_potential(b_, dPositions, phi.data()), "nbody_batch_field_potential");
        return phi;
    }
    // Bound pairs (nbody_batch_pairs.h): numSystems x maxBodies records laid out like the positions -- every body's partner by
    // the smallest two-body energy, whether the choice is mutual, and the pair's energy, semi-major axis, eccentricity,
    // inclination and separation in fp64 -- found on the device from the state in the caller's buffers.  Changes nothing the
    // handle keeps.  binaries(): per system the mutual pairs with negative energy of the last pairs() call (throws before one).
    std::vector<nbody_batch_pair_record> pairs(const float *dPositions, const float *dVelocities)
    {
        std::vector<nbody_batch_pair_record> r((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_pairs(b_, dPositions, dVelocities, r.data()), "nbody_batch_pairs");
        return r;
    }
    std::vector<std::int64_t> binaries()
    {
        std::vector<std::int64_t> n((size_t)systems_);
        check(nbody_batch_pairs_binaries(b_, n.data()), "nbody_batch_pairs_binaries");
        return n;
    }
    // Cluster structure (nbody_batch_structure.h): per system the density centre, the core radius and density, the total weight
    // and the Lagrangian radii about the centre that enclose the given fractions (up to eight), from every body's k-th
    // neighbour density (1 <= k <= 8; weight NBODY_BATCH_WEIGHT_MASS or _NUMBER), found on the device from the positions in the
    // caller's buffer.  The second form also fills numSystems x maxBodies per-body records laid out like the positions; the first
    // copies 120 bytes per system and nothing per body.  Changes nothing the handle keeps.
    std::vector<nbody_batch_structure_system> structure(const float *dPositions, int k, int weight, const std::vector<double> &fractions)
    {
        std::vector<nbody_batch_structure_system> s((size_t)systems_);
        check(nbody_batch_structure(b_, dPositions, k, weight, fractions.empty() ? nullptr : fractions.data(), (int)fractions.size(),
                                    s.data(), nullptr), "nbody_batch_structure");
        return s;
    }
    std::vector<nbody_batch_structure_system> structure(const float *dPositions, int k, int weight, const std::vector<double> &fractions,
                                                        std::vector<nbody_batch_structure_body> &bodies)
    {
        std::vector<nbody_batch_structure_system> s((size_t)systems_);
        bodies.resize((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_structure(b_, dPositions, k, weight, fractions.empty() ? nullptr : fractions.data(), (int)fractions.size(),
                                    s.data(), bodies.data()), "nbody_batch_structure");
        return s;
    }
    // Bound members (nbody_batch_members.h): iterative unbinding on the device from the state in the caller's buffers -- per
    // system the bound mass, its centre and velocity, the kinetic and potential energy of the final member sources, the member
    // counts and the iterations evaluated (1 <= maxIterations <= 64).  initial: numSystems x maxBodies bytes that pick the
    // starting set, or nullptr for every body.  The second form also fills numSystems x maxBodies per-body records (potential,
    // energy, member, removed_at) laid out like the positions; the first copies 88 bytes per system and nothing per body.
    // Changes nothing the handle keeps.
    std::vector<nbody_batch_member_system> members(const float *dPositions, const float *dVelocities, float softening,
                                                   int maxIterations = 32, const unsigned char *initial = nullptr)
    {
        std::vector<nbody_batch_member_system> s((size_t)systems_);
        check(nbody_batch_members(b_, dPositions, dVelocities, softening, maxIterations, initial, s.data(), nullptr),
              "nbody_batch_members");
        return s;
    }
    std::vector<nbody_batch_member_system> members(const float *dPositions, const float *dVelocities, float softening,
                                                   int maxIterations, const unsigned char *initial,
                                                   std::vector<nbody_batch_member_body> &bodies)
    {
        std::vector<nbody_batch_member_system> s((size_t)systems_);
        bodies.resize((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_members(b_, dPositions, dVelocities, softening, maxIterations, initial, s.data(), bodies.data()),
              "nbody_batch_members");
        return s;
    }
    // Hierarchies (nbody_batch_hierarchy.h): the nested bound pairs of every system from the state in the caller's buffers --
    // per system the nodes made, the live roots, the levels evaluated (1 <= maxLevels <= 16) and the singles, binaries, triples,
    // higher multiples and unstable roots.  A pair whose worst perturber's tide exceeds tidalTolerance of its own attraction is
    // no node; +inf accepts every bound mutual pair.  The second form also fills numSystems x maxBodies node records and
    // per-body records (parent, root, depth) laid out like the positions; the first copies 40 bytes per system alone.
    // Changes nothing the handle keeps.
    std::vector<nbody_batch_hierarchy_system> hierarchy(const float *dPositions, const float *dVelocities,
                                                        double tidalTolerance = std::numeric_limits<double>::infinity(),
                                                        int maxLevels = 8)
    {
        std::vector<nbody_batch_hierarchy_system> s((size_t)systems_);
        check(nbody_batch_hierarchy(b_, dPositions, dVelocities, tidalTolerance, maxLevels, s.data(), nullptr, nullptr),
              "nbody_batch_hierarchy");
        return s;
    }
    std::vector<nbody_batch_hierarchy_system> hierarchy(const float *dPositions, const float *dVelocities, double tidalTolerance,
                                                        int maxLevels, std::vector<nbody_batch_hierarchy_node> &nodes,
                                                        std::vector<nbody_batch_hierarchy_body> &bodies)
    {
        std::vector<nbody_batch_hierarchy_system> s((size_t)systems_);
        nodes.resize((size_t)systems_ * (size_t)maxBodies_);
        bodies.resize((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_hierarchy(b_, dPositions, dVelocities, tidalTolerance, maxLevels, s.data(), nodes.data(), bodies.data()),
              "nbody_batch_hierarchy");
        return s;
    }
    // Gravity at points (nbody_batch_gravity.h): the acceleration and potential that every system's sources exert at its own
    // bodies (dPoints == nullptr: numSystems x maxBodies records, each body skipping itself) or at numPoints device points
    // {x, y, z, ignored} per system (pointCounts: numSystems values in [0, numPoints], or nullptr for numPoints everywhere).
    // The second form also fills six floats {xx, xy, xz, yy, yz, zz} of the tidal tensor per row.  Changes nothing the handle
    // keeps.
    std::vector<nbody_batch_gravity_record> gravityAt(const float *dPositions, float softening, const float *dPoints = nullptr,
                                                      int64_t numPoints = 0, const int64_t *pointCounts = nullptr)
    {
        std::vector<nbody_batch_gravity_record> r((size_t)systems_ * (size_t)(dPoints ? numPoints : maxBodies_));
        check(nbody_batch_gravity(b_, dPositions, dPoints, numPoints, pointCounts, softening, r.data(), nullptr),
              "nbody_batch_gravity");
        return r;
    }
    std::vector<nbody_batch_gravity_record> gravityAt(const float *dPositions, float softening, const float *dPoints,
                                                      int64_t numPoints, const int64_t *pointCounts, std::vector<float> &tidal)
    {
        std::vector<nbody_batch_gravity_record> r((size_t)systems_ * (size_t)(dPoints ? numPoints : maxBodies_));
        tidal.resize(r.size() * 6);
        check(nbody_batch_gravity(b_, dPositions, dPoints, numPoints, pointCounts, softening, r.data(), tidal.data()),
              "nbody_batch_gravity");
        return r;
    }
    // Groups (nbody_batch_groups.h): friends-of-friends clumps from the state in the caller's buffers.  linkingLengths: one
    // value per system (host).  Per system the groups with at least minMembers members, the bodies in them, the singles, the
    // largest group, the sweeps run (1 <= maxSweeps <= 64) and whether they converged.  groups and bodies, where given, are
    // resized to numSystems x maxBodies and take the per-slot group records (filled at a group's root) and the per-body
    // {group, size}; nullptr skips that copy.  Changes nothing the handle keeps.
    std::vector<nbody_batch_group_system> groups(const float *dPositions, const float *dVelocities,
                                                 const std::vector<float> &linkingLengths, int minMembers = 2,
                                                 int weight = NBODY_BATCH_WEIGHT_MASS, int maxSweeps = NBODY_BATCH_GROUPS_MAX_SWEEPS,
                                                 std::vector<nbody_batch_group_record> *groups = nullptr,
                                                 std::vector<nbody_batch_group_body> *bodies = nullptr)
    {
        if (linkingLengths.size() != (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::groups: one linking length per system");
        std::vector<nbody_batch_group_system> s((size_t)systems_);
        if (groups)
            groups->resize((size_t)systems_ * (size_t)maxBodies_);
        if (bodies)
            bodies->resize((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_groups(b_, dPositions, dVelocities, linkingLengths.data(), minMembers, weight, maxSweeps, s.data(),
                                 groups ? groups->data() : nullptr, bodies ? bodies->data() : nullptr),
              "nbody_batch_groups");
        return s;
    }
    // Spanning trees (nbody_batch_span.h): the Euclidean minimum spanning tree of every system from the positions in the
    // caller's buffer.  subset: empty for all bodies, or numSystems x maxBodies bytes (host), non-zero where a body is a
    // vertex.  Per system the edges, the selected bodies, the rounds run, the total and the longest length and, with
    // separations, the mean separation of the selected bodies.  edges and bodies, where given, are resized to
    // numSystems x maxBodies and take the per-slot edges in ascending order and the per-body {degree, nearest}; nullptr skips
    // that copy.  Changes nothing the handle keeps.
    std::vector<nbody_batch_span_system> spanningTree(const float *dPositions, const std::vector<unsigned char> &subset = {},
                                                      bool separations = false,
                                                      std::vector<nbody_batch_span_edge> *edges = nullptr,
                                                      std::vector<nbody_batch_span_body> *bodies = nullptr)
    {
        if (!subset.empty() && subset.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::spanningTree: one subset byte per slot, or none");
        std::vector<nbody_batch_span_system> s((size_t)systems_);
        if (edges)
            edges->resize((size_t)systems_ * (size_t)maxBodies_);
        if (bodies)
            bodies->resize((size_t)systems_ * (size_t)maxBodies_);
        check(nbody_batch_span(b_, dPositions, subset.empty() ? nullptr : subset.data(), separations ? 1 : 0, s.data(),
                               edges ? edges->data() : nullptr, bodies ? bodies->data() : nullptr),
              "nbody_batch_span");
        return s;
    }
    // Nearest-neighbour lists (nbody_batch_neighbours.h): for every body of every system its k (1 ... 8) nearest sources
    // from the positions in the caller's buffer.  radii: empty, or one radius per system (host) for the bodies' `within`
    // counts.  sources: empty for all bodies, or numSystems x maxBodies bytes (host), non-zero where a body is a source; every
    // body gets a list all the same.  Per system the rows, the sources, the listed, complete and mutual rows and the mean
    // nearest and k-th distances.  bodies, where given, is resized to numSystems x maxBodies and takes the per-body {found,
    // within}; index and r2, given both or neither, are resized to numSystems x maxBodies x k and take the lists (-1 and +inf
    // from `found` on); nullptr skips that copy.  Changes nothing the handle keeps.
    std::vector<nbody_batch_neighbour_system> neighbours(const float *dPositions, int k = 6, const std::vector<float> &radii = {},
                                                         const std::vector<unsigned char> &sources = {},
                                                         std::vector<nbody_batch_neighbour_body> *bodies = nullptr,
                                                         std::vector<int> *index = nullptr, std::vector<float> *r2 = nullptr)
    {
        if (!radii.empty() && radii.size() != (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::neighbours: one radius per system, or none");
        if (!sources.empty() && sources.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::neighbours: one source byte per slot, or none");
        if (k < 1 || k > NBODY_BATCH_NEIGHBOURS_MAX)
            throw std::invalid_argument("nbody::Batch::neighbours: k must be 1 ... 8");
        std::vector<nbody_batch_neighbour_system> s((size_t)systems_);
        if (bodies)
            bodies->resize((size_t)systems_ * (size_t)maxBodies_);
        if (index)
            index->resize((size_t)systems_ * (size_t)maxBodies_ * (size_t)k);
        if (r2)
            r2->resize((size_t)systems_ * (size_t)maxBodies_ * (size_t)k);
        check(nbody_batch_neighbours(b_, dPositions, k, radii.empty() ? nullptr : radii.data(),
                                     sources.empty() ? nullptr : sources.data(), s.data(), bodies ? bodies->data() : nullptr,
                                     index ? index->data() : nullptr, r2 ? r2->data() : nullptr),
              "nbody_batch_neighbours");
        return s;
    }
    // Pair-separation counts (nbody_batch_correlation.h): for every system the ordered pairs (row, source) in each bin of
    // separation, from the positions in the caller's buffer.  edges: bins + 1 ascending values >= 0 (host), one set for all
    // systems, or numSystems sets, one per system; bins is 1 ... 32.  rows, sources: empty for all bodies, or numSystems x
    // maxBodies bytes (host), non-zero where a body is a row or a source.  Per system the rows, the sources, those that are
    // both, the pairs examined and those below the first edge, above the last and unmeasured.  counts, where given, is resized
    // to numSystems x bins and takes the bins; nullptr skips that copy.  Changes nothing the handle keeps.
    std::vector<nbody_batch_correlation_system> correlation(const float *dPositions, int bins, const std::vector<float> &edges,
                                                            const std::vector<unsigned char> &rows = {},
                                                            const std::vector<unsigned char> &sources = {},
                                                            std::vector<unsigned int> *counts = nullptr)
    {
        if (bins < 1 || bins > NBODY_BATCH_CORRELATION_MAX_BINS)
            throw std::invalid_argument("nbody::Batch::correlation: bins must be 1 ... 32");
        const size_t set = (size_t)bins + 1;
        if (edges.size() != set && edges.size() != (size_t)systems_ * set)
            throw std::invalid_argument("nbody::Batch::correlation: bins + 1 edges, or as many per system");
        if (!rows.empty() && rows.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::correlation: one row byte per slot, or none");
        if (!sources.empty() && sources.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::correlation: one source byte per slot, or none");
        std::vector<nbody_batch_correlation_system> s((size_t)systems_);
        if (counts)
            counts->resize((size_t)systems_ * (size_t)bins);
        const int perSystem = edges.size() == set ? 0 : 1;
        check(nbody_batch_correlation(b_, dPositions, bins, edges.data(), perSystem, rows.empty() ? nullptr : rows.data(),
                                      sources.empty() ? nullptr : sources.data(), s.data(), counts ? counts->data() : nullptr),
              "nbody_batch_correlation");
        return s;
    }
    // Contact lists (nbody_batch_contacts.h): for every system every unordered pair of bodies within a radius of each other, or
    // within the sum of their two radii, from the positions in the caller's buffer.  threshold: numSystems values (host), one
    // radius per system, or numSystems x maxBodies values, one radius per slot.  subset: empty for all bodies, or numSystems x
    // maxBodies bytes (host), non-zero where a body takes part.  capacity: the list entries kept per system; 0 only counts.
    // Per system the bodies taking part, those with a contact, the largest degree, the contacts (exact whatever the capacity),
    // those stored and the closest.  list, where given, is resized to numSystems x capacity and takes the entries (i, j, r2),
    // i < j, ascending in i and then in j, {-1, -1, +inf} from `stored` on; it must be given iff capacity > 0.  bodies, where
    // given, is resized to numSystems x maxBodies and takes the per-body records.  Changes nothing the handle keeps.
    std::vector<nbody_batch_contact_system> contacts(const float *dPositions, const std::vector<float> &threshold,
                                                     long long capacity = 0, std::vector<nbody_batch_contact> *list = nullptr,
                                                     const std::vector<unsigned char> &subset = {},
                                                     std::vector<nbody_batch_contact_body> *bodies = nullptr)
    {
        const size_t slots = (size_t)systems_ * (size_t)maxBodies_;
        const bool perBody = threshold.size() == slots && threshold.size() != (size_t)systems_;
        if (threshold.size() != (size_t)systems_ && !perBody)
            throw std::invalid_argument("nbody::Batch::contacts: one radius per system, or one per slot");
        if (!subset.empty() && subset.size() != slots)
            throw std::invalid_argument("nbody::Batch::contacts: one subset byte per slot, or none");
        if (capacity < 0 || (capacity > 0) != (list != nullptr))
            throw std::invalid_argument("nbody::Batch::contacts: a list iff capacity > 0");
        if (capacity > NBODY_BATCH_CONTACTS_MAX_ENTRIES / (long long)systems_)
            throw std::invalid_argument("nbody::Batch::contacts: numSystems x capacity must not exceed 2^28");
        std::vector<nbody_batch_contact_system> s((size_t)systems_);
        if (list)
            list->resize((size_t)systems_ * (size_t)capacity);
        if (bodies)
            bodies->resize(slots);
        check(nbody_batch_contacts(b_, dPositions, perBody ? nullptr : threshold.data(), perBody ? threshold.data() : nullptr,
                                   subset.empty() ? nullptr : subset.data(), capacity, s.data(), bodies ? bodies->data() : nullptr,
                                   list ? list->data() : nullptr),
              "nbody_batch_contacts");
        return s;
    }
    // Approach lists (nbody_batch_approaches.h): for every system every unordered pair of bodies that comes within a radius, or
    // within the sum of its two radii, before a horizon, with both bodies moved on straight lines at the velocities in the
    // caller's buffer.  horizon: numSystems values (host), finite and >= 0.  threshold, subset, capacity, list and bodies: as in
    // contacts().  Per system the bodies taking part, those with an approach, the largest degree, the approaches (exact whatever
    // the capacity), those stored, and the pairs within reach now, passing before the horizon and still closing at it.  list
    // takes the entries (i, j, r2, rv, v2, phase), i < j, ascending in i and then in j, {-1, -1, +inf, 0, 0, -1} from `stored`
    // on.  Changes nothing the handle keeps.
    std::vector<nbody_batch_approach_system> approaches(const float *dPositions, const float *dVelocities, const std::vector<float> &horizon,
                                                        const std::vector<float> &threshold, long long capacity = 0,
                                                        std::vector<nbody_batch_approach> *list = nullptr,
                                                        const std::vector<unsigned char> &subset = {},
                                                        std::vector<nbody_batch_approach_body> *bodies = nullptr)
    {
        const size_t slots = (size_t)systems_ * (size_t)maxBodies_;
        const bool perBody = threshold.size() == slots && threshold.size() != (size_t)systems_;
        if (horizon.size() != (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::approaches: one horizon per system");
        if (threshold.size() != (size_t)systems_ && !perBody)
            throw std::invalid_argument("nbody::Batch::approaches: one radius per system, or one per slot");
        if (!subset.empty() && subset.size() != slots)
            throw std::invalid_argument("nbody::Batch::approaches: one subset byte per slot, or none");
        if (capacity < 0 || (capacity > 0) != (list != nullptr))
            throw std::invalid_argument("nbody::Batch::approaches: a list iff capacity > 0");
        if (capacity > NBODY_BATCH_APPROACHES_MAX_ENTRIES / (long long)systems_)
            throw std::invalid_argument("nbody::Batch::approaches: numSystems x capacity must not exceed 2^27");
        std::vector<nbody_batch_approach_system> s((size_t)systems_);
        if (list)
            list->resize((size_t)systems_ * (size_t)capacity);
        if (bodies)
            bodies->resize(slots);
        check(nbody_batch_approaches(b_, dPositions, dVelocities, horizon.data(), perBody ? nullptr : threshold.data(),
                                     perBody ? threshold.data() : nullptr, subset.empty() ? nullptr : subset.data(), capacity,
                                     s.data(), bodies ? bodies->data() : nullptr, list ? list->data() : nullptr),
              "nbody_batch_approaches");
        return s;
    }
    // Radial profiles (nbody_batch_radial.h): for every system the bodies in up to 32 shells about a centre.  edges: shells + 1
    // ascending values >= 0 for all systems, or numSystems sets of them (told apart by the size: pass `shells`).  centre and
    // velocity: empty for zeros, or numSystems x 3 values.  weight: NBODY_BATCH_WEIGHT_MASS or _NUMBER.  projected: -1, or the
    // axis the radius leaves out.  subset: empty, or one byte per slot.  Returns the per-system records; records takes the
    // shells of every system (shell t of system s at s * shells + t) and bodies the per-body records.  Every sum runs over the
    // shell's members in ascending body index.  Changes nothing the handle keeps.
    std::vector<nbody_batch_radial_system> radialProfile(const float *dPositions, const float *dVelocities, int shells,
                                                         const std::vector<double> &edges,
                                                         std::vector<nbody_batch_radial_shell> *records = nullptr,
                                                         const std::vector<double> &centre = {}, const std::vector<double> &velocity = {},
                                                         int weight = NBODY_BATCH_WEIGHT_MASS, int projected = -1,
                                                         const std::vector<unsigned char> &subset = {},
                                                         std::vector<nbody_batch_radial_body> *bodies = nullptr)
    {
        const size_t slots = (size_t)systems_ * (size_t)maxBodies_;
        if (shells < 1 || shells > NBODY_BATCH_RADIAL_MAX_SHELLS)
            throw std::invalid_argument("nbody::Batch::radialProfile: shells must be 1 ... 32");
        const size_t given = (size_t)shells + 1;
        const bool perSystem = edges.size() == given * (size_t)systems_ && systems_ != 1;
        if (edges.size() != given && !perSystem)
            throw std::invalid_argument("nbody::Batch::radialProfile: shells + 1 edges, or as many per system");
        if ((!centre.empty() && centre.size() != 3 * (size_t)systems_) || (!velocity.empty() && velocity.size() != 3 * (size_t)systems_))
            throw std::invalid_argument("nbody::Batch::radialProfile: three values per system for centre and velocity, or none");
        if (!subset.empty() && subset.size() != slots)
            throw std::invalid_argument("nbody::Batch::radialProfile: one subset byte per slot, or none");
        std::vector<nbody_batch_radial_system> s((size_t)systems_);
        if (records)
            records->resize((size_t)systems_ * (size_t)shells);
        if (bodies)
            bodies->resize(slots);
        check(nbody_batch_radial_profile(b_, dPositions, dVelocities, shells, edges.data(), perSystem ? 1 : 0,
                                         centre.empty() ? nullptr : centre.data(), velocity.empty() ? nullptr : velocity.data(), weight,
                                         projected, subset.empty() ? nullptr : subset.data(), s.data(),
                                         records ? records->data() : nullptr, bodies ? bodies->data() : nullptr),
              "nbody_batch_radial_profile");
        return s;
    }
    // Surface maps (nbody_batch_surface.h): for every system the bodies in a grid of columns x rows cells (1 ... 64 each) in the
    // plane of a view.  edgesA: columns + 1 ascending values for all systems, or numSystems sets of them; edgesB likewise with
    // rows + 1 (both shared or both per system, told apart by edgesA's size).  centre and velocity: empty for zeros, or
    // numSystems x 3 values.  axes: empty for the identity (A = x, B = y, Q = z), or numSystems x 9 values, the rows A, B and Q
    // of every system.  weight: NBODY_BATCH_WEIGHT_MASS or _NUMBER.  subset: empty, or one byte per slot.  Returns the
    // per-system records; cells takes the cells of every system (cell (i, j) of system s at (s * rows + j) * columns + i) and
    // bodies the per-body records.  Every sum runs over the cell's members in ascending body index.  Changes nothing the
    // handle keeps.
    std::vector<nbody_batch_surface_system> surfaceMap(const float *dPositions, const float *dVelocities, int columns, int rows,
                                                       const std::vector<double> &edgesA, const std::vector<double> &edgesB,
                                                       std::vector<nbody_batch_surface_cell> *cells = nullptr,
                                                       const std::vector<double> &centre = {}, const std::vector<double> &velocity = {},
                                                       const std::vector<double> &axes = {}, int weight = NBODY_BATCH_WEIGHT_MASS,
                                                       const std::vector<unsigned char> &subset = {},
                                                       std::vector<nbody_batch_surface_body> *bodies = nullptr)
    {
        const size_t slots = (size_t)systems_ * (size_t)maxBodies_;
        if (columns < 1 || columns > NBODY_BATCH_SURFACE_MAX_SIDE || rows < 1 || rows > NBODY_BATCH_SURFACE_MAX_SIDE)
            throw std::invalid_argument("nbody::Batch::surfaceMap: columns and rows must be 1 ... 64");
        const size_t givenA = (size_t)columns + 1, givenB = (size_t)rows + 1;
        const bool perSystem = edgesA.size() == givenA * (size_t)systems_ && systems_ != 1;
        if (edgesA.size() != givenA * (perSystem ? (size_t)systems_ : 1) || edgesB.size() != givenB * (perSystem ? (size_t)systems_ : 1))
            throw std::invalid_argument("nbody::Batch::surfaceMap: columns + 1 and rows + 1 edges, or as many per system of both");
        if ((!centre.empty() && centre.size() != 3 * (size_t)systems_) || (!velocity.empty() && velocity.size() != 3 * (size_t)systems_))
            throw std::invalid_argument("nbody::Batch::surfaceMap: three values per system for centre and velocity, or none");
        if (!axes.empty() && axes.size() != 9 * (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::surfaceMap: nine values per system for axes, or none");
        if (!subset.empty() && subset.size() != slots)
            throw std::invalid_argument("nbody::Batch::surfaceMap: one subset byte per slot, or none");
        std::vector<nbody_batch_surface_system> s((size_t)systems_);
        if (cells)
            cells->resize((size_t)systems_ * (size_t)columns * (size_t)rows);
        if (bodies)
            bodies->resize(slots);
        check(nbody_batch_surface_map(b_, dPositions, dVelocities, columns, rows, edgesA.data(), edgesB.data(), perSystem ? 1 : 0,
                                      centre.empty() ? nullptr : centre.data(), velocity.empty() ? nullptr : velocity.data(),
                                      axes.empty() ? nullptr : axes.data(), weight, subset.empty() ? nullptr : subset.data(), s.data(),
                                      cells ? cells->data() : nullptr, bodies ? bodies->data() : nullptr),
              "nbody_batch_surface_map");
        return s;
    }
    // Shapes (nbody_batch_shape.h): for every system and each of `apertures` (1 ... 8) apertures the ellipsoid the iterated
    // moment tensor converges to.  radii: `apertures` values > 0 for all systems, or numSystems sets of them; inner: empty for
    // zeros, or like radii (ellipsoidal shells).  centre and velocity: empty for zeros, or numSystems x 3 values.  weight:
    // NBODY_BATCH_WEIGHT_MASS or _NUMBER.  reduced: the tensor's addends are divided by the squared elliptical radius.  subset:
    // empty, or one byte per slot.  Returns the per-system records; records takes the apertures of every system (aperture a of
    // system s at s * apertures + a) and bodies the per-body membership bits.  Changes nothing the handle keeps.
    std::vector<nbody_batch_shape_system> shape(const float *dPositions, const float *dVelocities, const std::vector<double> &radii,
                                                std::vector<nbody_batch_shape_aperture> *records)
    {
        return shape(dPositions, dVelocities, (int)radii.size(), radii, records);
    }
    std::vector<nbody_batch_shape_system> shape(const float *dPositions, const float *dVelocities, int apertures,
                                                const std::vector<double> &radii, std::vector<nbody_batch_shape_aperture> *records,
                                                const std::vector<double> &inner = {}, const std::vector<double> &centre = {},
                                                const std::vector<double> &velocity = {}, int weight = NBODY_BATCH_WEIGHT_MASS,
                                                bool reduced = true, double tol = 1e-3, int maxIterations = NBODY_BATCH_SHAPE_MAX_ITERATIONS,
                                                int minMembers = 10, const std::vector<unsigned char> &subset = {},
                                                std::vector<nbody_batch_shape_body> *bodies = nullptr)
    {
        const size_t slots = (size_t)systems_ * (size_t)maxBodies_;
        if (apertures < 1 || apertures > NBODY_BATCH_SHAPE_MAX_APERTURES)
            throw std::invalid_argument("nbody::Batch::shape: apertures must be 1 ... 8");
        const bool perSystem = radii.size() == (size_t)apertures * (size_t)systems_ && systems_ != 1;
        if (radii.size() != (size_t)apertures * (perSystem ? (size_t)systems_ : 1) || (!inner.empty() && inner.size() != radii.size()))
            throw std::invalid_argument("nbody::Batch::shape: `apertures` radii, or as many per system, and as many inner radii or none");
        if ((!centre.empty() && centre.size() != 3 * (size_t)systems_) || (!velocity.empty() && velocity.size() != 3 * (size_t)systems_))
            throw std::invalid_argument("nbody::Batch::shape: three values per system for centre and velocity, or none");
        if (!subset.empty() && subset.size() != slots)
            throw std::invalid_argument("nbody::Batch::shape: one subset byte per slot, or none");
        std::vector<nbody_batch_shape_system> s((size_t)systems_);
        if (records)
            records->resize((size_t)systems_ * (size_t)apertures);
        if (bodies)
            bodies->resize(slots);
        check(nbody_batch_shape(b_, dPositions, dVelocities, apertures, radii.data(), inner.empty() ? nullptr : inner.data(),
                                perSystem ? 1 : 0, centre.empty() ? nullptr : centre.data(), velocity.empty() ? nullptr : velocity.data(),
                                weight, reduced ? 1 : 0, tol, maxIterations, minMembers, subset.empty() ? nullptr : subset.data(), s.data(),
                                records ? records->data() : nullptr, bodies ? bodies->data() : nullptr),
              "nbody_batch_shape");
        return s;
    }
    // Pair velocity statistics (nbody_batch_pair_velocities.h): for every system and each bin of separation the count and
    // nine fp64 sums over the ordered pairs (row, source) of the bin, in a pinned order.  edges: bins + 1 ascending values
    // >= 0 (host), one set for all systems, or numSystems sets (bins taken from `bins`, or from the one set where bins is 0);
    // bins is 1 ... 32.  weight: NBODY_BATCH_WEIGHT_NUMBER or _MASS (the product of the two mass words).  rows, sources: empty
    // for all bodies, or numSystems x maxBodies bytes (host).  Returns the per-system records; records, where given, is
    // resized to numSystems x bins and takes the bins (bin t of system s at s * bins + t); nullptr skips that copy.  Changes
    // nothing the handle keeps.
    std::vector<nbody_batch_pair_velocities_system> pairVelocities(const float *dPositions, const float *dVelocities,
                                                                   const std::vector<float> &edges,
                                                                   std::vector<nbody_batch_pair_velocities_bin> *records,
                                                                   int weight = NBODY_BATCH_WEIGHT_NUMBER, int bins = 0,
                                                                   const std::vector<unsigned char> &rows = {},
                                                                   const std::vector<unsigned char> &sources = {})
    {
        if (bins == 0)
            bins = (int)edges.size() - 1;
        if (bins < 1 || bins > NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS)
            throw std::invalid_argument("nbody::Batch::pairVelocities: bins must be 1 ... 32");
        const size_t set = (size_t)bins + 1;
        if (edges.size() != set && edges.size() != (size_t)systems_ * set)
            throw std::invalid_argument("nbody::Batch::pairVelocities: bins + 1 edges, or as many per system");
        if (!rows.empty() && rows.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::pairVelocities: one row byte per slot, or none");
        if (!sources.empty() && sources.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::pairVelocities: one source byte per slot, or none");
        std::vector<nbody_batch_pair_velocities_system> s((size_t)systems_);
        if (records)
            records->resize((size_t)systems_ * (size_t)bins);
        const int perSystem = edges.size() == set ? 0 : 1;
        check(nbody_batch_pair_velocities(b_, dPositions, dVelocities, bins, edges.data(), perSystem, rows.empty() ? nullptr : rows.data(),
                                          sources.empty() ? nullptr : sources.data(), weight, s.data(),
                                          records ? records->data() : nullptr),
              "nbody_batch_pair_velocities");
        return s;
    }
    // Mutual gravity of labelled sets (nbody_batch_mutual_gravity.h): for every system and ordered pair (a, b) of `sets` (1 ... 8)
    // sets what set b does to set a -- potential, force, torque, virial, power -- as fp64 sums in a pinned order.  labels:
    // numSystems x maxBodies bytes (host), a value below sets or NBODY_BATCH_MUTUAL_GRAVITY_NO_SET.  centre, velocity: empty
    // for zeros, or numSystems x 3 doubles (host).  Returns the per-system records; matrix, where given, is resized to
    // numSystems x sets x sets and takes the entries (entry (a, b) of system s at (s * sets + a) * sets + b); nullptr skips
    // that copy.  Changes nothing the handle keeps.
    std::vector<nbody_batch_mutual_gravity_system> mutualGravity(const float *dPositions, const float *dVelocities, int sets,
                                                                 const std::vector<unsigned char> &labels,
                                                                 std::vector<nbody_batch_mutual_gravity_entry> *matrix,
                                                                 float softening = 0.f, const std::vector<double> &centre = {},
                                                                 const std::vector<double> &velocity = {})
    {
        if (sets < 1 || sets > NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS)
            throw std::invalid_argument("nbody::Batch::mutualGravity: sets must be 1 ... 8");
        if (labels.size() != (size_t)systems_ * (size_t)maxBodies_)
            throw std::invalid_argument("nbody::Batch::mutualGravity: one label byte per slot");
        if (!centre.empty() && centre.size() != 3 * (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::mutualGravity: three centre words per system, or none");
        if (!velocity.empty() && velocity.size() != 3 * (size_t)systems_)
            throw std::invalid_argument("nbody::Batch::mutualGravity: three velocity words per system, or none");
        std::vector<nbody_batch_mutual_gravity_system> s((size_t)systems_);
        if (matrix)
            matrix->resize((size_t)systems_ * (size_t)(sets * sets));
        check(nbody_batch_mutual_gravity(b_, dPositions, dVelocities, sets, labels.data(), softening, centre.empty() ? nullptr : centre.data(),
                                         velocity.empty() ? nullptr : velocity.data(), s.data(), matrix ? matrix->data() : nullptr),
              "nbody_batch_mutual_gravity");
        return s;
    }
    // per system {kinetic, potential, total} and {px, py, pz, mass}
    std::vector<System::Energy> energy(const float *dPositions, const float *dVelocities, float softening)
    {
        std::vector<double> e(3 * (size_t)systems_);
        check(nbody_batch_energy(b_, dPositions, dVelocities, softening, e.data()), "nbody_batch_energy");
        std::vector<System::Energy> out((size_t)systems_);
        for (size_t s = 0; s < out.size(); ++s)
            out[s] = {e[3 * s], e[3 * s + 1], e[3 * s + 2]};
        return out;
    }
    std::vector<double> momentum(const float *dPositions, const float *dVelocities)
    {
        std::vector<double> p(4 * (size_t)systems_);
        check(nbody_batch_momentum(b_, dPositions, dVelocities, p.data()), "nbody_batch_momentum");
        return p;
    }
    std::int64_t numSystems() const { return systems_; }
    std::int64_t maxBodies() const { return maxBodies_; }
    nbody_batch *handle() { return b_; }

private:
    void check(int status, const char *what)
    {
        if (status != NBODY_OK)
            throw std::runtime_error(std::string(what) + ": " + nbody_batch_last_error(b_) + " (" + nbody_status_string(status) + ")");
    }
    nbody_batch *b_ = nullptr;
    std::int64_t systems_ = 0, maxBodies_ = 0;
    int logCapacity_ = 0;
};

}  // namespace nbody
