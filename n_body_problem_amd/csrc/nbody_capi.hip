// nbody_capi.hip -- the C ABI of include/nbody.h: context lifecycle, owned buffers, plain setters, timing, diagnostics.
// Host side of the reference's buffer/interop boundary (main_project/kernel.cu:130-188, 1148-1160) for a headless MI355X; the
// step is nbody_capi_step.hip, the body order nbody_capi_order.hip.
#include "nbody_ctx.h"
#include "nbody_kernels.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>

using namespace nbody;

static thread_local std::string g_create_error;

int nbody::fail(nbody_ctx *c, int status, const std::string &msg)
{
    if (c)
        c->err = msg;
    else
        g_create_error = msg;
    return status;
}

int nbody::sync_streams(nbody_ctx *c)
{
    for (hipStream_t s : {c->stream, c->own_stream.h, c->aux_stream.h})
        HIP_TRY(c, hipStreamSynchronize(s));
    return NBODY_OK;
}

hipError_t nbody::get_event(nbody_ctx *c, OwnedEvent *e)
{
    if (!c->ev_pool.empty()) {
        *e = std::move(c->ev_pool.back());
        c->ev_pool.pop_back();
        return hipSuccess;
    }
    return hipEventCreate(&e->h);
}

// A long run with timing on holds a bounded number of live events: those of finished launches go back to the pool.
int nbody::drain(nbody_ctx *c, EventPairs &l, double &ms, int64_t &n, bool wait)
{
    size_t done = 0;
    for (; done < l.size(); ++done) {
        auto &p = l[done];
        if (wait)
            HIP_TRY(c, hipEventSynchronize(p.second));  // whichever stream the launch ran on
        else if (hipEventQuery(p.second) != hipSuccess)
            break;
        float t = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&t, p.first, p.second));
        ms += t;
        ++n;
    }
    for (size_t i = 0; i < done; ++i) {
        c->ev_pool.push_back(std::move(l[i].first));
        c->ev_pool.push_back(std::move(l[i].second));
    }
    l.erase(l.begin(), l.begin() + (ptrdiff_t)done);
    return NBODY_OK;
}

extern "C" {

int nbody_abi_version(void) { return NBODY_ABI_VERSION; }

const char *nbody_status_string(int s)
{
    switch (s) {
    case NBODY_OK: return "ok";
    case NBODY_ERR_INVALID: return "invalid argument";
    case NBODY_ERR_ALLOC: return "allocation failed";
    case NBODY_ERR_DEVICE: return "HIP error";
    case NBODY_ERR_NO_DEVICE: return "no usable gfx950 device";
    case NBODY_ERR_STATE: return "context buffers not initialised";
    default: return "unknown status";
    }
}

const char *nbody_last_error(const nbody_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int64_t nbody_default_split_len(int64_t n_total) { return default_split_len(n_total); }

int64_t nbody_pair_once_split_len(int64_t n_total) { return pair_once_split_len(n_total); }

int64_t nbody_split_len(const nbody_ctx *ctx) { return ctx ? ctx->split_len : 0; }
int64_t nbody_n_total(const nbody_ctx *ctx) { return ctx ? ctx->n_total : 0; }

int nbody_create_shard(nbody_ctx **out, int device, int64_t n_total, int64_t row_lo, int64_t row_count,
                       int64_t split_len)
{
    if (!out)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: out is NULL");
    *out = nullptr;
    if (n_total < 0 || n_total > (int64_t)1 << 30)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: n_total out of range [0, 2^30]");
    if (row_lo < 0 || row_count < 0 || row_lo + row_count > n_total)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: rows [row_lo,row_lo+row_count) not inside [0,n_total)");
    if (split_len == 0)
        split_len = nbody_default_split_len(n_total);
    if (split_len < 0 || split_len % 64 != 0)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: split_len must be a positive multiple of 64 (of 256 in the pair-once mode)");
    if (row_lo % split_len != 0)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: row_lo must be a multiple of split_len");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NBODY_ERR_NO_DEVICE,
                    std::string("nbody_create: no HIP device (") + hipGetErrorString(e) +
                        "); this library has no CPU path");
    if (device < 0 || device >= ndev)
        return fail(nullptr, NBODY_ERR_INVALID, "nbody_create: device index out of range");
    HIP_TRY(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, NBODY_ERR_NO_DEVICE,
                    std::string("nbody_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");

    nbody_ctx *c = new (std::nothrow) nbody_ctx;
    if (!c)
        return fail(nullptr, NBODY_ERR_ALLOC, "nbody_create: host allocation failed");
    c->device = device;
    c->n_total = n_total;
    c->row_lo = row_lo;
    c->row_count = row_count;
    c->split_len = split_len;
    c->n_splits = (int)((n_total + split_len - 1) / split_len);
    c->cu_count = prop.multiProcessorCount;
    c->split_done.assign((size_t)c->n_splits, 0);

    int rc = NBODY_OK;
    auto guard = [&](hipError_t he, const char *what) {
        if (he != hipSuccess && rc == NBODY_OK)
            rc = fail(nullptr, he == hipErrorOutOfMemory ? NBODY_ERR_ALLOC : NBODY_ERR_DEVICE,
                      std::string(what) + ": " + hipGetErrorString(he));
    };
    guard(hipStreamCreateWithFlags(&c->own_stream.h, hipStreamNonBlocking), "hipStreamCreate");
    guard(hipStreamCreateWithFlags(&c->aux_stream.h, hipStreamNonBlocking), "hipStreamCreate");
    for (OwnedEvent *ev : {&c->ev_fork, &c->ev_join, &c->ev_graph_in, &c->ev_graph_out, &c->ev_flags})
        guard(hipEventCreateWithFlags(&ev->h, hipEventDisableTiming), "hipEventCreate");
    c->stream = c->own_stream;
    size_t red = (size_t)std::max(1, energy_blocks((int)row_count)) * 4;
    if (rc == NBODY_OK)
        guard(c->reduce_dev.ensure(red), "hipMalloc(reduce)");
    if (rc == NBODY_OK)
        guard(c->split_mass.ensure((size_t)std::max(1, c->n_splits)), "hipMalloc(split_mass)");
    c->reduce_host.resize(red);
    if (rc != NBODY_OK) {  // whatever was created goes with the context
        nbody_destroy(c);
        return rc;
    }
    *out = c;
    return NBODY_OK;
}

int nbody_create(nbody_ctx **out, int device, int64_t n_total)
{
    return nbody_create_shard(out, device, n_total, 0, n_total, 0);
}

int nbody_create_auto(nbody_ctx **out, int device, int64_t n_total)
{
    const bool pair_once = n_total >= NBODY_PAIR_ONCE_MIN_BODIES;
    int rc = nbody_create_shard(out, device, n_total, 0, n_total, pair_once ? nbody_pair_once_split_len(n_total) : 0);
    if (rc != NBODY_OK)
        return rc;
    rc = nbody_set_force_mode(*out, pair_once ? NBODY_FORCE_SYMMETRIC : NBODY_FORCE_ONE_SIDED);
    if (rc != NBODY_OK) {
        g_create_error = (*out)->err;
        nbody_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int nbody_force_mode(const nbody_ctx *c) { return c ? c->force_mode : NBODY_ERR_INVALID; }

int nbody_destroy(nbody_ctx *c)
{
    if (!c)
        return NBODY_OK;
    (void)hipSetDevice(c->device);
    for (hipStream_t s : {c->own_stream.h, c->aux_stream.h})
        if (s) (void)hipStreamSynchronize(s);  // a context whose creation failed may lack them
    delete c;
    return NBODY_OK;
}

int nbody_set_stream(nbody_ctx *c, void *hip_stream)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->stream = (hipStream_t)hip_stream;  // verbatim: NULL is the HIP default stream
    return NBODY_OK;
}

int nbody_reset_stream(nbody_ctx *c)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->stream = c->own_stream;
    return NBODY_OK;
}

int nbody_sync(nbody_ctx *c)
{
    if (!c)
        return NBODY_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return NBODY_OK;
}

// ---- owned buffers --------------------------------------------------------------------------

int nbody_set_positions(nbody_ctx *c, const float *host)
{
    if (!c || !host)
        return fail(c, NBODY_ERR_INVALID, "nbody_set_positions: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->pos.ensure((size_t)c->n_total));
    if (c->n_total) {
        HIP_TRY(c, hipMemcpyAsync(c->pos.ptr, host, sizeof(float4) * (size_t)c->n_total, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->acc_valid = false;
    return NBODY_OK;
}

int nbody_set_velocities(nbody_ctx *c, const float *host)
{
    if (!c || !host)
        return fail(c, NBODY_ERR_INVALID, "nbody_set_velocities: NULL argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->vel.ensure((size_t)c->row_count));
    if (c->row_count) {
        HIP_TRY(c, hipMemcpyAsync(c->vel.ptr, host, sizeof(float4) * (size_t)c->row_count, hipMemcpyHostToDevice,
                                  c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return NBODY_OK;
}

int nbody_download(nbody_ctx *c, float *host_pos, float *host_vel)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if ((host_pos && !c->pos.ptr && c->n_total) || (host_vel && !c->vel.ptr && c->row_count))
        return fail(c, NBODY_ERR_STATE, "nbody_download: buffers were never set");
    HIP_TRY(c, hipSetDevice(c->device));
    if (host_pos && c->n_total)
        HIP_TRY(c, hipMemcpyAsync(host_pos, c->pos.ptr, sizeof(float4) * (size_t)c->n_total, hipMemcpyDeviceToHost,
                                  c->stream));
    if (host_vel && c->row_count)
        HIP_TRY(c, hipMemcpyAsync(host_vel, c->vel.ptr, sizeof(float4) * (size_t)c->row_count, hipMemcpyDeviceToHost,
                                  c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return NBODY_OK;
}

float *nbody_positions_device(nbody_ctx *c) { return c ? reinterpret_cast<float *>(c->pos.ptr) : nullptr; }
float *nbody_velocities_device(nbody_ctx *c) { return c ? reinterpret_cast<float *>(c->vel.ptr) : nullptr; }

// ---- timing ---------------------------------------------------------------------------------

int nbody_timing_enable(nbody_ctx *c, int on)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->timing = on != 0;
    return NBODY_OK;
}

int nbody_timing_read_ex(nbody_ctx *c, double *out6)
{
    if (!c || !out6)
        return NBODY_ERR_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = drain(c, c->ev_force, c->force_ms, c->force_launches, true);
    if (rc == NBODY_OK)
        rc = drain(c, c->ev_update, c->update_ms, c->update_launches, true);
    if (rc == NBODY_OK)
        rc = drain(c, c->ev_aux, c->aux_ms, c->aux_launches, true);
    if (rc != NBODY_OK)
        return rc;
    out6[0] = c->force_ms;
    out6[1] = (double)c->force_launches;
    out6[2] = c->update_ms;
    out6[3] = (double)c->update_launches;
    out6[4] = c->aux_ms;
    out6[5] = (double)c->aux_launches;
    c->force_ms = c->update_ms = c->aux_ms = 0;
    c->force_launches = c->update_launches = c->aux_launches = 0;
    return NBODY_OK;
}

int nbody_timing_read(nbody_ctx *c, double *force_ms, int64_t *force_launches, double *update_ms,
                      int64_t *update_launches)
{
    double v[6];
    int rc = nbody_timing_read_ex(c, v);
    if (rc != NBODY_OK)
        return rc;
    if (force_ms) *force_ms = v[0];
    if (force_launches) *force_launches = (int64_t)v[1];
    if (update_ms) *update_ms = v[2];
    if (update_launches) *update_launches = (int64_t)v[3];
    return NBODY_OK;
}

// ---- plain setters --------------------------------------------------------------------------

int nbody_set_particle_softening(nbody_ctx *c, const float *d_eps)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->eps_pp = d_eps;
    c->acc_valid = false;
    return NBODY_OK;
}

int nbody_upload_particle_softening(nbody_ctx *c, const float *h_eps)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if (!h_eps)
        return nbody_set_particle_softening(c, nullptr);
    if (c->n_total == 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->eps_own.ensure((size_t)c->n_total) != hipSuccess)
        return fail(c, NBODY_ERR_ALLOC, "nbody_upload_particle_softening: hipMalloc failed");
    HIP_TRY(c, hipMemcpyAsync(c->eps_own.ptr, h_eps, sizeof(float) * (size_t)c->n_total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return nbody_set_particle_softening(c, c->eps_own.ptr);
}

int nbody_set_equal_mass_path(nbody_ctx *c, int on)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->equal_mass_path = on != 0;
    c->acc_valid = false;
    c->flags_valid = false;
    return NBODY_OK;
}

int nbody_set_rows_per_lane(nbody_ctx *c, int rpl)
{
    if (!c || !(rpl == 0 || rpl == 1 || rpl == 2 || rpl == 4 || rpl == -4 || rpl == 8 || rpl == 40 || rpl == 41))
        return fail(c, NBODY_ERR_INVALID, "nbody_set_rows_per_lane: expected 0, 1, 2, 4, 8, -4, 40 or 41");
    c->rows_per_lane = rpl;
    return NBODY_OK;
}

int nbody_set_integrator(nbody_ctx *c, int integrator)
{
    if (c && integrator == NBODY_INTEGRATOR_HERMITE)
        return fail(c, NBODY_ERR_INVALID, "nbody_set_integrator: NBODY_INTEGRATOR_HERMITE exists for batched ensembles only "
                                          "(nbody_batch_set_integrator)");
    if (!c || (integrator != NBODY_INTEGRATOR_KICK_DRIFT && integrator != NBODY_INTEGRATOR_KDK))
        return fail(c, NBODY_ERR_INVALID, "nbody_set_integrator: unknown integrator");
    c->integrator = integrator;
    c->acc_valid = false;
    return NBODY_OK;
}

int nbody_set_graph_replay(nbody_ctx *c, int mode)
{
    if (!c || mode < -1 || mode > 1)
        return fail(c, NBODY_ERR_INVALID, "nbody_set_graph_replay: expected -1 (automatic), 0 or 1");
    c->graph_replay = mode;
    return NBODY_OK;
}

// ---- diagnostics ----------------------------------------------------------------------------

static int reduce_blocks(nbody_ctx *c, int blocks, int nvals, double *out)
{
    HIP_TRY(c, hipMemcpyAsync(c->reduce_host.data(), c->reduce_dev.ptr, sizeof(double) * (size_t)blocks * nvals,
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int v = 0; v < nvals; ++v)
        out[v] = 0.0;
    for (int b = 0; b < blocks; ++b)
        for (int v = 0; v < nvals; ++v)
            out[v] += c->reduce_host[(size_t)b * nvals + v];
    return NBODY_OK;
}

int nbody_energy(nbody_ctx *c, const float *d_pos, const float *d_vel, float softening, double *out3)
{
    if (!c || !out3 || ((!d_pos || !d_vel) && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_energy: NULL argument");
    out3[0] = out3[1] = out3[2] = 0.0;
    if (c->row_count == 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_energy(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel),
                             c->reduce_dev.ptr, (int)c->row_lo, (int)c->row_count, (int)c->n_total,
                             softening * softening, c->eps_pp, c->stream));
    double ku[2];
    int rc = reduce_blocks(c, energy_kernel_blocks((int)c->row_count), 2, ku);
    if (rc != NBODY_OK)
        return rc;
    out3[0] = ku[0];
    out3[1] = ku[1];
    out3[2] = ku[0] + ku[1];
    return NBODY_OK;
}

int nbody_momentum(nbody_ctx *c, const float *d_pos, const float *d_vel, double *out4)
{
    if (!c || !out4 || ((!d_pos || !d_vel) && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_momentum: NULL argument");
    out4[0] = out4[1] = out4[2] = out4[3] = 0.0;
    if (c->row_count == 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_momentum(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel),
                               c->reduce_dev.ptr, (int)c->row_lo, (int)c->row_count, c->stream));
    return reduce_blocks(c, energy_blocks((int)c->row_count), 4, out4);
}

int nbody_device_info(nbody_ctx *c, int64_t *out4, char *name, int name_len)
{
    if (!c || !out4)
        return NBODY_ERR_INVALID;
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
    out4[0] = prop.multiProcessorCount;
    out4[1] = prop.clockRate / 1000;  // kHz -> MHz
    out4[2] = prop.warpSize;
    out4[3] = (int64_t)prop.maxSharedMemoryPerMultiProcessor;
    if (name && name_len > 0) {
        std::snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    }
    return NBODY_OK;
}

}  // extern "C"
