// nbody_capi_order.hip -- the C ABI of include/nbody.h, body order: the Morton order on the host (nbody_morton_order) and, on the
// device (nbody_order.hip), the permutation of a context, the gathers through it and nbody_reorder.
#include "nbody_ctx.h"
#include "nbody_kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

using namespace nbody;

// ---- the Morton order on the host ---------------------------------------------------------------------------------

static int morton_order_impl(const float *xyzm, int64_t n, int64_t *perm)
{
    // the bounding cube of the finite positions
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    bool any = false;
    for (int64_t i = 0; i < n; ++i) {
        const float *p = xyzm + 4 * i;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])))
            continue;
        for (int a = 0; a < 3; ++a) {
            lo[a] = any ? std::min(lo[a], p[a]) : p[a];
            hi[a] = any ? std::max(hi[a], p[a]) : p[a];
        }
        any = true;
    }
    double extent = 0.0;
    for (int a = 0; a < 3; ++a)
        extent = std::max(extent, (double)hi[a] - (double)lo[a]);
    const double scale = extent > 0.0 ? 1048575.0 / extent : 0.0;  // 20 bits per axis
    auto spread = [](uint64_t v) {  // bit k of v to bit 3k
        v &= 0xfffffull;
        v = (v | v << 32) & 0x1f00000000ffffull;
        v = (v | v << 16) & 0x1f0000ff0000ffull;
        v = (v | v << 8) & 0x100f00f00f00f00full;
        v = (v | v << 4) & 0x10c30c30c30c30c3ull;
        v = (v | v << 2) & 0x1249249249249249ull;
        return v;
    };
    // few species: the mass first (rank of the mass among the distinct values), then the curve
    std::vector<uint32_t> species;
    bool few = true;
    uint32_t last_bits = 0;
    bool have_last = false;
    for (int64_t i = 0; i < n && few; ++i) {
        uint32_t bits;
        std::memcpy(&bits, xyzm + 4 * i + 3, 4);
        if (have_last && bits == last_bits)
            continue;
        last_bits = bits;
        have_last = true;
        if (std::find(species.begin(), species.end(), bits) == species.end()) {
            species.push_back(bits);
            few = species.size() <= NBODY_ORDER_MAX_SPECIES;
        }
    }
    if (few)
        std::sort(species.begin(), species.end(), [](uint32_t a, uint32_t b) {
            float fa, fb;
            std::memcpy(&fa, &a, 4);
            std::memcpy(&fb, &b, 4);
            return fa < fb || (!(fb < fa) && a < b);  // by value; NaNs and signed zeros by bit pattern
        });
    // key = species rank (4 bits) | curve (60 bits); bodies without a finite position last within their species.
    // Host threads over contiguous chunks (a refresh of the layout costs a run as much as this function takes).
    const int threads = (int)std::max<int64_t>(1, std::min<int64_t>({8, (int64_t)std::thread::hardware_concurrency(), n / 65536}));
    auto chunk = [&](int t) { return std::make_pair(n * t / threads, n * (t + 1) / threads); };
    auto in_parallel = [&](auto &&body) {  // chunks that get no thread run on this one: nothing is thrown across the C ABI
        std::vector<std::thread> pool;
        int started = 1;
        try {
            pool.reserve((size_t)threads);
            for (; started < threads; ++started)
                pool.emplace_back(body, started);
        } catch (...) {
        }
        body(0);
        for (int t = started; t < threads; ++t)
            body(t);
        for (auto &th : pool)
            th.join();
    };
    std::vector<uint64_t> keys((size_t)n), keys2((size_t)n);
    std::vector<int64_t> idx2((size_t)n);
    in_parallel([&](int t) {
        for (int64_t i = chunk(t).first; i < chunk(t).second; ++i) {
            const float *p = xyzm + 4 * i;
            const bool finite = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
            uint64_t curve = (1ull << 60) - 1;
            if (finite) {
                uint64_t q[3];
                for (int a = 0; a < 3; ++a)
                    q[a] = (uint64_t)std::min(1048575.0, std::max(0.0, ((double)p[a] - (double)lo[a]) * scale));
                curve = spread(q[0]) | spread(q[1]) << 1 | spread(q[2]) << 2;
            }
            uint64_t rank = 0;
            if (few) {
                uint32_t bits;
                std::memcpy(&bits, p + 3, 4);
                rank = (uint64_t)(std::find(species.begin(), species.end(), bits) - species.begin());
            }
            keys[(size_t)i] = rank << 60 | curve;
            perm[i] = i;
        }
    });
    // stable LSD radix sort, 16 bits a pass (ties keep the caller's order): per-thread histograms, then every thread
    // scatters its chunk behind the chunks before it
    std::vector<std::vector<int64_t>> count((size_t)threads, std::vector<int64_t>(65536));
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 16 * pass;
        in_parallel([&](int t) {
            std::fill(count[(size_t)t].begin(), count[(size_t)t].end(), 0);
            for (int64_t i = chunk(t).first; i < chunk(t).second; ++i)
                ++count[(size_t)t][(size_t)((keys[(size_t)i] >> shift) & 0xffff)];
        });
        int64_t at = 0;
        for (size_t d = 0; d < 65536; ++d)
            for (int t = 0; t < threads; ++t) {
                const int64_t c = count[(size_t)t][d];
                count[(size_t)t][d] = at;
                at += c;
            }
        in_parallel([&](int t) {
            for (int64_t i = chunk(t).first; i < chunk(t).second; ++i) {
                const int64_t to = count[(size_t)t][(size_t)((keys[(size_t)i] >> shift) & 0xffff)]++;
                keys2[(size_t)to] = keys[(size_t)i];
                idx2[(size_t)to] = perm[i];
            }
        });
        keys.swap(keys2);
        std::memcpy(perm, idx2.data(), sizeof(int64_t) * (size_t)n);
    }
    return NBODY_OK;
}

extern "C" {

int nbody_morton_order(const float *xyzm, int64_t n, int64_t *perm)
{
    if (n < 0 || (n > 0 && (!xyzm || !perm)))
        return NBODY_ERR_INVALID;
    try {
        return morton_order_impl(xyzm, n, perm);
    } catch (...) {  // host allocation
        return NBODY_ERR_ALLOC;
    }
}

// ---- body order on the device (nbody_order.hip) -------------------------------------------------------------------

// Room for `bytes` in one of the two byte buffers; they only grow.
static int ensure_bytes(nbody_ctx *c, DeviceArray<char> &buffer, size_t bytes)
{
    if (bytes <= buffer.capacity)
        return NBODY_OK;
    if (buffer.ptr)  // earlier order work may have been enqueued on either stream
        if (int rc = sync_streams(c))
            return rc;
    HIP_TRY(c, buffer.ensure(bytes));
    return NBODY_OK;
}

static int ensure_order_buffers(nbody_ctx *c, size_t tmp_bytes)
{
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->order_perm.ensure((size_t)c->n_total));
    if (int rc = ensure_bytes(c, c->order_scratch, order_scratch_bytes((int)c->n_total)))
        return rc;
    return ensure_bytes(c, c->order_tmp, tmp_bytes);
}

int nbody_order_compute(nbody_ctx *c, const float *d_xyzm, int64_t n, const int64_t *d_order)
{
    if (!c || n < 0 || n > c->n_total || (n > 0 && !d_xyzm))
        return fail(c, NBODY_ERR_INVALID, "nbody_order_compute: expected 0 <= n <= n_total bodies on the device");
    int rc = ensure_order_buffers(c, 0);
    if (rc != NBODY_OK)
        return rc;
    HIP_TRY(c, launch_morton_order(reinterpret_cast<const float4 *>(d_xyzm), (int)n, c->order_perm.ptr, c->order_scratch.ptr, c->stream,
                                   d_order));
    HIP_TRY(c, launch_identity_perm(c->order_perm.ptr, (int)n, (int)(c->n_total - n), c->stream));
    c->order_n = n;
    return NBODY_OK;
}

int nbody_order_gather(nbody_ctx *c, void *d_dst, const void *d_src, int64_t first, int64_t count, int floats_per_row)
{
    if (!c || first < 0 || count < 0 || first + count > c->n_total || (count > 0 && (!d_dst || !d_src)) ||
        !(floats_per_row == 1 || floats_per_row == 2 || floats_per_row == 4))
        return fail(c, NBODY_ERR_INVALID, "nbody_order_gather: rows [first, first + count) inside [0, n_total), 1, 2 or 4 floats a row");
    if (c->order_n < 0)
        return fail(c, NBODY_ERR_STATE, "nbody_order_gather: no permutation (nbody_order_compute first)");
    if (count == 0)
        return NBODY_OK;
    const bool in_place = d_dst == d_src;
    if (in_place && first != 0)
        return fail(c, NBODY_ERR_INVALID, "nbody_order_gather: in place only from row 0 (the source is indexed by body)");
    const size_t bytes = (size_t)count * (size_t)floats_per_row * sizeof(float);
    void *dst = d_dst;
    if (in_place) {
        int rc = ensure_order_buffers(c, bytes);
        if (rc != NBODY_OK)
            return rc;
        dst = c->order_tmp.ptr;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (floats_per_row == 4)
        HIP_TRY(c, launch_gather_float4(static_cast<float4 *>(dst), static_cast<const float4 *>(d_src), c->order_perm.ptr, (int)first,
                                        (int)count, c->stream));
    else if (floats_per_row == 2)
        HIP_TRY(c, launch_gather_int64(static_cast<int64_t *>(dst), static_cast<const int64_t *>(d_src), c->order_perm.ptr, (int)first,
                                       (int)count, c->stream));
    else
        HIP_TRY(c, launch_gather_float(static_cast<float *>(dst), static_cast<const float *>(d_src), c->order_perm.ptr, (int)first,
                                       (int)count, c->stream));
    if (in_place)
        HIP_TRY(c, hipMemcpyAsync(d_dst, dst, bytes, hipMemcpyDeviceToDevice, c->stream));
    return NBODY_OK;
}

int nbody_order_read(nbody_ctx *c, int64_t *d_perm)
{
    if (!c || (c->order_n > 0 && !d_perm))
        return fail(c, NBODY_ERR_INVALID, "nbody_order_read: NULL argument");
    if (c->order_n < 0)
        return fail(c, NBODY_ERR_STATE, "nbody_order_read: no permutation (nbody_order_compute first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_widen_perm(d_perm, c->order_perm.ptr, (int)c->order_n, c->stream));
    return NBODY_OK;
}

int nbody_order_set(nbody_ctx *c, const int64_t *d_order, int64_t n, int inverse)
{
    if (!c || n < 0 || n > c->n_total || (n > 0 && !d_order))
        return fail(c, NBODY_ERR_INVALID, "nbody_order_set: expected 0 <= n <= n_total indices on the device");
    int rc = ensure_order_buffers(c, 0);
    if (rc != NBODY_OK)
        return rc;
    HIP_TRY(c, launch_set_perm(c->order_perm.ptr, d_order, (int)n, inverse != 0, c->stream));
    HIP_TRY(c, launch_identity_perm(c->order_perm.ptr, (int)n, (int)(c->n_total - n), c->stream));
    c->order_n = n;
    return NBODY_OK;
}

int nbody_order_identity(nbody_ctx *c, int64_t *d_order, int64_t n)
{
    if (!c || n < 0 || (n > 0 && !d_order))
        return fail(c, NBODY_ERR_INVALID, "nbody_order_identity: bad argument");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_iota64(d_order, (int)n, c->stream));
    return NBODY_OK;
}

int nbody_order_permute_softening(nbody_ctx *c)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if (!c->eps_own.ptr || c->eps_pp != c->eps_own.ptr)
        return NBODY_OK;  // no copy of its own in use: a borrowed array is the caller's to permute (nbody_order_gather)
    c->acc_valid = false;
    return nbody_order_gather(c, c->eps_own.ptr, c->eps_own.ptr, 0, c->n_total, 1);
}

int nbody_morton_order_device(nbody_ctx *c, const float *d_xyzm, int64_t n, int64_t *d_perm)
{
    int rc = nbody_order_compute(c, d_xyzm, n, nullptr);
    return rc == NBODY_OK ? nbody_order_read(c, d_perm) : rc;
}

int nbody_reorder(nbody_ctx *c, float *d_pos, float *d_vel, float *d_eps, int64_t *d_order, int64_t n)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if (c->row_lo != 0 || c->row_count != c->n_total)
        return fail(c, NBODY_ERR_INVALID, "nbody_reorder: the context must own every row (shards: nbody_multi_reorder)");
    if (n < 0 || n > c->n_total || (n > 0 && (!d_pos || !d_vel)))
        return fail(c, NBODY_ERR_INVALID, "nbody_reorder: expected 0 <= n <= n_total and device positions and velocities");
    if (n == 0)
        return NBODY_OK;
    int rc = nbody_order_compute(c, d_pos, n, d_order);
    if (rc == NBODY_OK)
        rc = nbody_order_gather(c, d_pos, d_pos, 0, n, 4);
    if (rc == NBODY_OK)
        rc = nbody_order_gather(c, d_vel, d_vel, 0, n, 4);
    if (rc == NBODY_OK && d_eps)
        rc = nbody_order_gather(c, d_eps, d_eps, 0, n, 1);
    if (rc == NBODY_OK && d_eps != c->eps_own.ptr)
        rc = nbody_order_permute_softening(c);
    if (rc == NBODY_OK && d_order)
        rc = nbody_order_gather(c, d_order, d_order, 0, n, 2);
    if (rc == NBODY_OK)
        rc = nbody_invalidate_forces(c);
    return rc;
}

}  // extern "C"
