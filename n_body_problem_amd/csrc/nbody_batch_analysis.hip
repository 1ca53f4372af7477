// nbody_batch_analysis.hip -- what a batched ensemble (nbody_batch.hip) can be asked about a state: bound pairs, cluster
// structure, bound members, gravity at points, hierarchies, groups, spanning trees, neighbours, pair-separation counts, contact
// lists, approach lists, radial profiles, surface maps, shapes, pair velocity statistics, mutual gravity of labelled sets, energy and momentum (include/nbody.h, nbody_batch_pairs.h ... nbody_batch_surface.h).  Every kernel here is a sibling of the force kernels -- one workgroup per system,
// the columns broadcast from LDS, rows in registers -- that reads the caller's state and writes only records of its own: no
// integrator reads what these calls keep (BatchAnalysis below), and no call here touches a cache, a level or a report of the
// integrators.  The arithmetic of each kernel is in its HIP-free header (nbody_batch_*_math.h, nbody_batch_pairs_elements.h).
#include "nbody_batch_approaches_math.h"
#include "nbody_batch_contacts_math.h"
#include "nbody_batch_correlation_math.h"
#include "nbody_batch_gravity_math.h"
#include "nbody_batch_groups_math.h"
#include "nbody_batch_handle.h"
#include "nbody_batch_hierarchy_math.h"
#include "nbody_batch_members_math.h"
#include "nbody_batch_mutual_gravity_math.h"
#include "nbody_batch_neighbours_math.h"
#include "nbody_batch_pair_velocities_math.h"
#include "nbody_batch_pairs_elements.h"
#include "nbody_batch_radial_math.h"
#include "nbody_batch_radii_check.h"
#include "nbody_batch_shape_math.h"
#include "nbody_batch_span_math.h"
#include "nbody_batch_structure_math.h"
#include "nbody_batch_surface_math.h"
#include "nbody_kernels.h"

#include <cmath>
#include <new>

namespace nbody {
namespace {

// One launch of an analysis kernel with `lds` bytes of dynamic LDS.  The limit is raised first, always: positions and
// velocities of 4096 bodies are 128 KiB, above the default 64 KiB from 2049 bodies on.
template <class... P, class... A>
hipError_t launch_analysis_kernel(void (*kernel)(P...), dim3 grid, int threads, size_t lds, hipStream_t stream, const A &...args)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kernel, grid, dim3(threads), lds, stream, args...);
    return hipGetLastError();
}

// Rows per lane (batch_shape's 1, 2 or 4) as a template argument: f(integral_constant<int, RPL>).
template <class F>
hipError_t with_rpl(int rpl, F &&f)
{
    switch (rpl) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
    }
}

// The workgroup's sums of N values in a fixed order -- the lanes of a wave by shuffles, the waves in ascending order through
// red[16][N] -- returned to every lane.
template <int N>
__device__ inline void block_sum(double (&v)[N], double *red, int tid, int T)
{
#pragma unroll
    for (int c = 0; c < N; ++c)
        for (int off = 32; off > 0; off >>= 1)
            v[c] += __shfl_down(v[c], off, 64);
    __syncthreads();  // every lane has read what red held before
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c)
            red[(tid >> 6) * N + c] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) {
        double s = red[c];
        for (int w = 1; w < T / 64; ++w)
            s += red[w * N + c];
        v[c] = s;
    }
}

// The workgroup's minimum, returned to every lane.
__device__ inline double block_min(double v, double *red, int tid, int T)
{
    for (int off = 32; off > 0; off >>= 1)
        v = fmin(v, __shfl_down(v, off, 64));
    __syncthreads();
    if ((tid & 63) == 0)
        red[tid >> 6] = v;
    __syncthreads();
    double m = red[0];
    for (int w = 1; w < T / 64; ++w)
        m = fmin(m, red[w]);
    return m;
}

// Whether any lane of the workgroup says so: a ballot per wave, the waves through flags[16].  Every lane returns the same
// word, so a loop that leaves on it is left by the whole workgroup.  Its first barrier also ends the reads the lanes did
// before the call.
__device__ inline bool block_any(bool mine, int *flags, int tid, int T)
{
    const int wave = __ballot(mine) != 0 ? 1 : 0;
    __syncthreads();  // every lane is done with what it read before, the flags of the call before among it
    if ((tid & 63) == 0)
        flags[tid >> 6] = wave;
    __syncthreads();
    int any = 0;
    for (int w = 0; w < T / 64; ++w)
        any |= flags[w];
    return __builtin_amdgcn_readfirstlane(any) != 0;
}

// ---- bound pairs (include/nbody_batch_pairs.h): every row's partner by the smallest two-body energy, the fp64 record of the
// pair, and the binaries of every system.  A sibling of the force kernels: one workgroup per system with batch_shape's
// workgroup, the columns broadcast from LDS, RPL rows per lane at r = q * T + lane.  It reads the state and writes only the
// handle's records and counts.

static_assert(sizeof(BatchPairRecord) == sizeof(nbody_batch_pair_record) && sizeof(nbody_batch_pair_record) == 48 &&
                  offsetof(BatchPairRecord, mutual) == offsetof(nbody_batch_pair_record, mutual) &&
                  offsetof(BatchPairRecord, energy) == offsetof(nbody_batch_pair_record, energy) &&
                  offsetof(BatchPairRecord, separation) == offsetof(nbody_batch_pair_record, separation),
              "nbody_batch_pairs_elements.h mirrors the record of nbody_batch_pairs.h");

// LDS: sh[2 j] = {x, y, z, m} and sh[2 j + 1] = {vx, vy, vz, partner} of body j (the Hermite families' layout, 128 KiB at
// 4096 bodies); the partner's bits replace the unused fourth word of the velocity after the search.
// m: the candidates are the columns j < m (the massive ones, or all n); a row r >= m is a test particle and adds no mass.
// The search needs few registers at every RPL; the rolled fp64 record sets the kernel's count.  One row per lane is held to
// the 64 registers of eight waves per SIMD, batch_hermite_kernel<1>'s; the other two shapes are below theirs unasked.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_pairs_kernel(const float4 *pos, const float4 *vel, const int *counts,
                                                           const int *massive, int max_bodies, BatchPairRecord *records,
                                                           int *binaries)
{
    extern __shared__ float4 sh[];
    __shared__ int wave_binaries[16];
    const int n = counts[blockIdx.x];
    const int m = massive ? (massive[blockIdx.x] < n ? massive[blockIdx.x] : n) : n;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL];  // {x, y, z, the mass this row adds to mu}
    float3 v[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            x[q] = pos[base + r];
            const float4 w = vel[base + r];
            v[q] = make_float3(w.x, w.y, w.z);
            sh[2 * r] = x[q];
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (r >= m)
                x[q].w = 0.f;
        }
    }
    __syncthreads();
    float best[RPL];
    int bj[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        best[q] = __builtin_inff();
        bj[q] = -1;
    }
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
        const float4 pj = sh[2 * j], vj = sh[2 * j + 1];  // wave-uniform addresses: broadcast ds_read_b128
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const float dx = pj.x - x[q].x, dy = pj.y - x[q].y, dz = pj.z - x[q].z;
            const float wx = vj.x - v[q].x, wy = vj.y - v[q].y, wz = vj.z - v[q].z;
            const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const float v2 = __builtin_fmaf(wz, wz, __builtin_fmaf(wy, wy, wx * wx));
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float mu = pj.w + x[q].w;
            const float eps = __builtin_fmaf(-mu, inv, 0.5f * v2);
            const bool take = r2 > 0.f && eps < best[q];  // r2 == 0: the self pair and coincident bodies are no candidates
            best[q] = take ? eps : best[q];
            bj[q] = take ? j : bj[q];
        }
    }
    __syncthreads();  // every lane is done with the columns before the partners replace the velocities' fourth words
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n)
            sh[2 * r + 1].w = __int_as_float(bj[q]);
    }
    __syncthreads();
    // The records, one row at a time from LDS (the loop is kept rolled: the fp64 arithmetic is instantiated once).
    int mine = 0;
#pragma unroll 1
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r >= max_bodies)
            break;
        BatchPairRecord rec = batch_pair_empty();
        if (r < n) {
            const float4 xi = sh[2 * r], vi = sh[2 * r + 1];
            const int j = __float_as_int(vi.w);
            if (j >= 0) {
                const float4 xj = sh[2 * j], vj = sh[2 * j + 1];
                const int mutual = __float_as_int(vj.w) == r ? 1 : 0;
                const float pi[3] = {xi.x, xi.y, xi.z}, wi[3] = {vi.x, vi.y, vi.z};
                const float pj[3] = {xj.x, xj.y, xj.z}, wj[3] = {vj.x, vj.y, vj.z};
                const double mu = r < m ? (double)xj.w + (double)xi.w : (double)xj.w;
                rec = batch_pair_record(j, mutual, pi, wi, pj, wj, mu);
                mine += (mutual && rec.energy < 0.0 && r < j) ? 1 : 0;
            }
        }
        records[base + r] = rec;
    }
    // binaries of the system: lanes -> wave -> workgroup
    for (int off = 32; off > 0; off >>= 1)
        mine += __shfl_down(mine, off, 64);
    if ((tid & 63) == 0)
        wave_binaries[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < T / 64; ++w)
            total += wave_binaries[w];
        binaries[blockIdx.x] = total;
    }
}

// One launch over all systems.  Positions and velocities of a system's bodies in dynamic LDS, 128 KiB at 4096 bodies.
hipError_t launch_batch_pairs(const float4 *pos, const float4 *vel, const int *counts, const int *massive, int n_systems,
                              int max_bodies, BatchPairRecord *records, int *binaries, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = 2 * kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_pairs_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, vel, counts, massive,
                                      max_bodies, records, binaries);
    });
}

// ---- cluster structure (include/nbody_batch_structure.h): every row's k-th neighbour distance, neighbour weight and density,
// and per system the density centre, core radius and density, and the Lagrangian radii about the centre.  A sibling of
// batch_pairs_kernel: one workgroup per system with batch_shape's workgroup, the columns broadcast from LDS, RPL rows per
// lane at r = q * T + lane.  It reads the positions and writes only the handle's records.

static_assert(sizeof(BatchStructureBody) == sizeof(nbody_batch_structure_body) && sizeof(nbody_batch_structure_body) == 40 &&
                  offsetof(BatchStructureBody, radius) == offsetof(nbody_batch_structure_body, radius) &&
                  offsetof(BatchStructureBody, enclosed) == offsetof(nbody_batch_structure_body, enclosed) &&
                  offsetof(BatchStructureBody, neighbour_r2) == offsetof(nbody_batch_structure_body, neighbour_r2) &&
                  offsetof(BatchStructureBody, neighbour_weight) == offsetof(nbody_batch_structure_body, neighbour_weight) &&
                  offsetof(BatchStructureBody, inside) == offsetof(nbody_batch_structure_body, inside),
              "nbody_batch_structure_math.h mirrors the body record of nbody_batch_structure.h");
static_assert(sizeof(BatchStructureSystem) == sizeof(nbody_batch_structure_system) && sizeof(nbody_batch_structure_system) == 120 &&
                  offsetof(BatchStructureSystem, core_radius) == offsetof(nbody_batch_structure_system, core_radius) &&
                  offsetof(BatchStructureSystem, core_density) == offsetof(nbody_batch_structure_system, core_density) &&
                  offsetof(BatchStructureSystem, total_weight) == offsetof(nbody_batch_structure_system, total_weight) &&
                  offsetof(BatchStructureSystem, lagrange) == offsetof(nbody_batch_structure_system, lagrange) &&
                  offsetof(BatchStructureSystem, estimated) == offsetof(nbody_batch_structure_system, estimated),
              "nbody_batch_structure_math.h mirrors the system record of nbody_batch_structure.h");
static_assert(kStructureMaxNeighbour == NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR && kStructureFractions == NBODY_BATCH_STRUCTURE_FRACTIONS,
              "nbody_batch_structure_math.h mirrors the limits of nbody_batch_structure.h");

struct BatchStructureArgs {
    double fraction[kStructureFractions];
    int n_fractions, k, weight;
};

constexpr int kStructureSums = 10;  // sum rho, rho x, rho y, rho z, rho^2, w, w x, w y, w z, and the bodies with a k-th neighbour

// LDS: sh[j] = {x, y, z, w_j} of body j (64 KiB at 4096 bodies; with the reduction words above the default limit, which is
// raised before the launch); after the densities the same bytes hold {s_j, (double)w_j}, 16 bytes per body again.
// The eight smallest r2 of every row stay in registers (structure_insert); one row per lane is held to the 64 registers of
// eight waves per SIMD, batch_hermite_kernel<1>'s.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_structure_kernel(
    const float4 *pos, const int *counts, int max_bodies, BatchStructureArgs p, BatchStructureBody *bodies, BatchStructureSystem *systems)
{
    extern __shared__ float4 sh[];
    __shared__ double red[16 * kStructureSums];
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float inf = __builtin_inff();
    float4 x[RPL];  // {x, y, z, w}
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) {
            x[q] = pos[base + r];
            if (p.weight == NBODY_BATCH_WEIGHT_NUMBER)
                x[q].w = 1.f;
            sh[r] = x[q];
        }
    }
    __syncthreads();
    // Phase 1: the k-th smallest r2 > 0 of every row.
    float r2k[RPL];
    {
        float a[RPL][kStructureMaxNeighbour];
#pragma unroll
        for (int q = 0; q < RPL; ++q)
#pragma unroll
            for (int t = 0; t < kStructureMaxNeighbour; ++t)
                a[q][t] = inf;
        // Measured on an MI355X (profiles/batch_rate_structure.txt): unrolled by 4 the kernel is 4 % faster than by 2, and a
        // wave-uniform skip of the insertion (no lane's r2 below its list's largest; the same bits) costs 19 - 25 % at 1024
        // bodies and 2 - 7 % at 4096 -- some lane of 64 nearly always inserts, and the vote and branch are paid per column.
        // So: 4, no skip.
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const float4 pj = sh[j];  // a wave-uniform address: one broadcast LDS read (ds_read_b96: the weight is not needed)
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const float dx = pj.x - x[q].x, dy = pj.y - x[q].y, dz = pj.z - x[q].z;
                const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                structure_insert(a[q], r2 > 0.f ? r2 : inf);  // the self pair, coincident bodies and NaN are no neighbour pairs
            }
        }
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            r2k[q] = structure_kth(a[q], p.k);
    }
    // Phase 2: the pairs strictly inside the k-th distance, and their weight in ascending j.
    int inside[RPL];
    float nw[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        inside[q] = 0;
        nw[q] = 0.f;
    }
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float4 pj = sh[j];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const float dx = pj.x - x[q].x, dy = pj.y - x[q].y, dz = pj.z - x[q].z;
            const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            const bool in = r2 > 0.f && r2 < r2k[q];
            inside[q] += in ? 1 : 0;
            nw[q] += in ? pj.w : 0.f;  // + 0 leaves the sum's bits: no branch
        }
    }
    // Phase 3: densities, the system's sums, the centre.
    double rho[RPL], sum[kStructureSums];
#pragma unroll
    for (int c = 0; c < kStructureSums; ++c)
        sum[c] = 0.0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const bool live = q * T + tid < n;
        rho[q] = live ? structure_density(r2k[q], nw[q]) : 0.0;
        const double w = live ? (double)x[q].w : 0.0;
        sum[0] += rho[q];
        sum[1] += rho[q] * (double)x[q].x;
        sum[2] += rho[q] * (double)x[q].y;
        sum[3] += rho[q] * (double)x[q].z;
        sum[4] += rho[q] * rho[q];
        sum[5] += w;
        sum[6] += w * (double)x[q].x;
        sum[7] += w * (double)x[q].y;
        sum[8] += w * (double)x[q].z;
        sum[9] += live && r2k[q] < inf ? 1.0 : 0.0;
    }
    block_sum(sum, red, tid, T);  // its barriers: every lane is done with the columns
    const bool none = sum[0] == 0.0, zero = none && sum[5] == 0.0;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (!zero) {
        cx = none ? sum[6] / sum[5] : sum[1] / sum[0];
        cy = none ? sum[7] / sum[5] : sum[2] / sum[0];
        cz = none ? sum[8] / sum[5] : sum[3] / sum[0];
    }
    // Phase 4: radii about the centre, the core radius, the enclosed weights and the Lagrangian radii.
    double2 *sd = reinterpret_cast<double2 *>(sh);
    double s[RPL], core[1] = {0.0};
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        const double dx = (double)x[q].x - cx, dy = (double)x[q].y - cy, dz = (double)x[q].z - cz;
        s[q] = r < n ? dx * dx + dy * dy + dz * dz : 0.0;
        core[0] += rho[q] * rho[q] * s[q];
        if (r < n)
            sd[r] = make_double2(s[q], (double)x[q].w);
    }
    block_sum(core, red, tid, T);  // its barriers: the {s_j, w_j} are in place
    double enc[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        enc[q] = 0.0;
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const double2 cj = sd[j];  // broadcast ds_read_b128
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            enc[q] += cj.x <= s[q] ? cj.y : 0.0;
    }
    double radius[RPL], far = 0.0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        radius[q] = sqrt(s[q]);
        far = fmax(far, radius[q]);  // rows from the count on have s = 0
    }
    far = 0.0 - block_min(-far, red, tid, T);  // the largest radius; 0 without bodies
    // The system record, field by field: a record indexed by the fraction would live in scratch memory.
    BatchStructureSystem *out = systems + blockIdx.x;
    if (tid == 0) {
        out->centre[0] = cx;
        out->centre[1] = cy;
        out->centre[2] = cz;
        out->core_radius = none ? 0.0 : sqrt(core[0] / sum[4]);
        out->core_density = none ? 0.0 : sum[4] / sum[0];
        out->total_weight = zero ? 0.0 : sum[5];
        out->estimated = (int)sum[9];
        out->reserved = 0;
    }
#pragma unroll 1
    for (int f = 0; f < p.n_fractions; ++f) {
        const double target = p.fraction[f] * sum[5];
        double m = (double)inf;
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            m = (q * T + tid < n && enc[q] >= target) ? fmin(m, radius[q]) : m;
        m = block_min(m, red, tid, T);
        if (tid == 0)
            out->lagrange[f] = zero ? 0.0 : (m < (double)inf ? m : far);
    }
    if (tid == 0)
        for (int f = p.n_fractions; f < kStructureFractions; ++f)
            out->lagrange[f] = 0.0;  // unused slots
    if (bodies) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < max_bodies)
                bodies[base + r] = r < n ? BatchStructureBody{rho[q], radius[q], enc[q], r2k[q], nw[q], inside[q], 0}
                                         : structure_empty_body();
        }
    }
}

// One launch over all systems.  64 KiB of dynamic LDS at 4096 bodies beside the reduction words.  bodies may be NULL: the
// per-body records are then not stored.
hipError_t launch_batch_structure(const float4 *pos, const int *counts, int n_systems, int max_bodies, const BatchStructureArgs &p,
                                  BatchStructureBody *bodies, BatchStructureSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_structure_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, counts, max_bodies, p,
                                      bodies, systems);
    });
}

// ---- bound members (include/nbody_batch_members.h): iterative unbinding.  Every row's potential from the member sources and
// its energy in their rest frame, the rows with e >= 0 dropped, again with the survivors until nothing changes; then the bound
// mass, centre, velocity and energies of what is left.  A sibling of batch_structure_kernel: one workgroup per system with
// batch_shape's workgroup, the columns broadcast from LDS, RPL rows per lane at r = q * T + lane.  The iterations run inside
// the kernel: the member mask and the frame never leave the CU.  It reads the state and writes only the handle's records.

static_assert(sizeof(BatchMemberBody) == sizeof(nbody_batch_member_body) && sizeof(nbody_batch_member_body) == 24 &&
                  offsetof(BatchMemberBody, energy) == offsetof(nbody_batch_member_body, energy) &&
                  offsetof(BatchMemberBody, member) == offsetof(nbody_batch_member_body, member) &&
                  offsetof(BatchMemberBody, removed_at) == offsetof(nbody_batch_member_body, removed_at),
              "nbody_batch_members_math.h mirrors the body record of nbody_batch_members.h");
static_assert(sizeof(BatchMemberSystem) == sizeof(nbody_batch_member_system) && sizeof(nbody_batch_member_system) == 88 &&
                  offsetof(BatchMemberSystem, centre) == offsetof(nbody_batch_member_system, centre) &&
                  offsetof(BatchMemberSystem, velocity) == offsetof(nbody_batch_member_system, velocity) &&
                  offsetof(BatchMemberSystem, kinetic) == offsetof(nbody_batch_member_system, kinetic) &&
                  offsetof(BatchMemberSystem, potential) == offsetof(nbody_batch_member_system, potential) &&
                  offsetof(BatchMemberSystem, members) == offsetof(nbody_batch_member_system, members) &&
                  offsetof(BatchMemberSystem, sources) == offsetof(nbody_batch_member_system, sources) &&
                  offsetof(BatchMemberSystem, iterations) == offsetof(nbody_batch_member_system, iterations) &&
                  offsetof(BatchMemberSystem, converged) == offsetof(nbody_batch_member_system, converged),
              "nbody_batch_members_math.h mirrors the system record of nbody_batch_members.h");
static_assert(kMembersMaxIterations == NBODY_BATCH_MEMBERS_MAX_ITERATIONS, "nbody_batch_members_math.h mirrors the limit of nbody_batch_members.h");

// The final set's sums: mass, m x, m y, m z, m vx, m vy, m vz, kinetic, potential, members, member sources.
constexpr int kMembersSums = 11;

// One pass over the sources j < m for RPL rows: sum[q] += (double)(m_j inv) in ascending j, the fp32 term batch_diag_kernel
// forms for nbody_batch_energy (GUARD: the eps = 0 guard).  sh[j].w is the source's mass word, or 0 for a non-member: its
// term is +0, no branch.  Column reads are wave-uniform broadcasts.
template <int RPL, bool GUARD>
__device__ __forceinline__ void members_columns(const float4 *sh, int m, const float4 (&x)[RPL], int tid, int T, float eps2,
                                                double (&sum)[RPL])
{
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
        const float4 pj = sh[j];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const float dx = pj.x - x[q].x, dy = pj.y - x[q].y, dz = pj.z - x[q].z;
            const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, eps2)));
            float inv = __builtin_amdgcn_rsqf(GUARD ? guard_r2(r2) : r2);
            inv = j != q * T + tid ? inv : 0.f;
            sum[q] += (double)(pj.w * inv);
        }
    }
}

// LDS: sh[j] = {x, y, z, masked mass} of body j (64 KiB at 4096 bodies; with the reduction words above the default limit,
// which is raised before the launch).  The velocities stay in the rows' registers: only the frame needs them.
// The iteration loop holds barriers, so its trip count is workgroup-uniform: n, max_iterations and t are, and "removed" and
// "left" come out of one block_sum, which hands every lane the same words of red; no lane leaves on data of its own.
// One row per lane is held to the 64 registers of eight waves per SIMD, batch_hermite_kernel<1>'s.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_members_kernel(
    const float4 *pos, const float4 *vel, const int *counts, const int *massive, int max_bodies, float eps2, int max_iterations,
    const unsigned char *initial, BatchMemberBody *bodies, BatchMemberSystem *systems)
{
    extern __shared__ float4 sh[];
    __shared__ double red[16 * kMembersSums];
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int m = massive ? (massive[blockIdx.x] < n ? massive[blockIdx.x] : n) : n;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL];  // {x, y, z, the row's mass word as a source; 0 for a test particle}
    float3 v[RPL];
    bool in[RPL];   // member of the current set; never for a row from the count on
    int gone[RPL];  // the iteration that removed the row
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q] = make_float3(0.f, 0.f, 0.f);
        in[q] = false;
        gone[q] = 0;
        if (r < n) {
            x[q] = pos[base + r];
            const float4 w = vel[base + r];
            v[q] = make_float3(w.x, w.y, w.z);
            in[q] = initial ? initial[base + r] != 0 : true;
            if (r >= m)
                x[q].w = 0.f;
            sh[r] = make_float4(x[q].x, x[q].y, x[q].z, in[q] ? x[q].w : 0.f);
        }
    }
    double phi[RPL], e[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        phi[q] = e[q] = 0.0;
    double Vx = 0.0, Vy = 0.0, Vz = 0.0;
    int iterations = 0, converged = 1;  // a system without bodies evaluates nothing
    if (n > 0) {
        for (int t = 1;; ++t) {
            // The frame of the member sources.
            double f[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const double w = in[q] ? (double)x[q].w : 0.0;
                f[0] += w;
                f[1] += w * (double)v[q].x;
                f[2] += w * (double)v[q].y;
                f[3] += w * (double)v[q].z;
            }
            block_sum(f, red, tid, T);  // its barriers: the masked mass words are in place
            const bool massless = f[0] == 0.0;
            Vx = massless ? 0.0 : f[1] / f[0];
            Vy = massless ? 0.0 : f[2] / f[0];
            Vz = massless ? 0.0 : f[3] / f[0];
            // The potentials, the energies, the decision.
            double sum[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                sum[q] = 0.0;
            if (eps2 > 0.f)
                members_columns<RPL, false>(sh, m, x, tid, T, eps2, sum);
            else
                members_columns<RPL, true>(sh, m, x, tid, T, eps2, sum);
            double c[2] = {0.0, 0.0};  // removed by this iteration, members left
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                phi[q] = 0.0 - sum[q];
                e[q] = members_energy(v[q].x, v[q].y, v[q].z, Vx, Vy, Vz, phi[q]);
                const bool stays = members_stays(in[q], e[q]);
                const bool leaves = in[q] && !stays;
                gone[q] = leaves ? t : gone[q];
                in[q] = stays;
                c[0] += leaves ? 1.0 : 0.0;
                c[1] += stays ? 1.0 : 0.0;
            }
            block_sum(c, red, tid, T);  // its barriers: every lane is done with the columns
            // The same two words of red in every lane of every wave: the exit is the workgroup's.
            const int removed = __builtin_amdgcn_readfirstlane((int)c[0]), left = __builtin_amdgcn_readfirstlane((int)c[1]);
            iterations = t;
            converged = (removed == 0 || left == 0) ? 1 : 0;
            if (converged || t >= max_iterations)
                break;
            // Every lane masks its own rows' mass words for the next iteration; the next sum's barriers publish them.
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                if (r < m)
                    sh[r].w = in[q] ? x[q].w : 0.f;
            }
        }
    }
    // The final set.
    double g[kMembersSums];
#pragma unroll
    for (int c = 0; c < kMembersSums; ++c)
        g[c] = 0.0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const double w = in[q] ? (double)x[q].w : 0.0;
        g[0] += w;
        g[1] += w * (double)x[q].x;
        g[2] += w * (double)x[q].y;
        g[3] += w * (double)x[q].z;
        g[4] += w * (double)v[q].x;
        g[5] += w * (double)v[q].y;
        g[6] += w * (double)v[q].z;
        g[7] += in[q] ? w * members_kinetic(v[q].x, v[q].y, v[q].z, Vx, Vy, Vz) : 0.0;
        g[8] += in[q] ? 0.5 * w * phi[q] : 0.0;
        g[9] += in[q] ? 1.0 : 0.0;
        g[10] += in[q] && q * T + tid < m ? 1.0 : 0.0;
    }
    block_sum(g, red, tid, T);
    if (tid == 0) {
        const bool massless = g[0] == 0.0;
        BatchMemberSystem *out = systems + blockIdx.x;
        out->bound_mass = g[0];
        out->centre[0] = massless ? 0.0 : g[1] / g[0];
        out->centre[1] = massless ? 0.0 : g[2] / g[0];
        out->centre[2] = massless ? 0.0 : g[3] / g[0];
        out->velocity[0] = massless ? 0.0 : g[4] / g[0];
        out->velocity[1] = massless ? 0.0 : g[5] / g[0];
        out->velocity[2] = massless ? 0.0 : g[6] / g[0];
        out->kinetic = g[7];
        out->potential = g[8];
        out->members = (int)g[9];
        out->sources = (int)g[10];
        out->iterations = iterations;
        out->converged = converged;
    }
    if (bodies) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < max_bodies)
                bodies[base + r] = r < n ? BatchMemberBody{phi[q], e[q], in[q] ? 1 : 0, gone[q]} : members_empty_body();
        }
    }
}

// One launch over all systems.  64 KiB of dynamic LDS at 4096 bodies beside the reduction words.  massive, initial and bodies
// may be NULL.
hipError_t launch_batch_members(const float4 *pos, const float4 *vel, const int *counts, const int *massive, int n_systems,
                                int max_bodies, float eps2, int max_iterations, const unsigned char *initial, BatchMemberBody *bodies,
                                BatchMemberSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_members_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, vel, counts, massive,
                                      max_bodies, eps2, max_iterations, initial, bodies, systems);
    });
}

// ---- gravity at points (include/nbody_batch_gravity.h): the acceleration, the potential and the tidal tensor of every system
// at its own bodies (SELF) or at the caller's points.  A sibling of batch_members_kernel with a second grid dimension: a
// workgroup serves one system and one block of rows (gravity_plan_own / gravity_plan_points of nbody_batch_gravity_math.h),
// with the system's m sources in LDS as {x, y, z, m}, read by wave-uniform broadcasts; each lane holds RPL rows in registers,
// row gravity_row(block, RPL, T, q, lane).  Every pair and every sum goes through gravity_pair and GravityRow of that header,
// which are batch_forces' r2, inv, s and chain and members_columns' fp64 sum: a loop of its own, so that every kernel above
// stays the code it is (see batch_forces_jerks on OWN).  No atomics, no reduction: a row's outputs are its lane's alone.  It
// reads the state and writes only the handle's records.

static_assert(sizeof(BatchGravityRecord) == sizeof(nbody_batch_gravity_record) && sizeof(nbody_batch_gravity_record) == 24 &&
                  offsetof(BatchGravityRecord, acceleration) == offsetof(nbody_batch_gravity_record, acceleration) &&
                  offsetof(BatchGravityRecord, reserved) == offsetof(nbody_batch_gravity_record, reserved) &&
                  offsetof(BatchGravityRecord, potential) == offsetof(nbody_batch_gravity_record, potential),
              "nbody_batch_gravity_math.h mirrors the record of nbody_batch_gravity.h");
static_assert(kGravityMaxPoints == NBODY_BATCH_GRAVITY_MAX_POINTS, "nbody_batch_gravity_math.h mirrors the limit of nbody_batch_gravity.h");

// SELF: the rows are the bodies r < n of pos and `stride` is max_bodies; otherwise the rows are the points r < point_counts[s]
// (n_points where point_counts is null) of `points` and `stride` is n_points.  Rows from the count on up to `stride` receive the
// empty record; a block without a row below the count writes those and returns before it loads a source.  One row per lane is
// held to the 64 registers of eight waves per SIMD, as batch_members_kernel<1> is.
template <int RPL, bool GUARD, bool SELF, bool TIDAL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_gravity_kernel(
    const float4 *pos, const float4 *points, const int *counts, const int *massive, const int *point_counts, int max_bodies,
    int stride, float eps2, BatchGravityRecord *records, float *tidal)
{
    extern __shared__ float4 sh[];
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int m = massive ? (massive[blockIdx.x] < n ? massive[blockIdx.x] : n) : n;
    const int pc = SELF ? n : (point_counts ? point_counts[blockIdx.x] : stride);
    const int rows = pc < stride ? pc : stride;
    const int tid = threadIdx.x, T = blockDim.x;
    const int first = gravity_row(blockIdx.y, RPL, T, 0, 0);
    const size_t src = (size_t)blockIdx.x * (size_t)max_bodies, base = (size_t)blockIdx.x * (size_t)stride;
    if (first >= rows) {  // workgroup-uniform: no barrier is passed
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = gravity_row(blockIdx.y, RPL, T, q, tid);
            if (r < stride) {
                records[base + r] = gravity_empty_record();
                if (TIDAL) {
#pragma unroll
                    for (int c = 0; c < kGravityTidalWords; ++c)
                        tidal[(base + r) * kGravityTidalWords + c] = 0.f;
                }
            }
        }
        return;
    }
    for (int j = tid; j < m; j += T)
        sh[j] = pos[src + j];
    float4 x[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = gravity_row(blockIdx.y, RPL, T, q, tid);
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows)
            x[q] = SELF ? pos[src + r] : points[base + r];
    }
    __syncthreads();
    GravityRow<TIDAL> row[RPL];
#pragma unroll 4
    for (int j = 0; j < m; ++j) {
        const float4 pj = sh[j];  // wave-uniform address: broadcast ds_read_b128
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            row[q].add(gravity_pair<GUARD, TIDAL>(x[q].x, x[q].y, x[q].z, pj.x, pj.y, pj.z, pj.w, eps2,
                                                  SELF && j == gravity_row(blockIdx.y, RPL, T, q, tid)));
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = gravity_row(blockIdx.y, RPL, T, q, tid);
        if (r < stride) {
            float t[kGravityTidalWords] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (TIDAL && r < rows)
                row[q].tidal(t);
            records[base + r] = r < rows ? row[q].record() : gravity_empty_record();
            if (TIDAL) {
#pragma unroll
                for (int c = 0; c < kGravityTidalWords; ++c)
                    tidal[(base + r) * kGravityTidalWords + c] = t[c];
            }
        }
    }
}

// One launch over all systems and row blocks.  64 KiB of dynamic LDS at 4096 bodies.  points null: own-bodies mode.  massive,
// point_counts and tidal may be null.
hipError_t launch_batch_gravity(const float4 *pos, const float4 *points, const int *counts, const int *massive,
                                const int *point_counts, int n_systems, int max_bodies, int n_points, float eps2,
                                BatchGravityRecord *records, float *tidal, hipStream_t stream)
{
    const bool self = points == nullptr;
    const GravityPlan plan = self ? gravity_plan_own(max_bodies) : gravity_plan_points(n_points);
    const int stride = self ? max_bodies : n_points;
    const size_t lds = gravity_lds_bytes(max_bodies);
    const auto launch = [&](auto kernel) {
        return launch_analysis_kernel(kernel, dim3(n_systems, plan.blocks), plan.threads, lds, stream, pos, points, counts, massive,
                                      point_counts, max_bodies, stride, eps2, records, tidal);
    };
    const auto with_modes = [&](auto rpl, auto guard) {
        constexpr int R = decltype(rpl)::value;
        constexpr bool G = decltype(guard)::value;
        if (self)
            return tidal ? launch(batch_gravity_kernel<R, G, true, true>) : launch(batch_gravity_kernel<R, G, true, false>);
        return tidal ? launch(batch_gravity_kernel<R, G, false, true>) : launch(batch_gravity_kernel<R, G, false, false>);
    };
    return with_shape(plan.rpl, !(eps2 > 0.f), with_modes);
}

// ---- hierarchies (include/nbody_batch_hierarchy.h): nested bound pairs.  Level by level the live roots of a system look for
// partners as batch_pairs_kernel's rows do, the mutual bound pairs that their worst perturber lets stand become nodes with the
// merged body's state, and the search runs again over what is left.  A sibling of batch_pairs_kernel: one workgroup per
// system with batch_shape's workgroup, the columns broadcast from LDS, RPL rows per lane at r = q * T + lane.  The levels run
// inside the kernel.  It reads the state and writes only the handle's records.

static_assert(sizeof(BatchHierarchyNode) == sizeof(nbody_batch_hierarchy_node) && sizeof(nbody_batch_hierarchy_node) == 128 &&
                  offsetof(BatchHierarchyNode, parent) == offsetof(nbody_batch_hierarchy_node, parent) &&
                  offsetof(BatchHierarchyNode, stable) == offsetof(nbody_batch_hierarchy_node, stable) &&
                  offsetof(BatchHierarchyNode, mass) == offsetof(nbody_batch_hierarchy_node, mass) &&
                  offsetof(BatchHierarchyNode, perturbation) == offsetof(nbody_batch_hierarchy_node, perturbation) &&
                  offsetof(BatchHierarchyNode, mutual_inclination) == offsetof(nbody_batch_hierarchy_node, mutual_inclination) &&
                  offsetof(BatchHierarchyNode, h) == offsetof(nbody_batch_hierarchy_node, h),
              "nbody_batch_hierarchy_math.h mirrors the node record of nbody_batch_hierarchy.h");
static_assert(sizeof(BatchHierarchyBody) == sizeof(nbody_batch_hierarchy_body) && sizeof(nbody_batch_hierarchy_body) == 16 &&
                  offsetof(BatchHierarchyBody, depth) == offsetof(nbody_batch_hierarchy_body, depth),
              "nbody_batch_hierarchy_math.h mirrors the body record of nbody_batch_hierarchy.h");
static_assert(sizeof(BatchHierarchySystem) == sizeof(nbody_batch_hierarchy_system) && sizeof(nbody_batch_hierarchy_system) == 40 &&
                  offsetof(BatchHierarchySystem, singles) == offsetof(nbody_batch_hierarchy_system, singles) &&
                  offsetof(BatchHierarchySystem, unstable) == offsetof(nbody_batch_hierarchy_system, unstable),
              "nbody_batch_hierarchy_math.h mirrors the system record of nbody_batch_hierarchy.h");
static_assert(kHierarchyMaxLevels == NBODY_BATCH_HIERARCHY_MAX_LEVELS, "nbody_batch_hierarchy_math.h mirrors the limit of nbody_batch_hierarchy.h");

constexpr size_t kHierarchyBytesPerBody = 2 * kBatchBytesPerBody + sizeof(int);  // position, velocity, the slot's node id

// LDS: sh[2 j] = {x, y, z, m} and sh[2 j + 1] = {vx, vy, vz, word} of the root in slot j < m (batch_pairs_kernel's layout,
// 128 KiB at 4096 bodies), then nid[j], the id of that root or -1 for a dead slot (16 KiB): 144 KiB, with the few hundred
// bytes of made and red inside the 160 KiB of a workgroup.  The fourth word of the velocity holds the slot's partner after
// walk 1 and, in the higher slot of a mutual pair, the pair's g after walk 2.
// Dead slots: the mass word of a dead slot is NaN, and so is the row mass of a lane whose row is dead or no leaf.  mu, eps
// and s are then NaN and the searches' own comparisons never take them: no branch, no predicate beside the pairs kernel's.
// What a node needs of a composite child (a, h, stable, leaves) is read back from the node records in global memory, which
// this workgroup wrote at an earlier level with barriers between; LDS holds no per-node array.
// The level loop holds barriers, so its trip count is workgroup-uniform: m, max_levels and t are, and the nodes a level made
// are summed by every lane from the same words of `made`.  The record loop is kept rolled (the fp64 arithmetic is
// instantiated once); the creation order over r = q * T + lane is a ballot within the wave, the waves' counts in LDS and a
// running offset over q.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_hierarchy_kernel(
    const float4 *pos, const float4 *vel, const int *counts, const int *massive, int max_bodies, double tolerance, int max_levels,
    int fill, BatchHierarchyNode *nodes, BatchHierarchyBody *bodies, BatchHierarchySystem *systems)
{
    extern __shared__ float4 sh[];
    __shared__ int made[16];
    __shared__ double red[16 * 5];
    int *nid = reinterpret_cast<int *>(sh + 2 * (size_t)max_bodies);
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int m = massive ? (massive[blockIdx.x] < n ? massive[blockIdx.x] : n) : n;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float dead = __builtin_nanf("");
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < m) {
            const float4 w = vel[base + r];
            sh[2 * r] = pos[base + r];
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            nid[r] = r;
        }
    }
    int nodes_made = 0, levels = 0, converged = 1;  // a system of fewer than two leaves evaluates no level
    if (m >= 2) {
        for (int t = 1;; ++t) {
            __syncthreads();  // the roots of this level are in place
            float4 x[RPL];    // {x, y, z, m} of the row's root; m is NaN for a dead slot and for a row that is no leaf
            float3 v[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                x[q] = make_float4(0.f, 0.f, 0.f, dead);
                v[q] = make_float3(0.f, 0.f, 0.f);
                if (r < m) {
                    x[q] = sh[2 * r];
                    const float4 w = sh[2 * r + 1];
                    v[q] = make_float3(w.x, w.y, w.z);
                }
            }
            // Walk 1: batch_pairs_kernel's search.
            float best[RPL];
            int bj[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                best[q] = __builtin_inff();
                bj[q] = -1;
            }
#pragma unroll 4
            for (int j = 0; j < m; ++j) {
                const float4 pj = sh[2 * j], vj = sh[2 * j + 1];  // wave-uniform addresses: broadcast ds_read_b128
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const float dx = pj.x - x[q].x, dy = pj.y - x[q].y, dz = pj.z - x[q].z;
                    const float wx = vj.x - v[q].x, wy = vj.y - v[q].y, wz = vj.z - v[q].z;
                    const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    const float v2 = __builtin_fmaf(wz, wz, __builtin_fmaf(wy, wy, wx * wx));
                    const float inv = __builtin_amdgcn_rsqf(r2);
                    const float mu = pj.w + x[q].w;
                    const float eps = __builtin_fmaf(-mu, inv, 0.5f * v2);
                    const bool take = r2 > 0.f && eps < best[q];  // r2 == 0: the root itself and coincident roots
                    best[q] = take ? eps : best[q];
                    bj[q] = take ? j : bj[q];
                }
            }
            __syncthreads();  // every lane is done with the columns before the partners replace the fourth words
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                if (r < m)
                    sh[2 * r + 1].w = __int_as_float(bj[q]);
            }
            __syncthreads();
            // The mutual pairs, owned by the lane of the lower slot, and the position X of the node each would make.
            unsigned mut = 0;
            float3 X[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid, j = bj[q];
                X[q] = make_float3(x[q].x, x[q].y, x[q].z);
                if (j > r) {
                    const float4 pj = sh[2 * j];
                    if (__float_as_int(sh[2 * j + 1].w) == r) {
                        const double M = (double)x[q].w + (double)pj.w;
                        mut |= 1u << q;
                        X[q].x = hierarchy_merged(x[q].w, x[q].x, pj.w, pj.x, M);
                        X[q].y = hierarchy_merged(x[q].w, x[q].y, pj.w, pj.y, M);
                        X[q].z = hierarchy_merged(x[q].w, x[q].z, pj.w, pj.z, M);
                    }
                }
            }
            __syncthreads();  // every lane has read its partner's word before a pair's g replaces it
            // Walk 2: the worst perturber of every mutual pair (an unbound pair's g is dropped with the pair).
            float g[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                g[q] = 0.f;
#pragma unroll 4
            for (int k = 0; k < m; ++k) {
                const float4 pk = sh[2 * k];
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const float dx = pk.x - X[q].x, dy = pk.y - X[q].y, dz = pk.z - X[q].z;
                    const float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    const float inv = __builtin_amdgcn_rsqf(r2);
                    const float s = (pk.w * inv) * (inv * inv);
                    const bool take = (k != q * T + tid) & (k != bj[q]) & (s > g[q]);  // one predicate, no branch; a dead slot's s is NaN
                    g[q] = take ? s : g[q];
                }
            }
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                if ((mut >> q) & 1u)
                    sh[2 * bj[q] + 1].w = g[q];
            __syncthreads();  // every lane is done with the columns before the new nodes replace them
            // The records and the new nodes, one row at a time from LDS.  A pair's two slots are read and written by the
            // lane that owns the pair alone.
            int level_made = 0;
#pragma unroll 1
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                bool accept = false;
                BatchHierarchyNode rec = hierarchy_empty_node();
                float4 xi = make_float4(0.f, 0.f, 0.f, 0.f), vi = xi, xj = xi, vj = xi;
                int j = -1;
                if ((mut >> q) & 1u) {
                    xi = sh[2 * r], vi = sh[2 * r + 1];
                    j = __float_as_int(vi.w);
                    xj = sh[2 * j], vj = sh[2 * j + 1];
                    const float pi[3] = {xi.x, xi.y, xi.z}, wi[3] = {vi.x, vi.y, vi.z};
                    const float pj[3] = {xj.x, xj.y, xj.z}, wj[3] = {vj.x, vj.y, vj.z};
                    hierarchy_elements(pi, wi, xi.w, pj, wj, xj.w, rec);
                    rec.perturbation = hierarchy_perturbation(vj.w, rec.semi_major_axis, rec.eccentricity, (double)xj.w + (double)xi.w);
                    accept = hierarchy_accepts(rec.energy, rec.perturbation, tolerance);
                }
                // creation order: the accepted rows before this one in the wave, in the waves before, at the q before
                const unsigned long long votes = __ballot(accept);
                const int before = __popcll(votes & ((1ull << lane) - 1ull));
                __syncthreads();  // every lane has read the counts of the q before
                if (lane == 0)
                    made[wave] = __popcll(votes);
                __syncthreads();
                int lower = 0, total = 0;
                for (int w = 0; w < T / 64; ++w) {
                    const int c = made[w];
                    lower += w < wave ? c : 0;
                    total += c;
                }
                if (accept) {
                    const int k = nodes_made + level_made + lower + before, id = n + k;
                    const int ci = nid[r], cj = nid[j];
                    BatchHierarchyNode *out = nodes + base + k;
                    rec.child[0] = ci;
                    rec.child[1] = cj;
                    rec.level = t;
                    rec.slot = r;
                    *out = rec;  // leaves, stable and the mutual inclinations follow below: little is live across them
                    const float mass = xi.w + xj.w;
                    const double M = (double)xi.w + (double)xj.w;
                    sh[2 * r] = make_float4(hierarchy_merged(xi.w, xi.x, xj.w, xj.x, M), hierarchy_merged(xi.w, xi.y, xj.w, xj.y, M),
                                            hierarchy_merged(xi.w, xi.z, xj.w, xj.z, M), mass);
                    sh[2 * r + 1] = make_float4(hierarchy_merged(xi.w, vi.x, xj.w, vj.x, M), hierarchy_merged(xi.w, vi.y, xj.w, vj.y, M),
                                                hierarchy_merged(xi.w, vi.z, xj.w, vj.z, M), 0.f);
                    sh[2 * j].w = dead;
                    nid[r] = id;
                    nid[j] = -1;
                    int leaves = 0, stable = 1;
#pragma unroll 1
                    for (int c = 0; c < 2; ++c) {
                        const int cid = c ? cj : ci;
                        if (cid < n) {
                            leaves += 1;
                            continue;
                        }
                        BatchHierarchyNode *child = nodes + base + (cid - n);
                        const double mc = c ? (double)xj.w : (double)xi.w, mo = c ? (double)xi.w : (double)xj.w;
                        const double hc[3] = {child->h[0], child->h[1], child->h[2]};
                        const double imut = hierarchy_mutual_inclination(rec.h, hc);
                        const bool passes = hierarchy_child_passes(rec.semi_major_axis, rec.eccentricity, child->semi_major_axis,
                                                                   mo / mc, imut);
                        stable = (passes && child->stable) ? stable : 0;
                        leaves += child->leaves;
                        out->mutual_inclination[c] = imut;
                        child->parent = id;
                    }
                    out->leaves = leaves;
                    out->stable = stable;
                }
                level_made += total;
            }
            // The same words of `made` in every lane of every wave: the exit is the workgroup's.
            const int level_nodes = __builtin_amdgcn_readfirstlane(level_made);
            nodes_made += level_nodes;
            levels = t;
            converged = (level_nodes == 0 || m - nodes_made < 2) ? 1 : 0;
            if (converged || t >= max_levels)
                break;
        }
    }
    __syncthreads();  // the node records and ids of the last level are in place
    // The roots: singles, binaries, triples, higher, unstable.
    double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        const int id = r < m ? nid[r] : -1;
        if (id >= 0) {
            int leaves = 1, stable = 1;
            if (id >= n) {
                leaves = nodes[base + (id - n)].leaves;
                stable = nodes[base + (id - n)].stable;
            }
            c[0] += leaves == 1 ? 1.0 : 0.0;
            c[1] += leaves == 2 ? 1.0 : 0.0;
            c[2] += leaves == 3 ? 1.0 : 0.0;
            c[3] += leaves >= 4 ? 1.0 : 0.0;
            c[4] += stable ? 0.0 : 1.0;
        }
    }
    block_sum(c, red, tid, T);
    if (tid == 0)
        systems[blockIdx.x] = BatchHierarchySystem{nodes_made, m - nodes_made, levels, converged, (int)c[0], (int)c[1], (int)c[2],
                                                   (int)c[3], (int)c[4], 0};
    if (fill) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r >= nodes_made && r < max_bodies)
                nodes[base + r] = hierarchy_empty_node();
        }
    }
    if (bodies) {
        // Every leaf's parent from the nodes' children, in the LDS the roots no longer need; then every leaf climbs.
        int *up = reinterpret_cast<int *>(sh);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n)
                up[r] = -1;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < nodes_made) {
                const int c0 = nodes[base + r].child[0], c1 = nodes[base + r].child[1];
                if (c0 < n)
                    up[c0] = n + r;
                if (c1 < n)
                    up[c1] = n + r;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r >= max_bodies)
                continue;
            BatchHierarchyBody rec = hierarchy_empty_body();
            if (r < n) {
                rec.parent = up[r];
                rec.root = r;
                for (int p = rec.parent; p >= 0; p = nodes[base + (p - n)].parent) {
                    rec.root = p;
                    rec.depth += 1;
                }
            }
            bodies[base + r] = rec;
        }
    }
}

// One launch over all systems.  36 bytes of dynamic LDS per body, 144 KiB at 4096 bodies.  massive and bodies may be NULL;
// fill: write the empty records from the node count on.
hipError_t launch_batch_hierarchy(const float4 *pos, const float4 *vel, const int *counts, const int *massive, int n_systems,
                                  int max_bodies, double tolerance, int max_levels, bool fill, BatchHierarchyNode *nodes,
                                  BatchHierarchyBody *bodies, BatchHierarchySystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kHierarchyBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_hierarchy_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, vel, counts, massive,
                                      max_bodies, tolerance, max_levels, fill ? 1 : 0, nodes, bodies, systems);
    });
}

// ---- groups (include/nbody_batch_groups.h): friends-of-friends clumps at a linking length.  Every row's label is lowered to
// the smallest label among its friends, its root is hooked below, the labels are compressed, and again until a sweep lowers
// nothing; then every row sums its group's weight, position and velocity in fp64 and the roots write the records.  A sibling of
// batch_members_kernel: one workgroup per system with batch_shape's workgroup, the columns broadcast from LDS, RPL rows per lane
// at r = q * T + lane.  The labels never leave the CU.  It reads the state and writes only the handle's records.

static_assert(sizeof(BatchGroupBody) == sizeof(nbody_batch_group_body) && sizeof(nbody_batch_group_body) == 8 &&
                  offsetof(BatchGroupBody, group) == offsetof(nbody_batch_group_body, group) &&
                  offsetof(BatchGroupBody, size) == offsetof(nbody_batch_group_body, size),
              "nbody_batch_groups_math.h mirrors the body record of nbody_batch_groups.h");
static_assert(sizeof(BatchGroupRecord) == sizeof(nbody_batch_group_record) && sizeof(nbody_batch_group_record) == 64 &&
                  offsetof(BatchGroupRecord, weight) == offsetof(nbody_batch_group_record, weight) &&
                  offsetof(BatchGroupRecord, centre) == offsetof(nbody_batch_group_record, centre) &&
                  offsetof(BatchGroupRecord, velocity) == offsetof(nbody_batch_group_record, velocity) &&
                  offsetof(BatchGroupRecord, count) == offsetof(nbody_batch_group_record, count) &&
                  offsetof(BatchGroupRecord, sources) == offsetof(nbody_batch_group_record, sources),
              "nbody_batch_groups_math.h mirrors the group record of nbody_batch_groups.h");
static_assert(sizeof(BatchGroupSystem) == sizeof(nbody_batch_group_system) && sizeof(nbody_batch_group_system) == 32 &&
                  offsetof(BatchGroupSystem, groups) == offsetof(nbody_batch_group_system, groups) &&
                  offsetof(BatchGroupSystem, grouped) == offsetof(nbody_batch_group_system, grouped) &&
                  offsetof(BatchGroupSystem, singles) == offsetof(nbody_batch_group_system, singles) &&
                  offsetof(BatchGroupSystem, largest) == offsetof(nbody_batch_group_system, largest) &&
                  offsetof(BatchGroupSystem, largest_count) == offsetof(nbody_batch_group_system, largest_count) &&
                  offsetof(BatchGroupSystem, sweeps) == offsetof(nbody_batch_group_system, sweeps) &&
                  offsetof(BatchGroupSystem, converged) == offsetof(nbody_batch_group_system, converged) &&
                  offsetof(BatchGroupSystem, reserved) == offsetof(nbody_batch_group_system, reserved),
              "nbody_batch_groups_math.h mirrors the system record of nbody_batch_groups.h");
static_assert(kGroupsMaxSweeps == NBODY_BATCH_GROUPS_MAX_SWEEPS && kGroupsWeightMass == NBODY_BATCH_WEIGHT_MASS &&
                  kGroupsWeightNumber == NBODY_BATCH_WEIGHT_NUMBER,
              "nbody_batch_groups_math.h mirrors the limit of nbody_batch_groups.h and the weights of nbody_batch_structure.h");
static_assert(sizeof(int4) == kGroupsWords * sizeof(int) && kBatchBytesPerBody == sizeof(int4), "a column is one 16-byte read");

// The image {x, y, z, label} and, for the records, the labels in an array of their own while the image holds {x, y, z, w} and
// then {vx, vy, vz, w}: 20 bytes per body.
constexpr size_t kGroupsBytesPerBody = kBatchBytesPerBody + sizeof(int);

// LDS: img[j] = {x, y, z, label} of body j as four words, one ds_read_b128 per column (64 KiB at 4096 bodies), and lab[j]
// behind it for the records (16 KiB more; the limit is raised before the launch).  Rows from the count on carry NaN
// coordinates: they link to nothing, are lowered by nothing and write nothing.
// Every loop that holds a barrier has a workgroup-uniform trip count: n, t and max_sweeps are uniform, and "a label was
// lowered" and "a pass changed a label" come out of block_any; no lane leaves on data of its own.
// One row per lane is held to the 64 registers of eight waves per SIMD, as in batch_members_kernel<1>.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_groups_kernel(
    const float4 *pos, const float4 *vel, const int *counts, const int *massive, const float *linking2, int max_bodies,
    int min_members, int weight, int max_sweeps, BatchGroupBody *bodies, BatchGroupRecord *records, BatchGroupSystem *systems)
{
    extern __shared__ int4 img[];
    __shared__ int flags[16];
    __shared__ int tally[4];  // groups, grouped, singles, the largest key
    int *words = reinterpret_cast<int *>(img);
    int *lab = words + kGroupsWords * max_bodies;
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int m = massive ? (massive[blockIdx.x] < n ? massive[blockIdx.x] : n) : n;
    const float b2 = linking2[blockIdx.x];
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL];  // {x, y, z, the mass word}
    int L[RPL];     // the row's label
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        const float none = __int_as_float(0x7fc00000);
        x[q] = make_float4(none, none, none, 0.f);
        L[q] = r;
        if (r < n) {
            x[q] = pos[base + r];
            img[r] = make_int4(__float_as_int(x[q].x), __float_as_int(x[q].y), __float_as_int(x[q].z), r);
        }
    }
    if (tid == 0) {
        tally[0] = tally[1] = tally[2] = 0;
        tally[3] = kGroupsKeyNone;
    }
    // Phase 1, the sweeps.
    int sweeps = 0, converged = 1;  // a system without bodies runs no sweep
    if (n > 0) {
        for (int t = 1;; ++t) {
            __syncthreads();  // the image, or the labels the sweep before left, are in place
            int c[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                c[q] = L[q];
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const int4 pj = img[j];
                const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z);
#pragma unroll
                for (int q = 0; q < RPL; ++q)
                    c[q] = groups_link(c[q], x[q].x, x[q].y, x[q].z, xj, yj, zj, pj.w, b2);
            }
            bool low = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                low = low || groups_lowered(c[q], L[q]);
            const bool lowered = block_any(low, flags, tid, T);  // its barriers: every lane is done reading the labels
            sweeps = t;
            converged = lowered ? 0 : 1;
            if (!lowered)
                break;
            // Hook: the roots take the minimum of what their rows found.  An LDS integer atomic: the order does not matter.
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                if (groups_lowered(c[q], L[q]))
                    groups_hook(words, q * T + tid, L[q], c[q], [](int *address, int value) { atomicMin(address, value); });
            }
            // Compress: every row reads its root's label, then every row writes, until a pass changes nothing.
            for (;;) {
                __syncthreads();  // the hooks, or the pass before, are in place
                int next[RPL];
                bool moved = false;
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const int r = q * T + tid;
                    next[q] = L[q];
                    if (r < n) {
                        const int now = words[groups_label_at(r)];
                        next[q] = groups_compress(words, now);
                        moved = moved || next[q] != now;
                    }
                }
                const bool again = block_any(moved, flags, tid, T);  // its barriers: every row has read
#pragma unroll
                for (int q = 0; q < RPL; ++q) {
                    const int r = q * T + tid;
                    L[q] = next[q];
                    if (r < n)
                        words[groups_label_at(r)] = next[q];
                }
                if (!again)
                    break;
            }
            if (t >= max_sweeps)
                break;
        }
    }
    // Phase 2, the records: the image takes the weights, the labels move behind it.
    __syncthreads();  // every lane is done with the labels in the image
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            x[q].w = groups_weight(weight, x[q].w, r < m);
            words[groups_label_at(r)] = __float_as_int(x[q].w);
            lab[r] = L[q];
        }
    }
    __syncthreads();
    GroupSums sum[RPL];
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const int4 pj = img[j];
        const int lj = lab[j];
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            groups_add_position(sum[q], lj == L[q], j < m, __int_as_float(pj.w), __int_as_float(pj.x), __int_as_float(pj.y),
                                __int_as_float(pj.z));
    }
    if (records) {  // the same for every lane: a kernel argument
        __syncthreads();  // every lane is done with the positions
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float4 v = vel[base + r];
                img[r] = make_int4(__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), __float_as_int(x[q].w));
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const int4 pj = img[j];
            const int lj = lab[j];
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                groups_add_velocity(sum[q], lj == L[q], __int_as_float(pj.w), __int_as_float(pj.x), __int_as_float(pj.y),
                                    __int_as_float(pj.z));
        }
    }
    // The roots write their group's record and add themselves to the summary: integers, in any order.
    GroupTally mine;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        const bool root = r < n && L[q] == r;
        if (root)
            groups_tally_root(mine, sum[q].count, r, min_members);
        if (r < max_bodies) {
            if (records)
                records[base + r] = root ? groups_record(sum[q]) : groups_empty_record();
            if (bodies)
                bodies[base + r] = r < n ? BatchGroupBody{L[q], sum[q].count} : groups_empty_body();
        }
    }
    if (mine.key != kGroupsKeyNone) {
        atomicAdd(&tally[0], mine.groups);
        atomicAdd(&tally[1], mine.grouped);
        atomicAdd(&tally[2], mine.singles);
        atomicMax(&tally[3], mine.key);
    }
    __syncthreads();
    if (tid == 0)
        systems[blockIdx.x] = groups_summary(GroupTally{tally[0], tally[1], tally[2], tally[3]}, sweeps, converged);
}

// One launch over all systems.  20 bytes of dynamic LDS per body, 80 KiB at 4096 bodies.  massive, bodies and records may be
// NULL; without records the velocities are not read.
hipError_t launch_batch_groups(const float4 *pos, const float4 *vel, const int *counts, const int *massive, const float *linking2,
                               int n_systems, int max_bodies, int min_members, int weight, int max_sweeps, BatchGroupBody *bodies,
                               BatchGroupRecord *records, BatchGroupSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kGroupsBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_groups_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, vel, counts, massive,
                                      linking2, max_bodies, min_members, weight, max_sweeps, bodies, records, systems);
    });
}

// ---- spanning trees (include/nbody_batch_span.h): the Euclidean minimum spanning tree of every system's selected bodies by
// Boruvka's rounds.  Every row finds the cheapest edge that leaves its component, the components take the minimum of their
// rows' keys with a 64-bit LDS integer min, the roots decide, hook and record, the labels are compressed, and again until one
// component is left; then the recorded keys are sorted in LDS and the lengths summed in order.  A sibling of
// batch_groups_kernel: one workgroup per system with batch_shape's workgroup, the columns broadcast from LDS, RPL rows per lane
// at r = q * T + lane.  It reads the state and writes only the handle's records.

static_assert(sizeof(BatchSpanSystem) == sizeof(nbody_batch_span_system) && sizeof(nbody_batch_span_system) == 40 &&
                  offsetof(BatchSpanSystem, edges) == offsetof(nbody_batch_span_system, edges) &&
                  offsetof(BatchSpanSystem, selected) == offsetof(nbody_batch_span_system, selected) &&
                  offsetof(BatchSpanSystem, rounds) == offsetof(nbody_batch_span_system, rounds) &&
                  offsetof(BatchSpanSystem, reserved) == offsetof(nbody_batch_span_system, reserved) &&
                  offsetof(BatchSpanSystem, total_length) == offsetof(nbody_batch_span_system, total_length) &&
                  offsetof(BatchSpanSystem, longest) == offsetof(nbody_batch_span_system, longest) &&
                  offsetof(BatchSpanSystem, mean_separation) == offsetof(nbody_batch_span_system, mean_separation),
              "nbody_batch_span_math.h mirrors the system record of nbody_batch_span.h");
static_assert(sizeof(BatchSpanEdge) == sizeof(nbody_batch_span_edge) && sizeof(nbody_batch_span_edge) == 16 &&
                  offsetof(BatchSpanEdge, i) == offsetof(nbody_batch_span_edge, i) &&
                  offsetof(BatchSpanEdge, j) == offsetof(nbody_batch_span_edge, j) &&
                  offsetof(BatchSpanEdge, r2) == offsetof(nbody_batch_span_edge, r2) &&
                  offsetof(BatchSpanEdge, reserved) == offsetof(nbody_batch_span_edge, reserved),
              "nbody_batch_span_math.h mirrors the edge record of nbody_batch_span.h");
static_assert(sizeof(BatchSpanBody) == sizeof(nbody_batch_span_body) && sizeof(nbody_batch_span_body) == 8 &&
                  offsetof(BatchSpanBody, degree) == offsetof(nbody_batch_span_body, degree) &&
                  offsetof(BatchSpanBody, nearest) == offsetof(nbody_batch_span_body, nearest),
              "nbody_batch_span_math.h mirrors the body record of nbody_batch_span.h");
static_assert(kSpanMaxRounds == NBODY_BATCH_SPAN_MAX_ROUNDS, "nbody_batch_span_math.h mirrors the limit of nbody_batch_span.h");
static_assert(NBODY_BATCH_MAX_BODIES <= (1 << kSpanIndexBits), "an index fills 12 bits of the key");
static_assert(sizeof(SpanKey) == 8 && sizeof(double) == 8, "a 64-bit word holds a key, then a length");

// The image {x, y, z, component}, 16 bytes per body, and behind it one 64-bit word per slot of the sort, whose length is the
// capacity rounded up to a power of two: 24 bytes per body and 96 KiB at 4096 bodies.
inline size_t span_lds_bytes(int max_bodies)
{
    return kBatchBytesPerBody * (size_t)max_bodies + sizeof(SpanKey) * (size_t)span_sort_length(max_bodies);
}

// LDS: img[j] = {x, y, z, component} of body j as four words, one ds_read_b128 per column, and key[] behind it: a component's
// minimum at its root's slot while the rounds run, the row sums of the separations before them, the recorded keys and then the
// lengths after them.  Unselected rows carry kSpanNoComponent and are skipped as columns; rows from the count on are no columns.
// Every loop that holds a barrier has a workgroup-uniform trip count: n, the sort's length and the separations flag are
// uniform, the components left are read from LDS behind a barrier, and "a pass changed a label" comes out of block_any.
// The edge a component records lives in rec[q] of the lane that owns the row of its root: a root is absorbed once.
// One row per lane is held to the 64 registers of eight waves per SIMD, as in batch_groups_kernel<1>.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_span_kernel(
    const float4 *pos, const int *counts, const unsigned char *subset, int max_bodies, int separations, BatchSpanEdge *edges,
    BatchSpanBody *bodies, BatchSpanSystem *systems)
{
    extern __shared__ int4 img[];
    __shared__ int flags[16];
    __shared__ int left;  // the components left; before the rounds, the selected bodies
    int *words = reinterpret_cast<int *>(img);
    SpanKey *key = reinterpret_cast<SpanKey *>(img + max_bodies);
    double *term = reinterpret_cast<double *>(key);
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL];      // {x, y, z, the mass word}
    int L[RPL];         // the row's component; kSpanNoComponent for a row that is not selected
    int nearest[RPL];   // the first round's row result
    SpanKey rec[RPL];   // the edge the row's component recorded when it was absorbed
    if (tid == 0)
        left = 0;
    __syncthreads();
    int mine = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        L[q] = kSpanNoComponent;
        nearest[q] = -1;
        rec[q] = kSpanNoKey;
        if (r < n) {
            x[q] = pos[base + r];
            L[q] = !subset || subset[base + r] != 0 ? r : kSpanNoComponent;
            mine += L[q] != kSpanNoComponent ? 1 : 0;
            img[r] = make_int4(__float_as_int(x[q].x), __float_as_int(x[q].y), __float_as_int(x[q].z), L[q]);
        }
    }
    if (mine)
        atomicAdd(&left, mine);
    __syncthreads();  // the image and the count are in place
    const int selected = left;
    // The separations: every row's sum in ascending j, then thread 0 adds the rows in ascending i.
    double separation = 0.0;
    if (separations && selected > 1) {  // the same for every lane
        double sum[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            sum[q] = 0.0;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const int4 pj = img[j];
            const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z);
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                sum[q] += span_separation(pj.w != kSpanNoComponent && j != q * T + tid,
                                          groups_r2(x[q].x, x[q].y, x[q].z, xj, yj, zj));
        }
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n)
                term[r] = L[q] != kSpanNoComponent ? sum[q] : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < n; ++i)
                separation += term[i];
        }
    }
    // The rounds.
    int rounds = 0;
    for (;;) {
        __syncthreads();  // the labels and the count the round before left are in place; the words are free
        const int components = left;
        if (components <= 1 || rounds >= kSpanMaxRounds)
            break;
        ++rounds;
        SpanBest best[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n)
                key[r] = kSpanNoKey;
        }
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const int4 pj = img[j];
            const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z);
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                span_step(best[q], L[q], x[q].x, x[q].y, x[q].z, xj, yj, zj, pj.w, j);
        }
        __syncthreads();  // every word is cleared
        // The components' minima: an LDS integer atomic, so the order does not matter.
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            if (L[q] != kSpanNoComponent) {
                if (rounds == 1)
                    nearest[q] = best[q].j;
                const SpanKey k = span_row_key(best[q], q * T + tid);
                if (k != kSpanNoKey)
                    atomicMin(&key[L[q]], k);
            }
        }
        __syncthreads();  // the minima are in place
        // The roots decide: reads alone.
        int under[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            under[q] = kSpanNoComponent;
            if (L[q] == r) {  // a selected root
                const SpanKey k = key[r];
                if (k != kSpanNoKey) {
                    const int o = span_other(r, words[groups_label_at(span_key_i(k))], words[groups_label_at(span_key_j(k))]);
                    if (span_hooks(k, key[o], r, o)) {
                        under[q] = o;
                        rec[q] = k;
                    }
                }
            }
        }
        __syncthreads();  // every root has read
        int hooked = 0;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            if (under[q] != kSpanNoComponent) {
                words[groups_label_at(q * T + tid)] = under[q];
                ++hooked;
            }
        }
        if (hooked)
            atomicSub(&left, hooked);
        // Compress: every row reads its root's label, then every row writes, until a pass changes nothing.
        for (;;) {
            __syncthreads();  // the hooks, or the pass before, are in place
            int next[RPL];
            bool moved = false;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                next[q] = L[q];
                if (L[q] != kSpanNoComponent) {
                    const int now = words[groups_label_at(r)];
                    next[q] = span_compress(words, now);
                    moved = moved || next[q] != now;
                }
            }
            const bool again = block_any(moved, flags, tid, T);  // its barriers: every row has read
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                if (L[q] != kSpanNoComponent) {
                    L[q] = next[q];
                    words[groups_label_at(r)] = next[q];
                }
            }
            if (!again)
                break;
        }
    }
    // The sort: the recorded keys into the words, padded with all-ones keys to a power of two, and the image's fourth word
    // cleared for the degrees.  The last barrier of the rounds stands before this: every lane is done with the labels.
    const int recorded = selected - left;  // selected - 1 where the rounds ended with one component
    const int length = span_sort_length(n);
    for (int r = tid; r < length; r += T)
        key[r] = kSpanNoKey;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n)
            words[groups_label_at(r)] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        if (rec[q] != kSpanNoKey)
            key[q * T + tid] = rec[q];
    }
    __syncthreads();
    for (int k = 2; k <= length; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < length / 2; t += T)
                span_exchange(key, t, k, j);
            __syncthreads();
        }
    }
    // Slot e holds the e-th edge: its record, its ends' degrees (integer LDS adds) and, in its word, its length.
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int e = q * T + tid;
        if (e < max_bodies) {
            const SpanKey k = e < length ? key[e] : kSpanNoKey;
            const BatchSpanEdge edge = span_edge(k);
            if (k != kSpanNoKey) {
                atomicAdd(&words[groups_label_at(edge.i)], 1);
                atomicAdd(&words[groups_label_at(edge.j)], 1);
                term[e] = span_length(edge.r2);
            }
            if (edges)
                edges[base + e] = edge;
        }
    }
    __syncthreads();
    if (bodies) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < max_bodies)
                bodies[base + r] = L[q] != kSpanNoComponent ? BatchSpanBody{words[groups_label_at(r)], nearest[q]} : span_empty_body();
        }
    }
    if (tid == 0) {
        double total = 0.0, longest = 0.0;
        for (int e = 0; e < recorded; ++e) {
            longest = term[e];
            total += longest;
        }
        systems[blockIdx.x] = BatchSpanSystem{recorded, selected, rounds, 0, total, longest, span_mean_separation(separation, selected)};
    }
}

// One launch over all systems.  24 bytes of dynamic LDS per body at a power-of-two capacity, 96 KiB at 4096 bodies.  subset,
// edges and bodies may be NULL.
hipError_t launch_batch_span(const float4 *pos, const int *counts, const unsigned char *subset, int n_systems, int max_bodies,
                             int separations, BatchSpanEdge *edges, BatchSpanBody *bodies, BatchSpanSystem *systems,
                             hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_span_kernel<rpl()>, n_systems, sh.threads, span_lds_bytes(max_bodies), stream, pos,
                                      counts, subset, max_bodies, separations, edges, bodies, systems);
    });
}

// ---- neighbours (include/nbody_batch_neighbours.h): every row's k nearest sources by index and squared distance, the sources
// within a radius, and per system the listed, complete and mutual rows and the mean nearest and k-th distances.  A sibling of
// batch_structure_kernel, whose first phase this is with the indices kept: one workgroup per system with batch_shape's
// workgroup, the columns broadcast from LDS, RPL rows per lane at r = q * T + lane.  It reads the positions and writes only
// the handle's records.

static_assert(sizeof(BatchNeighbourSystem) == sizeof(nbody_batch_neighbour_system) && sizeof(nbody_batch_neighbour_system) == 40 &&
                  offsetof(BatchNeighbourSystem, bodies) == offsetof(nbody_batch_neighbour_system, bodies) &&
                  offsetof(BatchNeighbourSystem, sources) == offsetof(nbody_batch_neighbour_system, sources) &&
                  offsetof(BatchNeighbourSystem, listed) == offsetof(nbody_batch_neighbour_system, listed) &&
                  offsetof(BatchNeighbourSystem, complete) == offsetof(nbody_batch_neighbour_system, complete) &&
                  offsetof(BatchNeighbourSystem, mutual) == offsetof(nbody_batch_neighbour_system, mutual) &&
                  offsetof(BatchNeighbourSystem, reserved) == offsetof(nbody_batch_neighbour_system, reserved) &&
                  offsetof(BatchNeighbourSystem, mean_nearest) == offsetof(nbody_batch_neighbour_system, mean_nearest) &&
                  offsetof(BatchNeighbourSystem, mean_kth) == offsetof(nbody_batch_neighbour_system, mean_kth),
              "nbody_batch_neighbours_math.h mirrors the system record of nbody_batch_neighbours.h");
static_assert(sizeof(BatchNeighbourBody) == sizeof(nbody_batch_neighbour_body) && sizeof(nbody_batch_neighbour_body) == 8 &&
                  offsetof(BatchNeighbourBody, found) == offsetof(nbody_batch_neighbour_body, found) &&
                  offsetof(BatchNeighbourBody, within) == offsetof(nbody_batch_neighbour_body, within),
              "nbody_batch_neighbours_math.h mirrors the body record of nbody_batch_neighbours.h");
static_assert(kNeighboursMax == NBODY_BATCH_NEIGHBOURS_MAX, "nbody_batch_neighbours_math.h mirrors the limit of nbody_batch_neighbours.h");

constexpr int kNeighbourTallies = 4;  // sources, listed, complete, mutual

// LDS: img[j] = {x, y, z, source flag} of body j as four words, one ds_read_b128 per column (64 KiB at 4096 bodies; with the
// tallies above the default limit, which is raised before the launch).  After the walk the same bytes hold every row's nearest
// index, one word per row, for `mutual`, and after that every row's two terms of the means, 16 bytes per row again.
// The eight nearest (r2, index) pairs of every row stay in registers (neighbours_insert); one row per lane is held to the 64
// registers of eight waves per SIMD, batch_hermite_kernel<1>'s.  radius2 is b2 per system, or NULL; index and r2 are NULL
// together; bodies may be NULL.
template <int RPL>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_neighbours_kernel(
    const float4 *pos, const int *counts, const unsigned char *sources, const float *radius2, int max_bodies, int k,
    BatchNeighbourBody *bodies, int *index, float *r2, BatchNeighbourSystem *systems)
{
    extern __shared__ int4 img[];
    __shared__ int tally[kNeighbourTallies];
    int *nearest = reinterpret_cast<int *>(img);
    double2 *term = reinterpret_cast<double2 *>(img);
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float b2 = radius2 ? radius2[blockIdx.x] : kNeighboursNoRadius2;
    float4 x[RPL];  // {x, y, z, the mass word}
    if (tid < kNeighbourTallies)
        tally[tid] = 0;
    __syncthreads();
    int mine = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < n) {
            x[q] = pos[base + r];
            const int flag = !sources || sources[base + r] != 0 ? 1 : 0;
            mine += flag;
            img[r] = make_int4(__float_as_int(x[q].x), __float_as_int(x[q].y), __float_as_int(x[q].z), flag);
        }
    }
    if (mine)
        atomicAdd(&tally[0], mine);
    __syncthreads();  // the image is in place
    NeighbourList list[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        neighbours_clear(list[q]);
    // Measured on an MI355X (profiles/batch_rate_neighbours.txt, the lean call at k = 6): with the insertion for every column
    // 1.41 ms at 1024 x 1024 and 5.40 ms at 4096 x 256; skipped where no lane of the wave wants it for any of its rows (one
    // vote per column) 1.40 and 4.31; skipped per row group q (one vote per column and q: 64 rows, not 256, have to agree) 1.18
    // and 3.06.  The same bits all three.  Unlike in structure(), whose insertion is 16 operations, the 40 saved here pay for
    // the vote and the branch once the lists have settled, from a few hundred columns on.  So: a skip per row group.
    for (int j = 0; j < n; ++j) {
        const int4 pj = img[j];  // a wave-uniform address: one broadcast LDS read
        if (__builtin_amdgcn_readfirstlane(pj.w) == 0)
            continue;  // no source: the flag is the same in every lane, so the branch is a scalar one
        const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const float c = neighbours_measure(list[q], q * T + tid, x[q].x, x[q].y, x[q].z, xj, yj, zj, true, j, b2);
            if (__ballot(neighbours_wanted(list[q], c)) != 0)
                neighbours_insert(list[q], c, j);  // changes nothing in a lane that does not want it
        }
    }
    int found[RPL];
    float kth[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const bool live = q * T + tid < n;  // a row from the count on walked the columns from the origin: it holds nothing
        found[q] = live ? neighbours_found(list[q], k) : 0;
        kth[q] = neighbours_kth(list[q], k);
    }
    __syncthreads();  // every lane is done with the columns
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n)
            nearest[r] = list[q].index[0];
    }
    __syncthreads();
    int listed = 0, complete = 0, mutual = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        listed += found[q] >= 1 ? 1 : 0;
        complete += found[q] == k ? 1 : 0;
        mutual += r < n && neighbours_mutual(nearest, r) ? 1 : 0;
    }
    // Integers: the order of the additions does not matter.
    if (listed)
        atomicAdd(&tally[1], listed);
    if (complete)
        atomicAdd(&tally[2], complete);
    if (mutual)
        atomicAdd(&tally[3], mutual);
    __syncthreads();  // every lane is done with the nearest indices
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n)
            term[r] = make_double2(neighbours_term(found[q] >= 1, list[q].r2[0]), neighbours_term(found[q] == k, kth[q]));
    }
    __syncthreads();
    // The lists, k words per row, and the body records; slot by slot under t < k: a list indexed by the slot would live in
    // scratch memory.  A live row's slots from `found` on hold the empty values already.
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < max_bodies) {
            const bool live = r < n;
            if (index) {
                const size_t at = (base + r) * (size_t)k;
#pragma unroll
                for (int t = 0; t < kNeighboursMax; ++t) {
                    if (t < k) {
                        index[at + t] = live ? list[q].index[t] : kNeighboursNoIndex;
                        r2[at + t] = live ? list[q].r2[t] : neighbours_no_r2();
                    }
                }
            }
            if (bodies)
                bodies[base + r] = live ? BatchNeighbourBody{found[q], list[q].within} : neighbours_empty_body();
        }
    }
    // The two sums, by one thread in ascending i: the same bits in any slot, batch and capacity.
    if (tid == 0) {
        double nearest_sum = 0.0, kth_sum = 0.0;
        for (int i = 0; i < n; ++i) {
            const double2 t = term[i];
            nearest_sum += t.x;
            kth_sum += t.y;
        }
        systems[blockIdx.x] = BatchNeighbourSystem{n, tally[0], tally[1], tally[2], tally[3], 0, neighbours_mean(nearest_sum, tally[1]),
                                                   neighbours_mean(kth_sum, tally[2])};
    }
}

// One launch over all systems.  16 bytes of dynamic LDS per body, 64 KiB at 4096 bodies beside the tallies.  sources, radius2,
// bodies and the two list arrays may be NULL.
hipError_t launch_batch_neighbours(const float4 *pos, const int *counts, const unsigned char *sources, const float *radius2,
                                   int n_systems, int max_bodies, int k, BatchNeighbourBody *bodies, int *index, float *r2,
                                   BatchNeighbourSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_neighbours_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, counts, sources,
                                      radius2, max_bodies, k, bodies, index, r2, systems);
    });
}

// ---- correlation (include/nbody_batch_correlation.h): per system the ordered pairs (row, source) in each of up to 32 bins of
// separation, and those below the first edge, above the last and unmeasured.  A sibling of batch_neighbours_kernel, whose
// count within a radius this is at bins + 1 radii at once: one workgroup per system with batch_shape's workgroup, the columns
// broadcast from LDS, RPL rows per lane at r = q * T + lane.  It reads the positions and writes only the handle's records.

static_assert(sizeof(BatchCorrelationSystem) == sizeof(nbody_batch_correlation_system) && sizeof(nbody_batch_correlation_system) == 48 &&
                  offsetof(BatchCorrelationSystem, rows) == offsetof(nbody_batch_correlation_system, rows) &&
                  offsetof(BatchCorrelationSystem, sources) == offsetof(nbody_batch_correlation_system, sources) &&
                  offsetof(BatchCorrelationSystem, both) == offsetof(nbody_batch_correlation_system, both) &&
                  offsetof(BatchCorrelationSystem, bins) == offsetof(nbody_batch_correlation_system, bins) &&
                  offsetof(BatchCorrelationSystem, pairs) == offsetof(nbody_batch_correlation_system, pairs) &&
                  offsetof(BatchCorrelationSystem, below) == offsetof(nbody_batch_correlation_system, below) &&
                  offsetof(BatchCorrelationSystem, above) == offsetof(nbody_batch_correlation_system, above) &&
                  offsetof(BatchCorrelationSystem, unmeasured) == offsetof(nbody_batch_correlation_system, unmeasured) &&
                  offsetof(nbody_batch_correlation_system, pairs) == 16 && offsetof(nbody_batch_correlation_system, unmeasured) == 40,
              "nbody_batch_correlation_math.h mirrors the system record of nbody_batch_correlation.h");
static_assert(kCorrelationMaxBins == NBODY_BATCH_CORRELATION_MAX_BINS, "nbody_batch_correlation_math.h mirrors the limit of nbody_batch_correlation.h");

// The two loops, the same integers.  0: counters the wave shares -- per column and edge one v_cmp against a wave-uniform e2[t],
// whose lane mask is popcounted and added into a scalar register: no vector register per counter, whatever the rows per lane.
// 1: a counter per lane and edge, BINS + 2 more vector registers, summed over the wave once at the end; the compiler makes a
// compare, a select and half an add3 of each edge and pair, 2.6 vector instructions.
// Measured on an MI355X (profiles/batch_rate_correlation.txt; lean calls at 32 bins, ms): loop 0 2.68 at 1024 x 1024 and 10.40
// at 4096 x 256, loop 1 3.04 and 11.70.  Loop 0 is bound by the scalar unit, which the four SIMDs of a compute unit share: its
// first form, which AND-ed every edge's mask with the mask of the lanes that examine the pair (three scalar instructions per
// edge and pair), took 3.68 and 14.47 and lost to loop 1; hiding a pair that is not examined behind a NaN (one select per
// pair) leaves two scalar instructions per edge and pair, and wins.  So: loop 0.
#ifndef NBODY_BATCH_CORRELATION_LANE_COUNTERS
#define NBODY_BATCH_CORRELATION_LANE_COUNTERS 0
#endif

constexpr int kCorrelationTallies = 3;  // rows, sources, both

#if NBODY_BATCH_CORRELATION_LANE_COUNTERS
using CorrelationAdd = CorrelationAddOne;
// The wave's sum of its lanes' counters, in lane 0.
__device__ inline unsigned int correlation_wave_total(unsigned int word)
{
    for (int off = 32; off > 0; off >>= 1)
        word += __shfl_down(word, off, 64);
    return word;
}
#else
// The counter of a wave takes the number of its lanes whose flag is set.  A pair that is not examined shows a NaN, one select
// per pair, so that the flag is a compare alone, whose result is a lane mask already: the builtin takes it as that (__ballot
// would make a word per lane of it and compare again), and the count and the addition are scalar instructions.
struct CorrelationAdd {
    __device__ float seen(bool examined, float r2) const { return examined ? r2 : __builtin_nanf(""); }
    __device__ void operator()(unsigned int &word, bool, bool flag) const
    {
        word += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(flag));
    }
};
__device__ inline unsigned int correlation_wave_total(unsigned int word) { return word; }
#endif

// LDS: img[j] = {x, y, z, source flag} of body j as four words, one ds_read_b128 per column (64 KiB at 4096 bodies; with the
// totals above the default limit, which is raised before the launch).  edges2 holds BINS + 1 squared edges per system
// (edge_stride = BINS + 1) or one set for all (edge_stride = 0), the edges from `bins` on copies of edge `bins`: their
// counters equal within[bins] and are not read.  BINS is a template argument and every loop over the edges is unrolled, so
// that no edge index ever becomes a register index.  rows, sources and counts_out may be NULL.
template <int RPL, int BINS>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_correlation_kernel(
    const float4 *__restrict__ pos, const int *__restrict__ counts, const unsigned char *__restrict__ rows,
    const unsigned char *__restrict__ sources, const float *__restrict__ edges2, int edge_stride, int max_bodies, int bins,
    unsigned int *__restrict__ counts_out, BatchCorrelationSystem *__restrict__ systems)
{
    constexpr int EDGES = BINS + 1;
    extern __shared__ int4 img[];
    __shared__ unsigned int total[EDGES + 1];  // within[0 ... BINS], measured
    __shared__ int tally[kCorrelationTallies];
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float *mine2 = edges2 + (size_t)blockIdx.x * (size_t)edge_stride;
    float e2[EDGES];  // the same in every lane
#pragma unroll
    for (int t = 0; t < EDGES; ++t)
        e2[t] = mine2[t];
    if (tid < EDGES + 1)
        total[tid] = 0;
    if (tid < kCorrelationTallies)
        tally[tid] = 0;
    __syncthreads();
    float4 x[RPL];  // {x, y, z, the mass word}
    bool row[RPL];
    int n_rows = 0, n_sources = 0, n_both = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        row[q] = false;
        if (r < n) {
            x[q] = pos[base + r];
            const bool source = !sources || sources[base + r] != 0;
            row[q] = !rows || rows[base + r] != 0;
            n_rows += row[q] ? 1 : 0;
            n_sources += source ? 1 : 0;
            n_both += row[q] && source ? 1 : 0;
            img[r] = make_int4(__float_as_int(x[q].x), __float_as_int(x[q].y), __float_as_int(x[q].z), source ? 1 : 0);
        }
    }
    // Integers: the order of the additions does not matter.
    if (n_rows)
        atomicAdd(&tally[0], n_rows);
    if (n_sources)
        atomicAdd(&tally[1], n_sources);
    if (n_both)
        atomicAdd(&tally[2], n_both);
    __syncthreads();  // the image is in place
    CorrelationCounters<EDGES> c;
    correlation_clear(c);
    for (int j = 0; j < n; ++j) {
        const int4 pj = img[j];  // a wave-uniform address: one broadcast LDS read
        if (__builtin_amdgcn_readfirstlane(pj.w) == 0)
            continue;  // no source: the flag is the same in every lane, so the branch is a scalar one
        const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z);
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            correlation_step(c, correlation_examined(row[q], true, q * T + tid, j), x[q].x, x[q].y, x[q].z, xj, yj, zj, e2, CorrelationAdd{});
    }
    // Every wave adds its counters into the totals; t is a constant in every copy of the body.
#pragma unroll
    for (int t = 0; t < EDGES; ++t) {
        const unsigned int w = correlation_wave_total(c.within[t]);
        if ((tid & 63) == 0 && w)
            atomicAdd(&total[t], w);
    }
    const unsigned int m = correlation_wave_total(c.measured);
    if ((tid & 63) == 0 && m)
        atomicAdd(&total[EDGES], m);
    __syncthreads();
    // One lane per word: the bins by differences of their two edges, and the record.
    if (counts_out && tid < bins)
        counts_out[(size_t)blockIdx.x * (size_t)bins + tid] = correlation_bin(total[tid], total[tid + 1]);
    if (tid == 0)
        systems[blockIdx.x] = correlation_record(tally[0], tally[1], tally[2], bins, total, total[EDGES]);
}

// One launch over all systems.  16 bytes of dynamic LDS per body, 64 KiB at 4096 bodies beside the totals.  The call runs the
// instantiation of correlation_padded_bins(bins), for which edges2 is laid out.  rows, sources and counts_out may be NULL.
hipError_t launch_batch_correlation(const float4 *pos, const int *counts, const unsigned char *rows, const unsigned char *sources,
                                    const float *edges2, int edge_stride, int n_systems, int max_bodies, int bins,
                                    unsigned int *counts_out, BatchCorrelationSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        const auto launch = [&](auto padded) {
            return launch_analysis_kernel(batch_correlation_kernel<rpl(), padded()>, n_systems, sh.threads, lds, stream, pos, counts,
                                          rows, sources, edges2, edge_stride, max_bodies, bins, counts_out, systems);
        };
        switch (correlation_padded_bins(bins)) {
        case 8: return launch(std::integral_constant<int, 8>{});
        case 16: return launch(std::integral_constant<int, 16>{});
        default: return launch(std::integral_constant<int, kCorrelationMaxBins>{});
        }
    });
}

// ---- contacts (include/nbody_batch_contacts.h): per system every unordered pair of bodies within a radius, or within the sum
// of its two bodies' radii, as a list (i, j, r2) ascending in i and then in j, with per body its contacts and their place in
// the list and per system their number and the closest.  A sibling of batch_correlation_kernel: one workgroup per system with
// batch_shape's workgroup, the columns broadcast from LDS, RPL rows per lane at r = q * T + lane.  It reads the positions and
// writes only the handle's records.  The first result here of variable length: the kernel counts, places and fills in one
// launch, and no choice in it depends on the schedule -- the counts are integers, the places a prefix sum in ascending row
// index, and every entry has one place that only its row writes.

static_assert(sizeof(BatchContactSystem) == sizeof(nbody_batch_contact_system) && sizeof(nbody_batch_contact_system) == 48 &&
                  offsetof(BatchContactSystem, bodies) == offsetof(nbody_batch_contact_system, bodies) &&
                  offsetof(BatchContactSystem, touching) == offsetof(nbody_batch_contact_system, touching) &&
                  offsetof(BatchContactSystem, max_degree) == offsetof(nbody_batch_contact_system, max_degree) &&
                  offsetof(BatchContactSystem, reserved) == offsetof(nbody_batch_contact_system, reserved) &&
                  offsetof(BatchContactSystem, pairs) == offsetof(nbody_batch_contact_system, pairs) &&
                  offsetof(BatchContactSystem, stored) == offsetof(nbody_batch_contact_system, stored) &&
                  offsetof(BatchContactSystem, closest_i) == offsetof(nbody_batch_contact_system, closest_i) &&
                  offsetof(BatchContactSystem, closest_j) == offsetof(nbody_batch_contact_system, closest_j) &&
                  offsetof(BatchContactSystem, closest_r2) == offsetof(nbody_batch_contact_system, closest_r2) &&
                  offsetof(BatchContactSystem, reserved2) == offsetof(nbody_batch_contact_system, reserved2) &&
                  offsetof(nbody_batch_contact_system, pairs) == 16 && offsetof(nbody_batch_contact_system, reserved2) == 44,
              "nbody_batch_contacts_math.h mirrors the system record of nbody_batch_contacts.h");
static_assert(sizeof(BatchContactBody) == sizeof(nbody_batch_contact_body) && sizeof(nbody_batch_contact_body) == 16 &&
                  offsetof(BatchContactBody, degree) == offsetof(nbody_batch_contact_body, degree) &&
                  offsetof(BatchContactBody, upper) == offsetof(nbody_batch_contact_body, upper) &&
                  offsetof(BatchContactBody, first) == offsetof(nbody_batch_contact_body, first) &&
                  offsetof(BatchContactBody, nearest) == offsetof(nbody_batch_contact_body, nearest),
              "nbody_batch_contacts_math.h mirrors the body record of nbody_batch_contacts.h");
static_assert(sizeof(BatchContact) == sizeof(nbody_batch_contact) && sizeof(nbody_batch_contact) == 12 &&
                  offsetof(BatchContact, i) == offsetof(nbody_batch_contact, i) && offsetof(BatchContact, j) == offsetof(nbody_batch_contact, j) &&
                  offsetof(BatchContact, r2) == offsetof(nbody_batch_contact, r2),
              "nbody_batch_contacts_math.h mirrors the list entry of nbody_batch_contacts.h");
static_assert(kContactsMaxEntries == NBODY_BATCH_CONTACTS_MAX_ENTRIES, "nbody_batch_contacts_math.h mirrors the limit of nbody_batch_contacts.h");

// The fill, the same entries either way.  0: a wave none of whose rows has an entry to write below the capacity skips the
// second walk -- one ballot, so the branch is a scalar one.  1: every wave repeats the walk.
// Measured on an MI355X (profiles/batch_rate_contacts.txt; the listing call without the body records at 1024 x 1024, 256 x 4096
// and 4096 x 256, ms): with few contacts (0.2 mean spacings) fill 0 0.97, 0.41 and 3.12, fill 1 0.96, 0.42 and 3.09; with many
// (1.0 spacings, a list of 24 to 30 MB whose copy to the host is most of the call) fill 0 6.54, 7.03 and 8.18 -- 6.81, 7.11 and
// 8.40 when run again -- and fill 1 6.84, 7.43 and 8.81.  The same bytes.  The difference is inside the spread of the repeats:
// the second walk starts above the wave's first row and is short beside the first.  So: fill 0, which never does more work.
#ifndef NBODY_BATCH_CONTACTS_FILL_ALWAYS
#define NBODY_BATCH_CONTACTS_FILL_ALWAYS 0
#endif

constexpr int kContactTallies = 3;   // bodies, touching, max_degree
constexpr int kContactUnits = 64;    // rows per lane x waves, at most: 4 x 16

// The inclusive sum of `word` over the lanes of a wave up to the lane's own: lane l holds word[0] + ... + word[l].
__device__ inline int contacts_wave_scan(int word, int lane)
{
    for (int off = 1; off < kContactsWave; off <<= 1) {
        const int below = __shfl_up(word, off, kContactsWave);
        word += lane >= off ? below : 0;
    }
    return word;
}

// LDS: img[j] = {x, y, z, w} of body j as four words, one ds_read_b128 per column (64 KiB at 4096 bodies; with the totals
// above the default limit, which is raised before the launch).  RADII: w is the body's radius, a NaN where the body does not
// take part, which is within no threshold; else w is the take-part flag, and a column without it is skipped on the scalar
// unit.  The sums of `upper` over the 64 rows of every unit (a wave's rows of one q) are the only other LDS: the places inside
// a unit come from shuffles.  radius2 is b2 per system (!RADII), radii one radius per slot (RADII); subset and bodies may be
// NULL; list is NULL iff capacity == 0.
template <int RPL, bool RADII>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_contacts_kernel(
    const float4 *__restrict__ pos, const int *__restrict__ counts, const unsigned char *__restrict__ subset,
    const float *__restrict__ radius2, const float *__restrict__ radii, int max_bodies, long long capacity,
    BatchContactBody *__restrict__ bodies, BatchContact *__restrict__ list, BatchContactSystem *__restrict__ systems)
{
    extern __shared__ int4 img[];
    __shared__ int totals[kContactUnits];
    __shared__ int tally[kContactTallies];
    __shared__ SpanKey closest;
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kContactsWave - 1), wave = tid / kContactsWave, waves = T / kContactsWave;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float b2 = RADII ? 0.f : radius2[blockIdx.x];
    if (tid < kContactUnits)
        totals[tid] = 0;
    if (tid < kContactTallies)
        tally[tid] = 0;
    if (tid == 0)
        closest = kSpanNoKey;
    __syncthreads();
    float4 x[RPL];  // {x, y, z, the mass word}
    float rad[RPL];
    bool take[RPL];
    int taking = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        rad[q] = contacts_no_radius();
        take[q] = false;
        if (r < n) {
            x[q] = pos[base + r];
            take[q] = !subset || subset[base + r] != 0;
            if (RADII)
                rad[q] = take[q] ? radii[base + r] : contacts_no_radius();
            taking += take[q] ? 1 : 0;
            img[r] = make_int4(__float_as_int(x[q].x), __float_as_int(x[q].y), __float_as_int(x[q].z),
                               RADII ? __float_as_int(rad[q]) : (take[q] ? 1 : 0));
        }
    }
    if (taking)
        atomicAdd(&tally[0], taking);  // integers: the order of the additions does not matter
    __syncthreads();                   // the image is in place
    // Count: every row walks every column.
    ContactRow row[RPL];
    for (int j = 0; j < n; ++j) {
        const int4 pj = img[j];  // a wave-uniform address: one broadcast LDS read
        if (!RADII && __builtin_amdgcn_readfirstlane(pj.w) == 0)
            continue;  // takes no part: the flag is the same in every lane, so the branch is a scalar one
        const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z), wj = __int_as_float(pj.w);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            contacts_step(row[q], contacts_examined(take[q], true, r, j), r, j, groups_r2(x[q].x, x[q].y, x[q].z, xj, yj, zj),
                          RADII ? contacts_radii_t2(rad[q], wj) : b2);
        }
    }
    int touching = 0, max_degree = 0;
    SpanKey key = kSpanNoKey;
    int within[RPL];  // the inclusive sum of upper over the lower lanes of the row's unit, and the row
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        touching += row[q].degree >= 1 ? 1 : 0;
        max_degree = row[q].degree > max_degree ? row[q].degree : max_degree;
        const SpanKey mine = contacts_row_key(row[q], q * T + tid);
        key = mine < key ? mine : key;
        within[q] = contacts_wave_scan(row[q].upper, lane);
        if (lane == kContactsWave - 1)
            totals[contacts_unit(q, waves, wave)] = within[q];
    }
    // Integers again: a sum, a maximum and a minimum, in any order.
    if (touching)
        atomicAdd(&tally[1], touching);
    if (max_degree)
        atomicMax(&tally[2], max_degree);
    if (key != kSpanNoKey)
        atomicMin(&closest, key);
    __syncthreads();
    // Place: the units in ascending order hold the rows in ascending order, so a row starts at the sum of the units below its
    // own and of the lower rows of its own.  A slot from the count on, or a body that takes no part, has no entry and takes
    // the running sum like any other row.
    int first[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        first[q] = contacts_units_below(totals, contacts_unit(q, waves, wave)) + within[q] - row[q].upper;
    const long long pairs = (long long)contacts_units_below(totals, RPL * waves);
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (bodies && r < max_bodies)
            bodies[base + r] = contacts_body(row[q], first[q]);
    }
    if (tid == 0)
        systems[blockIdx.x] = contacts_system(tally[0], tally[1], tally[2], pairs, capacity, closest);
    if (capacity == 0)
        return;  // the same in every lane; no barrier follows
    // Fill: a row walks the columns above it again and writes its entries from `first` on while they are below the capacity.
    // No row of this wave is below its first lane's row of q = 0, so no column up to that one is above any of them.
    BatchContact *mine = list + (size_t)blockIdx.x * (size_t)capacity;
    bool fills = false;
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        fills = fills || contacts_row_fills(first[q], row[q].upper, capacity);
    if (NBODY_BATCH_CONTACTS_FILL_ALWAYS || __ballot(fills) != 0) {
        int t[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            t[q] = 0;
        for (int j = wave * kContactsWave + 1; j < n; ++j) {
            const int4 pj = img[j];
            if (!RADII && __builtin_amdgcn_readfirstlane(pj.w) == 0)
                continue;
            const float xj = __int_as_float(pj.x), yj = __int_as_float(pj.y), zj = __int_as_float(pj.z), wj = __int_as_float(pj.w);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                contacts_fill(mine, capacity, first[q], t[q], contacts_examined(take[q], true, r, j), r, j,
                              groups_r2(x[q].x, x[q].y, x[q].z, xj, yj, zj), RADII ? contacts_radii_t2(rad[q], wj) : b2);
            }
        }
    }
    // The pads, from `stored` on.
    for (long long k = contacts_stored(pairs, capacity) + tid; k < capacity; k += T)
        mine[k] = contacts_pad();
}

// One launch over all systems.  16 bytes of dynamic LDS per body, 64 KiB at 4096 bodies beside the totals.  Exactly one of
// radius2 and radii is given; subset and bodies may be NULL; list is NULL iff capacity == 0.
hipError_t launch_batch_contacts(const float4 *pos, const int *counts, const unsigned char *subset, const float *radius2,
                                 const float *radii, int n_systems, int max_bodies, long long capacity, BatchContactBody *bodies,
                                 BatchContact *list, BatchContactSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        const auto launch = [&](auto mode) {
            return launch_analysis_kernel(batch_contacts_kernel<rpl(), mode()>, n_systems, sh.threads, lds, stream, pos, counts, subset,
                                          radius2, radii, max_bodies, capacity, bodies, list, systems);
        };
        return radii ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

// ---- approaches (include/nbody_batch_approaches.h): per system every unordered pair of bodies that comes within a radius, or
// within the sum of its two bodies' radii, on straight lines at the current velocities before a horizon, as a list
// (i, j, r2, rv, v2, phase) ascending in i and then in j, with per body its approaches and their place in the list and per
// system their number by phase.  batch_contacts_kernel's sibling, with its count, place and fill in one launch and its units,
// over the position-plus-velocity image of batch_pairs_kernel.  It reads the state and writes only the handle's records; no
// choice in it depends on the schedule, and it computes no time and no distance.

static_assert(sizeof(BatchApproachSystem) == sizeof(nbody_batch_approach_system) && sizeof(nbody_batch_approach_system) == 48 &&
                  offsetof(BatchApproachSystem, bodies) == offsetof(nbody_batch_approach_system, bodies) &&
                  offsetof(BatchApproachSystem, approaching) == offsetof(nbody_batch_approach_system, approaching) &&
                  offsetof(BatchApproachSystem, max_degree) == offsetof(nbody_batch_approach_system, max_degree) &&
                  offsetof(BatchApproachSystem, reserved) == offsetof(nbody_batch_approach_system, reserved) &&
                  offsetof(BatchApproachSystem, pairs) == offsetof(nbody_batch_approach_system, pairs) &&
                  offsetof(BatchApproachSystem, stored) == offsetof(nbody_batch_approach_system, stored) &&
                  offsetof(BatchApproachSystem, now) == offsetof(nbody_batch_approach_system, now) &&
                  offsetof(BatchApproachSystem, passing) == offsetof(nbody_batch_approach_system, passing) &&
                  offsetof(BatchApproachSystem, ending) == offsetof(nbody_batch_approach_system, ending) &&
                  offsetof(BatchApproachSystem, reserved2) == offsetof(nbody_batch_approach_system, reserved2) &&
                  offsetof(nbody_batch_approach_system, pairs) == 16 && offsetof(nbody_batch_approach_system, reserved2) == 44,
              "nbody_batch_approaches_math.h mirrors the system record of nbody_batch_approaches.h");
static_assert(sizeof(BatchApproachBody) == sizeof(nbody_batch_approach_body) && sizeof(nbody_batch_approach_body) == 16 &&
                  offsetof(BatchApproachBody, degree) == offsetof(nbody_batch_approach_body, degree) &&
                  offsetof(BatchApproachBody, upper) == offsetof(nbody_batch_approach_body, upper) &&
                  offsetof(BatchApproachBody, first) == offsetof(nbody_batch_approach_body, first) &&
                  offsetof(BatchApproachBody, now) == offsetof(nbody_batch_approach_body, now),
              "nbody_batch_approaches_math.h mirrors the body record of nbody_batch_approaches.h");
static_assert(sizeof(BatchApproach) == sizeof(nbody_batch_approach) && sizeof(nbody_batch_approach) == 24 &&
                  offsetof(BatchApproach, i) == offsetof(nbody_batch_approach, i) && offsetof(BatchApproach, j) == offsetof(nbody_batch_approach, j) &&
                  offsetof(BatchApproach, r2) == offsetof(nbody_batch_approach, r2) && offsetof(BatchApproach, rv) == offsetof(nbody_batch_approach, rv) &&
                  offsetof(BatchApproach, v2) == offsetof(nbody_batch_approach, v2) &&
                  offsetof(BatchApproach, phase) == offsetof(nbody_batch_approach, phase),
              "nbody_batch_approaches_math.h mirrors the list entry of nbody_batch_approaches.h");
static_assert(kApproachesMaxEntries == NBODY_BATCH_APPROACHES_MAX_ENTRIES, "nbody_batch_approaches_math.h mirrors the limit of nbody_batch_approaches.h");
static_assert(kApproachNow == NBODY_BATCH_APPROACH_NOW && kApproachPassage == NBODY_BATCH_APPROACH_PASSAGE && kApproachEnd == NBODY_BATCH_APPROACH_END,
              "nbody_batch_approaches_math.h mirrors the phases of nbody_batch_approaches.h");

// The separation at the horizon (m2, six fused operations), the same phases either way.  0: it is computed for a column only
// where a ballot finds a lane whose pair is decided at the horizon -- a scalar branch.  1: every lane computes it for every pair.
// Measured on an MI355X (profiles/batch_rate_approaches.txt; Plummer spheres at 0.2 mean spacings and a horizon of one
// crossing, the counting call and the listing call without the body records at 1024 x 1024, 4096 x 256 and 256 x 4096, ms):
// behind the ballot 1.87, 7.17 and 0.55 counting and 3.97, 13.30 and 1.63 listing; in every lane 1.48, 5.62 and 0.45 counting
// and 3.23, 10.27 and 1.46 listing.  The same bytes (the list's checksum agrees).  Half of all pairs are closing, and a
// distant closing pair has its closest point beyond a short horizon, so nearly every column finds such a lane in its wave: the
// branch saves nothing and adds its compare and its wait.  So: every lane, which lost in no case.
#ifndef NBODY_BATCH_APPROACHES_END_ALWAYS
#define NBODY_BATCH_APPROACHES_END_ALWAYS 1
#endif
// The fill's second walk, as NBODY_BATCH_CONTACTS_FILL_ALWAYS: 0 skips it in a wave with nothing to write.
#ifndef NBODY_BATCH_APPROACHES_FILL_ALWAYS
#define NBODY_BATCH_APPROACHES_FILL_ALWAYS 0
#endif

constexpr int kApproachTallies = 3 + kApproachPhases;  // bodies, approaching, max_degree, then the pairs of each phase

// The phases of the RPL pairs of one column: words[q] and phase[q] of row q against pj.
template <int RPL>
__device__ inline void approaches_column(const ApproachPoint (&mine)[RPL], const float (&t2)[RPL], const ApproachPoint &pj, float h,
                                         ApproachWords (&words)[RPL], int (&phase)[RPL])
{
    bool ends = false;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        words[q] = approaches_words(mine[q], pj);
        ends = ends || approaches_ends(words[q], t2[q], h);
    }
    const bool reach = NBODY_BATCH_APPROACHES_END_ALWAYS || __ballot(ends) != 0;  // the same in every lane of the wave
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        phase[q] = approaches_phase(words[q], t2[q], h, reach ? approaches_m2(mine[q], pj, h) : __builtin_inff());
}

// LDS: img[2 j] = {x, y, z, radius} and img[2 j + 1] = {vx, vy, vz, take} of body j, two ds_read_b128 per column (128 KiB at
// 4096 bodies, batch_pairs_kernel's image, under the limit raised before the launch).  The radius is 0 in radius mode and in
// radii mode a NaN where the body takes no part, which is within no threshold; the take-part flag replaces the velocity's unused
// fourth word, and a column without it is skipped on the scalar unit.  The sums of `upper` over the 64 rows of every unit are
// the only other LDS.  radius2 is b2 per system (!RADII), radii one radius per slot (RADII), horizon H per system; subset and
// bodies may be NULL; list is NULL iff capacity == 0.
template <int RPL, bool RADII>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4))) void batch_approaches_kernel(
    const float4 *__restrict__ pos, const float4 *__restrict__ vel, const int *__restrict__ counts,
    const unsigned char *__restrict__ subset, const float *__restrict__ radius2, const float *__restrict__ radii,
    const float *__restrict__ horizon, int max_bodies, long long capacity, BatchApproachBody *__restrict__ bodies,
    BatchApproach *__restrict__ list, BatchApproachSystem *__restrict__ systems)
{
    extern __shared__ int4 img[];
    __shared__ int totals[kContactUnits];
    __shared__ int tally[kApproachTallies];
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kContactsWave - 1), wave = tid / kContactsWave, waves = T / kContactsWave;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float b2 = RADII ? 0.f : radius2[blockIdx.x];
    const float h = horizon[blockIdx.x];
    if (tid < kContactUnits)
        totals[tid] = 0;
    if (tid < kApproachTallies)
        tally[tid] = 0;
    __syncthreads();
    ApproachPoint x[RPL];
    float rad[RPL];
    bool take[RPL];
    int taking = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = ApproachPoint{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        rad[q] = contacts_no_radius();
        take[q] = false;
        if (r < n) {
            const float4 p = pos[base + r], v = vel[base + r];
            x[q] = ApproachPoint{p.x, p.y, p.z, v.x, v.y, v.z};
            take[q] = !subset || subset[base + r] != 0;
            if (RADII)
                rad[q] = take[q] ? radii[base + r] : contacts_no_radius();
            taking += take[q] ? 1 : 0;
            img[2 * r] = make_int4(__float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z), RADII ? __float_as_int(rad[q]) : 0);
            img[2 * r + 1] = make_int4(__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), take[q] ? 1 : 0);
        }
    }
    if (taking)
        atomicAdd(&tally[0], taking);  // integers: the order of the additions does not matter
    __syncthreads();                   // the image is in place
    // Count: every row walks every column.
    ApproachRow row[RPL];
    int phases[kApproachPhases] = {0, 0, 0};
    float t2[RPL];
    ApproachWords words[RPL];
    int phase[RPL];
    for (int j = 0; j < n; ++j) {
        const int4 pj = img[2 * j], vj = img[2 * j + 1];  // wave-uniform addresses: broadcast LDS reads
        if (__builtin_amdgcn_readfirstlane(vj.w) == 0)
            continue;  // takes no part: the flag is the same in every lane, so the branch is a scalar one
        const ApproachPoint column{__int_as_float(pj.x), __int_as_float(pj.y), __int_as_float(pj.z),
                                   __int_as_float(vj.x), __int_as_float(vj.y), __int_as_float(vj.z)};
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            t2[q] = RADII ? contacts_radii_t2(rad[q], __int_as_float(pj.w)) : b2;
        approaches_column<RPL>(x, t2, column, h, words, phase);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            approaches_step(row[q], phases, contacts_examined(take[q], true, r, j), r, j, phase[q]);
        }
    }
    int approaching = 0, max_degree = 0;
    int within[RPL];  // the inclusive sum of upper over the lower lanes of the row's unit, and the row
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        approaching += row[q].degree >= 1 ? 1 : 0;
        max_degree = row[q].degree > max_degree ? row[q].degree : max_degree;
        within[q] = contacts_wave_scan(row[q].upper, lane);
        if (lane == kContactsWave - 1)
            totals[contacts_unit(q, waves, wave)] = within[q];
    }
    // Integers again: sums and a maximum, in any order.
    if (approaching)
        atomicAdd(&tally[1], approaching);
    if (max_degree)
        atomicMax(&tally[2], max_degree);
#pragma unroll
    for (int k = 0; k < kApproachPhases; ++k)
        if (phases[k])
            atomicAdd(&tally[3 + k], phases[k]);
    __syncthreads();
    // Place, as batch_contacts_kernel does: the units in ascending order hold the rows in ascending order.
    int first[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        first[q] = contacts_units_below(totals, contacts_unit(q, waves, wave)) + within[q] - row[q].upper;
    const long long pairs = (long long)contacts_units_below(totals, RPL * waves);
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (bodies && r < max_bodies)
            bodies[base + r] = approaches_body(row[q], first[q]);
    }
    if (tid == 0)
        systems[blockIdx.x] = approaches_system(tally[0], tally[1], tally[2], pairs, capacity, tally[3 + kApproachNow],
                                                tally[3 + kApproachPassage], tally[3 + kApproachEnd]);
    if (capacity == 0)
        return;  // the same in every lane; no barrier follows
    // Fill: a row walks the columns above it again and writes its entries from `first` on while they are below the capacity.
    // No row of this wave is below its first lane's row of q = 0, so no column up to that one is above any of them.
    BatchApproach *mine = list + (size_t)blockIdx.x * (size_t)capacity;
    bool fills = false;
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        fills = fills || approaches_row_fills(first[q], row[q].upper, capacity);
    if (NBODY_BATCH_APPROACHES_FILL_ALWAYS || __ballot(fills) != 0) {
        int t[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q)
            t[q] = 0;
        for (int j = wave * kContactsWave + 1; j < n; ++j) {
            const int4 pj = img[2 * j], vj = img[2 * j + 1];
            if (__builtin_amdgcn_readfirstlane(vj.w) == 0)
                continue;
            const ApproachPoint column{__int_as_float(pj.x), __int_as_float(pj.y), __int_as_float(pj.z),
                                       __int_as_float(vj.x), __int_as_float(vj.y), __int_as_float(vj.z)};
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                t2[q] = RADII ? contacts_radii_t2(rad[q], __int_as_float(pj.w)) : b2;
            approaches_column<RPL>(x, t2, column, h, words, phase);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                approaches_fill(mine, capacity, first[q], t[q], contacts_examined(take[q], true, r, j), r, j, words[q], phase[q]);
            }
        }
    }
    // The pads, from `stored` on.
    for (long long k = contacts_stored(pairs, capacity) + tid; k < capacity; k += T)
        mine[k] = approaches_pad();
}

// One launch over all systems.  32 bytes of dynamic LDS per body, 128 KiB at 4096 bodies beside the totals: the figure
// launch_batch_pairs runs at.  Exactly one of radius2 and radii is given; subset and bodies may be NULL; list is NULL iff
// capacity == 0.
hipError_t launch_batch_approaches(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *subset,
                                   const float *radius2, const float *radii, const float *horizon, int n_systems, int max_bodies,
                                   long long capacity, BatchApproachBody *bodies, BatchApproach *list, BatchApproachSystem *systems,
                                   hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = 2 * kBatchBytesPerBody * (size_t)max_bodies;
    return with_rpl(sh.rpl, [&](auto rpl) {
        const auto launch = [&](auto mode) {
            return launch_analysis_kernel(batch_approaches_kernel<rpl(), mode()>, n_systems, sh.threads, lds, stream, pos, vel, counts,
                                          subset, radius2, radii, horizon, max_bodies, capacity, bodies, list, systems);
        };
        return radii ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

// ---- radial profiles (include/nbody_batch_radial.h): per system the bodies in up to 32 shells about a centre and per shell
// the count and 23 fp64 sums, each over the shell's members in ascending body index.  A sibling of the other analysis kernels:
// one workgroup per system with batch_shape's workgroup over the position-plus-velocity image of batch_pairs_kernel.  It reads
// the state and writes only the handle's records.  The arithmetic is nbody_batch_radial_math.h's, which the CPU driver runs too.

static_assert(sizeof(BatchRadialShell) == sizeof(nbody_batch_radial_shell) && sizeof(nbody_batch_radial_shell) == 192 &&
                  offsetof(BatchRadialShell, count) == offsetof(nbody_batch_radial_shell, count) &&
                  offsetof(BatchRadialShell, weight) == offsetof(nbody_batch_radial_shell, weight) &&
                  offsetof(BatchRadialShell, radius) == offsetof(nbody_batch_radial_shell, radius) &&
                  offsetof(BatchRadialShell, vr1) == offsetof(nbody_batch_radial_shell, vr1) &&
                  offsetof(BatchRadialShell, vr2) == offsetof(nbody_batch_radial_shell, vr2) &&
                  offsetof(BatchRadialShell, vt2) == offsetof(nbody_batch_radial_shell, vt2) &&
                  offsetof(BatchRadialShell, L) == offsetof(nbody_batch_radial_shell, L) &&
                  offsetof(BatchRadialShell, U) == offsetof(nbody_batch_radial_shell, U) &&
                  offsetof(BatchRadialShell, M) == offsetof(nbody_batch_radial_shell, M) &&
                  offsetof(BatchRadialShell, V) == offsetof(nbody_batch_radial_shell, V) && offsetof(nbody_batch_radial_shell, L) == 48 &&
                  offsetof(nbody_batch_radial_shell, V) == 144,
              "nbody_batch_radial_math.h mirrors the shell record of nbody_batch_radial.h");
static_assert(sizeof(BatchRadialSystem) == sizeof(nbody_batch_radial_system) && sizeof(nbody_batch_radial_system) == 80 &&
                  offsetof(BatchRadialSystem, selected) == offsetof(nbody_batch_radial_system, selected) &&
                  offsetof(BatchRadialSystem, below) == offsetof(nbody_batch_radial_system, below) &&
                  offsetof(BatchRadialSystem, above) == offsetof(nbody_batch_radial_system, above) &&
                  offsetof(BatchRadialSystem, unmeasured) == offsetof(nbody_batch_radial_system, unmeasured) &&
                  offsetof(BatchRadialSystem, shells) == offsetof(nbody_batch_radial_system, shells) &&
                  offsetof(BatchRadialSystem, projected) == offsetof(nbody_batch_radial_system, projected) &&
                  offsetof(BatchRadialSystem, total_weight) == offsetof(nbody_batch_radial_system, total_weight) &&
                  offsetof(BatchRadialSystem, centre) == offsetof(nbody_batch_radial_system, centre) &&
                  offsetof(BatchRadialSystem, velocity) == offsetof(nbody_batch_radial_system, velocity) &&
                  offsetof(nbody_batch_radial_system, total_weight) == 24 && offsetof(nbody_batch_radial_system, velocity) == 56,
              "nbody_batch_radial_math.h mirrors the system record of nbody_batch_radial.h");
static_assert(sizeof(BatchRadialBody) == sizeof(nbody_batch_radial_body) && sizeof(nbody_batch_radial_body) == 24 &&
                  offsetof(BatchRadialBody, shell) == offsetof(nbody_batch_radial_body, shell) &&
                  offsetof(BatchRadialBody, reserved) == offsetof(nbody_batch_radial_body, reserved) &&
                  offsetof(BatchRadialBody, radius) == offsetof(nbody_batch_radial_body, radius) &&
                  offsetof(BatchRadialBody, radial_velocity) == offsetof(nbody_batch_radial_body, radial_velocity),
              "nbody_batch_radial_math.h mirrors the body record of nbody_batch_radial.h");
static_assert(kRadialMaxShells == NBODY_BATCH_RADIAL_MAX_SHELLS && kRadialBelow == NBODY_BATCH_RADIAL_BELOW &&
                  kRadialUnmeasured == NBODY_BATCH_RADIAL_UNMEASURED && kRadialNotTaking == NBODY_BATCH_RADIAL_NOT_TAKING,
              "nbody_batch_radial_math.h mirrors the limit and the shell words of nbody_batch_radial.h");

// The ascending walk (phase 2), the same bytes either way (the shell records' checksum agrees).  1: one walker per (shell, term
// group), 6 x 32 walkers in three waves, each wave running two groups' code (one wave's lanes go round three times where the
// workgroup is one wave).  0: one walker per shell adding all 23 terms, 32 lanes of one wave.  Measured on an MI355X
// (profiles/batch_rate_radial.txt; Plummer spheres, the call with the shell records alone at 1024 x 1024, 4096 x 256 and
// 256 x 4096, medians of 31, ms): split 2.31, 3.10 and 6.85 at 32 shells and 1.48, 3.19 and 2.00 at 8; whole 2.13, 2.66 and 6.97
// at 32 shells and 1.59, 2.24 and 1.86 at 8.  The whole walk wins where the walk is long (4096 bodies: by 14 % and 30 %) and is
// within the run-to-run scatter of the split elsewhere: every wave of the split forms the words of every body again, and the
// square root and the division once more, and a wave with members in most shells gains no idle lanes from the split.  So:
// whole, which no case lost beyond the scatter.
#ifndef NBODY_BATCH_RADIAL_SPLIT_WALK
#define NBODY_BATCH_RADIAL_SPLIT_WALK 0
#endif

constexpr int kRadialTallies = 4;  // selected, below, above, unmeasured

// The image of a system as the walk reads it: wave-uniform addresses, broadcast LDS reads.
struct RadialImage {
    const int4 *img;
    const signed char *shells;
    __host__ __device__ int shell(int j) const { return shells[j]; }
    __host__ __device__ RadialPoint point(int j) const
    {
        const int4 p = img[2 * j], v = img[2 * j + 1];
        return RadialPoint{__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), __int_as_float(p.w),
                           __int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z)};
    }
};

// LDS: img[2 j] = {x, y, z, m} and img[2 j + 1] = {vx, vy, vz, 0} of body j (128 KiB at 4096 bodies, batch_pairs_kernel's
// image, under the limit raised before the launch), then one byte per body, its shell word (-3 ... 32).  The squared edges and
// the frame of the system are in LDS too: every read of them is a broadcast.  edges2: the squared edges, those of system s at
// s * edges_stride (0: one set for all); frames: centre[3], velocity[3] per system.  subset, bodies and shells_out may be NULL.
// No waves_per_eu: the walker of a whole shell holds 24 fp64 words beside those of the body, which 64 registers do not hold.
template <int RPL, bool SPLIT>
__global__ __launch_bounds__(1024) void batch_radial_kernel(const float4 *__restrict__ pos, const float4 *__restrict__ vel,
                                                            const int *__restrict__ counts, const unsigned char *__restrict__ subset,
                                                            const double *__restrict__ edges2, int edges_stride,
                                                            const double *__restrict__ frames, int max_bodies, int shells, int projected,
                                                            int weight, BatchRadialBody *__restrict__ bodies,
                                                            BatchRadialShell *__restrict__ shells_out, BatchRadialSystem *__restrict__ systems)
{
    extern __shared__ int4 img[];
    __shared__ double e2[kRadialMaxShells + 1];
    __shared__ double frame[kRadialFrameWords];
    __shared__ int tally[kRadialTallies];
    signed char *shell_of = reinterpret_cast<signed char *>(img + 2 * (size_t)max_bodies);
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    if (tid <= shells)  // shells + 1 <= 33 edges, and no workgroup is below 64 lanes
        e2[tid] = edges2[(size_t)blockIdx.x * (size_t)edges_stride + tid];
    if (tid < kRadialFrameWords)
        frame[tid] = frames[(size_t)blockIdx.x * kRadialFrameWords + tid];
    if (tid < kRadialTallies)
        tally[tid] = 0;
    __syncthreads();
    // Phase 1: every row decides its shell on squares and writes its shell byte and its body record.
    int selected = 0, below = 0, above = 0, unmeasured = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        BatchRadialBody record = radial_body_absent();
        if (r < n) {
            const float4 p = pos[base + r], v = vel[base + r];
            img[2 * r] = make_int4(__float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z), __float_as_int(p.w));
            img[2 * r + 1] = make_int4(__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), 0);
            int sh = kRadialNotTaking;
            if (!subset || subset[base + r] != 0) {
                const RadialWords b = radial_words(RadialPoint{p.x, p.y, p.z, p.w, v.x, v.y, v.z}, frame, projected);
                sh = radial_shell(b, e2, shells);
                selected += 1;
                below += sh == kRadialBelow ? 1 : 0;
                above += sh == shells ? 1 : 0;
                unmeasured += sh == kRadialUnmeasured ? 1 : 0;
                if (bodies)
                    record = radial_body(sh, b);
            }
            shell_of[r] = (signed char)sh;
        }
        if (bodies && r < max_bodies)
            bodies[base + r] = record;
    }
    // Integers: the order of the additions does not matter.
    if (selected)
        atomicAdd(&tally[0], selected);
    if (below)
        atomicAdd(&tally[1], below);
    if (above)
        atomicAdd(&tally[2], above);
    if (unmeasured)
        atomicAdd(&tally[3], unmeasured);
    __syncthreads();  // the image, the shell bytes and the tallies are in place
    // Phase 2: the walkers, each through j = 0 ... n - 1.  Walker 0 is lane 0's first, and it alone adds total_weight.
    const RadialImage image{img, shell_of};
    double total = 0.0;
    for (int w = tid; w < radial_walkers(SPLIT); w += T)
        radial_walker(SPLIT, w, image, n, shells, frame, projected, weight,
                      shells_out ? shells_out + (size_t)blockIdx.x * (size_t)shells : nullptr, &total);
    if (tid == 0)
        systems[blockIdx.x] = radial_system(tally[0], tally[1], tally[2], tally[3], shells, projected, total, frame);
}

// One launch over all systems.  32 bytes of dynamic LDS per body for the image and one for the shell byte, rounded up to 16.
hipError_t launch_batch_radial(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *subset, const double *edges2,
                               int edges_stride, const double *frames, int n_systems, int max_bodies, int shells, int projected, int weight,
                               BatchRadialBody *bodies, BatchRadialShell *shells_out, BatchRadialSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = 2 * kBatchBytesPerBody * (size_t)max_bodies + ((size_t)max_bodies + 15) / 16 * 16;
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_radial_kernel<rpl(), NBODY_BATCH_RADIAL_SPLIT_WALK != 0>, n_systems, sh.threads, lds, stream, pos,
                                      vel, counts, subset, edges2, edges_stride, frames, max_bodies, shells, projected, weight, bodies,
                                      shells_out, systems);
    });
}

// ---- surface maps (include/nbody_batch_surface.h): per system the bodies in a grid of up to 64 x 64 cells in a plane of the
// caller's choice and per cell the count and seven fp64 sums, each over the cell's members in ascending body index.  A sibling
// of batch_radial_kernel over the same position-plus-velocity image; where that kernel gives each of at most 32 shells a lane
// that walks every body, this one sorts the bodies by cell first, stably and inside the workgroup, so that the lane of a cell
// walks its own members alone.  It reads the state and writes only the handle's records.  The arithmetic is
// nbody_batch_surface_math.h's, which the CPU driver runs too.

static_assert(sizeof(BatchSurfaceCell) == sizeof(nbody_batch_surface_cell) && sizeof(nbody_batch_surface_cell) == 64 &&
                  offsetof(BatchSurfaceCell, count) == offsetof(nbody_batch_surface_cell, count) &&
                  offsetof(BatchSurfaceCell, weight) == offsetof(nbody_batch_surface_cell, weight) &&
                  offsetof(BatchSurfaceCell, v1) == offsetof(nbody_batch_surface_cell, v1) &&
                  offsetof(BatchSurfaceCell, v2) == offsetof(nbody_batch_surface_cell, v2) &&
                  offsetof(BatchSurfaceCell, pa) == offsetof(nbody_batch_surface_cell, pa) &&
                  offsetof(BatchSurfaceCell, pb) == offsetof(nbody_batch_surface_cell, pb) &&
                  offsetof(BatchSurfaceCell, z1) == offsetof(nbody_batch_surface_cell, z1) &&
                  offsetof(BatchSurfaceCell, z2) == offsetof(nbody_batch_surface_cell, z2) && offsetof(nbody_batch_surface_cell, z2) == 56,
              "nbody_batch_surface_math.h mirrors the cell record of nbody_batch_surface.h");
static_assert(sizeof(BatchSurfaceSystem) == sizeof(nbody_batch_surface_system) && sizeof(nbody_batch_surface_system) == 88 &&
                  offsetof(BatchSurfaceSystem, selected) == offsetof(nbody_batch_surface_system, selected) &&
                  offsetof(BatchSurfaceSystem, outside) == offsetof(nbody_batch_surface_system, outside) &&
                  offsetof(BatchSurfaceSystem, unmeasured) == offsetof(nbody_batch_surface_system, unmeasured) &&
                  offsetof(BatchSurfaceSystem, columns) == offsetof(nbody_batch_surface_system, columns) &&
                  offsetof(BatchSurfaceSystem, rows) == offsetof(nbody_batch_surface_system, rows) &&
                  offsetof(BatchSurfaceSystem, occupied) == offsetof(nbody_batch_surface_system, occupied) &&
                  offsetof(BatchSurfaceSystem, peak) == offsetof(nbody_batch_surface_system, peak) &&
                  offsetof(BatchSurfaceSystem, peak_count) == offsetof(nbody_batch_surface_system, peak_count) &&
                  offsetof(BatchSurfaceSystem, total_weight) == offsetof(nbody_batch_surface_system, total_weight) &&
                  offsetof(BatchSurfaceSystem, centre) == offsetof(nbody_batch_surface_system, centre) &&
                  offsetof(BatchSurfaceSystem, velocity) == offsetof(nbody_batch_surface_system, velocity) &&
                  offsetof(nbody_batch_surface_system, total_weight) == 32 && offsetof(nbody_batch_surface_system, velocity) == 64,
              "nbody_batch_surface_math.h mirrors the system record of nbody_batch_surface.h");
static_assert(sizeof(BatchSurfaceBody) == sizeof(nbody_batch_surface_body) && sizeof(nbody_batch_surface_body) == 24 &&
                  offsetof(BatchSurfaceBody, cell) == offsetof(nbody_batch_surface_body, cell) &&
                  offsetof(BatchSurfaceBody, reserved) == offsetof(nbody_batch_surface_body, reserved) &&
                  offsetof(BatchSurfaceBody, a) == offsetof(nbody_batch_surface_body, a) &&
                  offsetof(BatchSurfaceBody, b) == offsetof(nbody_batch_surface_body, b),
              "nbody_batch_surface_math.h mirrors the body record of nbody_batch_surface.h");
static_assert(kSurfaceMaxSide == NBODY_BATCH_SURFACE_MAX_SIDE && kSurfaceOutside == NBODY_BATCH_SURFACE_OUTSIDE &&
                  kSurfaceUnmeasured == NBODY_BATCH_SURFACE_UNMEASURED && kSurfaceNotTaking == NBODY_BATCH_SURFACE_NOT_TAKING &&
                  NBODY_BATCH_MAX_BODIES <= 4096,
              "nbody_batch_surface_math.h mirrors the limit and the cell words of nbody_batch_surface.h; surface_key holds a body index in 12 bits");

constexpr int kSurfaceTallies = 5;  // selected, outside, unmeasured; then occupied and the peak key

// The image of a system as the walks read it.
struct SurfaceImage {
    const int4 *img;
    const unsigned short *words, *places, *starts;
    __host__ __device__ int word(int j) const { return words[j]; }
    __host__ __device__ int order(int k) const { return places[k]; }
    __host__ __device__ int start(int c) const { return starts[c]; }
    __host__ __device__ SurfacePoint point(int j) const
    {
        const int4 p = img[2 * j], v = img[2 * j + 1];
        return SurfacePoint{__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), __int_as_float(p.w),
                            __int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z)};
    }
};

// The words of max_bodies rounded up to the eight that one 16-byte LDS read holds.
__host__ __device__ inline int surface_padded(int max_bodies) { return (max_bodies + 7) / 8 * 8; }

// LDS: batch_radial_kernel's image, img[2 j] = {x, y, z, m} and img[2 j + 1] = {vx, vy, vz, 0} (128 KiB at 4096 bodies), then
// three arrays of 16-bit words: the cell word of every body (surface_word: the cell, or a sentinel above 4095), order[] (the
// members sorted by (cell, index)) and the start of every cell in order[].  The edges of both axes, the frame and the view are
// in static LDS.
//   Phase 1, decide: every row forms its six words, decides its cell and writes its cell word and its body record.  Two
//     neighbouring lanes write the two halves of one dword; the stores are ds_write_b16, which leave the other half alone.
//   Phase 2, sort: the rank walk.  Row i's place is the number of bodies whose (word, index) is below its own (surface_key).
//     The cell words are read eight at a time at a wave-uniform address -- one ds_read_b128 broadcast per eight columns, no
//     bank conflict whatever the 16-bit packing -- and each costs every row a compare and an add.  No atomics, no scan, no
//     ordering between waves.  The starts of the cells fall out of order[] where the cell word changes.
//   Phase 3, walk: one lane per cell, striding over columns x rows, adds its members' seven terms through order[] from its
//     start; these reads are gathers (the lanes of a wave are at different places).  occupied and peak are integer
//     reductions through LDS atomics.  Lane 0 also walks j = 0 ... n - 1 for total_weight.
// Only this sort is built: the alternative of a histogram, a scan and a placement by ballots was not, so nothing compares them.
// No waves_per_eu, as for batch_radial_kernel: the rows' keys and ranks and the walker's eight fp64 words are held at once.
template <int RPL>
__global__ __launch_bounds__(1024) void batch_surface_kernel(const float4 *__restrict__ pos, const float4 *__restrict__ vel,
                                                             const int *__restrict__ counts, const unsigned char *__restrict__ subset,
                                                             const double *__restrict__ edges_a, int stride_a,
                                                             const double *__restrict__ edges_b, int stride_b,
                                                             const double *__restrict__ frames, int max_bodies, int columns, int rows,
                                                             int weight, BatchSurfaceBody *__restrict__ bodies,
                                                             BatchSurfaceCell *__restrict__ cells_out, BatchSurfaceSystem *__restrict__ systems)
{
    extern __shared__ int4 img[];
    __shared__ double ea[kSurfaceMaxSide + 1], eb[kSurfaceMaxSide + 1];
    __shared__ double frame[kSurfaceFrameWords];
    __shared__ unsigned tally[kSurfaceTallies];
    const int padded = surface_padded(max_bodies), cells = columns * rows;
    unsigned short *cell_of = reinterpret_cast<unsigned short *>(img + 2 * (size_t)max_bodies);
    unsigned short *order = cell_of + padded;
    unsigned short *starts = order + padded;
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    for (int t = tid; t <= columns; t += T)
        ea[t] = edges_a[(size_t)blockIdx.x * (size_t)stride_a + t];
    for (int t = tid; t <= rows; t += T)
        eb[t] = edges_b[(size_t)blockIdx.x * (size_t)stride_b + t];
    if (tid < kSurfaceFrameWords)
        frame[tid] = frames[(size_t)blockIdx.x * kSurfaceFrameWords + tid];
    if (tid < kSurfaceTallies)
        tally[tid] = 0;
    for (int c = tid; c < cells; c += T)
        starts[c] = (unsigned short)kSurfaceNoStart;
    __syncthreads();
    // Phase 1: every row decides its cell and writes its cell word and its body record.
    unsigned key[RPL];
    int selected = 0, outside = 0, unmeasured = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        BatchSurfaceBody record = surface_body_absent();
        int word = kSurfaceWordNotTaking;
        if (r < n) {
            const float4 p = pos[base + r], v = vel[base + r];
            img[2 * r] = make_int4(__float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z), __float_as_int(p.w));
            img[2 * r + 1] = make_int4(__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), 0);
            if (!subset || subset[base + r] != 0) {
                const SurfaceWords b = surface_words(SurfacePoint{p.x, p.y, p.z, p.w, v.x, v.y, v.z}, frame);
                const int cell = surface_cell(b, ea, columns, eb, rows);
                word = surface_word(cell);
                selected += 1;
                outside += cell == kSurfaceOutside ? 1 : 0;
                unmeasured += cell == kSurfaceUnmeasured ? 1 : 0;
                if (bodies)
                    record = surface_body(cell, b);
            }
        }
        if (r < padded)
            cell_of[r] = (unsigned short)word;  // the words from n on are sentinels: the rank walk reads them in eights
        key[q] = surface_key(word, r);
        if (bodies && r < max_bodies)
            bodies[base + r] = record;
    }
    // Integers: the order of the additions does not matter.
    if (selected)
        atomicAdd(&tally[0], (unsigned)selected);
    if (outside)
        atomicAdd(&tally[1], (unsigned)outside);
    if (unmeasured)
        atomicAdd(&tally[2], (unsigned)unmeasured);
    __syncthreads();  // the image, the cell words and the tallies are in place
    const int m = (int)(tally[0] - tally[1] - tally[2]);  // the members of all cells: the places of order[]
    // Phase 2: the rank walk, eight columns per broadcast read.
    int rank[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q)
        rank[q] = 0;
    const uint4 *eights = reinterpret_cast<const uint4 *>(cell_of);
    for (int g = 0; g < (n + 7) / 8; ++g) {
        const uint4 w = eights[g];
        const unsigned two[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int j = 8 * g + 2 * h, lo = (int)(two[h] & 0xFFFFu), hi = (int)(two[h] >> 16);
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                rank[q] += surface_rank_step(key[q], lo, j) + surface_rank_step(key[q], hi, j + 1);
        }
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n && surface_word_inside((int)(key[q] >> 12)) && rank[q] < m)
            order[rank[q]] = (unsigned short)r;
    }
    __syncthreads();  // order[] is in place
    for (int k = tid; k < m; k += T) {
        const int here = cell_of[order[k]], before = k > 0 ? cell_of[order[k - 1]] : here;
        if (surface_is_start(k, here, before) && here < cells)
            starts[here] = (unsigned short)k;
    }
    __syncthreads();  // the starts are in place
    // Phase 3: the walkers, one per cell; lane 0 also adds total_weight.
    const SurfaceImage image{img, cell_of, order, starts};
    int occupied = 0;
    unsigned peak = 0;
    for (int c = tid; c < cells; c += T) {
        const BatchSurfaceCell cell = surface_walk(image, m, c, frame, weight, cells_out != nullptr);
        if (cells_out)
            cells_out[(size_t)blockIdx.x * (size_t)cells + c] = cell;
        occupied += cell.count > 0 ? 1 : 0;
        const unsigned mine = surface_peak_key(cell.count, c);
        peak = mine > peak ? mine : peak;
    }
    if (occupied) {
        atomicAdd(&tally[3], (unsigned)occupied);
        atomicMax(&tally[4], peak);
    }
    double total = 0.0;
    if (tid == 0)
        total = surface_walk_total(image, n, weight);
    __syncthreads();  // occupied and the peak are in place
    if (tid == 0)
        systems[blockIdx.x] = surface_system((int)tally[0], (int)tally[1], (int)tally[2], columns, rows, (int)tally[3], tally[4], total, frame);
}

// The dynamic LDS of one workgroup: 32 bytes per body for the image and three arrays of 16-bit words, the cell words and
// order[] over the padded capacity and the starts over the cells, each a multiple of 16 bytes.  At 4096 bodies and 64 x 64
// cells 131072 + 8192 + 8192 + 8192 = 155648 bytes; with the 1216 bytes of static LDS (two sets of 65 edges, 15 words of frame
// and view, the tallies; the compiler's figure, padding included) 156864 bytes, 153.2 KiB of the 160 KiB of a gfx950 workgroup.
inline size_t surface_lds_bytes(int max_bodies, int cells)
{
    return 2 * kBatchBytesPerBody * (size_t)max_bodies + 2 * sizeof(unsigned short) * (size_t)surface_padded(max_bodies) +
           (sizeof(unsigned short) * (size_t)cells + 15) / 16 * 16;
}

// One launch over all systems.
hipError_t launch_batch_surface(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *subset, const double *edges_a,
                                int stride_a, const double *edges_b, int stride_b, const double *frames, int n_systems, int max_bodies,
                                int columns, int rows, int weight, BatchSurfaceBody *bodies, BatchSurfaceCell *cells_out,
                                BatchSurfaceSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = surface_lds_bytes(max_bodies, columns * rows);
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_surface_kernel<rpl()>, n_systems, sh.threads, lds, stream, pos, vel, counts, subset, edges_a,
                                      stride_a, edges_b, stride_b, frames, max_bodies, columns, rows, weight, bodies, cells_out, systems);
    });
}

// ---- shapes (include/nbody_batch_shape.h): per system and each of up to 8 apertures the ellipsoid that the iterated moment
// tensor converges to, and what lies inside it.  A sibling of batch_radial_kernel over the same position-plus-velocity image.
// It reads the state and writes only the handle's records.  The arithmetic is nbody_batch_shape_math.h's, which the CPU driver
// runs too.

static_assert(sizeof(BatchShapeAperture) == sizeof(nbody_batch_shape_aperture) && sizeof(nbody_batch_shape_aperture) == 256 &&
                  offsetof(BatchShapeAperture, status) == offsetof(nbody_batch_shape_aperture, status) &&
                  offsetof(BatchShapeAperture, iterations) == offsetof(nbody_batch_shape_aperture, iterations) &&
                  offsetof(BatchShapeAperture, count) == offsetof(nbody_batch_shape_aperture, count) &&
                  offsetof(BatchShapeAperture, radius) == offsetof(nbody_batch_shape_aperture, radius) &&
                  offsetof(BatchShapeAperture, inner) == offsetof(nbody_batch_shape_aperture, inner) &&
                  offsetof(BatchShapeAperture, q) == offsetof(nbody_batch_shape_aperture, q) &&
                  offsetof(BatchShapeAperture, s) == offsetof(nbody_batch_shape_aperture, s) &&
                  offsetof(BatchShapeAperture, change) == offsetof(nbody_batch_shape_aperture, change) &&
                  offsetof(BatchShapeAperture, eigenvalues) == offsetof(nbody_batch_shape_aperture, eigenvalues) &&
                  offsetof(BatchShapeAperture, axes) == offsetof(nbody_batch_shape_aperture, axes) &&
                  offsetof(BatchShapeAperture, weight) == offsetof(nbody_batch_shape_aperture, weight) &&
                  offsetof(BatchShapeAperture, D) == offsetof(nbody_batch_shape_aperture, D) &&
                  offsetof(BatchShapeAperture, M) == offsetof(nbody_batch_shape_aperture, M) &&
                  offsetof(BatchShapeAperture, L) == offsetof(nbody_batch_shape_aperture, L) && offsetof(nbody_batch_shape_aperture, axes) == 80 &&
                  offsetof(nbody_batch_shape_aperture, L) == 232,
              "nbody_batch_shape_math.h mirrors the aperture record of nbody_batch_shape.h");
static_assert(sizeof(BatchShapeSystem) == sizeof(nbody_batch_shape_system) && sizeof(nbody_batch_shape_system) == 80 &&
                  offsetof(BatchShapeSystem, selected) == offsetof(nbody_batch_shape_system, selected) &&
                  offsetof(BatchShapeSystem, unmeasured) == offsetof(nbody_batch_shape_system, unmeasured) &&
                  offsetof(BatchShapeSystem, apertures) == offsetof(nbody_batch_shape_system, apertures) &&
                  offsetof(BatchShapeSystem, reduced) == offsetof(nbody_batch_shape_system, reduced) &&
                  offsetof(BatchShapeSystem, converged) == offsetof(nbody_batch_shape_system, converged) &&
                  offsetof(BatchShapeSystem, reserved) == offsetof(nbody_batch_shape_system, reserved) &&
                  offsetof(BatchShapeSystem, total_weight) == offsetof(nbody_batch_shape_system, total_weight) &&
                  offsetof(BatchShapeSystem, centre) == offsetof(nbody_batch_shape_system, centre) &&
                  offsetof(BatchShapeSystem, velocity) == offsetof(nbody_batch_shape_system, velocity) &&
                  offsetof(nbody_batch_shape_system, total_weight) == 24 && offsetof(nbody_batch_shape_system, velocity) == 56,
              "nbody_batch_shape_math.h mirrors the system record of nbody_batch_shape.h");
static_assert(sizeof(BatchShapeBody) == sizeof(nbody_batch_shape_body) && sizeof(nbody_batch_shape_body) == 8 &&
                  offsetof(BatchShapeBody, inside) == offsetof(nbody_batch_shape_body, inside) &&
                  offsetof(BatchShapeBody, reserved) == offsetof(nbody_batch_shape_body, reserved),
              "nbody_batch_shape_math.h mirrors the body record of nbody_batch_shape.h");
static_assert(kShapeMaxApertures == NBODY_BATCH_SHAPE_MAX_APERTURES && kShapeMaxIterations == NBODY_BATCH_SHAPE_MAX_ITERATIONS &&
                  kShapeConverged == NBODY_BATCH_SHAPE_CONVERGED && kShapeMax == NBODY_BATCH_SHAPE_MAX && kShapeFew == NBODY_BATCH_SHAPE_FEW &&
                  kShapeDegenerate == NBODY_BATCH_SHAPE_DEGENERATE && kShapeBlock == 64,
              "nbody_batch_shape_math.h mirrors the limits and the status words of nbody_batch_shape.h; a block is a wave's width");

constexpr int kShapeTallies = 3;  // selected, unmeasured, converged

// The image of a system as a lane reads it: lane k at body 64 k + j, which shape_image_slot spreads over the banks.
struct ShapeImage {
    const int4 *img;
    __device__ ShapePoint point(int i) const
    {
        const int at = shape_image_slot(i);
        const int4 p = img[at], v = img[at + 1];
        return ShapePoint{__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), __int_as_float(p.w),
                          __int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z)};
    }
};

// The partial that lane k of the wave holds, in every lane.
template <int N>
__device__ inline ShapePartial<N> shape_partial_of_lane(const ShapePartial<N> &mine, int k)
{
    ShapePartial<N> p;
#pragma unroll
    for (int c = 0; c < N; ++c)
        p.v[c] = __shfl(mine.v[c], k, 64);
    p.count = __shfl(mine.count, k, 64);
    return p;
}

// A word that every lane of the wave holds alike, told to the compiler: it then lives in scalar registers, which the walk's
// fp64 operations read as they read vector ones.  The state, the frame and the aperture are such words, 19 doubles that would
// otherwise cost every lane 38 registers beside its sums.
__device__ inline double shape_uniform(double v)
{
    const long long bits = __double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)bits), hi = __builtin_amdgcn_readfirstlane((unsigned)(bits >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ inline void shape_uniform(ShapeState &st)
{
#pragma unroll
    for (int c = 0; c < 9; ++c)
        st.e[c] = shape_uniform(st.e[c]);
    st.w2 = shape_uniform(st.w2);
    st.w3 = shape_uniform(st.w3);
}

// One wave per aperture: the waves of the workgroup take the apertures in turn, wave w the apertures w, w + waves, ...  In
// every pass lane k walks block k (bodies 64 k ... 64 k + 63) through LDS: the level-1 partial.  Then every lane of the wave
// adds the partials of lanes 0 ... blocks - 1 in that order, read by shuffles -- the level-2 sum -- and runs the Jacobi
// iteration and the update on what are the same words in all 64 lanes: the new state is in registers everywhere and nothing
// is published through LDS, and the loop's exit is the same in every lane.  The other mapping, all waves of the workgroup
// splitting the blocks of one aperture, was not built: nothing compares them.
// LDS: the image at 32 B per body, img[slot] = {x, y, z, m} and img[slot + 1] = {vx, vy, vz, 0} with slot = 2 i + i / 64
// (shape_image_slot: 2 KiB apart the 64 lanes' reads would all fall on one 16-byte bank group; half a body per block puts 16
// consecutive lanes on 16 groups), x = NaN for a body that is a member of nothing, then one membership byte per body at
// i + 4 (i / 64), one bit per aperture.  At 4096 bodies: 16 * (2 * 4096 + 64) + 4352 = 136448 bytes dynamic and 320 bytes
// static (the apertures, the frame and three tallies, as the compiler reports them), 136768 bytes in all, under the limit
// launch_analysis_kernel raises.  The compiler reports 132 VGPRs, 106 SGPRs and no scratch for each of the three
// instantiations; the workgroup is kept at eight waves (shape_threads) because at sixteen, with 128 registers, it spilled.
// aps: radius, inner, out2, in2 per aperture, those of system s at s * aps_stride (0: one set for all); frames: centre[3],
// velocity[3] per system.  subset, bodies and apertures_out may be NULL.
template <int RPL>
__global__ __launch_bounds__(kShapeMaxThreads) void batch_shape_kernel(const float4 *__restrict__ pos, const float4 *__restrict__ vel,
                                                           const int *__restrict__ counts, const unsigned char *__restrict__ subset,
                                                           const double *__restrict__ aps, int aps_stride, const double *__restrict__ frames,
                                                           int max_bodies, int apertures, int weight, int reduced, double tol,
                                                           int max_iterations, int min_members, BatchShapeBody *__restrict__ bodies,
                                                           BatchShapeAperture *__restrict__ apertures_out,
                                                           BatchShapeSystem *__restrict__ systems)
{
    extern __shared__ int4 img[];
    __shared__ double ap[kShapeMaxApertures * kShapeApertureWords];
    __shared__ double frame[kShapeFrameWords];
    __shared__ int tally[kShapeTallies];
    unsigned *inside = reinterpret_cast<unsigned *>(img + shape_image_slots(max_bodies));
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    if (tid < apertures * kShapeApertureWords)  // at most 32 words, and no workgroup is below 64 lanes
        ap[tid] = aps[(size_t)blockIdx.x * (size_t)aps_stride + tid];
    if (tid < kShapeFrameWords)
        frame[tid] = frames[(size_t)blockIdx.x * kShapeFrameWords + tid];
    if (tid < kShapeTallies)
        tally[tid] = 0;
    for (int w = tid; w < shape_inside_bytes(max_bodies) / 4; w += T)
        inside[w] = 0u;
    // Phase 1: every row decides whether it can be a member of anything and writes its words to the image.
    int selected = 0, unmeasured = 0;
    const int rows = shape_rows(RPL, T, max_bodies);  // RPL, or 2 RPL where the workgroup was kept at eight waves
    for (int q0 = 0; q0 < rows; q0 += RPL)
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = (q0 + q) * T + tid;
        if (r < n) {
            const float4 p = pos[base + r], v = vel[base + r];
            const ShapePoint given{p.x, p.y, p.z, p.w, v.x, v.y, v.z};
            const bool takes = !subset || subset[base + r] != 0, measured = shape_measured(given);
            selected += takes ? 1 : 0;
            unmeasured += takes && !measured ? 1 : 0;
            const ShapePoint held = shape_image_point(given, takes && measured);
            const int at = shape_image_slot(r);
            img[at] = make_int4(__float_as_int(held.x), __float_as_int(held.y), __float_as_int(held.z), __float_as_int(held.m));
            img[at + 1] = make_int4(__float_as_int(held.vx), __float_as_int(held.vy), __float_as_int(held.vz), 0);
        }
    }
    __syncthreads();  // the tallies are zeroed
    // Integers: the order of the additions does not matter.
    if (selected)
        atomicAdd(&tally[0], selected);
    if (unmeasured)
        atomicAdd(&tally[1], unmeasured);
    __syncthreads();  // the image, the zeroed membership bytes, the apertures, the frame and the tallies are in place
    const ShapeImage image{img};
    const int lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const int blocks = shape_blocks(n), first = lane * kShapeBlock, last = shape_block_end(lane, n);
    double total_weight = 0.0;
    if (wave == 0) {
        ShapePartial<1> part{};
        for (int i = first; i < last; ++i)
            shape_total_step(part, image.point(i), weight);
        total_weight = shape_level2<1>([&](int k) { return shape_partial_of_lane(part, k); }, blocks).v[0];
    }
    double centred[kShapeFrameWords];
#pragma unroll
    for (int c = 0; c < kShapeFrameWords; ++c)
        centred[c] = shape_uniform(frame[c]);
    for (int a = wave; a < apertures; a += waves) {
        const double radius = ap[kShapeApertureWords * a], inner = ap[kShapeApertureWords * a + 1];
        const double out2 = shape_uniform(ap[kShapeApertureWords * a + 2]), in2 = shape_uniform(ap[kShapeApertureWords * a + 3]);
        ShapeProgress g = shape_start();
        // Every lane holds the same g: the loop is left by the whole wave at once, at most after max_iterations <= 64 passes.
        for (int pass = 0; pass < kShapeMaxIterations && !g.done; ++pass) {
            ShapePartial<kShapePassWords> part{};
            for (int i = first; i < last; ++i)
                shape_pass_step(part, image.point(i), centred, g.state, in2, out2, weight, reduced != 0);
            const ShapePartial<kShapePassWords> sum =
                shape_level2<kShapePassWords>([&](int k) { return shape_partial_of_lane(part, k); }, blocks);
            shape_update(g, sum, tol, max_iterations, min_members);
            shape_uniform(g.state);
        }
        ShapePartial<kShapeFinalWords> part{};
        for (int i = first; i < last; ++i)
            if (shape_final_step(part, image.point(i), centred, g.state, in2, out2, weight)) {
                const int at = shape_inside_at(i);
                atomicOr(&inside[at >> 2], 1u << (8 * (at & 3) + a));
            }
        const ShapePartial<kShapeFinalWords> sum =
            shape_level2<kShapeFinalWords>([&](int k) { return shape_partial_of_lane(part, k); }, blocks);
        if (lane == 0) {
            if (apertures_out)
                apertures_out[(size_t)blockIdx.x * (size_t)apertures + a] = shape_record(g, radius, inner, sum);
            if (g.status == kShapeConverged)
                atomicAdd(&tally[2], 1);
        }
    }
    __syncthreads();  // every aperture's membership bits and the count of the converged are in
    if (bodies) {
        for (int q = 0; q < rows; ++q) {
            const int r = q * T + tid;
            if (r < max_bodies) {
                const int at = shape_inside_at(r);
                bodies[base + r] = shape_body(r < n ? (inside[at >> 2] >> (8 * (at & 3))) & 0xFFu : 0u);
            }
        }
    }
    if (tid == 0)
        systems[blockIdx.x] = shape_system(tally[0], tally[1], apertures, reduced != 0 ? 1 : 0, tally[2], total_weight, frame);
}

// The dynamic LDS of one launch: the shifted image and the membership bytes.
inline size_t shape_lds_bytes(int max_bodies)
{
    return sizeof(int4) * (size_t)shape_image_slots(max_bodies) + (size_t)shape_inside_bytes(max_bodies);
}

// One launch over all systems.
hipError_t launch_batch_shape(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *subset, const double *aps,
                              int aps_stride, const double *frames, int n_systems, int max_bodies, int apertures, int weight, int reduced,
                              double tol, int max_iterations, int min_members, BatchShapeBody *bodies, BatchShapeAperture *apertures_out,
                              BatchShapeSystem *systems, hipStream_t stream)
{
    const BatchShape sh = batch_shape(max_bodies);
    const size_t lds = shape_lds_bytes(max_bodies);
    return with_rpl(sh.rpl, [&](auto rpl) {
        return launch_analysis_kernel(batch_shape_kernel<rpl()>, n_systems, shape_threads(sh.threads), lds, stream, pos, vel, counts, subset, aps, aps_stride,
                                      frames, max_bodies, apertures, weight, reduced, tol, max_iterations, min_members, bodies, apertures_out,
                                      systems);
    });
}

// ---- pair velocities (include/nbody_batch_pair_velocities.h): per system and bin of separation the fp64 sums over the ordered
// pairs (row, source) of the bin, in the header's pinned order.  A sibling of batch_correlation_kernel, whose bin decision it
// runs: one workgroup per system with batch_shape's workgroup, the columns broadcast from LDS, rows at r = q * T + lane, so
// that a block of 64 rows is one wave at one q and its tree is six shuffles per term.  It reads the state and writes only the
// handle's records.

static_assert(sizeof(BatchPairVelocitiesBin) == sizeof(nbody_batch_pair_velocities_bin) && sizeof(nbody_batch_pair_velocities_bin) == 96 &&
                  offsetof(BatchPairVelocitiesBin, count) == offsetof(nbody_batch_pair_velocities_bin, count) &&
                  offsetof(BatchPairVelocitiesBin, approaching) == offsetof(nbody_batch_pair_velocities_bin, approaching) &&
                  offsetof(BatchPairVelocitiesBin, receding) == offsetof(nbody_batch_pair_velocities_bin, receding) &&
                  offsetof(BatchPairVelocitiesBin, weight) == offsetof(nbody_batch_pair_velocities_bin, weight) &&
                  offsetof(BatchPairVelocitiesBin, r1) == offsetof(nbody_batch_pair_velocities_bin, r1) &&
                  offsetof(BatchPairVelocitiesBin, r2) == offsetof(nbody_batch_pair_velocities_bin, r2) &&
                  offsetof(BatchPairVelocitiesBin, rv) == offsetof(nbody_batch_pair_velocities_bin, rv) &&
                  offsetof(BatchPairVelocitiesBin, vr1) == offsetof(nbody_batch_pair_velocities_bin, vr1) &&
                  offsetof(BatchPairVelocitiesBin, vr2) == offsetof(nbody_batch_pair_velocities_bin, vr2) &&
                  offsetof(BatchPairVelocitiesBin, vt2) == offsetof(nbody_batch_pair_velocities_bin, vt2) &&
                  offsetof(BatchPairVelocitiesBin, v1) == offsetof(nbody_batch_pair_velocities_bin, v1) &&
                  offsetof(BatchPairVelocitiesBin, v2) == offsetof(nbody_batch_pair_velocities_bin, v2) &&
                  offsetof(nbody_batch_pair_velocities_bin, weight) == 24 && offsetof(nbody_batch_pair_velocities_bin, v2) == 88,
              "nbody_batch_pair_velocities_math.h mirrors the bin record of nbody_batch_pair_velocities.h");
static_assert(sizeof(BatchPairVelocitiesSystem) == sizeof(nbody_batch_pair_velocities_system) && sizeof(nbody_batch_pair_velocities_system) == 56 &&
                  offsetof(BatchPairVelocitiesSystem, rows) == offsetof(nbody_batch_pair_velocities_system, rows) &&
                  offsetof(BatchPairVelocitiesSystem, sources) == offsetof(nbody_batch_pair_velocities_system, sources) &&
                  offsetof(BatchPairVelocitiesSystem, both) == offsetof(nbody_batch_pair_velocities_system, both) &&
                  offsetof(BatchPairVelocitiesSystem, bins) == offsetof(nbody_batch_pair_velocities_system, bins) &&
                  offsetof(BatchPairVelocitiesSystem, weight) == offsetof(nbody_batch_pair_velocities_system, weight) &&
                  offsetof(BatchPairVelocitiesSystem, reserved) == offsetof(nbody_batch_pair_velocities_system, reserved) &&
                  offsetof(BatchPairVelocitiesSystem, pairs) == offsetof(nbody_batch_pair_velocities_system, pairs) &&
                  offsetof(BatchPairVelocitiesSystem, below) == offsetof(nbody_batch_pair_velocities_system, below) &&
                  offsetof(BatchPairVelocitiesSystem, above) == offsetof(nbody_batch_pair_velocities_system, above) &&
                  offsetof(BatchPairVelocitiesSystem, unmeasured) == offsetof(nbody_batch_pair_velocities_system, unmeasured) &&
                  offsetof(nbody_batch_pair_velocities_system, pairs) == 24 && offsetof(nbody_batch_pair_velocities_system, unmeasured) == 48,
              "nbody_batch_pair_velocities_math.h mirrors the system record of nbody_batch_pair_velocities.h");
static_assert(kPairVelocitiesMaxBins == NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS, "nbody_batch_pair_velocities_math.h mirrors the limit of nbody_batch_pair_velocities.h");

// 1: a column none of whose 64 pairs falls into a bin of the pass is left on the scalar unit before any fp64 word is formed.
// 0: every column reaches the masked add.  The same bytes either way.
#ifndef NBODY_BATCH_PAIR_VELOCITIES_SKIP
#define NBODY_BATCH_PAIR_VELOCITIES_SKIP 1
#endif

constexpr int kPairVelocitiesTallies = 3;  // rows, sources, both

// The wave's sum of its lanes' integers, in lane 0: integers, any order.
__device__ inline unsigned int pair_velocities_wave_total(unsigned int word)
{
    for (int off = 32; off > 0; off >>= 1)
        word += __shfl_down(word, off, 64);
    return word;
}

__device__ inline PairVelocityPoint pair_velocities_point(const int4 &p, const int4 &v)
{
    return PairVelocityPoint{__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), __int_as_float(v.w),
                             __int_as_float(v.x), __int_as_float(v.y), __int_as_float(v.z)};
}

// The workgroup: batch_shape's, held to NBODY_BATCH_PAIR_VELOCITIES_MAX_THREADS lanes.  At 256 -- four waves, one per SIMD -- a
// lane may use all 512 registers and holds the sums of G = 8 bins; its rows follow one another, so fewer lanes cost no pass.
// At batch_shape's own 1024 lanes a lane has 128 registers, which hold G = 2 (DESIGN.md 3.6 has both measured).
#ifndef NBODY_BATCH_PAIR_VELOCITIES_MAX_THREADS
#define NBODY_BATCH_PAIR_VELOCITIES_MAX_THREADS 256
#endif
constexpr int kPairVelocitiesMaxThreads = NBODY_BATCH_PAIR_VELOCITIES_MAX_THREADS;
inline int pair_velocities_threads(int threads) { return threads < kPairVelocitiesMaxThreads ? threads : kPairVelocitiesMaxThreads; }

// LDS: img[2 j] = {x, y, z, flags} and img[2 j + 1] = {vx, vy, vz, mass word} of body j, batch_approaches_kernel's image with
// the flags (source, row, measurable velocity) in the free word, two broadcast ds_read_b128 per column, 128 KiB at 4096 bodies;
// behind it the partials of one round, G x 9 doubles per wave (2.25 KiB at four waves and G = 8).  A lane holds the sums of one
// row at a time -- G x 9 doubles.  A round is the T rows from q0 on: wave w walks block q0 / 64 + w, lane l its row
// r = q0 + 64 w + l over all columns; six shuffles per sum make the block's partial; the partials of the round go through LDS
// and the lane of each sum adds them to its total in ascending block order; then the next round.  Every pass walks all rounds
// again.  The order of the header is that of body indices, so neither G nor the workgroup's shape nor the number of rounds
// shows in a record.  The fp32 r2 chain and the bin decision come first; the fp64 terms are formed under the mask of the lanes
// whose pair is a member of one of the pass's bins.
// edges2 holds pair_velocities_padded_edges(bins, G) squared edges per system (edge_stride that many) or one set for all
// (edge_stride = 0).  rows, sources and bins_out may be NULL.
// The compiler's figures for the instantiation built are in DESIGN.md 3.6: no scratch.
template <int G>
__global__ __launch_bounds__(kPairVelocitiesMaxThreads) void batch_pair_velocities_kernel(
    const float4 *__restrict__ pos, const float4 *__restrict__ vel, const int *__restrict__ counts, const unsigned char *__restrict__ rows,
    const unsigned char *__restrict__ sources, const float *__restrict__ edges2, int edge_stride, int max_bodies, int bins, int weight,
    BatchPairVelocitiesBin *__restrict__ bins_out, BatchPairVelocitiesSystem *__restrict__ systems)
{
    constexpr int SUMS = G * kPairVelocitiesTerms;                                          // the sums of one pass
    constexpr int SLOTS = (SUMS + kPairVelocitiesBlock - 1) / kPairVelocitiesBlock;        // of them per lane, in the smallest workgroup
    extern __shared__ int4 img[];
    __shared__ unsigned int totals[3 * G + 3];  // count, approaching, receding of the pass's bins; the system's three counters
    __shared__ int tally[kPairVelocitiesTallies];
    double *partials = reinterpret_cast<double *>(img + 2 * (size_t)max_bodies);  // [wave][G][9]
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kPairVelocitiesBlock - 1), wave = tid / kPairVelocitiesBlock;
    const int waves = T / kPairVelocitiesBlock;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const float *mine2 = edges2 + (size_t)blockIdx.x * (size_t)edge_stride;
    if (tid < 3 * G + 3)
        totals[tid] = 0;
    if (tid < kPairVelocitiesTallies)
        tally[tid] = 0;
    __syncthreads();
    int n_rows = 0, n_sources = 0, n_both = 0;
    for (int r = tid; r < n; r += T) {
        const float4 p = pos[base + r], v = vel[base + r];
        const bool source = !sources || sources[base + r] != 0, row = !rows || rows[base + r] != 0;
        const PairVelocityPoint given{p.x, p.y, p.z, p.w, v.x, v.y, v.z};
        n_rows += row ? 1 : 0;
        n_sources += source ? 1 : 0;
        n_both += row && source ? 1 : 0;
        img[2 * r] = make_int4(__float_as_int(p.x), __float_as_int(p.y), __float_as_int(p.z),
                               pair_velocities_flags(row, source, pair_velocities_body_measured(given)));
        img[2 * r + 1] = make_int4(__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z), __float_as_int(p.w));
    }
    // Integers: the order of the additions does not matter.
    if (n_rows)
        atomicAdd(&tally[0], n_rows);
    if (n_sources)
        atomicAdd(&tally[1], n_sources);
    if (n_both)
        atomicAdd(&tally[2], n_both);
    __syncthreads();  // the image is in place
    const int passes = pair_velocities_passes(bins, G), blocks = pair_velocities_blocks(n);
    const float first = mine2[0], last = mine2[bins];
    PairVelocitySystemCounts seen;
    pair_velocities_clear(seen);
    for (int pass = 0; pass < passes; ++pass) {
        float e2[G + 1];  // the same in every lane
#pragma unroll
        for (int t = 0; t <= G; ++t)
            e2[t] = mine2[pass * G + t];
        PairVelocityCounts<G> c;
        pair_velocities_clear(c);
        double total[SLOTS];  // of sum tid + i T, in the lanes that have one
#pragma unroll
        for (int i = 0; i < SLOTS; ++i)
            total[i] = 0.0;
        for (int q0 = 0; q0 < n; q0 += T) {  // a round: the same for every lane of the workgroup
            const int r0 = q0 + wave * kPairVelocitiesBlock, r = r0 + lane;
            if (r0 < n) {  // the wave's block holds a row: the same in every lane of the wave
                PairVelocityPoint mine{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                int flags = 0;
                if (r < n) {
                    const int4 p = img[2 * r], v = img[2 * r + 1];
                    mine = pair_velocities_point(p, v);
                    flags = p.w;
                }
                const bool row = (flags & kPairVelocitiesRow) != 0, row_measured = (flags & kPairVelocitiesMeasured) != 0;
                PairVelocitySums<G> a;
                pair_velocities_clear(a);
#pragma unroll 1
                for (int j = 0; j < n; ++j) {
                    const int4 pj = img[2 * j], vj = img[2 * j + 1];  // wave-uniform addresses: broadcast LDS reads
                    const int fj = __builtin_amdgcn_readfirstlane(pj.w);
                    if ((fj & kPairVelocitiesSource) == 0)
                        continue;  // no source: the flag is the same in every lane, so the branch is a scalar one
                    const PairVelocityPoint column = pair_velocities_point(pj, vj);
                    const float r2 = pair_velocities_r2(correlation_examined(row, true, r, j),
                                                        row_measured && (fj & kPairVelocitiesMeasured) != 0, mine, column);
                    if (pass == 0)
                        pair_velocities_system_step(seen, r2, first, last);
                    const int bin = pair_velocities_bin<G>(r2, e2);
                    const bool member = pair_velocities_member<G>(bin);
                    if (NBODY_BATCH_PAIR_VELOCITIES_SKIP && __builtin_amdgcn_ballot_w64(member) == 0)
                        continue;  // the same in every lane of the wave
                    if (member)
                        pair_velocities_add<G>(a, c, bin, mine, column, weight);
                }
                // The block's partial of every sum: the halving tree over the 64 row sums, the result in lane 0.
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int k = 0; k < kPairVelocitiesTerms; ++k)
                        for (int off = kPairVelocitiesBlock / 2; off > 0; off >>= 1)
                            a.w[g][k] = pair_velocities_tree_step(a.w[g][k], __shfl_down(a.w[g][k], off, kPairVelocitiesBlock));
                if (lane == 0) {
#pragma unroll
                    for (int g = 0; g < G; ++g)
#pragma unroll
                        for (int k = 0; k < kPairVelocitiesTerms; ++k)
                            partials[wave * SUMS + g * kPairVelocitiesTerms + k] = a.w[g][k];
                }
            }
            __syncthreads();  // the partials of the round are in
            const int left = blocks - q0 / kPairVelocitiesBlock;  // the round's blocks that hold a row, in ascending order
#pragma unroll
            for (int i = 0; i < SLOTS; ++i)
                if (tid + i * T < SUMS)
                    total[i] = pair_velocities_total(total[i], partials + tid + i * T, SUMS, left < waves ? left : waves);
            __syncthreads();  // read before the next round writes
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const unsigned int count = pair_velocities_wave_total(c.count[g]), approaching = pair_velocities_wave_total(c.approaching[g]),
                               receding = pair_velocities_wave_total(c.receding[g]);
            if (lane == 0 && count) {
                atomicAdd(&totals[g], count);
                atomicAdd(&totals[G + g], approaching);
                atomicAdd(&totals[2 * G + g], receding);
            }
        }
        if (pass == 0) {
            const unsigned int within_first = pair_velocities_wave_total(seen.within_first),
                               within_last = pair_velocities_wave_total(seen.within_last), measured = pair_velocities_wave_total(seen.measured);
            if (lane == 0) {
                atomicAdd(&totals[3 * G], within_first);
                atomicAdd(&totals[3 * G + 1], within_last);
                atomicAdd(&totals[3 * G + 2], measured);
            }
        }
        __syncthreads();  // the integers of the pass are in
        // One lane per word of the pass's records: a sum from its total, an integer from the workgroup's.
        if (bins_out) {
            BatchPairVelocitiesBin *out = bins_out + (size_t)blockIdx.x * (size_t)bins + (size_t)pass * G;
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                const int sum = tid + i * T, g = sum / kPairVelocitiesTerms;
                if (sum < SUMS && pass * G + g < bins)
                    pair_velocities_store(out + g, kPairVelocitiesIntegers + sum % kPairVelocitiesTerms, total[i]);
            }
            if (tid < kPairVelocitiesIntegers * G && pass * G + tid % G < bins)
                pair_velocities_store(out + tid % G, tid / G, totals[tid]);
        }
        __syncthreads();  // the integers are read
        if (tid < 3 * G)
            totals[tid] = 0;
        __syncthreads();  // cleared before the next pass adds
    }
    if (tid == 0)
        systems[blockIdx.x] = pair_velocities_system(tally[0], tally[1], tally[2], bins, weight,
                                                     PairVelocitySystemCounts{totals[3 * G], totals[3 * G + 1], totals[3 * G + 2]});
}

// The dynamic LDS of one launch: the image, and the partials of one round, one set per wave.
inline size_t pair_velocities_lds_bytes(int max_bodies, int threads, int g)
{
    return 2 * sizeof(int4) * (size_t)max_bodies + sizeof(double) * (size_t)(threads / kPairVelocitiesBlock) * (size_t)(g * kPairVelocitiesTerms);
}

// One launch over all systems, G = kPairVelocitiesPassBins, for which edges2 is laid out.
hipError_t launch_batch_pair_velocities(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *rows,
                                        const unsigned char *sources, const float *edges2, int edge_stride, int n_systems, int max_bodies,
                                        int bins, int weight, BatchPairVelocitiesBin *bins_out, BatchPairVelocitiesSystem *systems,
                                        hipStream_t stream)
{
    const int threads = pair_velocities_threads(batch_shape(max_bodies).threads);
    return launch_analysis_kernel(batch_pair_velocities_kernel<kPairVelocitiesPassBins>, n_systems, threads,
                                  pair_velocities_lds_bytes(max_bodies, threads, kPairVelocitiesPassBins), stream, pos, vel, counts, rows,
                                  sources, edges2, edge_stride, max_bodies, bins, weight, bins_out, systems);
}

// ---- mutual gravity (include/nbody_batch_mutual_gravity.h): per system and ordered pair (a, b) of labelled sets, what set b
// does to set a -- potential, force, torque, virial and power as fp64 sums in the header's pinned order.  A sibling of
// batch_pair_velocities_kernel at a fraction of its registers: one workgroup per system sorts the bodies by set into LDS, so
// that the sources of a set are a contiguous range in ascending body index and a block of 64 rows holds rows of one set; a wave
// takes a row block and walks every set's range as a broadcast column loop.  It reads the state and writes only the handle's
// records.

static_assert(sizeof(BatchMutualGravityEntry) == sizeof(nbody_batch_mutual_gravity_entry) && sizeof(nbody_batch_mutual_gravity_entry) == 80 &&
                  offsetof(BatchMutualGravityEntry, pairs) == offsetof(nbody_batch_mutual_gravity_entry, pairs) &&
                  offsetof(BatchMutualGravityEntry, potential) == offsetof(nbody_batch_mutual_gravity_entry, potential) &&
                  offsetof(BatchMutualGravityEntry, force) == offsetof(nbody_batch_mutual_gravity_entry, force) &&
                  offsetof(BatchMutualGravityEntry, torque) == offsetof(nbody_batch_mutual_gravity_entry, torque) &&
                  offsetof(BatchMutualGravityEntry, virial) == offsetof(nbody_batch_mutual_gravity_entry, virial) &&
                  offsetof(BatchMutualGravityEntry, power) == offsetof(nbody_batch_mutual_gravity_entry, power) &&
                  offsetof(nbody_batch_mutual_gravity_entry, potential) == 8 && offsetof(nbody_batch_mutual_gravity_entry, force) == 16 &&
                  offsetof(nbody_batch_mutual_gravity_entry, torque) == 40 && offsetof(nbody_batch_mutual_gravity_entry, virial) == 64 &&
                  offsetof(nbody_batch_mutual_gravity_entry, power) == 72,
              "nbody_batch_mutual_gravity_math.h mirrors the entry of nbody_batch_mutual_gravity.h");
static_assert(sizeof(BatchMutualGravitySystem) == sizeof(nbody_batch_mutual_gravity_system) && sizeof(nbody_batch_mutual_gravity_system) == 128 &&
                  offsetof(BatchMutualGravitySystem, sets) == offsetof(nbody_batch_mutual_gravity_system, sets) &&
                  offsetof(BatchMutualGravitySystem, selected) == offsetof(nbody_batch_mutual_gravity_system, selected) &&
                  offsetof(BatchMutualGravitySystem, left_out) == offsetof(nbody_batch_mutual_gravity_system, left_out) &&
                  offsetof(BatchMutualGravitySystem, unmeasured) == offsetof(nbody_batch_mutual_gravity_system, unmeasured) &&
                  offsetof(BatchMutualGravitySystem, pairs) == offsetof(nbody_batch_mutual_gravity_system, pairs) &&
                  offsetof(BatchMutualGravitySystem, coincident) == offsetof(nbody_batch_mutual_gravity_system, coincident) &&
                  offsetof(BatchMutualGravitySystem, members) == offsetof(nbody_batch_mutual_gravity_system, members) &&
                  offsetof(BatchMutualGravitySystem, mass) == offsetof(nbody_batch_mutual_gravity_system, mass) &&
                  offsetof(nbody_batch_mutual_gravity_system, pairs) == 16 && offsetof(nbody_batch_mutual_gravity_system, coincident) == 24 &&
                  offsetof(nbody_batch_mutual_gravity_system, members) == 32 && offsetof(nbody_batch_mutual_gravity_system, mass) == 64,
              "nbody_batch_mutual_gravity_math.h mirrors the system record of nbody_batch_mutual_gravity.h");
static_assert(kMutualGravityMaxSets == NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS && kMutualGravityNoSet == NBODY_BATCH_MUTUAL_GRAVITY_NO_SET,
              "nbody_batch_mutual_gravity_math.h mirrors the limits of nbody_batch_mutual_gravity.h");
static_assert(sizeof(MutualGravityColumn) == sizeof(float4), "a column is one 16-byte read");

// The workgroup: batch_shape's, held to NBODY_BATCH_MUTUAL_GRAVITY_MAX_THREADS lanes.  A lane holds one row, four accumulators
// and nine addends, so every shape up to 1024 lanes fits its registers (DESIGN.md 3.6 has the compiler's figures); the units of
// work -- the row blocks of all sets -- go round the waves, so fewer waves cost no pass.
#ifndef NBODY_BATCH_MUTUAL_GRAVITY_MAX_THREADS
#define NBODY_BATCH_MUTUAL_GRAVITY_MAX_THREADS 1024
#endif
constexpr int kMutualGravityMaxThreads = NBODY_BATCH_MUTUAL_GRAVITY_MAX_THREADS;
inline int mutual_gravity_threads(int threads) { return threads < kMutualGravityMaxThreads ? threads : kMutualGravityMaxThreads; }

// The set of body i of the system (i below the count): its label, unless one of its seven words is not finite.  p and v take
// the body's words.
__device__ inline int mutual_gravity_body(const float4 *pos, const float4 *vel, const unsigned char *labels, size_t at, int sets, float4 &p,
                                          float4 &v, bool &labelled)
{
    p = pos[at];
    v = vel[at];
    const int label = labels[at];
    labelled = mutual_gravity_labelled(label, sets);
    return mutual_gravity_set(label, sets, mutual_gravity_measured(p.x, p.y, p.z, p.w, v.x, v.y, v.z));
}

// LDS: cols[slot] = {x, y, z, m} of the body sorted into `slot`, one broadcast ds_read_b128 per column, 64 KiB at 4096 bodies;
// behind it the partials of every unit, sets x 9 doubles each (41 KiB at 4096 bodies in 8 sets), and order[slot], the body of
// the slot, through which a row finds its velocity (16 KiB).  The sort: chunk c is bodies 64 c ... 64 c + 63, one wave at a
// time; the ballot of "my set is a" gives the chunk's count and every lane's rank, a lane per set walks the prefix over the
// chunks, and a second walk over the chunks places the bodies.  Unlabelled and unmeasured bodies get no slot.  Then unit u --
// block u - unit_start[a] of set a -- goes to wave u mod waves: lane l holds rank 64 k + l of the set, walks the range of every
// set b with four accumulators, forms the nine addends and six shuffles per sum make the block's partial; after the barrier
// lane (a, b, k) adds the partials of set a's blocks in ascending order.  The order of the header is that of body indices, so
// neither the workgroup's shape nor which wave took which unit shows in a record.
// frames holds {centre, velocity} of every system, six doubles.
__global__ __launch_bounds__(kMutualGravityMaxThreads) void batch_mutual_gravity_kernel(
    const float4 *__restrict__ pos, const float4 *__restrict__ vel, const int *__restrict__ counts, const unsigned char *__restrict__ labels,
    const double *__restrict__ frames, int max_bodies, int sets, double e2, BatchMutualGravityEntry *__restrict__ entries,
    BatchMutualGravitySystem *__restrict__ systems)
{
    extern __shared__ float4 sorted[];
    __shared__ int chunk_count[kMutualGravityMaxChunks * kMutualGravityMaxSets], chunk_offset[kMutualGravityMaxChunks * kMutualGravityMaxSets];
    __shared__ int members[kMutualGravityMaxSets], start[kMutualGravityMaxSets + 1], unit_start[kMutualGravityMaxSets + 1];
    __shared__ int tally[3];  // selected, left out, unmeasured
    __shared__ unsigned int coincident_total;
    MutualGravityColumn *cols = reinterpret_cast<MutualGravityColumn *>(sorted);
    double *partials = reinterpret_cast<double *>(sorted + max_bodies);  // [unit][sets][9]
    int *order = reinterpret_cast<int *>(partials + (size_t)mutual_gravity_max_units(max_bodies, sets) * sets * kMutualGravityTerms);
    const int n = counts[blockIdx.x] < max_bodies ? counts[blockIdx.x] : max_bodies;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & (kMutualGravityBlock - 1), wave = tid / kMutualGravityBlock;
    const int waves = T / kMutualGravityBlock, chunks = mutual_gravity_chunks(n);
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    if (tid < 3)
        tally[tid] = 0;
    if (tid == 0)
        coincident_total = 0;
    __syncthreads();
    // The counts of every chunk and set, and who is selected, left out and unmeasured.
    for (int c = wave; c < chunks; c += waves) {  // the same for every lane of the wave
        const int i = c * kMutualGravityBlock + lane;
        const bool below = i < n;
        bool labelled = false;
        int set = -1;
        if (below) {
            float4 p, v;
            set = mutual_gravity_body(pos, vel, labels, base + i, sets, p, v, labelled);
        }
        const int selected = mutual_gravity_chunk_count(__builtin_amdgcn_ballot_w64(set >= 0));
        const int left_out = mutual_gravity_chunk_count(__builtin_amdgcn_ballot_w64(below && !labelled));
        const int unmeasured = mutual_gravity_chunk_count(__builtin_amdgcn_ballot_w64(labelled && set < 0));
        for (int a = 0; a < sets; ++a) {
            const int count = mutual_gravity_chunk_count(__builtin_amdgcn_ballot_w64(set == a));
            if (lane == 0)
                chunk_count[c * kMutualGravityMaxSets + a] = count;
        }
        if (lane == 0) {  // integers: the order of the additions does not matter
            atomicAdd(&tally[0], selected);
            atomicAdd(&tally[1], left_out);
            atomicAdd(&tally[2], unmeasured);
        }
    }
    __syncthreads();
    if (tid < sets)
        members[tid] = mutual_gravity_prefix(chunk_count, chunks, tid, chunk_offset);
    __syncthreads();
    if (tid == 0)
        mutual_gravity_starts(members, sets, start, unit_start);
    __syncthreads();
    // The bodies into their slots.
    for (int c = wave; c < chunks; c += waves) {
        const int i = c * kMutualGravityBlock + lane;
        bool labelled = false;
        int set = -1;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f), v = p;
        if (i < n)
            set = mutual_gravity_body(pos, vel, labels, base + i, sets, p, v, labelled);
        for (int a = 0; a < sets; ++a) {
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(set == a);
            if (set == a) {
                const int slot = mutual_gravity_slot(start, chunk_offset, c, a, mutual_gravity_chunk_rank(mask, lane));
                sorted[slot] = p;
                order[slot] = i;
            }
        }
    }
    __syncthreads();  // the image is in place
    const double *frame = frames + (size_t)blockIdx.x * 6;
    const double centre[3] = {frame[0], frame[1], frame[2]}, velocity[3] = {frame[3], frame[4], frame[5]};
    const int units = unit_start[sets];
    unsigned int coincident = 0;
    for (int u = wave; u < units; u += waves) {  // the same for every lane of the wave
        const int a = mutual_gravity_unit_set(unit_start, u);
        const int rank = (u - unit_start[a]) * kMutualGravityBlock + lane, slot = start[a] + rank;
        const bool present = rank < members[a];
        MutualGravityRow row = mutual_gravity_row(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
        if (present) {
            const float4 p = sorted[slot], v = vel[base + order[slot]];
            row = mutual_gravity_row(p.x, p.y, p.z, p.w, v.x, v.y, v.z);
        }
        for (int b = 0; b < sets; ++b) {
            MutualGravitySums sums;
            mutual_gravity_clear(sums);
            const int last = start[b + 1];
#pragma unroll 1
            for (int j = start[b]; j < last; ++j)  // wave-uniform addresses: broadcast LDS reads
                mutual_gravity_step(sums, coincident, present && j != slot, row, cols[j], e2);
            double w[kMutualGravityTerms];
            mutual_gravity_addends(present, row, sums, centre, velocity, w);
            // The block's partial of every sum: the halving tree over the 64 addends, the result in lane 0.
#pragma unroll
            for (int k = 0; k < kMutualGravityTerms; ++k)
                for (int off = kMutualGravityBlock / 2; off > 0; off >>= 1)
                    w[k] = pair_velocities_tree_step(w[k], __shfl_down(w[k], off, kMutualGravityBlock));
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < kMutualGravityTerms; ++k)
                    partials[((size_t)u * sets + b) * kMutualGravityTerms + k] = w[k];
            }
        }
    }
    coincident = pair_velocities_wave_total(coincident);
    if (lane == 0 && coincident)
        atomicAdd(&coincident_total, coincident);
    __syncthreads();  // every partial is in
    BatchMutualGravityEntry *out = entries + (size_t)blockIdx.x * (size_t)(sets * sets);
    for (int word = tid; word < sets * sets * kMutualGravityTerms; word += T) {
        const int k = word % kMutualGravityTerms, b = word / kMutualGravityTerms % sets, a = word / (kMutualGravityTerms * sets);
        mutual_gravity_store(out + a * sets + b, k,
                             mutual_gravity_total(partials, unit_start[a], unit_start[a + 1] - unit_start[a], sets, b, k));
    }
    for (int e = tid; e < sets * sets; e += T)
        out[e].pairs = mutual_gravity_pairs(members[e / sets], members[e % sets], e / sets == e % sets);
    if (tid < kMutualGravityMaxSets) {
        systems[blockIdx.x].members[tid] = tid < sets ? members[tid] : 0;
        systems[blockIdx.x].mass[tid] = tid < sets ? mutual_gravity_mass(cols, start[tid], start[tid + 1]) : 0.0;
    }
    if (tid == 0) {
        long long pairs = 0;
        for (int e = 0; e < sets * sets; ++e)
            pairs += mutual_gravity_pairs(members[e / sets], members[e % sets], e / sets == e % sets);
        systems[blockIdx.x].sets = sets;
        systems[blockIdx.x].selected = tally[0];
        systems[blockIdx.x].left_out = tally[1];
        systems[blockIdx.x].unmeasured = tally[2];
        systems[blockIdx.x].pairs = pairs;
        systems[blockIdx.x].coincident = (long long)coincident_total;
    }
}

// The dynamic LDS of one launch: the sorted columns, the partials of every unit, the body of every slot.
inline size_t mutual_gravity_lds_bytes(int max_bodies, int sets)
{
    return sizeof(float4) * (size_t)max_bodies + sizeof(double) * (size_t)mutual_gravity_max_units(max_bodies, sets) * (size_t)(sets * kMutualGravityTerms) +
           sizeof(int) * (size_t)max_bodies;
}

// One launch over all systems.
hipError_t launch_batch_mutual_gravity(const float4 *pos, const float4 *vel, const int *counts, const unsigned char *labels,
                                       const double *frames, int n_systems, int max_bodies, int sets, double e2,
                                       BatchMutualGravityEntry *entries, BatchMutualGravitySystem *systems, hipStream_t stream)
{
    if (max_bodies > kMutualGravityMaxChunks * kMutualGravityBlock)
        return hipErrorInvalidValue;  // the chunk counts are laid out for 4096 bodies
    const int threads = mutual_gravity_threads(batch_shape(max_bodies).threads);
    return launch_analysis_kernel(batch_mutual_gravity_kernel, n_systems, threads, mutual_gravity_lds_bytes(max_bodies, sets), stream, pos, vel,
                                  counts, labels, frames, max_bodies, sets, e2, entries, systems);
}

// ---- diagnostics: per system {kinetic, potential, px, py, pz, mass} (fp32 pair terms, fp64 sums), nbody_energy's and
// nbody_momentum's definitions.  Not the hot path: one workgroup per system, one row per thread at a time.
constexpr int kDiagThreads = 256;  // kDiagValues: nbody_batch_handle.h, whose handle holds the results

// POT = false: momentum and mass only (no pair loop).
template <bool GUARD, bool POT>
__global__ __launch_bounds__(kDiagThreads) void batch_diag_kernel(const float4 *pos, const float4 *vel, const int *counts,
                                                                  int max_bodies, float eps2, double *out)
{
    extern __shared__ float4 sp[];
    __shared__ double red[kDiagValues][kDiagThreads / 64];
    const int n = counts[blockIdx.x];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    for (int j = tid; j < n; j += kDiagThreads)
        sp[j] = pos[base + j];
    __syncthreads();
    double acc[kDiagValues] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kDiagThreads) {
        const float4 pi = sp[i];
        const float4 w = vel[base + i];
        double phi = 0.0;
        for (int j = 0; j < (POT ? n : 0); ++j) {
            const float4 pj = sp[j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            float r2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, __builtin_fmaf(dx, dx, eps2)));
            float inv = __builtin_amdgcn_rsqf(GUARD ? guard_r2(r2) : r2);
            inv = j != i ? inv : 0.f;
            phi += (double)(pj.w * inv);
        }
        acc[0] += 0.5 * (double)pi.w * ((double)w.x * w.x + (double)w.y * w.y + (double)w.z * w.z);
        acc[1] += -0.5 * (double)pi.w * phi;
        acc[2] += (double)pi.w * w.x;
        acc[3] += (double)pi.w * w.y;
        acc[4] += (double)pi.w * w.z;
        acc[5] += (double)pi.w;
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < kDiagValues; ++c) {
        double s = acc[c];
        for (int off = 32; off > 0; off >>= 1)
            s += __shfl_down(s, off, 64);
        if (lane == 0)
            red[c][wave] = s;
    }
    __syncthreads();
    if (tid < kDiagValues) {
        double s = 0.0;
        for (int q = 0; q < kDiagThreads / 64; ++q)
            s += red[tid][q];
        out[(size_t)blockIdx.x * kDiagValues + tid] = s;
    }
}

hipError_t launch_batch_diag(const float4 *pos, const float4 *vel, const int *counts, int n_systems, int max_bodies,
                             float eps2, bool potential, double *out, hipStream_t stream)
{
    const size_t lds = sizeof(float4) * (size_t)max_bodies;
    const auto kernel = !potential    ? batch_diag_kernel<false, false>
                        : eps2 > 0.f ? batch_diag_kernel<false, true> : batch_diag_kernel<true, true>;
    hipLaunchKernelGGL(kernel, dim3(n_systems), dim3(kDiagThreads), lds, stream, pos, vel, counts, max_bodies, eps2, out);
    return hipGetLastError();
}

// ---- what the calls keep on the handle, and the calls (the C ABI) ----------------------------------------------------------

// DeviceArray, a device array that its owner frees, and copy_out: nbody_batch_handle.h, whose handle holds its arrays so too.

}  // namespace

// What the analysis calls keep on a handle: the records of each call's last launch, allocated by the first call that asks for
// them, and the host copies that outlive a call.  Nothing forgets them and no integrator reads them.
struct BatchAnalysis {
    DeviceArray<BatchPairRecord> pairs;  // [n_systems][max_bodies]
    DeviceArray<int> pairs_binaries;     // [n_systems]
    std::vector<int> pairs_binaries_host;  // the last call's, empty before any call (nbody_batch_pairs_binaries)
    DeviceArray<BatchStructureSystem> structure_systems;  // [n_systems]
    DeviceArray<BatchStructureBody> structure_bodies;     // [n_systems][max_bodies]
    DeviceArray<BatchMemberSystem> members_systems;  // [n_systems]
    DeviceArray<BatchMemberBody> members_bodies;     // [n_systems][max_bodies]
    DeviceArray<unsigned char> members_initial;      // [n_systems][max_bodies], the device copy of `initial`
    DeviceArray<BatchHierarchySystem> hierarchy_systems;  // [n_systems]
    DeviceArray<BatchHierarchyNode> hierarchy_nodes;      // [n_systems][max_bodies]; the kernel reads its own nodes back
    DeviceArray<BatchHierarchyBody> hierarchy_bodies;     // [n_systems][max_bodies]
    DeviceArray<BatchGravityRecord> gravity_records;  // one per row of the largest call so far
    DeviceArray<float> gravity_tidal;                 // kGravityTidalWords per row of the largest call that asked for them
    DeviceArray<int> gravity_counts;                  // [n_systems], the device copy of the point counts
    std::vector<int> gravity_counts_host;             // the last call's point counts: the copy's source until the stream is idle
    DeviceArray<BatchGroupSystem> groups_systems;  // [n_systems]
    DeviceArray<BatchGroupRecord> groups_records;  // [n_systems][max_bodies]
    DeviceArray<BatchGroupBody> groups_bodies;     // [n_systems][max_bodies]
    DeviceArray<float> groups_linking2;            // [n_systems]
    std::vector<float> groups_linking2_host;       // the last call's b[s] b[s]
    DeviceArray<BatchSpanSystem> span_systems;  // [n_systems]
    DeviceArray<BatchSpanEdge> span_edges;      // [n_systems][max_bodies]
    DeviceArray<BatchSpanBody> span_bodies;     // [n_systems][max_bodies]
    DeviceArray<unsigned char> span_subset;     // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<BatchNeighbourSystem> neighbours_systems;  // [n_systems]
    DeviceArray<BatchNeighbourBody> neighbours_bodies;     // [n_systems][max_bodies]
    DeviceArray<int> neighbours_index;                     // [n_systems][max_bodies][k] of the largest k that asked for lists
    DeviceArray<float> neighbours_r2;                      // the same
    DeviceArray<unsigned char> neighbours_sources;         // [n_systems][max_bodies], the device copy of `sources`
    DeviceArray<float> neighbours_radius2;                 // [n_systems]
    std::vector<float> neighbours_radius2_host;            // the last call's b[s] b[s]
    DeviceArray<BatchCorrelationSystem> correlation_systems;  // [n_systems]
    DeviceArray<unsigned int> correlation_counts;             // [n_systems][bins] of the largest call that asked for counts
    DeviceArray<unsigned char> correlation_rows;              // [n_systems][max_bodies], the device copy of `rows`
    DeviceArray<unsigned char> correlation_sources;           // [n_systems][max_bodies], the device copy of `sources`
    DeviceArray<float> correlation_edges2;                    // one set or [n_systems] sets of padded bins + 1 squared edges
    std::vector<float> correlation_edges2_host;               // the last call's: the copy's source until the stream is idle
    DeviceArray<BatchContactSystem> contacts_systems;  // [n_systems]
    DeviceArray<BatchContactBody> contacts_bodies;     // [n_systems][max_bodies]
    DeviceArray<BatchContact> contacts_list;           // [n_systems][capacity] of the largest call so far
    DeviceArray<unsigned char> contacts_subset;        // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<float> contacts_radius2;               // [n_systems]
    std::vector<float> contacts_radius2_host;          // the last call's b[s] b[s]
    DeviceArray<float> contacts_radii;                 // [n_systems][max_bodies], the device copy of `radii`
    DeviceArray<BatchApproachSystem> approaches_systems;  // [n_systems]
    DeviceArray<BatchApproachBody> approaches_bodies;     // [n_systems][max_bodies]
    DeviceArray<BatchApproach> approaches_list;           // [n_systems][capacity] of the largest call so far
    DeviceArray<unsigned char> approaches_subset;         // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<float> approaches_radius2;                // [n_systems]
    std::vector<float> approaches_radius2_host;           // the last call's b[s] b[s]
    DeviceArray<float> approaches_radii;                  // [n_systems][max_bodies], the device copy of `radii`
    DeviceArray<float> approaches_horizon;                // [n_systems], the device copy of `horizon`
    DeviceArray<BatchRadialSystem> radial_systems;  // [n_systems]
    DeviceArray<BatchRadialShell> radial_shells;    // [n_systems][shells] of the largest call that asked for shells
    DeviceArray<BatchRadialBody> radial_bodies;     // [n_systems][max_bodies]
    DeviceArray<unsigned char> radial_subset;       // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<double> radial_edges2;              // one set or [n_systems] sets of shells + 1 squared edges
    std::vector<double> radial_edges2_host;         // the last call's: the copy's source until the stream is idle
    DeviceArray<double> radial_frames;              // [n_systems][6]: centre, velocity
    std::vector<double> radial_frames_host;         // the last call's
    DeviceArray<BatchSurfaceSystem> surface_systems;  // [n_systems]
    DeviceArray<BatchSurfaceCell> surface_cells;      // [n_systems][rows][columns] of the largest call that asked for cells
    DeviceArray<BatchSurfaceBody> surface_bodies;     // [n_systems][max_bodies]
    DeviceArray<unsigned char> surface_subset;        // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<double> surface_edges;                // the sets of columns + 1 edges, then the sets of rows + 1
    std::vector<double> surface_edges_host;           // the last call's: the copy's source until the stream is idle
    DeviceArray<double> surface_frames;               // [n_systems][15]: centre, velocity, A, B, Q
    std::vector<double> surface_frames_host;          // the last call's
    DeviceArray<BatchShapeSystem> shape_systems;      // [n_systems]
    DeviceArray<BatchShapeAperture> shape_apertures;  // [n_systems][apertures] of the largest call that asked for them
    DeviceArray<BatchShapeBody> shape_bodies;         // [n_systems][max_bodies]
    DeviceArray<unsigned char> shape_subset;          // [n_systems][max_bodies], the device copy of `subset`
    DeviceArray<double> shape_aps;                    // one set or [n_systems] sets of apertures x {radius, inner, out2, in2}
    std::vector<double> shape_aps_host;               // the last call's: the copy's source until the stream is idle
    DeviceArray<double> shape_frames;                 // [n_systems][6]: centre, velocity
    std::vector<double> shape_frames_host;            // the last call's
    DeviceArray<BatchPairVelocitiesSystem> pair_velocities_systems;  // [n_systems]
    DeviceArray<BatchPairVelocitiesBin> pair_velocities_bins;        // [n_systems][bins] of the largest call that asked for them
    DeviceArray<unsigned char> pair_velocities_rows;                 // [n_systems][max_bodies], the device copy of `rows`
    DeviceArray<unsigned char> pair_velocities_sources;              // [n_systems][max_bodies], the device copy of `sources`
    DeviceArray<float> pair_velocities_edges2;                       // one set or [n_systems] sets of padded squared edges
    std::vector<float> pair_velocities_edges2_host;                  // the last call's: the copy's source until the stream is idle
    DeviceArray<BatchMutualGravitySystem> mutual_gravity_systems;  // [n_systems]
    DeviceArray<BatchMutualGravityEntry> mutual_gravity_entries;   // [n_systems][sets][sets] of the largest call so far
    DeviceArray<unsigned char> mutual_gravity_labels;              // [n_systems][max_bodies], the device copy of `labels`
    DeviceArray<double> mutual_gravity_frames;                     // [n_systems][6]: centre, velocity
    std::vector<double> mutual_gravity_frames_host;                // the last call's: the copy's source until the stream is idle
};

// Every member frees itself, in one walk that no new array can be left out of.
void batch_analysis_destroy(nbody_batch *b)
{
    delete b->analysis;
    b->analysis = nullptr;
}

}  // namespace nbody

using namespace nbody;

// The handle's analysis state in `a`, created by the first analysis call.
static hipError_t batch_analysis(nbody_batch *b, BatchAnalysis *&a)
{
    if (!b->analysis)
        b->analysis = new (std::nothrow) BatchAnalysis;
    a = b->analysis;
    return a ? hipSuccess : hipErrorOutOfMemory;  // which BATCH_TRY returns as NBODY_ERR_ALLOC
}

extern "C" {

int nbody_batch_pairs(nbody_batch *b, const float *d_pos, const float *d_vel, nbody_batch_pair_record *records_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_pairs: batch is NULL");
    if (!d_pos || !d_vel || !records_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pairs: NULL argument");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->pairs.ensure(slots));
    BATCH_TRY(b, a->pairs_binaries.ensure(B));
    std::vector<int> found;
    found.assign(B, 0);
    BATCH_TRY(b, launch_batch_pairs(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                    b->config.massive_set ? b->massive_dev.ptr : nullptr, (int)b->n_systems, (int)b->max_bodies,
                                    a->pairs.ptr, a->pairs_binaries.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, records_out, a->pairs, slots));
    BATCH_TRY(b, copy_out(b, found.data(), a->pairs_binaries, B));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    a->pairs_binaries_host.swap(found);
    return NBODY_OK;
}

int nbody_batch_pairs_binaries(nbody_batch *b, int64_t *count_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_pairs_binaries: batch is NULL");
    if (!count_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pairs_binaries: NULL argument");
    if (!b->analysis || b->analysis->pairs_binaries_host.empty())
        return bfail(b, NBODY_ERR_STATE, "nbody_batch_pairs_binaries: no nbody_batch_pairs call has been made");
    for (size_t s = 0; s < (size_t)b->n_systems; ++s)
        count_out[s] = b->analysis->pairs_binaries_host[s];
    return NBODY_OK;
}

int nbody_batch_structure(nbody_batch *b, const float *d_pos, int k, int weight, const double *fractions, int n_fractions,
                          nbody_batch_structure_system *systems_out, nbody_batch_structure_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_structure: batch is NULL");
    if (!d_pos || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: NULL argument");
    if (k < 1 || k > NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: k must be 1 ... 8");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    if (n_fractions < 0 || n_fractions > NBODY_BATCH_STRUCTURE_FRACTIONS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: n_fractions must be 0 ... 8");
    if (n_fractions > 0 && !fractions)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: fractions is NULL");
    BatchStructureArgs p{};
    p.n_fractions = n_fractions;
    p.k = k;
    p.weight = weight;
    for (int q = 0; q < n_fractions; ++q) {
        if (!(fractions[q] > 0.0 && fractions[q] <= 1.0))  // NaN is refused too
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_structure: a fraction must be in (0, 1]");
        p.fraction[q] = fractions[q];
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->structure_systems.ensure(B));
    BATCH_TRY(b, a->structure_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, launch_batch_structure(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr, (int)b->n_systems, (int)b->max_bodies, p,
                                        bodies_out ? a->structure_bodies.ptr : nullptr, a->structure_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->structure_systems, B));
    BATCH_TRY(b, copy_out(b, bodies_out, a->structure_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_members(nbody_batch *b, const float *d_pos, const float *d_vel, float softening, int max_iterations,
                        const unsigned char *initial, nbody_batch_member_system *systems_out, nbody_batch_member_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_members: batch is NULL");
    if (!d_pos || !d_vel || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_members: NULL argument");
    if (max_iterations < 1 || max_iterations > NBODY_BATCH_MEMBERS_MAX_ITERATIONS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_members: max_iterations must be 1 ... 64");
    if (!batch_softening_ok(softening))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_members: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9)");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->members_systems.ensure(B));
    BATCH_TRY(b, a->members_bodies.ensure(bodies_out ? slots : 0));
    if (initial) {
        BATCH_TRY(b, a->members_initial.ensure(slots));
        BATCH_TRY(b, hipMemcpyAsync(a->members_initial.ptr, initial, slots, hipMemcpyHostToDevice, b->stream));
    }
    BATCH_TRY(b, launch_batch_members(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                      b->config.massive_set ? b->massive_dev.ptr : nullptr, (int)b->n_systems, (int)b->max_bodies,
                                      softening * softening, max_iterations, initial ? a->members_initial.ptr : nullptr,
                                      bodies_out ? a->members_bodies.ptr : nullptr, a->members_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->members_systems, B));
    BATCH_TRY(b, copy_out(b, bodies_out, a->members_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_hierarchy(nbody_batch *b, const float *d_pos, const float *d_vel, double tidal_tolerance, int max_levels,
                          nbody_batch_hierarchy_system *systems_out, nbody_batch_hierarchy_node *nodes_out,
                          nbody_batch_hierarchy_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_hierarchy: batch is NULL");
    if (!d_pos || !d_vel || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_hierarchy: NULL argument");
    if (max_levels < 1 || max_levels > NBODY_BATCH_HIERARCHY_MAX_LEVELS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_hierarchy: max_levels must be 1 ... 16");
    if (!(tidal_tolerance >= 0.0))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_hierarchy: tidal_tolerance must be >= 0 (+inf accepts every pair), not NaN");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->hierarchy_systems.ensure(B));
    BATCH_TRY(b, a->hierarchy_nodes.ensure(slots));
    BATCH_TRY(b, a->hierarchy_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, launch_batch_hierarchy(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                        b->config.massive_set ? b->massive_dev.ptr : nullptr, (int)b->n_systems, (int)b->max_bodies,
                                        tidal_tolerance, max_levels, nodes_out != nullptr, a->hierarchy_nodes.ptr,
                                        bodies_out ? a->hierarchy_bodies.ptr : nullptr, a->hierarchy_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->hierarchy_systems, B));
    BATCH_TRY(b, copy_out(b, nodes_out, a->hierarchy_nodes, slots));
    BATCH_TRY(b, copy_out(b, bodies_out, a->hierarchy_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_gravity(nbody_batch *b, const float *d_pos, const float *d_points, int64_t n_points, const int64_t *host_point_counts,
                        float softening, nbody_batch_gravity_record *records_out, float *tidal_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_gravity: batch is NULL");
    if (!d_pos || !records_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_gravity: NULL argument");
    if (!d_points && (n_points != 0 || host_point_counts))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_gravity: n_points or host_point_counts given without points (own-bodies mode "
                                           "takes n_points = 0 and no point counts)");
    if (d_points && (n_points < 1 || n_points > NBODY_BATCH_GRAVITY_MAX_POINTS))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_gravity: n_points must be 1 ... NBODY_BATCH_GRAVITY_MAX_POINTS (1048576)");
    const size_t B = (size_t)b->n_systems;
    if (host_point_counts)
        for (size_t s = 0; s < B; ++s)
            if (host_point_counts[s] < 0 || host_point_counts[s] > n_points)
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_gravity: the point count of system " + std::to_string(s) + " is " +
                                                       std::to_string(host_point_counts[s]) + ", outside [0, n_points]");
    if (!batch_softening_ok(softening))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_gravity: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9)");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t rows = B * (size_t)(d_points ? n_points : b->max_bodies);
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->gravity_records.ensure(rows));  // these two grow when a call needs more rows
    BATCH_TRY(b, a->gravity_tidal.ensure(tidal_out ? kGravityTidalWords * rows : 0));
    if (host_point_counts) {
        BATCH_TRY(b, a->gravity_counts.ensure(B));
        a->gravity_counts_host.assign(B, 0);
        for (size_t s = 0; s < B; ++s)
            a->gravity_counts_host[s] = (int)host_point_counts[s];
        BATCH_TRY(b, hipMemcpyAsync(a->gravity_counts.ptr, a->gravity_counts_host.data(), sizeof(int) * B, hipMemcpyHostToDevice,
                                    b->stream));
    }
    BATCH_TRY(b, launch_batch_gravity(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_points), b->counts_dev.ptr,
                                      b->config.massive_set ? b->massive_dev.ptr : nullptr,
                                      host_point_counts ? a->gravity_counts.ptr : nullptr, (int)b->n_systems, (int)b->max_bodies,
                                      (int)n_points, softening * softening, a->gravity_records.ptr,
                                      tidal_out ? a->gravity_tidal.ptr : nullptr, b->stream));
    BATCH_TRY(b, copy_out(b, records_out, a->gravity_records, rows));
    BATCH_TRY(b, copy_out(b, tidal_out, a->gravity_tidal, kGravityTidalWords * rows));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_groups(nbody_batch *b, const float *d_pos, const float *d_vel, const float *linking_lengths, int min_members,
                       int weight, int max_sweeps, nbody_batch_group_system *systems_out, nbody_batch_group_record *groups_out,
                       nbody_batch_group_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_groups: batch is NULL");
    if (!d_pos || !d_vel || !linking_lengths || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_groups: NULL argument");
    if (min_members < 1)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_groups: min_members must be >= 1");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_groups: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    if (max_sweeps < 1 || max_sweeps > NBODY_BATCH_GROUPS_MAX_SWEEPS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_groups: max_sweeps must be 1 ... 64");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    for (size_t s = 0; s < B; ++s) {
        if (!std::isfinite(linking_lengths[s]) || linking_lengths[s] < 0.f)
            return bfail(b, NBODY_ERR_INVALID,
                         "nbody_batch_groups: the linking length of system " + std::to_string(s) + " must be finite and >= 0");
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->groups_linking2_host.assign(linking_lengths, linking_lengths + B);
    for (float &l : a->groups_linking2_host)
        l = l * l;  // b2: one fp32 product
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->groups_systems.ensure(B));
    BATCH_TRY(b, a->groups_linking2.ensure(B));
    BATCH_TRY(b, a->groups_records.ensure(groups_out ? slots : 0));
    BATCH_TRY(b, a->groups_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, hipMemcpyAsync(a->groups_linking2.ptr, a->groups_linking2_host.data(), sizeof(float) * B, hipMemcpyHostToDevice,
                                b->stream));
    BATCH_TRY(b, launch_batch_groups(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                     b->config.massive_set ? b->massive_dev.ptr : nullptr, a->groups_linking2.ptr, (int)b->n_systems,
                                     (int)b->max_bodies, min_members, weight, max_sweeps, bodies_out ? a->groups_bodies.ptr : nullptr,
                                     groups_out ? a->groups_records.ptr : nullptr, a->groups_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->groups_systems, B));
    BATCH_TRY(b, copy_out(b, groups_out, a->groups_records, slots));
    BATCH_TRY(b, copy_out(b, bodies_out, a->groups_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_span(nbody_batch *b, const float *d_pos, const unsigned char *subset, int separations,
                     nbody_batch_span_system *systems_out, nbody_batch_span_edge *edges_out, nbody_batch_span_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_span: batch is NULL");
    if (!d_pos || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_span: NULL argument");
    if (separations != 0 && separations != 1)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_span: separations must be 0 or 1");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->span_systems.ensure(B));
    BATCH_TRY(b, a->span_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->span_edges.ensure(edges_out ? slots : 0));
    BATCH_TRY(b, a->span_bodies.ensure(bodies_out ? slots : 0));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->span_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_span(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr, subset ? a->span_subset.ptr : nullptr,
                                   (int)b->n_systems, (int)b->max_bodies, separations, edges_out ? a->span_edges.ptr : nullptr,
                                   bodies_out ? a->span_bodies.ptr : nullptr, a->span_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->span_systems, B));
    BATCH_TRY(b, copy_out(b, edges_out, a->span_edges, slots));
    BATCH_TRY(b, copy_out(b, bodies_out, a->span_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_neighbours(nbody_batch *b, const float *d_pos, int k, const float *radii, const unsigned char *sources,
                           nbody_batch_neighbour_system *systems_out, nbody_batch_neighbour_body *bodies_out, int *index_out,
                           float *r2_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_neighbours: batch is NULL");
    if (!d_pos || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_neighbours: NULL argument");
    if (k < 1 || k > NBODY_BATCH_NEIGHBOURS_MAX)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_neighbours: k must be 1 ... 8");
    if (!index_out != !r2_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_neighbours: index_out and r2_out must be given both or neither");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, words = index_out ? slots * (size_t)k : 0;
    for (size_t s = 0; radii && s < B; ++s) {
        if (!(radii[s] >= 0.f))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_neighbours: the radius of system " + std::to_string(s) + " must be >= 0");
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    if (radii) {
        a->neighbours_radius2_host.assign(radii, radii + B);
        for (float &r : a->neighbours_radius2_host)
            r = r * r;  // b2: one fp32 product
    }
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->neighbours_systems.ensure(B));
    BATCH_TRY(b, a->neighbours_radius2.ensure(radii ? B : 0));
    BATCH_TRY(b, a->neighbours_sources.ensure(sources ? slots : 0));
    BATCH_TRY(b, a->neighbours_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->neighbours_index.ensure(words));
    BATCH_TRY(b, a->neighbours_r2.ensure(words));
    if (radii)
        BATCH_TRY(b, hipMemcpyAsync(a->neighbours_radius2.ptr, a->neighbours_radius2_host.data(), sizeof(float) * B,
                                    hipMemcpyHostToDevice, b->stream));
    if (sources)
        BATCH_TRY(b, hipMemcpyAsync(a->neighbours_sources.ptr, sources, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_neighbours(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr,
                                         sources ? a->neighbours_sources.ptr : nullptr, radii ? a->neighbours_radius2.ptr : nullptr,
                                         (int)b->n_systems, (int)b->max_bodies, k, bodies_out ? a->neighbours_bodies.ptr : nullptr,
                                         index_out ? a->neighbours_index.ptr : nullptr, index_out ? a->neighbours_r2.ptr : nullptr,
                                         a->neighbours_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->neighbours_systems, B));
    BATCH_TRY(b, copy_out(b, bodies_out, a->neighbours_bodies, slots));
    BATCH_TRY(b, copy_out(b, index_out, a->neighbours_index, words));
    BATCH_TRY(b, copy_out(b, r2_out, a->neighbours_r2, words));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_correlation(nbody_batch *b, const float *d_pos, int bins, const float *edges, int per_system,
                            const unsigned char *rows, const unsigned char *sources, nbody_batch_correlation_system *systems_out,
                            unsigned int *counts_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_correlation: batch is NULL");
    if (!d_pos || !edges || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_correlation: NULL argument");
    if (bins < 1 || bins > NBODY_BATCH_CORRELATION_MAX_BINS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_correlation: bins must be 1 ... 32");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, sets = per_system ? B : 1;
    const size_t given = (size_t)bins + 1, padded = (size_t)correlation_padded_bins(bins) + 1;
    for (size_t s = 0; s < sets; ++s) {
        const float *e = edges + s * given;
        const std::string which = per_system ? " of system " + std::to_string(s) : std::string(" of all systems");
        for (size_t t = 0; t < given; ++t) {
            if (!correlation_edge_valid(e[t]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_correlation: edge " + std::to_string(t) + which + " must be finite and >= 0");
            if (t > 0 && !(e[t] > e[t - 1]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_correlation: edge " + std::to_string(t) + which +
                                                       " is not above edge " + std::to_string(t - 1) + ": the edges must be strictly ascending");
        }
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->correlation_edges2_host.resize(sets * padded);
    for (size_t s = 0; s < sets; ++s)
        for (size_t t = 0; t < padded; ++t)  // e2: one fp32 product; from `bins` on copies of the last edge
            a->correlation_edges2_host[s * padded + t] = correlation_edge2(edges[s * given + (t < given ? t : given - 1)]);
    const size_t words = counts_out ? B * (size_t)bins : 0;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->correlation_systems.ensure(B));
    BATCH_TRY(b, a->correlation_edges2.ensure(sets * padded));
    BATCH_TRY(b, a->correlation_rows.ensure(rows ? slots : 0));
    BATCH_TRY(b, a->correlation_sources.ensure(sources ? slots : 0));
    BATCH_TRY(b, a->correlation_counts.ensure(words));
    BATCH_TRY(b, hipMemcpyAsync(a->correlation_edges2.ptr, a->correlation_edges2_host.data(), sizeof(float) * sets * padded,
                                hipMemcpyHostToDevice, b->stream));
    if (rows)
        BATCH_TRY(b, hipMemcpyAsync(a->correlation_rows.ptr, rows, slots, hipMemcpyHostToDevice, b->stream));
    if (sources)
        BATCH_TRY(b, hipMemcpyAsync(a->correlation_sources.ptr, sources, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_correlation(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr,
                                          rows ? a->correlation_rows.ptr : nullptr, sources ? a->correlation_sources.ptr : nullptr,
                                          a->correlation_edges2.ptr, per_system ? (int)padded : 0, (int)b->n_systems,
                                          (int)b->max_bodies, bins, counts_out ? a->correlation_counts.ptr : nullptr,
                                          a->correlation_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->correlation_systems, B));
    BATCH_TRY(b, copy_out(b, counts_out, a->correlation_counts, words));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_contacts(nbody_batch *b, const float *d_pos, const float *radius, const float *radii, const unsigned char *subset,
                         long long capacity, nbody_batch_contact_system *systems_out, nbody_batch_contact_body *bodies_out,
                         nbody_batch_contact *list_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_contacts: batch is NULL");
    if (!d_pos || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: NULL argument");
    if (!radius == !radii)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: exactly one of radius and radii must be given");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    for (size_t s = 0; radius && s < B; ++s) {
        if (!correlation_edge_valid(radius[s]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: the radius of system " + std::to_string(s) + " must be finite and >= 0");
    }
    std::string refused;
    if (radii && !batch_radii_ok(radii, b->counts.data(), b->n_systems, b->max_bodies, &refused))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: " + refused);
    if (capacity < 0)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: capacity must be >= 0");
    if ((capacity > 0) != (list_out != nullptr))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: list_out must be given iff capacity > 0");
    if (capacity > kContactsMaxEntries / (long long)B)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_contacts: n_systems x capacity must not exceed 2^28");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    if (radius) {
        a->contacts_radius2_host.resize(B);
        for (size_t s = 0; s < B; ++s)
            a->contacts_radius2_host[s] = contacts_radius_t2(radius[s]);  // b2: one fp32 product
    }
    const size_t entries = B * (size_t)capacity;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->contacts_systems.ensure(B));
    BATCH_TRY(b, a->contacts_radius2.ensure(radius ? B : 0));
    BATCH_TRY(b, a->contacts_radii.ensure(radii ? slots : 0));
    BATCH_TRY(b, a->contacts_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->contacts_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->contacts_list.ensure(entries));
    if (radius)
        BATCH_TRY(b, hipMemcpyAsync(a->contacts_radius2.ptr, a->contacts_radius2_host.data(), sizeof(float) * B, hipMemcpyHostToDevice,
                                    b->stream));
    if (radii)
        BATCH_TRY(b, hipMemcpyAsync(a->contacts_radii.ptr, radii, sizeof(float) * slots, hipMemcpyHostToDevice, b->stream));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->contacts_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_contacts(reinterpret_cast<const float4 *>(d_pos), b->counts_dev.ptr,
                                       subset ? a->contacts_subset.ptr : nullptr, radius ? a->contacts_radius2.ptr : nullptr,
                                       radii ? a->contacts_radii.ptr : nullptr, (int)b->n_systems, (int)b->max_bodies, capacity,
                                       bodies_out ? a->contacts_bodies.ptr : nullptr, capacity > 0 ? a->contacts_list.ptr : nullptr,
                                       a->contacts_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->contacts_systems, B));
    BATCH_TRY(b, copy_out(b, bodies_out, a->contacts_bodies, slots));
    BATCH_TRY(b, copy_out(b, list_out, a->contacts_list, entries));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_approaches(nbody_batch *b, const float *d_pos, const float *d_vel, const float *horizon, const float *radius,
                           const float *radii, const unsigned char *subset, long long capacity, nbody_batch_approach_system *systems_out,
                           nbody_batch_approach_body *bodies_out, nbody_batch_approach *list_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_approaches: batch is NULL");
    if (!d_pos || !d_vel || !horizon || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: NULL argument");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies;
    for (size_t s = 0; s < B; ++s) {
        if (!approaches_horizon_valid(horizon[s]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: the horizon of system " + std::to_string(s) + " must be finite and >= 0");
    }
    if (!radius == !radii)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: exactly one of radius and radii must be given");
    for (size_t s = 0; radius && s < B; ++s) {
        if (!correlation_edge_valid(radius[s]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: the radius of system " + std::to_string(s) + " must be finite and >= 0");
    }
    std::string refused;
    if (radii && !batch_radii_ok(radii, b->counts.data(), b->n_systems, b->max_bodies, &refused))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: " + refused);
    if (capacity < 0)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: capacity must be >= 0");
    if ((capacity > 0) != (list_out != nullptr))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: list_out must be given iff capacity > 0");
    if (capacity > kApproachesMaxEntries / (long long)B)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_approaches: n_systems x capacity must not exceed 2^27");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    if (radius) {
        a->approaches_radius2_host.resize(B);
        for (size_t s = 0; s < B; ++s)
            a->approaches_radius2_host[s] = contacts_radius_t2(radius[s]);  // b2: one fp32 product
    }
    const size_t entries = B * (size_t)capacity;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->approaches_systems.ensure(B));
    BATCH_TRY(b, a->approaches_horizon.ensure(B));
    BATCH_TRY(b, a->approaches_radius2.ensure(radius ? B : 0));
    BATCH_TRY(b, a->approaches_radii.ensure(radii ? slots : 0));
    BATCH_TRY(b, a->approaches_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->approaches_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->approaches_list.ensure(entries));
    BATCH_TRY(b, hipMemcpyAsync(a->approaches_horizon.ptr, horizon, sizeof(float) * B, hipMemcpyHostToDevice, b->stream));
    if (radius)
        BATCH_TRY(b, hipMemcpyAsync(a->approaches_radius2.ptr, a->approaches_radius2_host.data(), sizeof(float) * B, hipMemcpyHostToDevice,
                                    b->stream));
    if (radii)
        BATCH_TRY(b, hipMemcpyAsync(a->approaches_radii.ptr, radii, sizeof(float) * slots, hipMemcpyHostToDevice, b->stream));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->approaches_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_approaches(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                         subset ? a->approaches_subset.ptr : nullptr, radius ? a->approaches_radius2.ptr : nullptr,
                                         radii ? a->approaches_radii.ptr : nullptr, a->approaches_horizon.ptr, (int)b->n_systems,
                                         (int)b->max_bodies, capacity, bodies_out ? a->approaches_bodies.ptr : nullptr,
                                         capacity > 0 ? a->approaches_list.ptr : nullptr, a->approaches_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->approaches_systems, B));
    BATCH_TRY(b, copy_out(b, bodies_out, a->approaches_bodies, slots));
    BATCH_TRY(b, copy_out(b, list_out, a->approaches_list, entries));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_radial_profile(nbody_batch *b, const float *d_pos, const float *d_vel, int shells, const double *edges, int per_system,
                               const double *centre, const double *velocity, int weight, int projected, const unsigned char *subset,
                               nbody_batch_radial_system *systems_out, nbody_batch_radial_shell *shells_out,
                               nbody_batch_radial_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_radial_profile: batch is NULL");
    if (!d_pos || !d_vel || !edges || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: NULL argument");
    if (shells < 1 || shells > NBODY_BATCH_RADIAL_MAX_SHELLS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: shells must be 1 ... 32");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    if (projected < kRadialSpherical || projected > 2)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: projected must be -1 ... 2");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, sets = per_system ? B : 1;
    const size_t given = (size_t)shells + 1;
    for (size_t s = 0; s < sets; ++s) {
        const double *e = edges + s * given;
        const std::string which = per_system ? " of system " + std::to_string(s) : std::string(" of all systems");
        for (size_t t = 0; t < given; ++t) {
            if (!radial_edge_valid(e[t]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: edge " + std::to_string(t) + which + " must be finite and >= 0");
            if (t > 0 && !(e[t] > e[t - 1]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: edge " + std::to_string(t) + which +
                                                       " is not above edge " + std::to_string(t - 1) + ": the edges must be strictly ascending");
        }
    }
    for (size_t k = 0; k < 3 * B; ++k) {
        if (centre && !radial_finite(centre[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: the centre of system " + std::to_string(k / 3) + " must be finite");
        if (velocity && !radial_finite(velocity[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_radial_profile: the velocity of system " + std::to_string(k / 3) + " must be finite");
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->radial_edges2_host.resize(sets * given);
    for (size_t k = 0; k < sets * given; ++k)
        a->radial_edges2_host[k] = radial_edge2(edges[k]);  // e2: one fp64 product
    a->radial_frames_host.resize(B * kRadialFrameWords);
    for (size_t s = 0; s < B; ++s)
        for (size_t c = 0; c < 3; ++c) {
            a->radial_frames_host[s * kRadialFrameWords + c] = centre ? centre[3 * s + c] : 0.0;
            a->radial_frames_host[s * kRadialFrameWords + 3 + c] = velocity ? velocity[3 * s + c] : 0.0;
        }
    const size_t records = shells_out ? B * (size_t)shells : 0;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->radial_systems.ensure(B));
    BATCH_TRY(b, a->radial_edges2.ensure(sets * given));
    BATCH_TRY(b, a->radial_frames.ensure(B * kRadialFrameWords));
    BATCH_TRY(b, a->radial_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->radial_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->radial_shells.ensure(records));
    BATCH_TRY(b, hipMemcpyAsync(a->radial_edges2.ptr, a->radial_edges2_host.data(), sizeof(double) * sets * given, hipMemcpyHostToDevice,
                                b->stream));
    BATCH_TRY(b, hipMemcpyAsync(a->radial_frames.ptr, a->radial_frames_host.data(), sizeof(double) * B * kRadialFrameWords,
                                hipMemcpyHostToDevice, b->stream));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->radial_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_radial(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                     subset ? a->radial_subset.ptr : nullptr, a->radial_edges2.ptr, per_system ? (int)given : 0,
                                     a->radial_frames.ptr, (int)b->n_systems, (int)b->max_bodies, shells, projected, weight,
                                     bodies_out ? a->radial_bodies.ptr : nullptr, shells_out ? a->radial_shells.ptr : nullptr,
                                     a->radial_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->radial_systems, B));
    BATCH_TRY(b, copy_out(b, shells_out, a->radial_shells, records));
    BATCH_TRY(b, copy_out(b, bodies_out, a->radial_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_surface_map(nbody_batch *b, const float *d_pos, const float *d_vel, int columns, int rows, const double *edges_a,
                            const double *edges_b, int per_system, const double *centre, const double *velocity, const double *axes,
                            int weight, const unsigned char *subset, nbody_batch_surface_system *systems_out,
                            nbody_batch_surface_cell *cells_out, nbody_batch_surface_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_surface_map: batch is NULL");
    if (!d_pos || !d_vel || !edges_a || !edges_b || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: NULL argument");
    if (columns < 1 || columns > NBODY_BATCH_SURFACE_MAX_SIDE || rows < 1 || rows > NBODY_BATCH_SURFACE_MAX_SIDE)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: columns and rows must be 1 ... 64");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, sets = per_system ? B : 1;
    const size_t given_a = (size_t)columns + 1, given_b = (size_t)rows + 1;
    for (int axis = 0; axis < 2; ++axis) {
        const size_t given = axis ? given_b : given_a;
        for (size_t s = 0; s < sets; ++s) {
            const double *e = (axis ? edges_b : edges_a) + s * given;
            const std::string which = std::string(axis ? " of axis b" : " of axis a") +
                                      (per_system ? " of system " + std::to_string(s) : std::string(" of all systems"));
            for (size_t t = 0; t < given; ++t) {
                if (!surface_finite(e[t]))
                    return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: edge " + std::to_string(t) + which + " must be finite");
                if (t > 0 && !(e[t] > e[t - 1]))
                    return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: edge " + std::to_string(t) + which + " is not above edge " +
                                                           std::to_string(t - 1) + ": the edges must be strictly ascending");
            }
        }
    }
    for (size_t k = 0; k < 3 * B; ++k) {
        if (centre && !surface_finite(centre[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: the centre of system " + std::to_string(k / 3) + " must be finite");
        if (velocity && !surface_finite(velocity[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: the velocity of system " + std::to_string(k / 3) + " must be finite");
    }
    for (size_t k = 0; axes && k < 9 * B; ++k)
        if (!surface_finite(axes[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_surface_map: the axes of system " + std::to_string(k / 9) + " must be finite");
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->surface_edges_host.assign(edges_a, edges_a + sets * given_a);
    a->surface_edges_host.insert(a->surface_edges_host.end(), edges_b, edges_b + sets * given_b);
    a->surface_frames_host.resize(B * kSurfaceFrameWords);
    for (size_t s = 0; s < B; ++s) {
        double *f = a->surface_frames_host.data() + s * kSurfaceFrameWords;
        for (size_t c = 0; c < 3; ++c) {
            f[c] = centre ? centre[3 * s + c] : 0.0;
            f[3 + c] = velocity ? velocity[3 * s + c] : 0.0;
        }
        for (size_t k = 0; k < 9; ++k)
            f[kSurfaceViewAt + k] = axes ? axes[9 * s + k] : surface_identity((int)k);
    }
    const size_t edge_words = sets * (given_a + given_b), records = cells_out ? B * (size_t)columns * (size_t)rows : 0;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->surface_systems.ensure(B));
    BATCH_TRY(b, a->surface_edges.ensure(edge_words));
    BATCH_TRY(b, a->surface_frames.ensure(B * kSurfaceFrameWords));
    BATCH_TRY(b, a->surface_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->surface_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->surface_cells.ensure(records));
    BATCH_TRY(b, hipMemcpyAsync(a->surface_edges.ptr, a->surface_edges_host.data(), sizeof(double) * edge_words, hipMemcpyHostToDevice,
                                b->stream));
    BATCH_TRY(b, hipMemcpyAsync(a->surface_frames.ptr, a->surface_frames_host.data(), sizeof(double) * B * kSurfaceFrameWords,
                                hipMemcpyHostToDevice, b->stream));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->surface_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_surface(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                      subset ? a->surface_subset.ptr : nullptr, a->surface_edges.ptr, per_system ? (int)given_a : 0,
                                      a->surface_edges.ptr + sets * given_a, per_system ? (int)given_b : 0, a->surface_frames.ptr,
                                      (int)b->n_systems, (int)b->max_bodies, columns, rows, weight,
                                      bodies_out ? a->surface_bodies.ptr : nullptr, cells_out ? a->surface_cells.ptr : nullptr,
                                      a->surface_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->surface_systems, B));
    BATCH_TRY(b, copy_out(b, cells_out, a->surface_cells, records));
    BATCH_TRY(b, copy_out(b, bodies_out, a->surface_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_shape(nbody_batch *b, const float *d_pos, const float *d_vel, int apertures, const double *radii, const double *inner,
                      int per_system, const double *centre, const double *velocity, int weight, int reduced, double tol, int max_iterations,
                      int min_members, const unsigned char *subset, nbody_batch_shape_system *systems_out,
                      nbody_batch_shape_aperture *apertures_out, nbody_batch_shape_body *bodies_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_shape: batch is NULL");
    if (!d_pos || !d_vel || !radii || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: NULL argument");
    if (apertures < 1 || apertures > NBODY_BATCH_SHAPE_MAX_APERTURES)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: apertures must be 1 ... 8");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    if (!shape_finite(tol) || tol < 0.0)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: tol must be finite and >= 0");
    if (max_iterations < 1 || max_iterations > NBODY_BATCH_SHAPE_MAX_ITERATIONS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: max_iterations must be 1 ... 64");
    if (min_members < kShapeLeastMembers)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: min_members must be >= 4");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, sets = per_system ? B : 1;
    const size_t given = (size_t)apertures;
    for (size_t s = 0; s < sets; ++s)
        for (size_t t = 0; t < given; ++t) {
            const std::string which = " of aperture " + std::to_string(t) +
                                      (per_system ? " of system " + std::to_string(s) : std::string(" of all systems"));
            const double R = radii[s * given + t];
            if (!shape_finite(R) || !(R > 0.0))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: the radius" + which + " must be finite and > 0");
            if (inner && (!shape_finite(inner[s * given + t]) || !(inner[s * given + t] >= 0.0) || !(inner[s * given + t] < R)))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: the inner radius" + which + " must be finite, >= 0 and below its radius");
        }
    for (size_t k = 0; k < 3 * B; ++k) {
        if (centre && !shape_finite(centre[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: the centre of system " + std::to_string(k / 3) + " must be finite");
        if (velocity && !shape_finite(velocity[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_shape: the velocity of system " + std::to_string(k / 3) + " must be finite");
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->shape_aps_host.resize(sets * given * kShapeApertureWords);
    for (size_t k = 0; k < sets * given; ++k) {
        double *w = a->shape_aps_host.data() + k * kShapeApertureWords;
        w[0] = radii[k];
        w[1] = inner ? inner[k] : 0.0;
        w[2] = shape_square(w[0]);  // out2 and in2: one fp64 product each
        w[3] = shape_square(w[1]);
    }
    a->shape_frames_host.resize(B * kShapeFrameWords);
    for (size_t s = 0; s < B; ++s)
        for (size_t c = 0; c < 3; ++c) {
            a->shape_frames_host[s * kShapeFrameWords + c] = centre ? centre[3 * s + c] : 0.0;
            a->shape_frames_host[s * kShapeFrameWords + 3 + c] = velocity ? velocity[3 * s + c] : 0.0;
        }
    const size_t records = apertures_out ? B * given : 0, ap_words = sets * given * kShapeApertureWords;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->shape_systems.ensure(B));
    BATCH_TRY(b, a->shape_aps.ensure(ap_words));
    BATCH_TRY(b, a->shape_frames.ensure(B * kShapeFrameWords));
    BATCH_TRY(b, a->shape_subset.ensure(subset ? slots : 0));
    BATCH_TRY(b, a->shape_bodies.ensure(bodies_out ? slots : 0));
    BATCH_TRY(b, a->shape_apertures.ensure(records));
    BATCH_TRY(b, hipMemcpyAsync(a->shape_aps.ptr, a->shape_aps_host.data(), sizeof(double) * ap_words, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, hipMemcpyAsync(a->shape_frames.ptr, a->shape_frames_host.data(), sizeof(double) * B * kShapeFrameWords,
                                hipMemcpyHostToDevice, b->stream));
    if (subset)
        BATCH_TRY(b, hipMemcpyAsync(a->shape_subset.ptr, subset, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_shape(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                    subset ? a->shape_subset.ptr : nullptr, a->shape_aps.ptr,
                                    per_system ? (int)(given * kShapeApertureWords) : 0, a->shape_frames.ptr, (int)b->n_systems,
                                    (int)b->max_bodies, apertures, weight, reduced != 0 ? 1 : 0, tol, max_iterations, min_members,
                                    bodies_out ? a->shape_bodies.ptr : nullptr, apertures_out ? a->shape_apertures.ptr : nullptr,
                                    a->shape_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->shape_systems, B));
    BATCH_TRY(b, copy_out(b, apertures_out, a->shape_apertures, records));
    BATCH_TRY(b, copy_out(b, bodies_out, a->shape_bodies, slots));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_pair_velocities(nbody_batch *b, const float *d_pos, const float *d_vel, int bins, const float *edges, int per_system,
                                const unsigned char *rows, const unsigned char *sources, int weight,
                                nbody_batch_pair_velocities_system *systems_out, nbody_batch_pair_velocities_bin *bins_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: batch is NULL");
    if (!d_pos || !d_vel || !edges || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: NULL argument");
    if (bins < 1 || bins > NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: bins must be 1 ... 32");
    if (weight != NBODY_BATCH_WEIGHT_MASS && weight != NBODY_BATCH_WEIGHT_NUMBER)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER");
    const size_t B = (size_t)b->n_systems, slots = B * (size_t)b->max_bodies, sets = per_system ? B : 1;
    const size_t given = (size_t)bins + 1, padded = (size_t)pair_velocities_padded_edges(bins, kPairVelocitiesPassBins);
    for (size_t s = 0; s < sets; ++s) {
        const float *e = edges + s * given;
        const std::string which = per_system ? " of system " + std::to_string(s) : std::string(" of all systems");
        for (size_t t = 0; t < given; ++t) {
            if (!correlation_edge_valid(e[t]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: edge " + std::to_string(t) + which + " must be finite and >= 0");
            if (t > 0 && !(e[t] > e[t - 1]))
                return bfail(b, NBODY_ERR_INVALID, "nbody_batch_pair_velocities: edge " + std::to_string(t) + which +
                                                       " is not above edge " + std::to_string(t - 1) + ": the edges must be strictly ascending");
        }
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->pair_velocities_edges2_host.resize(sets * padded);
    for (size_t s = 0; s < sets; ++s)
        for (size_t t = 0; t < padded; ++t)  // e2: one fp32 product; from `bins` on copies of the last edge
            a->pair_velocities_edges2_host[s * padded + t] = correlation_edge2(edges[s * given + (t < given ? t : given - 1)]);
    const size_t records = bins_out ? B * (size_t)bins : 0;
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->pair_velocities_systems.ensure(B));
    BATCH_TRY(b, a->pair_velocities_edges2.ensure(sets * padded));
    BATCH_TRY(b, a->pair_velocities_rows.ensure(rows ? slots : 0));
    BATCH_TRY(b, a->pair_velocities_sources.ensure(sources ? slots : 0));
    BATCH_TRY(b, a->pair_velocities_bins.ensure(records));
    BATCH_TRY(b, hipMemcpyAsync(a->pair_velocities_edges2.ptr, a->pair_velocities_edges2_host.data(), sizeof(float) * sets * padded,
                                hipMemcpyHostToDevice, b->stream));
    if (rows)
        BATCH_TRY(b, hipMemcpyAsync(a->pair_velocities_rows.ptr, rows, slots, hipMemcpyHostToDevice, b->stream));
    if (sources)
        BATCH_TRY(b, hipMemcpyAsync(a->pair_velocities_sources.ptr, sources, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, launch_batch_pair_velocities(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel),
                                              b->counts_dev.ptr, rows ? a->pair_velocities_rows.ptr : nullptr,
                                              sources ? a->pair_velocities_sources.ptr : nullptr, a->pair_velocities_edges2.ptr,
                                              per_system ? (int)padded : 0, (int)b->n_systems, (int)b->max_bodies, bins, weight,
                                              bins_out ? a->pair_velocities_bins.ptr : nullptr, a->pair_velocities_systems.ptr, b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->pair_velocities_systems, B));
    BATCH_TRY(b, copy_out(b, bins_out, a->pair_velocities_bins, records));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_mutual_gravity(nbody_batch *b, const float *d_pos, const float *d_vel, int sets, const unsigned char *labels, float softening,
                               const double *centre, const double *velocity, nbody_batch_mutual_gravity_system *systems_out,
                               nbody_batch_mutual_gravity_entry *matrix_out)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: batch is NULL");
    if (!d_pos || !d_vel || !labels || !systems_out)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: NULL argument");
    if (sets < 1 || sets > NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: sets must be 1 ... 8");
    if (!batch_softening_ok(softening))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9)");
    const size_t B = (size_t)b->n_systems, n = (size_t)b->max_bodies, slots = B * n;
    for (size_t k = 0; k < slots; ++k)
        if (!mutual_gravity_label_valid(labels[k], sets))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: the label " + std::to_string((int)labels[k]) + " of body " +
                                                   std::to_string(k % n) + " of system " + std::to_string(k / n) + " must be below sets (" +
                                                   std::to_string(sets) + ") or 255");
    for (size_t k = 0; k < 3 * B; ++k) {
        if (centre && !radial_finite(centre[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: the centre of system " + std::to_string(k / 3) + " must be finite");
        if (velocity && !radial_finite(velocity[k]))
            return bfail(b, NBODY_ERR_INVALID, "nbody_batch_mutual_gravity: the velocity of system " + std::to_string(k / 3) + " must be finite");
    }
    BatchAnalysis *a = nullptr;
    BATCH_TRY(b, batch_analysis(b, a));
    a->mutual_gravity_frames_host.resize(B * 6);
    for (size_t s = 0; s < B; ++s)
        for (size_t c = 0; c < 3; ++c) {
            a->mutual_gravity_frames_host[s * 6 + c] = centre ? centre[3 * s + c] : 0.0;
            a->mutual_gravity_frames_host[s * 6 + 3 + c] = velocity ? velocity[3 * s + c] : 0.0;
        }
    const size_t records = B * (size_t)(sets * sets);
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, a->mutual_gravity_systems.ensure(B));
    BATCH_TRY(b, a->mutual_gravity_entries.ensure(records));
    BATCH_TRY(b, a->mutual_gravity_labels.ensure(slots));
    BATCH_TRY(b, a->mutual_gravity_frames.ensure(B * 6));
    BATCH_TRY(b, hipMemcpyAsync(a->mutual_gravity_labels.ptr, labels, slots, hipMemcpyHostToDevice, b->stream));
    BATCH_TRY(b, hipMemcpyAsync(a->mutual_gravity_frames.ptr, a->mutual_gravity_frames_host.data(), sizeof(double) * B * 6, hipMemcpyHostToDevice,
                                b->stream));
    BATCH_TRY(b, launch_batch_mutual_gravity(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                             a->mutual_gravity_labels.ptr, a->mutual_gravity_frames.ptr, (int)b->n_systems, (int)b->max_bodies,
                                             sets, mutual_gravity_e2(softening), a->mutual_gravity_entries.ptr, a->mutual_gravity_systems.ptr,
                                             b->stream));
    BATCH_TRY(b, copy_out(b, systems_out, a->mutual_gravity_systems, B));
    BATCH_TRY(b, copy_out(b, matrix_out, a->mutual_gravity_entries, matrix_out ? records : 0));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

static int batch_diag(nbody_batch *b, const float *d_pos, const float *d_vel, float softening, bool potential)
{
    BATCH_TRY(b, hipSetDevice(b->device));
    BATCH_TRY(b, launch_batch_diag(reinterpret_cast<const float4 *>(d_pos), reinterpret_cast<const float4 *>(d_vel), b->counts_dev.ptr,
                                   (int)b->n_systems, (int)b->max_bodies, softening * softening, potential, b->diag_dev.ptr, b->stream));
    BATCH_TRY(b, hipMemcpyAsync(b->diag_host.data(), b->diag_dev.ptr, sizeof(double) * b->diag_host.size(), hipMemcpyDeviceToHost,
                                b->stream));
    BATCH_TRY(b, hipStreamSynchronize(b->stream));
    return NBODY_OK;
}

int nbody_batch_energy(nbody_batch *b, const float *d_pos, const float *d_vel, float softening, double *out3B)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_energy: batch is NULL");
    if (!d_pos || !d_vel || !out3B)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_energy: NULL argument");
    if (!batch_softening_ok(softening))
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_energy: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9)");
    const int rc = batch_diag(b, d_pos, d_vel, softening, true);
    if (rc != NBODY_OK)
        return rc;
    for (int64_t s = 0; s < b->n_systems; ++s) {
        const double *d = &b->diag_host[(size_t)s * kDiagValues];
        out3B[3 * s] = d[0];
        out3B[3 * s + 1] = d[1];
        out3B[3 * s + 2] = d[0] + d[1];
    }
    return NBODY_OK;
}

int nbody_batch_momentum(nbody_batch *b, const float *d_pos, const float *d_vel, double *out4B)
{
    if (!b)
        return bfail(nullptr, NBODY_ERR_INVALID, "nbody_batch_momentum: batch is NULL");
    if (!d_pos || !d_vel || !out4B)
        return bfail(b, NBODY_ERR_INVALID, "nbody_batch_momentum: NULL argument");
    const int rc = batch_diag(b, d_pos, d_vel, 1.f, false);
    if (rc != NBODY_OK)
        return rc;
    for (int64_t s = 0; s < b->n_systems; ++s)
        for (int c = 0; c < 4; ++c)
            out4B[4 * s + c] = b->diag_host[(size_t)s * kDiagValues + 2 + c];
    return NBODY_OK;
}

}  // extern "C"