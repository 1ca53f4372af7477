// nbody_batch_gravity_math.h -- the arithmetic of nbody_batch_gravity (include/nbody_batch_gravity.h) that needs no GPU: the
// record and the empty record, the pair term of one row from one source with its tidal products, the sums of a row, and the
// launch plan for P rows.  Plain C++17 without HIP, like nbody_batch_members_math.h: batch_gravity_kernel (nbody_batch_analysis.hip)
// forms every pair and every sum through these functions, and a stand-alone driver (tests/batch_gravity_driver.cpp) calls them
// on the CPU, where tests/test_batch_gravity_cpu.py checks hand-picked rows and the plan.  On the device the reciprocal square
// root is v_rsq_f32; on the host it is 1 / sqrtf.  Internal; the public surface is include/nbody_batch_gravity.h.
#pragma once
#include "nbody_batch_choice.h"

#include <cmath>
#include <cstdint>

#ifndef NBODY_HD
#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif
#endif

namespace nbody {

constexpr int64_t kGravityMaxPoints = 1048576;  // NBODY_BATCH_GRAVITY_MAX_POINTS
constexpr int kGravityTidalWords = 6;           // {xx, xy, xz, yy, yz, zz}

// nbody_batch_gravity_record's layout (nbody_batch_analysis.hip asserts it): 24 bytes.
struct BatchGravityRecord {
    float acceleration[3], reserved;
    double potential;
};

// Rows from the count on, and every row of a block that has no row below it.
NBODY_HD inline BatchGravityRecord gravity_empty_record() { return BatchGravityRecord{{0.f, 0.f, 0.f}, 0.f, 0.0}; }

// guard_r2 of nbody_kernels.h, usable on the host: at eps = 0 an r2 below 2^-84 becomes +inf, whose rsq is 0.
constexpr float kGravityGuardMin = 0x1p-84f;
NBODY_HD inline float gravity_guard_r2(float r2) { return r2 >= kGravityGuardMin ? r2 : __builtin_inff(); }

NBODY_HD inline float gravity_rsq(float r2)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(r2);
#else
    return 1.f / sqrtf(r2);
#endif
}

// What one source adds to one row.  u and p are formed only with TIDAL.
struct GravityPair {
    float dx, dy, dz;  // d = x_j - x
    float mi, s;       // m_j inv and (m_j inv) inv^2
    float px, py, pz;  // p_a = u d_a, u = (3 s) inv^2
};

// The pair term of the row at (x, y, z) from the source {sx, sy, sz, sm}: batch_forces' r2, inv and s, operation for operation.
// GUARD: eps = 0.  skip: the source is the row itself (own-bodies mode), inv = 0 as members_columns has it.
template <bool GUARD, bool TIDAL>
NBODY_HD inline GravityPair gravity_pair(float x, float y, float z, float sx, float sy, float sz, float sm, float eps2, bool skip)
{
    GravityPair g;
    g.dx = sx - x;
    g.dy = sy - y;
    g.dz = sz - z;
    float r2 = __builtin_fmaf(g.dx, g.dx, eps2);
    r2 = __builtin_fmaf(g.dy, g.dy, r2);
    r2 = __builtin_fmaf(g.dz, g.dz, r2);
    if (GUARD)
        r2 = gravity_guard_r2(r2);
    float inv = gravity_rsq(r2);
    inv = skip ? 0.f : inv;
    g.mi = sm * inv;
    const float inv2 = inv * inv;
    g.s = g.mi * inv2;
    g.px = g.py = g.pz = 0.f;
    if (TIDAL) {
        const float u = (3.f * g.s) * inv2;
        g.px = u * g.dx;
        g.py = u * g.dy;
        g.pz = u * g.dz;
    }
    return g;
}

// The sums of one row: three fp32 chains for the acceleration, the fp64 sum of the potential's terms, and with TIDAL six fp32
// chains and the chain of s.  add() in ascending j; the outputs after the last source.
template <bool TIDAL>
struct GravityRow {
    float ax = 0.f, ay = 0.f, az = 0.f;
    double sum = 0.0;
    float txx = 0.f, txy = 0.f, txz = 0.f, tyy = 0.f, tyz = 0.f, tzz = 0.f, tr = 0.f;

    NBODY_HD inline void add(const GravityPair &g)
    {
        ax = __builtin_fmaf(g.dx, g.s, ax);
        ay = __builtin_fmaf(g.dy, g.s, ay);
        az = __builtin_fmaf(g.dz, g.s, az);
        sum += (double)g.mi;
        if (TIDAL) {
            txx = __builtin_fmaf(g.px, g.dx, txx);
            txy = __builtin_fmaf(g.px, g.dy, txy);
            txz = __builtin_fmaf(g.px, g.dz, txz);
            tyy = __builtin_fmaf(g.py, g.dy, tyy);
            tyz = __builtin_fmaf(g.py, g.dz, tyz);
            tzz = __builtin_fmaf(g.pz, g.dz, tzz);
            tr = tr + g.s;
        }
    }
    NBODY_HD inline BatchGravityRecord record() const { return BatchGravityRecord{{ax, ay, az}, 0.f, 0.0 - sum}; }
    // {xx, xy, xz, yy, yz, zz}: the diagonal less the chain of s
    NBODY_HD inline void tidal(float *t) const
    {
        t[0] = txx - tr;
        t[1] = txy;
        t[2] = txz;
        t[3] = tyy - tr;
        t[4] = tyz;
        t[5] = tzz - tr;
    }
};

// The launch plan for the rows of a system: the grid is (n_systems, blocks), a workgroup of `threads` lanes serves one system
// and the rpl * threads rows from block * rpl * threads on; gravity_row(block, rpl, threads, q, lane) is row q of the lane.
// Every row is served exactly once, and no result depends on the plan.  The system's sources sit in LDS, 16 bytes each.
struct GravityPlan {
    int rpl, threads, blocks;
    int rows_per_block() const { return rpl * threads; }
};

// The row that lane `lane` of row block `block` holds as its row q, in a workgroup of `threads` lanes with rpl rows each.
NBODY_HD inline int gravity_row(int block, int rpl, int threads, int q, int lane) { return block * (rpl * threads) + q * threads + lane; }

// Own-bodies mode: batch_shape(max_bodies)'s workgroup, one block -- the shape of the siblings.
inline GravityPlan gravity_plan_own(int max_bodies)
{
    const BatchShape sh = batch_shape(max_bodies);
    return {sh.rpl, sh.threads, 1};
}

// Points mode, by the number of points per system P alone: up to 4096 points one block of batch_shape(P)'s workgroup; beyond,
// blocks of 1024 lanes with four rows each (4096 rows a block, so that every broadcast LDS read feeds four pairs and a block
// reads its system's sources once for 4096 rows).
inline GravityPlan gravity_plan_points(int64_t n_points)
{
    constexpr int64_t kRows = 4096;
    if (n_points <= kRows) {
        const BatchShape sh = batch_shape((int)n_points);
        return {sh.rpl, sh.threads, 1};
    }
    return {4, 1024, (int)((n_points + kRows - 1) / kRows)};
}

// Dynamic LDS of a launch: the sources of a system as {x, y, z, m}.
inline size_t gravity_lds_bytes(int max_bodies) { return kBatchBytesPerBody * (size_t)max_bodies; }

}  // namespace nbody
