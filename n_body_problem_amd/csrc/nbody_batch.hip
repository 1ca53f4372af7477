// nbody_batch.hip -- batched ensembles (include/nbody.h, nbody_batch_*): B independent systems of up to
// NBODY_BATCH_MAX_BODIES bodies each, stepped together, ONE workgroup per system, k steps per launch with the system's
// state resident on chip.  HBM is read at the start of a launch and written at its end; between the steps of a launch the
// positions live in LDS (the column side, read by broadcast) and in registers (the row side, with velocities and
// accelerations).
//
// Summation order (what makes every result a function of the system alone): row i of a system of n_b bodies sums its
// columns j = 0 .. n_b - 1 in ascending order in ONE fp32 FMA chain per component, the self pair included (it adds exactly
// 0 for eps > 0, and the guard drops it for eps = 0).  Neither the slot of the system, nor B, nor max_bodies (which picks
// rows per lane and workgroup size), nor any other system changes a bit.  The pair term is the one of force_kernel
// (nbody_kernels.hip): d = x_j - x_i, r^2 + eps^2 by an FMA chain, v_rsq_f32, s = (m_j inv) (inv inv), a = fma(d, s, a).
// The update is update_kernel's: v <- (float)fma((double)a, (double)dt, (double)v), x <- (float)fma((double)v, ...).
// Hermite (NBODY_INTEGRATOR_HERMITE) runs a sibling kernel, batch_hermite_kernel: the same order, with the jerk summed
// beside the acceleration and a fourth-order predict-evaluate-correct step (see there).
// Here: the integrators' kernels and their launchers.  The host code behind their C ABI is in nbody_batch_capi.hip, which
// reaches them through nbody_batch_launch.h; what a state can be asked (pairs ... spanning trees, energy, momentum) is in
// nbody_batch_analysis.hip.
#include "nbody_batch_launch.h"
#include "nbody_kernels.h"

namespace nbody {
namespace {

static_assert(NBODY_BATCH_MAX_BODIES == 4096, "LDS per workgroup: 64 KiB of positions for the step kernels (two workgroups on a "
                                              "CU's 160 KiB), 128 KiB of positions and velocities for the Hermite families");
static_assert(sizeof(float4) == kBatchBytesPerBody, "nbody_batch_choice.h counts the dynamic LDS in float4");

// BatchLaunch, what the launches of a call share: nbody_batch_launch.h.

// One launch of a batch kernel, one workgroup per system, with the choice's workgroup and dynamic LDS.  The Hermite families
// raise their limit first: above the default 64 KiB of dynamic LDS from 2049 bodies on (128 KiB at 4096).
template <class... P, class... A>
hipError_t launch_batch_kernel(void (*kernel)(P...), const BatchLaunch &l, const A &...args)
{
    const BatchChoice &c = l.choice;
    if (c.raises_lds_limit()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)c.lds);
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kernel, dim3(l.n_systems), dim3(c.threads), c.lds, l.stream, args...);
    return hipGetLastError();
}

// Accelerations of the lane's RPL rows from the n columns in LDS, ascending j, one chain per row and component.
// OWN: batch_forces_jerks' tag (see there); batch_step_massive_kernel passes 1.
template <int RPL, bool GUARD, int OWN = 0>
__device__ __forceinline__ void batch_forces(const float4 *sp, int n, const float4 (&x)[RPL], float eps2, float (&ax)[RPL],
                                             float (&ay)[RPL], float (&az)[RPL])
{
#pragma unroll
    for (int k = 0; k < RPL; ++k)
        ax[k] = ay[k] = az[k] = 0.f;
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
        const float4 pj = sp[j];  // wave-uniform address: broadcast ds_read_b128
#pragma unroll
        for (int k = 0; k < RPL; ++k) {
            const float dx = pj.x - x[k].x, dy = pj.y - x[k].y, dz = pj.z - x[k].z;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            r2 = __builtin_fmaf(dz, dz, r2);
            if (GUARD)  // eps == 0: a pair at zero distance (the self pair) contributes 0
                r2 = guard_r2(r2);
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float s = (pj.w * inv) * (inv * inv);
            ax[k] = __builtin_fmaf(dx, s, ax[k]);
            ay[k] = __builtin_fmaf(dy, s, ay[k]);
            az[k] = __builtin_fmaf(dz, s, az[k]);
        }
    }
}

// kick v += a h, drift x += v h: fp64 FMA rounded to fp32, the arithmetic of update_kernel / kdk_kick_drift_kernel
__device__ __forceinline__ void batch_kick(float4 &v, float ax, float ay, float az, double h)
{
    v.x = (float)__builtin_fma((double)ax, h, (double)v.x);
    v.y = (float)__builtin_fma((double)ay, h, (double)v.y);
    v.z = (float)__builtin_fma((double)az, h, (double)v.z);
}
__device__ __forceinline__ void batch_drift(float4 &x, const float4 &v, double h)
{
    x.x = (float)__builtin_fma((double)v.x, h, (double)x.x);
    x.y = (float)__builtin_fma((double)v.y, h, (double)x.y);
    x.z = (float)__builtin_fma((double)v.z, h, (double)x.z);
}

// One workgroup = system blockIdx.x.  Row r of the system is row k of lane t with r = k * blockDim.x + t.  Slots
// r >= n_b are neither read nor written (their lanes compute on zeros and drop the result).
// KDK: acc holds the accelerations at the current positions when have_acc, and receives them at the end.
template <int RPL, bool GUARD, bool KDK>
__global__ __launch_bounds__(1024) void batch_step_kernel(float4 *pos, float4 *vel, float4 *acc, const int *counts,
                                                          int max_bodies, int k, float dt, float eps2, int have_acc)
{
    extern __shared__ float4 sp[];  // the system's positions, max_bodies float4
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL], v[RPL];
    float ax[RPL], ay[RPL], az[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        ax[q] = ay[q] = az[q] = 0.f;
        if (r < n) {
            x[q] = pos[base + r];
            v[q] = vel[base + r];
            sp[r] = x[q];
            if (KDK && have_acc) {
                const float4 a = acc[base + r];
                ax[q] = a.x;
                ay[q] = a.y;
                az[q] = a.z;
            }
        }
    }
    __syncthreads();
    const double h = (double)dt, hh = 0.5 * (double)dt;
    if (KDK && !have_acc) {
        batch_forces<RPL, GUARD>(sp, n, x, eps2, ax, ay, az);
        __syncthreads();  // every lane is done reading before the first drift rewrites the positions
    }
    for (int s = 0; s < k; ++s) {
        if (KDK) {
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                batch_kick(v[q], ax[q], ay[q], az[q], hh);
                batch_drift(x[q], v[q], h);
                const int r = q * T + tid;
                if (r < n)
                    sp[r] = x[q];
            }
            __syncthreads();
            batch_forces<RPL, GUARD>(sp, n, x, eps2, ax, ay, az);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                batch_kick(v[q], ax[q], ay[q], az[q], hh);
        } else {
            batch_forces<RPL, GUARD>(sp, n, x, eps2, ax, ay, az);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                batch_kick(v[q], ax[q], ay[q], az[q], h);
                batch_drift(x[q], v[q], h);
                const int r = q * T + tid;
                if (r < n)
                    sp[r] = x[q];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            pos[base + r] = x[q];  // .w (mass) unchanged
            vel[base + r] = v[q];  // .w unchanged
            if (KDK)
                acc[base + r] = make_float4(ax[q], ay[q], az[q], 0.f);
        }
    }
}

// ---- fourth-order Hermite: one predict-evaluate-correct (PEC) step per step, shared h ----
//   xp = x0 + v0 h + a0 h^2/2 + j0 h^3/6          vp = v0 + a0 h + j0 h^2/2
//   (a1, j1) = F(xp, vp)                           the one force evaluation of the step
//   v1 = v0 + (a0 + a1) h/2 + (j0 - j1) h^2/12     x1 = x0 + (v0 + v1) h/2 + (a0 - a1) h^2/12
// The column side lives in LDS, 32 B per body: body j's predicted {x, y, z, m} at sh[2j] and {vx, vy, vz, 0} at sh[2j + 1]
// (128 KiB at 4096 bodies: one workgroup per CU, as the registers of a 1024-thread workgroup allow anyway).

// The collision threshold of a pair with per-body radii (include/nbody_batch_radii.h): fmaf(S, S, eps^2), S = R_i + R_j.
__device__ __forceinline__ float radii_threshold(float ri, float rj, float eps2)
{
    const float S = ri + rj;
    return __builtin_fmaf(S, S, eps2);
}

// Accelerations and jerks of G rows at their predicted state (xp, vp) from the n columns in LDS, ascending j, one fp32
// chain per row and component.  Pair term: d = x_j - x_i, e = v_j - v_i, r^2 + eps^2 by batch_forces' FMA chain,
// inv = v_rsq_f32, inv2 = inv inv, s = (m_j inv) inv2 (batch_forces' s), rv = fma(dz, ez, fma(dy, ey, dx ex)),
// c = (3 rv) inv2; a = fma(d, s, a), j = fma(fma(-c, d, e), s, j).  27 VALU + 1 v_rsq_f32 per interaction.  GUARD: a
// zero-distance pair has inv = 0, so s = c = 0 and it adds exactly 0 to a and j.
// STOP (include/nbody_batch_stop.h): near2[k] receives, one bit per lane, whether row k met r^2 + eps^2 <= thr (the value
// before the guard) in at least TWO columns.  The self pair always meets it (its r^2 + eps^2 is eps^2 exactly and
// thr >= eps^2), so two columns mean a column j != i within the collision radius -- without an index or a compare against
// the row in the loop.  Per interaction one v_cmp into a scalar pair and three scalar mask operations (seen twice |=
// seen once & now; seen once |= now): no vector register, and a, j are summed by the same instructions.
// OWN (here, in hermite_evaluate and in hermite_evaluate_request): a tag without meaning that gives a kernel instantiations
// of its own.  A template instantiation is optimised once before it is inlined, and one more caller changes what the existing
// callers inline: batch_hermite_merge_kernel passes 1, so that the kernels before it stay the code they were.
// RADII (include/nbody_batch_radii.h, with STOP): the threshold is the pair's own, fmaf(S, S, eps^2) with S = R_row + R_j, one
// fp32 add; R_j rides in the fourth word of the column's velocity, which the broadcast read brings anyway, and rr[k] is the
// row's radius.  Two more VALU per interaction; the self pair still meets its threshold (eps^2 <= fmaf(2 R, 2 R, eps^2)).
// OWN = kOwnFate (batch_hermite_fate_kernel, with STOP): near1_out[k] receives the rows that met their threshold in at least
// ONE column.  The tag is a template argument, so the other instantiations do not contain the copy.
constexpr int kOwnFate = 4;
template <int G, bool GUARD, bool STOP = false, int OWN = 0, bool RADII = false>
__device__ __forceinline__ void batch_forces_jerks(const float4 *sh, int n, const float3 (&xp)[G], const float3 (&vp)[G],
                                                   float eps2, float3 (&a)[G], float3 (&jk)[G], float thr = 0.f,
                                                   unsigned long long *near2 = nullptr, const float *rr = nullptr,
                                                   unsigned long long *near1_out = nullptr)
{
    unsigned long long near1[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        a[k] = jk[k] = make_float3(0.f, 0.f, 0.f);
        near1[k] = 0;
        if (STOP)
            near2[k] = 0;
    }
#pragma unroll 1  // two rows of 27 VALU per column; unrolling would spill at RPL = 4
    for (int j = 0; j < n; ++j) {
        const float4 pj = sh[2 * j];  // wave-uniform addresses: two broadcast ds_read_b128 per column
        const float4 wj = sh[2 * j + 1];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const float dx = pj.x - xp[k].x, dy = pj.y - xp[k].y, dz = pj.z - xp[k].z;
            const float ex = wj.x - vp[k].x, ey = wj.y - vp[k].y, ez = wj.z - vp[k].z;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            r2 = __builtin_fmaf(dz, dz, r2);
            if (STOP) {
                const unsigned long long now = __ballot(r2 <= (RADII ? radii_threshold(rr[k], wj.w, eps2) : thr));
                near2[k] |= near1[k] & now;
                near1[k] |= now;
            }
            if (GUARD)
                r2 = guard_r2(r2);
            const float inv = __builtin_amdgcn_rsqf(r2);
            const float inv2 = inv * inv;
            const float s = (pj.w * inv) * inv2;
            const float rv = __builtin_fmaf(dz, ez, __builtin_fmaf(dy, ey, dx * ex));
            const float c = (3.f * rv) * inv2;
            a[k].x = __builtin_fmaf(dx, s, a[k].x);
            a[k].y = __builtin_fmaf(dy, s, a[k].y);
            a[k].z = __builtin_fmaf(dz, s, a[k].z);
            jk[k].x = __builtin_fmaf(__builtin_fmaf(-c, dx, ex), s, jk[k].x);
            jk[k].y = __builtin_fmaf(__builtin_fmaf(-c, dy, ey), s, jk[k].y);
            jk[k].z = __builtin_fmaf(__builtin_fmaf(-c, dz, ez), s, jk[k].z);
        }
    }
    if (OWN == kOwnFate) {  // include/nbody_batch_fate.h: a row without a column of its own is judged by one column
#pragma unroll
        for (int k = 0; k < G; ++k)
            near1_out[k] = near1[k];
    }
}

// Predictor and corrector, per component in fp64 from the fp32 operands, each result rounded once to fp32
// (h2 = h/2, h3 = h/3, h6 = h/6 in fp64):
//   xp = x + h (v + h2 (a + h3 j))       vp = v + h (a + h2 j)
//   v1 = v0 + h2 ((a0 + a1) + h6 (j0 - j1))       x1 = x0 + h2 ((v0 + v1) + h6 (a0 - a1)), v1 the rounded fp32 value
// The predictor and the corrector both widen x0, v0, a0 and j0 to fp64; left alone, the compiler keeps the fp64 copies of
// the predictor alive across the column loop for the corrector (twice the registers of the fp32 state: scratch at RPL = 4).
// An empty asm statement after the prediction makes the fp32 values new ones, so they are widened again where used.
__device__ __forceinline__ void renew_f32(float3 &u)
{
    asm volatile("" : "+v"(u.x), "+v"(u.y), "+v"(u.z));
}

struct HermiteSteps {
    double h, h2, h3, h6;
};
__device__ __forceinline__ float hermite_predict_x(float x, float v, float a, float j, const HermiteSteps &t)
{
    return (float)__builtin_fma(t.h, __builtin_fma(t.h2, __builtin_fma(t.h3, (double)j, (double)a), (double)v), (double)x);
}
__device__ __forceinline__ float hermite_predict_v(float v, float a, float j, const HermiteSteps &t)
{
    return (float)__builtin_fma(t.h, __builtin_fma(t.h2, (double)j, (double)a), (double)v);
}
__device__ __forceinline__ void hermite_correct(float &x, float &v, float a0, float a1, float j0, float j1,
                                                const HermiteSteps &t)
{
    const float v1 = (float)__builtin_fma(t.h2, __builtin_fma(t.h6, (double)j0 - (double)j1, (double)a0 + (double)a1),
                                          (double)v);
    x = (float)__builtin_fma(t.h2, __builtin_fma(t.h6, (double)a0 - (double)a1, (double)v + (double)v1), (double)x);
    v = v1;
}

// BatchStopArgs, the stopping conditions as the kernels take them: nbody_batch_launch.h.
constexpr int kStopCollision = 1, kStopEscape = 2;

// What the wave found in one row per lane, wave-uniform: kStopCollision when a row r < n (valid) saw a second column within
// the threshold (batch_forces_jerks), kStopEscape when a row r < n lies outside the escape radius at x.
__device__ __forceinline__ int stop_examine(unsigned long long near2, const float3 &x, bool valid, const BatchStopArgs &sa)
{
    const float d2 = __builtin_fmaf(x.z, x.z, __builtin_fmaf(x.y, x.y, x.x * x.x));
    return ((near2 & __ballot(valid)) != 0 ? kStopCollision : 0) | (__any(valid && d2 > sa.re2) ? kStopEscape : 0);
}

// Evaluate (a1, j1) for the lane's rows from the predicted state in LDS and, when CORRECT, apply the corrector; then
// (a, j) = (a1, j1).  The rows go in groups of at most two, each group one pass over the columns with its own predicted
// state reread from LDS: four rows at once (x0, v0, a0, j0 live beside the predicted state and the sums) would not fit
// 128 VGPRs without scratch.  A group's corrector writes only registers, so the next group still reads the predicted state.
// STOP (the evaluation at the current state, without the corrector): *found receives the stopping conditions the wave's
// rows meet there, the escape test on the positions the columns hold.
template <int RPL, bool GUARD, bool CORRECT, bool STOP = false, int OWN = 0>
__device__ __forceinline__ void hermite_evaluate(const float4 *sh, int n, int tid, int T, float eps2, float4 (&x)[RPL],
                                                 float3 (&v)[RPL], float3 (&a)[RPL], float3 (&jk)[RPL], const HermiteSteps &t,
                                                 const BatchStopArgs *sa = nullptr, int *found = nullptr)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    static_assert(!(STOP && CORRECT), "with the corrector the conditions are examined by hermite_evaluate_request");
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {  // xyz only: ds_read_b96
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
            }
        }
        if (STOP) {
            unsigned long long near2[G];
            batch_forces_jerks<G, GUARD, true, OWN>(sh, n, xp, vp, eps2, a1, j1, sa->thr, near2);
#pragma unroll
            for (int i = 0; i < G; ++i)
                *found |= stop_examine(near2[i], xp[i], (g + i) * T + tid < n, *sa);
        } else {
            batch_forces_jerks<G, GUARD, false, OWN>(sh, n, xp, vp, eps2, a1, j1);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i;
            if (CORRECT) {
                hermite_correct(x[q].x, v[q].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, t);
                hermite_correct(x[q].y, v[q].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, t);
                hermite_correct(x[q].z, v[q].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, t);
            }
            a[q] = a1[i];
            jk[q] = j1[i];
        }
    }
}

// One workgroup = system blockIdx.x, rows as in batch_step_kernel.  acc / jerk hold a0 and j0 at the current state when
// have_acc (otherwise they are evaluated first), and receive them at the end.  Slots r >= n_b are neither read nor written.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                             const int *counts, int max_bodies, int k, float dt, float eps2,
                                                             int have_acc)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const double h = (double)dt;
    const HermiteSteps t{h, 0.5 * h, h / 3.0, h / 6.0};
    float4 x[RPL];  // {x, y, z, m}
    float3 v[RPL], a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q] = a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            x[q] = pos[base + r];
            const float4 w = vel[base + r];
            v[q] = make_float3(w.x, w.y, w.z);
            if (have_acc) {
                const float4 a0 = acc[base + r], j0 = jerk[base + r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!have_acc) {  // (a0, j0) at the current state
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                sh[2 * r] = x[q];
                sh[2 * r + 1] = make_float4(v[q].x, v[q].y, v[q].z, 0.f);
            }
        }
        __syncthreads();
        hermite_evaluate<RPL, GUARD, false>(sh, n, tid, T, eps2, x, v, a, jk, t);
        __syncthreads();  // every lane is done reading before the first prediction rewrites the columns
    }
    for (int s = 0; s < k; ++s) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                sh[2 * r] = make_float4(hermite_predict_x(x[q].x, v[q].x, a[q].x, jk[q].x, t),
                                        hermite_predict_x(x[q].y, v[q].y, a[q].y, jk[q].y, t),
                                        hermite_predict_x(x[q].z, v[q].z, a[q].z, jk[q].z, t), x[q].w);
                sh[2 * r + 1] = make_float4(hermite_predict_v(v[q].x, a[q].x, jk[q].x, t),
                                            hermite_predict_v(v[q].y, a[q].y, jk[q].y, t),
                                            hermite_predict_v(v[q].z, a[q].z, jk[q].z, t), 0.f);
            }
            float3 xq = make_float3(x[q].x, x[q].y, x[q].z);
            renew_f32(xq);
            x[q] = make_float4(xq.x, xq.y, xq.z, x[q].w);
            renew_f32(v[q]);
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        hermite_evaluate<RPL, GUARD, true>(sh, n, tid, T, eps2, x, v, a, jk, t);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            pos[base + r] = x[q];  // .w (mass) unchanged
            float *w = reinterpret_cast<float *>(vel + base + r);
            w[0] = v[q].x;  // .w left alone
            w[1] = v[q].y;
            w[2] = v[q].z;
            acc[base + r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[base + r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
}

hipError_t launch_batch_hermite(const BatchLaunch &l, int k, float dt, float eps2, int have_acc)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts, l.max_bodies,
                                   k, dt, eps2, have_acc);
    });
}

// ---- adaptive shared steps (include/nbody_batch_evolve.h): every system on its own step h = dt_max 2^-L, to a common tick.
// A sibling of batch_hermite_kernel, which stays as it is: the step is its step (hermite_predict_*, batch_forces_jerks,
// hermite_correct, the same row groups), followed by Aarseth's criterion per row in fp64, the largest level any row asks for
// over the workgroup (the level of the smallest request) and the level rule, all workgroup-uniform.

// BatchEvolveState, per system in HBM between launches and calls: nbody_batch_handle.h, whose handle keeps a host copy.

// BatchEvolveArgs, dt_max and what every step needs of it: nbody_batch_launch.h.  kEvolveNoLevel: nbody_batch_handle.h.

// A value every lane holds, moved to scalar registers: the step constants must not cost vector registers.  The empty asm
// statement pins the result there (the compiler otherwise folds the readfirstlane of a value it knows to be uniform and
// keeps the fp64 constants in VGPRs).
__device__ __forceinline__ int uniform_i32(int x)
{
    int s = __builtin_amdgcn_readfirstlane(x);
    asm("" : "+s"(s));
    return s;
}
__device__ __forceinline__ long long uniform_i64(long long x)
{
    const unsigned lo = (unsigned)uniform_i32((int)(unsigned)x);
    const unsigned hi = (unsigned)uniform_i32((int)(unsigned)((unsigned long long)x >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double uniform_f64(double x) { return __longlong_as_double(uniform_i64(__double_as_longlong(x))); }

__device__ __forceinline__ double pow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }  // 2^k, |k| < 1023

// The step constants of a level: h = dt_max 2^-level exactly, HermiteSteps as batch_hermite_kernel forms them from its h.
struct EvolveSteps {
    HermiteSteps t;
    double ih2, ih3, h6;  // 1 / h^2, 1 / h^3, 6 h
};
__device__ __forceinline__ EvolveSteps evolve_steps(const BatchEvolveArgs &p, int level)
{
    const double s = pow2(-level);
    EvolveSteps e;
    e.t = HermiteSteps{uniform_f64(p.dt * s), uniform_f64(p.dt_half * s), uniform_f64(p.dt_third * s), uniform_f64(p.dt_sixth * s)};
    e.ih2 = uniform_f64(p.inv_dt2 * pow2(2 * level));
    e.ih3 = uniform_f64(p.inv_dt3 * pow2(3 * level));
    e.h6 = uniform_f64(p.dt_six * s);
    return e;
}

// Aarseth's criterion of one body from the accelerations and jerks at both ends of the step just taken (the header's
// formulas): dt^2 = num / den with num = eta (|a1| |a2_1| + |j1|^2), den = |j1| |a3| + |a2_1|^2.  Nothing is divided: a step
// of square h2 is too long for the body when h2 den > num (never for den = 0, the header's +inf).
struct EvolveNorms {
    double a1 = 0.0, a2 = 0.0, j1 = 0.0, a3 = 0.0;  // |a1|^2, |a2_1|^2, |j1|^2, |a3|^2, summed x, y, z
};
__device__ __forceinline__ void evolve_norms(EvolveNorms &s, float a0, float a1, float j0, float j1, const EvolveSteps &e)
{
    const double d = (double)a0 - (double)a1;
    const double s2 = (-6.0 * d - e.t.h * (4.0 * (double)j0 + 2.0 * (double)j1)) * e.ih2;
    const double s3 = (12.0 * d + e.h6 * ((double)j0 + (double)j1)) * e.ih3;
    const double s21 = s2 + e.t.h * s3;
    s.a1 += (double)a1 * (double)a1;
    s.a2 += s21 * s21;
    s.j1 += (double)j1 * (double)j1;
    s.a3 += s3 * s3;
}

// The level a wave asks for so far, in scalar registers: the smallest L whose squared step dt_max^2 4^-L is too long for
// none of the rows seen (at most `levels`; clamped: some row finds even that too long).  The system's request is the
// minimum over its bodies; L is monotone in it, so the level of the minimum is the largest level any body asks for -- an
// integer maximum, exact and free of order like the minimum, found without moving a double between lanes: one wave-wide
// vote per level (evolve_raise), then a maximum over the waves' words in LDS (evolve_publish / evolve_collect).
struct EvolveWant {
    int level = 0;  // levels + 1: clamped at `levels`
};
__device__ __forceinline__ void evolve_raise(EvolveWant &w, bool valid, double num, double den, const BatchEvolveArgs &p)
{
    while (w.level <= p.levels && __any(valid && p.dt2 * pow2(-2 * w.level) * den > num))
        ++w.level;
}

// hermite_evaluate<RPL, GUARD, true>, and the level the wave's rows ask for (rows r >= n ask for nothing).  x0 and v0 of
// a group's rows are read from the state arrays before the group's column loop (which hides the latency) and the corrected
// ones written back after it: held in registers for all four rows through both loops, as batch_hermite_kernel holds them,
// they leave no room for the criterion.  Each row votes as soon as its criterion is formed: nothing of it is carried
// across the next group's column loop.  STOP: *found receives the stopping conditions the wave's rows meet, the collision
// test in the column loop (at the predicted positions), the escape test on the corrected positions.
template <int RPL, bool GUARD, bool STOP = false, int OWN = 0>
__device__ __forceinline__ EvolveWant hermite_evaluate_request(const float4 *sh, int n, int tid, int T, float eps2, float4 *pos,
                                                               float4 *vel, float3 (&a)[RPL], float3 (&jk)[RPL],
                                                               const EvolveSteps &e, const BatchEvolveArgs &p,
                                                               const BatchStopArgs *sa = nullptr, int *found = nullptr)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    EvolveWant want;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G], x[G], v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = x[i] = v[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
                x[i] = *reinterpret_cast<const float3 *>(&pos[r]);
                v[i] = *reinterpret_cast<const float3 *>(&vel[r]);
            }
        }
        unsigned long long near2[G];
        if (STOP)
            batch_forces_jerks<G, GUARD, true, OWN>(sh, n, xp, vp, eps2, a1, j1, sa->thr, near2);
        else
            batch_forces_jerks<G, GUARD, false, OWN>(sh, n, xp, vp, eps2, a1, j1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            hermite_correct(x[i].x, v[i].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, e.t);
            hermite_correct(x[i].y, v[i].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, e.t);
            hermite_correct(x[i].z, v[i].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, e.t);
            if (STOP)
                *found |= stop_examine(near2[i], x[i], r < n, *sa);
            if (r < n) {  // x, y, z only: the masses and the velocities' w stay as they are
                *reinterpret_cast<float3 *>(&pos[r]) = x[i];
                *reinterpret_cast<float3 *>(&vel[r]) = v[i];
            }
            float3 a0 = a[q], j0 = jk[q];
            renew_f32(a0);  // widened again below, one component at a time: the corrector's fp64 copies end here
            renew_f32(j0);
            renew_f32(a1[i]);
            renew_f32(j1[i]);
            a[q] = a1[i];
            jk[q] = j1[i];
            EvolveNorms s;
            evolve_norms(s, a0.x, a1[i].x, j0.x, j1[i].x, e);
            evolve_norms(s, a0.y, a1[i].y, j0.y, j1[i].y, e);
            evolve_norms(s, a0.z, a1[i].z, j0.z, j1[i].z, e);
            const double num = p.eta * (__builtin_sqrt(s.a1 * s.a2) + s.j1), den = __builtin_sqrt(s.j1 * s.a3) + s.a2;
            evolve_raise(want, r < n, num, den, p);
        }
    }
    return want;
}

// The workgroup's level from the waves': red[] holds one word per wave.  The caller's barrier lies between evolve_publish and
// evolve_collect.  red[] is written between the two barriers of a step and read after the second, before the first
// barrier of the next step: no barrier of its own.
__device__ __forceinline__ void evolve_publish(int *red, const EvolveWant &w, int tid)
{
    if ((tid & 63) == 0)
        red[uniform_i32(tid >> 6)] = w.level;
}
__device__ __forceinline__ EvolveWant evolve_collect(const int *red, int T)
{
    int m = red[0];
    for (int w = 1; w < (T >> 6); ++w)
        m = red[w] > m ? red[w] : m;
    EvolveWant want;
    want.level = uniform_i32(m);
    return want;
}

// One workgroup = system blockIdx.x, rows and LDS as in batch_hermite_kernel.  The workgroup steps until its system is at
// the target tick, the launch's budget is spent or the call's max_steps are; then it writes its state, the caches and
// state[blockIdx.x], and counts itself in counters[0] if unfinished (counters[1]: unfinished and out of steps).
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_adaptive_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                      const int *counts, BatchEvolveState *state,
                                                                      int *counters, int max_bodies, BatchEvolveArgs p)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    __shared__ int red[16];         // the waves' levels
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    // Registers hold the rows' accelerations and jerks only.  Positions and velocities stay in the state arrays between
    // the steps: the predictor reads them, the corrector reads them again and writes them back (each lane its own rows, so
    // program order is all the ordering needed); the masses stay in LDS (sh[2 r].w, written once: the predictor rewrites
    // x, y, z only).  The same fp32 bits as in registers; per row and step two 16-byte reads and two 12-byte writes that
    // the caches serve, beside 2 x n_b column reads.
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!p.have_acc) {  // (a0, j0) at the current state, which the columns hold
        __syncthreads();
        const HermiteSteps unused{0.0, 0.0, 0.0, 0.0};
        float4 x4[RPL];  // not used without the corrector
        float3 v3[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            x4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            v3[q] = make_float3(0.f, 0.f, 0.f);
        }
        hermite_evaluate<RPL, GUARD, false>(sh, n, tid, T, p.eps2, x4, v3, a, jk, unused);
    }
    if (!p.have_level) {  // the first step: dt = eta_start |a| / |j|, compared as squares
        EvolveWant want;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
            const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
            evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);  // dt^2 = eta_start^2 |a|^2 / |j|^2
        }
        evolve_publish(red, want, tid);
    }
    __syncthreads();  // every lane is done reading before the first prediction rewrites the columns; red[] is complete
    if (!p.have_level) {
        const EvolveWant want = evolve_collect(red, T);
        level = want.level > p.levels ? p.levels : want.level;
        clamped += want.level > p.levels ? 1 : 0;
    }
    for (int run = 0; tick < p.target && run < p.budget && steps < p.max_steps; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        const EvolveWant mine = hermite_evaluate_request<RPL, GUARD>(sh, n, tid, T, p.eps2, pos, vel, a, jk, e, p);
        evolve_publish(red, mine, tid);
        __syncthreads();
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick += 1ll << (p.levels - level);
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
}

// BatchStopReport, per system beside BatchEvolveState, what a stopping condition found: nbody_batch_handle.h.

// The waves' findings (kStopCollision | kStopEscape) through LDS, as their levels: written where evolve_publish writes, read
// where evolve_collect reads.
__device__ __forceinline__ void stop_publish(int *red, int found, int tid)
{
    if ((tid & 63) == 0)
        red[uniform_i32(tid >> 6)] = found;
}
__device__ __forceinline__ int stop_collect(const int *red, int T)
{
    int m = red[0];
    for (int w = 1; w < (T >> 6); ++w)
        m |= red[w];
    return uniform_i32(m);
}

// The cold path of a system that stops (workgroup-uniform `found`): the colliding pair of smallest r^2 + eps^2 -- ties to
// the smallest i, then the smallest j, i < j -- among the columns LDS still holds, and the escaper of smallest index among
// the positions in the state array.  Every row rescans the columns after its own (a pair's two rows form the same r^2:
// the differences only change sign) and the workgroup takes a 64-bit minimum in LDS of the key {r^2 bits, i, j}; r^2 >= 0,
// so its bits order as the values, and an integer minimum does not depend on the order it is taken in.
__device__ __forceinline__ void stop_report(const float4 *sh, const float4 *pos, int n, int tid, int T, int rpl, float eps2,
                                            const BatchStopArgs &sa, int found, long long tick, BatchStopReport *out)
{
    __shared__ unsigned long long best;
    __shared__ int escaper;
    if (tid == 0) {
        best = ~0ull;
        escaper = 0x7fffffff;
    }
    __syncthreads();
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r >= n)
            continue;
        if (found & kStopCollision) {
            const float4 pi = sh[2 * r];
            unsigned long long mine = ~0ull;
            for (int j = r + 1; j < n; ++j) {
                const float4 pj = sh[2 * j];
                const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
                float r2 = __builtin_fmaf(dx, dx, eps2);
                r2 = __builtin_fmaf(dy, dy, r2);
                r2 = __builtin_fmaf(dz, dz, r2);
                if (r2 <= sa.thr) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(r2) << 24) | ((unsigned)r << 12) | (unsigned)j;
                    mine = key < mine ? key : mine;
                }
            }
            if (mine != ~0ull)
                atomicMin(&best, mine);
        }
        if (found & kStopEscape) {
            const float4 xi = pos[r];  // this lane's own writes: the corrected positions
            if (__builtin_fmaf(xi.z, xi.z, __builtin_fmaf(xi.y, xi.y, xi.x * xi.x)) > sa.re2)
                atomicMin(&escaper, r);
        }
    }
    __syncthreads();
    if (tid == 0) {
        BatchStopReport rep{tick, found, -1, -1, -1, 0.f, 0};
        if ((found & kStopCollision) && best != ~0ull) {
            rep.pair_i = (int)((best >> 12) & 0xfff);
            rep.pair_j = (int)(best & 0xfff);
            const float4 pi = sh[2 * rep.pair_i], pj = sh[2 * rep.pair_j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            rep.separation = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
        }
        if ((found & kStopEscape) && escaper != 0x7fffffff)
            rep.escaper = escaper;
        *out = rep;
    }
}

// batch_hermite_adaptive_kernel with the stopping conditions of include/nbody_batch_stop.h: a sibling, so that the kernel
// above stays the code it was.  The same loop; the system also leaves it after the step in which a condition is met,
// writes report[blockIdx.x] and is neither stepped nor counted as unfinished from then on (frozen).
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_stop_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                  const int *counts, BatchEvolveState *state, int *counters,
                                                                  int max_bodies, BatchEvolveArgs p, BatchStopArgs sa,
                                                                  BatchStopReport *report)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    __shared__ int red[16];         // the waves' levels
    __shared__ int red_stop[16];    // the waves' stopping conditions
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    const bool frozen = uniform_i32(report[blockIdx.x].reason) != 0;
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (frozen || tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target && !frozen) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    // Registers hold the rows' accelerations and jerks only.  Positions and velocities stay in the state arrays between
    // the steps: the predictor reads them, the corrector reads them again and writes them back (each lane its own rows, so
    // program order is all the ordering needed); the masses stay in LDS (sh[2 r].w, written once: the predictor rewrites
    // x, y, z only).  The same fp32 bits as in registers; per row and step two 16-byte reads and two 12-byte writes that
    // the caches serve, beside 2 x n_b column reads.
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!p.have_acc) {  // (a0, j0) at the current state, which the columns hold
        __syncthreads();
        const HermiteSteps unused{0.0, 0.0, 0.0, 0.0};
        float4 x4[RPL];  // not used without the corrector
        float3 v3[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            x4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            v3[q] = make_float3(0.f, 0.f, 0.f);
        }
        int found = 0;
        hermite_evaluate<RPL, GUARD, false, true>(sh, n, tid, T, p.eps2, x4, v3, a, jk, unused, &sa, &found);
        stop_publish(red_stop, found, tid);
    }
    if (!p.have_level) {  // the first step: dt = eta_start |a| / |j|, compared as squares
        EvolveWant want;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
            const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
            evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);  // dt^2 = eta_start^2 |a|^2 / |j|^2
        }
        evolve_publish(red, want, tid);
    }
    __syncthreads();  // every lane is done reading before the first prediction rewrites the columns; red[] is complete
    if (!p.have_level) {
        const EvolveWant want = evolve_collect(red, T);
        level = want.level > p.levels ? p.levels : want.level;
        clamped += want.level > p.levels ? 1 : 0;
    }
    int stop = 0;  // workgroup-uniform: the conditions met, which end the loop
    if (!p.have_acc)
        stop = stop_collect(red_stop, T);
    for (int run = 0; tick < p.target && run < p.budget && steps < p.max_steps && !stop; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        int found = 0;
        const EvolveWant mine = hermite_evaluate_request<RPL, GUARD, true>(sh, n, tid, T, p.eps2, pos, vel, a, jk, e, p, &sa, &found);
        stop_publish(red_stop, found, tid);
        evolve_publish(red, mine, tid);
        __syncthreads();
        stop = stop_collect(red_stop, T);
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick += 1ll << (p.levels - level);
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target && !stop) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
    if (stop)  // the columns still hold the positions the conditions were examined at
        stop_report(sh, pos, n, tid, T, RPL, p.eps2, sa, stop, tick, &report[blockIdx.x]);
}

// ---- mergers (include/nbody_batch_merge.h): a system whose bodies collide merges the pair and carries its run on.

// BatchMergeArgs, per launch the systems' merger counts and logs: nbody_batch_launch.h.

// One component of the merged body: fp64 from the fp32 operands, rounded once; M = (double)m_i + (double)m_j.
__device__ __forceinline__ float merge_mean(float mi, float ui, float mj, float uj, double M)
{
    if (M == 0.0)
        return (float)(0.5 * ((double)ui + (double)uj));
    return (float)(__builtin_fma((double)mj, (double)uj, (double)mi * (double)ui) / M);
}

// The cold path of a system that merges (workgroup-uniform): the pair as stop_report finds it -- the same rescan of the
// columns LDS still holds, the same key and 64-bit LDS minimum -- then lane 0 merges the pair in the state arrays (the
// corrected state: every lane's writes lie before the caller's last barrier), swaps the absorbed body with the last one and
// logs the event; after a barrier the columns are refilled from the current state of the n - 1 bodies left, and a last
// barrier completes them.  Returns whether a pair was found (always, when a row saw the threshold met: the rescan forms the
// evaluation's own r^2), workgroup-uniform.
__device__ __forceinline__ bool merge_absorb(float4 *sh, float4 *pos, float4 *vel, int n, int tid, int T, int rpl, float eps2,
                                             const BatchStopArgs &sa, long long tick, const BatchMergeArgs &ma,
                                             unsigned long long &best)
{
    asm volatile("" : "+v"(tid));  // the rows' addresses are formed here, not carried through the steps from the kernel's top
    if (tid == 0)
        best = ~0ull;
    __syncthreads();
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r >= n)
            continue;
        const float4 pi = sh[2 * r];
        unsigned long long mine = ~0ull;
        for (int j = r + 1; j < n; ++j) {
            const float4 pj = sh[2 * j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            r2 = __builtin_fmaf(dz, dz, r2);
            if (r2 <= sa.thr) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(r2) << 24) | ((unsigned)r << 12) | (unsigned)j;
                mine = key < mine ? key : mine;
            }
        }
        if (mine != ~0ull)
            atomicMin(&best, mine);
    }
    __syncthreads();
    const unsigned long long key = best;
    if (key == ~0ull)
        return false;
    if (tid == 0) {
        const int i = (int)((key >> 12) & 0xfff), j = (int)(key & 0xfff), last = n - 1;
        const float4 ci = sh[2 * i], cj = sh[2 * j];  // the positions of the evaluation that found the pair
        const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
        const float4 xi = pos[i], xj = pos[j], xl = pos[last], vi = vel[i], vj = vel[j], vl = vel[last];
        const float ex = vj.x - vi.x, ey = vj.y - vi.y, ez = vj.z - vi.z;
        const double M = (double)xi.w + (double)xj.w;
        pos[i] = make_float4(merge_mean(xi.w, xi.x, xj.w, xj.x, M), merge_mean(xi.w, xi.y, xj.w, xj.y, M),
                             merge_mean(xi.w, xi.z, xj.w, xj.z, M), xi.w + xj.w);
        vel[i] = make_float4(merge_mean(xi.w, vi.x, xj.w, vj.x, M), merge_mean(xi.w, vi.y, xj.w, vj.y, M),
                             merge_mean(xi.w, vi.z, xj.w, vj.z, M), vi.w);
        if (j != last) {
            pos[j] = xl;
            vel[j] = vl;
        }
        pos[last] = xj;
        vel[last] = vj;
        int sys = blockIdx.x;  // formed here: an address formed at the kernel's top would be carried through the steps
        asm volatile("" : "+s"(sys));
        const int merges = ma.merges[sys];  // the system's mergers so far: this one's place in the log
        ma.merges[sys] = merges + 1;
        if (merges < ma.capacity) {
            nbody_batch_merge_event ev;
            ev.tick = tick;
            ev.survivor = i;
            ev.absorbed = j;
            ev.count_before = n;
            ev.separation = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
            ev.relative_speed = __builtin_sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
            ev.mass_survivor = xi.w;
            ev.mass_absorbed = xj.w;
            ev.reserved = 0;
            ma.events[(size_t)sys * (size_t)ma.capacity + (size_t)merges] = ev;
        }
    }
    __syncthreads();  // the merged state is in the arrays, and every lane is done with the columns
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r < n - 1) {
            const float4 w = vel[r];
            sh[2 * r] = pos[r];
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
        }
    }
    __syncthreads();
    return true;
}

// The report of a system that stops under MERGE: an escaper only, found as stop_report finds it -- the smallest index among
// the positions in the state array that satisfy the test, a 32-bit LDS minimum.  The reason never has the collision bit.
__device__ __forceinline__ void merge_report_escaper(const float4 *pos, int n, int tid, int T, int rpl, const BatchStopArgs &sa,
                                                     long long tick, BatchStopReport *out, int &escaper)
{
    if (tid == 0)
        escaper = 0x7fffffff;
    __syncthreads();
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r >= n)
            continue;
        const float4 xi = pos[r];
        if (__builtin_fmaf(xi.z, xi.z, __builtin_fmaf(xi.y, xi.y, xi.x * xi.x)) > sa.re2)
            atomicMin(&escaper, r);
    }
    __syncthreads();
    if (tid == 0)
        *out = BatchStopReport{tick, kStopEscape, -1, -1, escaper != 0x7fffffff ? escaper : -1, 0.f, 0};
}

// The smallest level whose step 2^(levels - L) divides the tick (0 for tick 0).
__device__ __forceinline__ int merge_tick_level(long long tick, int levels)
{
    if (tick == 0)
        return 0;
    const int tz = __builtin_ctzll((unsigned long long)tick);
    return tz >= levels ? 0 : levels - tz;
}

// batch_hermite_stop_kernel with the collision action MERGE of include/nbody_batch_merge.h: a sibling again, so that the
// kernels above stay the code they are.  The same step; the body count is a workgroup-uniform scalar that a merger
// decrements (written back to counts at exit).  The evaluation at the current state and the first-step rule, which the
// kernels above run once at their top, are one block here that the loop enters again after every merger.  Launched only
// with a collision radius; reason never receives the collision bit.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_merge_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                   int *counts, BatchEvolveState *state, int *counters,
                                                                   int max_bodies, BatchEvolveArgs p, BatchStopArgs sa,
                                                                   BatchStopReport *report, BatchMergeArgs ma)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    __shared__ int red[16];         // the waves' levels
    __shared__ int red_stop[16];    // the waves' stopping conditions
    __shared__ unsigned long long cold_best;  // the cold paths' words: merge_absorb's minimum, merge_report_escaper's
    __shared__ int cold_escaper;
    int n = uniform_i32(counts[blockIdx.x]);
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    const bool frozen = uniform_i32(report[blockIdx.x].reason) != 0;
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (frozen || tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target && !frozen) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    // Registers hold the rows' accelerations and jerks only; positions and velocities stay in the state arrays and the
    // masses in LDS, as in batch_hermite_stop_kernel.
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    int stop = 0;                 // workgroup-uniform: the conditions met at the last evaluation
    int run = 0;
    bool evaluate = !p.have_acc;  // (a0, j0) are to be evaluated at the current state, which the columns hold
    bool choose = !p.have_level;  // the level is to come from the first-step rule
    // The evaluation at the current state and the first-step rule, then the steps until the target, the budget, max_steps or
    // a condition; after a collision the merger, and the same again.
    for (;;) {
        if (evaluate) {
            __syncthreads();
            const HermiteSteps unused{0.0, 0.0, 0.0, 0.0};
            float4 x4[RPL];  // not used without the corrector
            float3 v3[RPL];
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                x4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                v3[q] = make_float3(0.f, 0.f, 0.f);
            }
            int found = 0;
            hermite_evaluate<RPL, GUARD, false, true, 1>(sh, n, tid, T, p.eps2, x4, v3, a, jk, unused, &sa, &found);
            stop_publish(red_stop, found, tid);
        }
        if (choose) {  // dt = eta_start |a| / |j|, compared as squares
            EvolveWant want;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
                const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
                evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);
            }
            evolve_publish(red, want, tid);
        }
        __syncthreads();  // every lane is done reading before a prediction rewrites the columns; red[], red_stop[] are complete
        if (choose) {     // never coarser than the tick allows (tick 0 allows every level)
            const EvolveWant want = evolve_collect(red, T);
            const int floor_level = merge_tick_level(tick, p.levels);
            level = want.level > p.levels ? p.levels : want.level;
            level = level < floor_level ? floor_level : level;
            clamped += want.level > p.levels ? 1 : 0;
        }
        if (evaluate)
            stop = stop_collect(red_stop, T);
        for (; tick < p.target && run < p.budget && steps < p.max_steps && !stop; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        int found = 0;
        const EvolveWant mine = hermite_evaluate_request<RPL, GUARD, true, 1>(sh, n, tid, T, p.eps2, pos, vel, a, jk, e, p, &sa, &found);
        stop_publish(red_stop, found, tid);
        evolve_publish(red, mine, tid);
        __syncthreads();
        stop = stop_collect(red_stop, T);
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick += 1ll << (p.levels - level);
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
        }
        if (!(stop & kStopCollision))
            break;
        // the columns still hold the positions the collision was found at
        if (!merge_absorb(sh, pos, vel, n, tid, T, RPL, p.eps2, sa, tick, ma, cold_best)) {
            stop &= ~kStopCollision;
            break;
        }
        --n;
        evaluate = choose = true;
    }
    int lane = tid;  // the rows' indices formed anew: the offsets of the kernel's top are not carried through the steps for this
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + lane;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        counts[blockIdx.x] = n;
        if (tick < p.target && !stop) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
    if (stop)  // an escaper: among the corrected positions, or the current ones after a merger
        merge_report_escaper(pos, n, lane, T, RPL, sa, tick, &report[blockIdx.x], cold_escaper);
}

hipError_t launch_batch_merge(const BatchLaunch &l, const BatchEvolveArgs &p, const BatchStopArgs &sa, const BatchMergeArgs &ma)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_merge_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts, l.state,
                                   l.counters, l.max_bodies, p, sa, l.report, ma);
    });
}

// ---- per-body radii (include/nbody_batch_radii.h): a pair collides when it is within the sum of its own two radii.

// BatchRadiiArgs, per launch the radii and the collision action: nbody_batch_launch.h.

// hermite_evaluate<.., CORRECT = false, STOP = true> and hermite_evaluate_request<.., STOP = true> with radii: siblings, so
// that those stay the code they are for the kernels above.  The same row groups; a row's radius is read with its predicted
// velocity, one ds_read_b128 where those read 12 bytes, reread for every group, and handed to batch_forces_jerks, which
// forms the pair's threshold.  Nothing of it outlives the group's column loop.
template <int RPL, bool GUARD>
__device__ __forceinline__ void radii_evaluate(const float4 *sh, int n, int tid, int T, float eps2, float3 (&a)[RPL],
                                               float3 (&jk)[RPL], const BatchStopArgs &sa, int *found)
{
    constexpr int G = RPL < 2 ? RPL : 2;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G];
        float rr[G];
        unsigned long long near2[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = make_float3(0.f, 0.f, 0.f);
            rr[i] = 0.f;
            if (r < n) {
                const float4 w = sh[2 * r + 1];
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = make_float3(w.x, w.y, w.z);
                rr[i] = w.w;
            }
        }
        batch_forces_jerks<G, GUARD, true, 2, true>(sh, n, xp, vp, eps2, a1, j1, 0.f, near2, rr);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            *found |= stop_examine(near2[i], xp[i], (g + i) * T + tid < n, sa);
            a[g + i] = a1[i];
            jk[g + i] = j1[i];
        }
    }
}

template <int RPL, bool GUARD>
__device__ __forceinline__ EvolveWant radii_evaluate_request(const float4 *sh, int n, int tid, int T, float eps2, float4 *pos,
                                                             float4 *vel, float3 (&a)[RPL], float3 (&jk)[RPL], const EvolveSteps &e,
                                                             const BatchEvolveArgs &p, const BatchStopArgs &sa, int *found)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    EvolveWant want;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G], x[G], v[G];
        float rr[G];
        unsigned long long near2[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = x[i] = v[i] = make_float3(0.f, 0.f, 0.f);
            rr[i] = 0.f;
            if (r < n) {
                const float4 w = sh[2 * r + 1];
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = make_float3(w.x, w.y, w.z);
                rr[i] = w.w;
                x[i] = *reinterpret_cast<const float3 *>(&pos[r]);
                v[i] = *reinterpret_cast<const float3 *>(&vel[r]);
            }
        }
        batch_forces_jerks<G, GUARD, true, 2, true>(sh, n, xp, vp, eps2, a1, j1, 0.f, near2, rr);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            hermite_correct(x[i].x, v[i].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, e.t);
            hermite_correct(x[i].y, v[i].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, e.t);
            hermite_correct(x[i].z, v[i].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, e.t);
            *found |= stop_examine(near2[i], x[i], r < n, sa);
            if (r < n) {  // x, y, z only: the masses and the velocities' w stay as they are
                *reinterpret_cast<float3 *>(&pos[r]) = x[i];
                *reinterpret_cast<float3 *>(&vel[r]) = v[i];
            }
            float3 a0 = a[q], j0 = jk[q];
            renew_f32(a0);  // widened again below, one component at a time: the corrector's fp64 copies end here
            renew_f32(j0);
            renew_f32(a1[i]);
            renew_f32(j1[i]);
            a[q] = a1[i];
            jk[q] = j1[i];
            EvolveNorms s;
            evolve_norms(s, a0.x, a1[i].x, j0.x, j1[i].x, e);
            evolve_norms(s, a0.y, a1[i].y, j0.y, j1[i].y, e);
            evolve_norms(s, a0.z, a1[i].z, j0.z, j1[i].z, e);
            const double num = p.eta * (__builtin_sqrt(s.a1 * s.a2) + s.j1), den = __builtin_sqrt(s.j1 * s.a3) + s.a2;
            evolve_raise(want, r < n, num, den, p);
        }
    }
    return want;
}

// The pair stop_report and merge_absorb would name, with the threshold of each pair its own: the same rescan of the columns
// LDS still holds (positions at sh[2 j], radii at sh[2 j + 1].w), the same key and 64-bit LDS minimum.  S = R_i + R_j is
// the sum both of the pair's rows formed in the column loop (an fp32 add commutes).  Returns the key, workgroup-uniform;
// ~0: no pair.  The barrier that follows in every caller lies before the next use of `best`.
__device__ __forceinline__ unsigned long long radii_find_pair(const float4 *sh, int n, int tid, int T, int rpl, float eps2,
                                                              unsigned long long &best)
{
    if (tid == 0)
        best = ~0ull;
    __syncthreads();
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r >= n)
            continue;
        const float4 pi = sh[2 * r];
        const float ri = sh[2 * r + 1].w;
        unsigned long long mine = ~0ull;
        for (int j = r + 1; j < n; ++j) {
            const float4 pj = sh[2 * j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            r2 = __builtin_fmaf(dz, dz, r2);
            if (r2 <= radii_threshold(ri, sh[2 * j + 1].w, eps2)) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(r2) << 24) | ((unsigned)r << 12) | (unsigned)j;
                mine = key < mine ? key : mine;
            }
        }
        if (mine != ~0ull)
            atomicMin(&best, mine);
    }
    __syncthreads();
    return best;
}

// stop_report with per-pair thresholds: the pair of radii_find_pair when the collision bit is set, the escaper of smallest
// index when the escape bit is.  Under MERGE the collision bit never arrives here.
__device__ __forceinline__ void radii_stop_report(const float4 *sh, const float4 *pos, int n, int tid, int T, int rpl, float eps2,
                                                  const BatchStopArgs &sa, int found, long long tick, BatchStopReport *out,
                                                  unsigned long long &best, int &escaper)
{
    unsigned long long key = ~0ull;
    if (found & kStopCollision)
        key = radii_find_pair(sh, n, tid, T, rpl, eps2, best);
    if (tid == 0)
        escaper = 0x7fffffff;
    __syncthreads();
    if (found & kStopEscape)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            if (r >= n)
                continue;
            const float4 xi = pos[r];  // this lane's own writes: the corrected positions
            if (__builtin_fmaf(xi.z, xi.z, __builtin_fmaf(xi.y, xi.y, xi.x * xi.x)) > sa.re2)
                atomicMin(&escaper, r);
        }
    __syncthreads();
    if (tid == 0) {
        BatchStopReport rep{tick, found, -1, -1, -1, 0.f, 0};
        if (key != ~0ull) {
            rep.pair_i = (int)((key >> 12) & 0xfff);
            rep.pair_j = (int)(key & 0xfff);
            const float4 pi = sh[2 * rep.pair_i], pj = sh[2 * rep.pair_j];
            const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
            rep.separation = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
        }
        if ((found & kStopEscape) && escaper != 0x7fffffff)
            rep.escaper = escaper;
        *out = rep;
    }
}

// The survivor's radius: volumes add.  fp64 from the fp32 operands, the cubes by two products each, rounded once to fp32.
__device__ __forceinline__ float merge_radius(float ri, float rj)
{
    const double a = (double)ri, b = (double)rj;
    return (float)cbrt(a * a * a + b * b * b);
}

// merge_absorb with radii: the pair of radii_find_pair; lane 0 merges it in the state arrays, swaps the absorbed body with
// the last one and logs the event, as there.  The radii: every lane reads those of the pair and of the last body from the
// columns before the barrier, and the refill gives each row its own -- the survivor's the merged radius, slot j the last
// body's, slot n - 1 the absorbed body's (beyond the new count: to the array only) -- the lanes that own those three rows
// writing them to the radii array too.  Returns whether a pair was found, workgroup-uniform.
__device__ __forceinline__ bool radii_merge_absorb(float4 *sh, float4 *pos, float4 *vel, float *rad, int n, int tid, int T, int rpl,
                                                   float eps2, long long tick, const BatchMergeArgs &ma, unsigned long long &best)
{
    asm volatile("" : "+v"(tid));  // the rows' addresses are formed here, not carried through the steps from the kernel's top
    const unsigned long long key = radii_find_pair(sh, n, tid, T, rpl, eps2, best);
    if (key == ~0ull)
        return false;
    const int i = (int)((key >> 12) & 0xfff), j = (int)(key & 0xfff), last = n - 1;
    const float ri = sh[2 * i + 1].w, rj = sh[2 * j + 1].w, rl = sh[2 * last + 1].w;
    if (tid == 0) {
        const float4 ci = sh[2 * i], cj = sh[2 * j];  // the positions of the evaluation that found the pair
        const float dx = cj.x - ci.x, dy = cj.y - ci.y, dz = cj.z - ci.z;
        const float4 xi = pos[i], xj = pos[j], xl = pos[last], vi = vel[i], vj = vel[j], vl = vel[last];
        const float ex = vj.x - vi.x, ey = vj.y - vi.y, ez = vj.z - vi.z;
        const double M = (double)xi.w + (double)xj.w;
        pos[i] = make_float4(merge_mean(xi.w, xi.x, xj.w, xj.x, M), merge_mean(xi.w, xi.y, xj.w, xj.y, M),
                             merge_mean(xi.w, xi.z, xj.w, xj.z, M), xi.w + xj.w);
        vel[i] = make_float4(merge_mean(xi.w, vi.x, xj.w, vj.x, M), merge_mean(xi.w, vi.y, xj.w, vj.y, M),
                             merge_mean(xi.w, vi.z, xj.w, vj.z, M), vi.w);
        if (j != last) {
            pos[j] = xl;
            vel[j] = vl;
        }
        pos[last] = xj;
        vel[last] = vj;
        int sys = blockIdx.x;
        asm volatile("" : "+s"(sys));
        const int merges = ma.merges[sys];  // the system's mergers so far: this one's place in the log
        ma.merges[sys] = merges + 1;
        if (merges < ma.capacity) {
            nbody_batch_merge_event ev;
            ev.tick = tick;
            ev.survivor = i;
            ev.absorbed = j;
            ev.count_before = n;
            ev.separation = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
            ev.relative_speed = __builtin_sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
            ev.mass_survivor = xi.w;
            ev.mass_absorbed = xj.w;
            ev.reserved = 0;
            ma.events[(size_t)sys * (size_t)ma.capacity + (size_t)merges] = ev;
        }
    }
    __syncthreads();  // the merged state is in the arrays, and every lane is done with the columns
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r >= n)
            continue;
        float R = sh[2 * r + 1].w;  // the row's own word: no other lane writes it
        if (r == i)
            R = merge_radius(ri, rj);
        else if (r == last)
            R = rj;
        else if (r == j)
            R = rl;
        if (r == i || r == j || r == last)
            rad[r] = R;
        if (r < last) {
            const float4 w = vel[r];
            sh[2 * r] = pos[r];
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, R);
        }
    }
    __syncthreads();
    return true;
}

// batch_hermite_merge_kernel with per-body radii, for both collision actions: a sibling once more (OWN = 2), so that the
// kernels above stay the code they are.  The same loop.  A body's radius rides in sh[2 r + 1].w: the fills write it there and
// the predictor, which rewrites x, y, z only, leaves it.  With ra.merge a collision is merged as there, radii included;
// without, the system leaves the loop after the step that found it and reports the pair, as batch_hermite_stop_kernel does.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_radii_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                   int *counts, BatchEvolveState *state, int *counters,
                                                                   int max_bodies, BatchEvolveArgs p, BatchStopArgs sa,
                                                                   BatchStopReport *report, BatchMergeArgs ma, BatchRadiiArgs ra)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies, and their radii
    __shared__ int red[16];         // the waves' levels
    __shared__ int red_stop[16];    // the waves' stopping conditions
    __shared__ unsigned long long cold_best;  // the cold paths' words
    __shared__ int cold_escaper;
    int n = uniform_i32(counts[blockIdx.x]);
    if (n <= 0)
        return;
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    const bool frozen = uniform_i32(report[blockIdx.x].reason) != 0;
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (frozen || tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target && !frozen) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    // Registers hold the rows' accelerations and jerks only; positions and velocities stay in the state arrays and the
    // masses and radii in LDS, as in batch_hermite_stop_kernel.
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float *rad = ra.radii + (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, rad[r]);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    int stop = 0;                 // workgroup-uniform: the conditions met at the last evaluation
    int run = 0;
    bool evaluate = !p.have_acc;  // (a0, j0) are to be evaluated at the current state, which the columns hold
    bool choose = !p.have_level;  // the level is to come from the first-step rule
    for (;;) {
        if (evaluate) {
            __syncthreads();
            int found = 0;
            radii_evaluate<RPL, GUARD>(sh, n, tid, T, p.eps2, a, jk, sa, &found);
            stop_publish(red_stop, found, tid);
        }
        if (choose) {  // dt = eta_start |a| / |j|, compared as squares
            EvolveWant want;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
                const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
                evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);
            }
            evolve_publish(red, want, tid);
        }
        __syncthreads();  // every lane is done reading before a prediction rewrites the columns; red[], red_stop[] are complete
        if (choose) {     // never coarser than the tick allows (tick 0 allows every level)
            const EvolveWant want = evolve_collect(red, T);
            const int floor_level = merge_tick_level(tick, p.levels);
            level = want.level > p.levels ? p.levels : want.level;
            level = level < floor_level ? floor_level : level;
            clamped += want.level > p.levels ? 1 : 0;
        }
        if (evaluate)
            stop = stop_collect(red_stop, T);
        for (; tick < p.target && run < p.budget && steps < p.max_steps && !stop; ++run) {
            const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                if (r < n) {  // x, y, z only: the masses and the radii stay
                    const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                    *reinterpret_cast<float3 *>(&sh[2 * r]) =
                        make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                    hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                    *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                        make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                    hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
                }
                renew_f32(a[q]);
                renew_f32(jk[q]);
            }
            __syncthreads();
            int found = 0;
            const EvolveWant mine = radii_evaluate_request<RPL, GUARD>(sh, n, tid, T, p.eps2, pos, vel, a, jk, e, p, sa, &found);
            stop_publish(red_stop, found, tid);
            evolve_publish(red, mine, tid);
            __syncthreads();
            stop = stop_collect(red_stop, T);
            EvolveWant want = evolve_collect(red, T);
            clamped += want.level > p.levels ? 1 : 0;
            want.level = want.level > p.levels ? p.levels : want.level;
            tick += 1ll << (p.levels - level);
            ++steps;
            min_level = level < min_level ? level : min_level;
            max_level = level > max_level ? level : max_level;
            if (want.level > level)
                level = want.level;
            else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
                --level;  // one level, on a tick the coarser step divides
        }
        if (!(stop & kStopCollision) || !ra.merge)
            break;
        // the columns still hold the positions the collision was found at
        if (!radii_merge_absorb(sh, pos, vel, rad, n, tid, T, RPL, p.eps2, tick, ma, cold_best)) {
            stop &= ~kStopCollision;
            break;
        }
        --n;
        evaluate = choose = true;
    }
    int lane = tid;  // the rows' indices formed anew: the offsets of the kernel's top are not carried through the steps for this
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + lane;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        counts[blockIdx.x] = n;
        if (tick < p.target && !stop) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
    if (stop)  // the columns still hold the positions the conditions were examined at
        radii_stop_report(sh, pos, n, lane, T, RPL, p.eps2, sa, stop, tick, &report[blockIdx.x], cold_best, cold_escaper);
}

hipError_t launch_batch_radii(const BatchLaunch &l, const BatchEvolveArgs &p, const BatchStopArgs &sa, const BatchMergeArgs &ma,
                              const BatchRadiiArgs &ra)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_radii_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts, l.state,
                                   l.counters, l.max_bodies, p, sa, l.report, ma, ra);
    });
}

// BatchKernel::stop: batch_hermite_stop_kernel; BatchKernel::adaptive, no stopping conditions: batch_hermite_adaptive_kernel
hipError_t launch_batch_adaptive(const BatchLaunch &l, const BatchEvolveArgs &p, const BatchStopArgs &sa)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        if (l.choice.kernel == BatchKernel::stop)
            return launch_batch_kernel(batch_hermite_stop_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts,
                                       l.state, l.counters, l.max_bodies, p, sa, l.report);
        return launch_batch_kernel(batch_hermite_adaptive_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts,
                                   l.state, l.counters, l.max_bodies, p);
    });
}

hipError_t launch_batch_step(const BatchLaunch &l, bool kdk, int k, float dt, float eps2, int have_acc)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        if (kdk)
            return launch_batch_kernel(batch_step_kernel<rpl(), guard(), true>, l, l.pos, l.vel, l.acc, l.counts, l.max_bodies, k,
                                       dt, eps2, have_acc);
        return launch_batch_kernel(batch_step_kernel<rpl(), guard(), false>, l, l.pos, l.vel, l.acc, l.counts, l.max_bodies, k,
                                   dt, eps2, have_acc);
    });
}

// ---- test particles (include/nbody_batch_massive.h): the first m = min(massive[s], n) bodies of system s are massive, the
// bodies after them are rows like any other and never columns.  Siblings of batch_step_kernel, batch_hermite_kernel and
// batch_hermite_adaptive_kernel, which stay the code they are (OWN = 1 for batch_forces, OWN = 3 for batch_forces_jerks):
// the same kernels with the column loop ending at m, a workgroup-uniform scalar read once.  The row guards stay r < n; the
// workgroup shape and the LDS layout are batch_shape's.  m = 0: no column, every acceleration and jerk is exactly +0.

// batch_step_kernel with the column bound m.  Only the rows r < m are published to LDS: no row reads the others.
template <int RPL, bool GUARD, bool KDK>
__global__ __launch_bounds__(1024) void batch_step_massive_kernel(float4 *pos, float4 *vel, float4 *acc, const int *counts,
                                                                  const int *massive, int max_bodies, int k, float dt,
                                                                  float eps2, int have_acc)
{
    extern __shared__ float4 sp[];  // the massive bodies' positions, at most max_bodies float4
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int mc = massive[blockIdx.x];
    const int m = mc < n ? mc : n;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    float4 x[RPL], v[RPL];
    float ax[RPL], ay[RPL], az[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        ax[q] = ay[q] = az[q] = 0.f;
        if (r < n) {
            x[q] = pos[base + r];
            v[q] = vel[base + r];
            if (r < m)
                sp[r] = x[q];
            if (KDK && have_acc) {
                const float4 a = acc[base + r];
                ax[q] = a.x;
                ay[q] = a.y;
                az[q] = a.z;
            }
        }
    }
    __syncthreads();
    const double h = (double)dt, hh = 0.5 * (double)dt;
    if (KDK && !have_acc) {
        batch_forces<RPL, GUARD, 1>(sp, m, x, eps2, ax, ay, az);
        __syncthreads();  // every lane is done reading before the first drift rewrites the positions
    }
    for (int s = 0; s < k; ++s) {
        if (KDK) {
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                batch_kick(v[q], ax[q], ay[q], az[q], hh);
                batch_drift(x[q], v[q], h);
                const int r = q * T + tid;
                if (r < m)
                    sp[r] = x[q];
            }
            __syncthreads();
            batch_forces<RPL, GUARD, 1>(sp, m, x, eps2, ax, ay, az);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < RPL; ++q)
                batch_kick(v[q], ax[q], ay[q], az[q], hh);
        } else {
            batch_forces<RPL, GUARD, 1>(sp, m, x, eps2, ax, ay, az);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                batch_kick(v[q], ax[q], ay[q], az[q], h);
                batch_drift(x[q], v[q], h);
                const int r = q * T + tid;
                if (r < m)
                    sp[r] = x[q];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            pos[base + r] = x[q];  // .w (the mass word) unchanged
            vel[base + r] = v[q];  // .w unchanged
            if (KDK)
                acc[base + r] = make_float4(ax[q], ay[q], az[q], 0.f);
        }
    }
}

// hermite_evaluate<RPL, GUARD, CORRECT> (without STOP) with the column bound m beside the row bound n: a sibling, so that
// hermite_evaluate stays the code it is for the kernels above.  The same row groups; every row r < n rereads its own
// predicted state from LDS, whether or not it is a column.
template <int RPL, bool GUARD, bool CORRECT>
__device__ __forceinline__ void massive_evaluate(const float4 *sh, int n, int m, int tid, int T, float eps2, float4 (&x)[RPL],
                                                 float3 (&v)[RPL], float3 (&a)[RPL], float3 (&jk)[RPL], const HermiteSteps &t)
{
    constexpr int G = RPL < 2 ? RPL : 2;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {  // xyz only: ds_read_b96
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
            }
        }
        batch_forces_jerks<G, GUARD, false, 3>(sh, m, xp, vp, eps2, a1, j1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i;
            if (CORRECT) {
                hermite_correct(x[q].x, v[q].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, t);
                hermite_correct(x[q].y, v[q].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, t);
                hermite_correct(x[q].z, v[q].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, t);
            }
            a[q] = a1[i];
            jk[q] = j1[i];
        }
    }
}

// hermite_evaluate_request<RPL, GUARD> (without STOP) with the column bound m: a sibling as massive_evaluate is.  Every row
// r < n forms its criterion and votes: test particles count in the time step.
template <int RPL, bool GUARD>
__device__ __forceinline__ EvolveWant massive_evaluate_request(const float4 *sh, int n, int m, int tid, int T, float eps2,
                                                               float4 *pos, float4 *vel, float3 (&a)[RPL], float3 (&jk)[RPL],
                                                               const EvolveSteps &e, const BatchEvolveArgs &p)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    EvolveWant want;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G], x[G], v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = x[i] = v[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
                x[i] = *reinterpret_cast<const float3 *>(&pos[r]);
                v[i] = *reinterpret_cast<const float3 *>(&vel[r]);
            }
        }
        batch_forces_jerks<G, GUARD, false, 3>(sh, m, xp, vp, eps2, a1, j1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            hermite_correct(x[i].x, v[i].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, e.t);
            hermite_correct(x[i].y, v[i].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, e.t);
            hermite_correct(x[i].z, v[i].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, e.t);
            if (r < n) {  // x, y, z only: the mass words and the velocities' w stay as they are
                *reinterpret_cast<float3 *>(&pos[r]) = x[i];
                *reinterpret_cast<float3 *>(&vel[r]) = v[i];
            }
            float3 a0 = a[q], j0 = jk[q];
            renew_f32(a0);  // widened again below, one component at a time: the corrector's fp64 copies end here
            renew_f32(j0);
            renew_f32(a1[i]);
            renew_f32(j1[i]);
            a[q] = a1[i];
            jk[q] = j1[i];
            EvolveNorms s;
            evolve_norms(s, a0.x, a1[i].x, j0.x, j1[i].x, e);
            evolve_norms(s, a0.y, a1[i].y, j0.y, j1[i].y, e);
            evolve_norms(s, a0.z, a1[i].z, j0.z, j1[i].z, e);
            const double num = p.eta * (__builtin_sqrt(s.a1 * s.a2) + s.j1), den = __builtin_sqrt(s.j1 * s.a3) + s.a2;
            evolve_raise(want, r < n, num, den, p);
        }
    }
    return want;
}

// batch_hermite_kernel with the column bound m.  Every row r < n writes its predicted state to LDS: a row reads its own
// back from there.  A test particle's mass word travels through x[q].w and LDS like any other and is read by no column loop.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_massive_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                     const int *counts, const int *massive, int max_bodies,
                                                                     int k, float dt, float eps2, int have_acc)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int mc = massive[blockIdx.x];
    const int m = mc < n ? mc : n;
    const int tid = threadIdx.x, T = blockDim.x;
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    const double h = (double)dt;
    const HermiteSteps t{h, 0.5 * h, h / 3.0, h / 6.0};
    float4 x[RPL];  // {x, y, z, m}
    float3 v[RPL], a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        x[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        v[q] = a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            x[q] = pos[base + r];
            const float4 w = vel[base + r];
            v[q] = make_float3(w.x, w.y, w.z);
            if (have_acc) {
                const float4 a0 = acc[base + r], j0 = jerk[base + r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!have_acc) {  // (a0, j0) at the current state
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                sh[2 * r] = x[q];
                sh[2 * r + 1] = make_float4(v[q].x, v[q].y, v[q].z, 0.f);
            }
        }
        __syncthreads();
        massive_evaluate<RPL, GUARD, false>(sh, n, m, tid, T, eps2, x, v, a, jk, t);
        __syncthreads();  // every lane is done reading before the first prediction rewrites the columns
    }
    for (int s = 0; s < k; ++s) {
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                sh[2 * r] = make_float4(hermite_predict_x(x[q].x, v[q].x, a[q].x, jk[q].x, t),
                                        hermite_predict_x(x[q].y, v[q].y, a[q].y, jk[q].y, t),
                                        hermite_predict_x(x[q].z, v[q].z, a[q].z, jk[q].z, t), x[q].w);
                sh[2 * r + 1] = make_float4(hermite_predict_v(v[q].x, a[q].x, jk[q].x, t),
                                            hermite_predict_v(v[q].y, a[q].y, jk[q].y, t),
                                            hermite_predict_v(v[q].z, a[q].z, jk[q].z, t), 0.f);
            }
            float3 xq = make_float3(x[q].x, x[q].y, x[q].z);
            renew_f32(xq);
            x[q] = make_float4(xq.x, xq.y, xq.z, x[q].w);
            renew_f32(v[q]);
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        massive_evaluate<RPL, GUARD, true>(sh, n, m, tid, T, eps2, x, v, a, jk, t);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            pos[base + r] = x[q];  // .w (the mass word) unchanged
            float *w = reinterpret_cast<float *>(vel + base + r);
            w[0] = v[q].x;  // .w left alone
            w[1] = v[q].y;
            w[2] = v[q].z;
            acc[base + r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[base + r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
}

// batch_hermite_adaptive_kernel with the column bound m: the same loop, the same level rule, every row r < n in the
// criterion.  With m = 0 both the first-step rule and the criterion have a zero denominator (the header's +inf): level 0.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_adaptive_massive_kernel(float4 *pos, float4 *vel, float4 *acc,
                                                                              float4 *jerk, const int *counts,
                                                                              const int *massive, BatchEvolveState *state,
                                                                              int *counters, int max_bodies, BatchEvolveArgs p)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    __shared__ int red[16];         // the waves' levels
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int mc = massive[blockIdx.x];
    const int m = uniform_i32(mc < n ? mc : n);
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    // Registers hold the rows' accelerations and jerks only; positions and velocities stay in the state arrays and the mass
    // words in LDS, as in batch_hermite_adaptive_kernel.
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!p.have_acc) {  // (a0, j0) at the current state, which the columns hold
        __syncthreads();
        const HermiteSteps unused{0.0, 0.0, 0.0, 0.0};
        float4 x4[RPL];  // not used without the corrector
        float3 v3[RPL];
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            x4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            v3[q] = make_float3(0.f, 0.f, 0.f);
        }
        massive_evaluate<RPL, GUARD, false>(sh, n, m, tid, T, p.eps2, x4, v3, a, jk, unused);
    }
    if (!p.have_level) {  // the first step: dt = eta_start |a| / |j|, compared as squares
        EvolveWant want;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
            const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
            evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);  // dt^2 = eta_start^2 |a|^2 / |j|^2
        }
        evolve_publish(red, want, tid);
    }
    __syncthreads();  // every lane is done reading before the first prediction rewrites the columns; red[] is complete
    if (!p.have_level) {
        const EvolveWant want = evolve_collect(red, T);
        level = want.level > p.levels ? p.levels : want.level;
        clamped += want.level > p.levels ? 1 : 0;
    }
    for (int run = 0; tick < p.target && run < p.budget && steps < p.max_steps; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        const EvolveWant mine = massive_evaluate_request<RPL, GUARD>(sh, n, m, tid, T, p.eps2, pos, vel, a, jk, e, p);
        evolve_publish(red, mine, tid);
        __syncthreads();
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick += 1ll << (p.levels - level);
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
}

hipError_t launch_batch_step_massive(const BatchLaunch &l, bool kdk, int k, float dt, float eps2, int have_acc)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        if (kdk)
            return launch_batch_kernel(batch_step_massive_kernel<rpl(), guard(), true>, l, l.pos, l.vel, l.acc, l.counts,
                                       l.massive, l.max_bodies, k, dt, eps2, have_acc);
        return launch_batch_kernel(batch_step_massive_kernel<rpl(), guard(), false>, l, l.pos, l.vel, l.acc, l.counts, l.massive,
                                   l.max_bodies, k, dt, eps2, have_acc);
    });
}

hipError_t launch_batch_hermite_massive(const BatchLaunch &l, int k, float dt, float eps2, int have_acc)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_massive_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts,
                                   l.massive, l.max_bodies, k, dt, eps2, have_acc);
    });
}

hipError_t launch_batch_adaptive_massive(const BatchLaunch &l, const BatchEvolveArgs &p)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_adaptive_massive_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk,
                                   l.counts, l.massive, l.state, l.counters, l.max_bodies, p);
    });
}

// ---- external fields (include/nbody_batch_field.h): a static analytic background next to the pair sum, up to four components
// per system.  The components are workgroup-uniform: one launch reads them once, through uniform_i32, into scalar registers,
// and every kind is chosen by a scalar branch.

// BatchFieldTerm, one component as the kernels take it: nbody_batch_handle.h.
static_assert(sizeof(BatchFieldTerm) == 16 && sizeof(nbody_batch_field_component) == 16, "one dwordx4 per component");

struct BatchField {
    BatchFieldTerm term[NBODY_BATCH_FIELD_MAX_COMPONENTS];
};

__device__ __forceinline__ float uniform_f32(float x) { return __int_as_float(uniform_i32(__float_as_int(x))); }

// The system's components in scalar registers.  `terms` is [n_systems][NBODY_BATCH_FIELD_MAX_COMPONENTS]; components the
// caller did not give are NONE.
__device__ __forceinline__ BatchField field_load(const BatchFieldTerm *terms)
{
    BatchField f;
    terms += (size_t)blockIdx.x * NBODY_BATCH_FIELD_MAX_COMPONENTS;
#pragma unroll
    for (int c = 0; c < NBODY_BATCH_FIELD_MAX_COMPONENTS; ++c) {
        const BatchFieldTerm u = terms[c];
        f.term[c] = BatchFieldTerm{uniform_i32(u.kind), uniform_f32(u.c0), uniform_f32(u.c1), uniform_f32(u.c2)};
    }
    return f;
}

// The three kinds for one row at its predicted state (x, v), added to the row's sums (a, j): the header's operation
// order, to the letter.  Per row, by reading the ISA: PLUMMER 26 VALU + 1 v_rsq_f32, the column interaction's, and 4 more for
// the guard (b is known at run time only); LOG_HALO 20 VALU + 1 v_rcp_f32; MIYAMOTO_NAGAI 32 VALU + 2 v_rsq_f32.
__device__ __forceinline__ void field_plummer(float M, float b2, const float3 &x, const float3 &v, float3 &a, float3 &j)
{
    const float dx = 0.f - x.x, dy = 0.f - x.y, dz = 0.f - x.z;
    const float ex = 0.f - v.x, ey = 0.f - v.y, ez = 0.f - v.z;
    float r2 = __builtin_fmaf(dx, dx, b2);
    r2 = __builtin_fmaf(dy, dy, r2);
    r2 = __builtin_fmaf(dz, dz, r2);
    if (!(b2 > 0.f))  // uniform: b = 0 takes the guard, as a zero-distance pair does
        r2 = guard_r2(r2);
    const float inv = __builtin_amdgcn_rsqf(r2);
    const float inv2 = inv * inv;
    const float s = (M * inv) * inv2;
    const float rv = __builtin_fmaf(dz, ez, __builtin_fmaf(dy, ey, dx * ex));
    const float c = (3.f * rv) * inv2;
    a.x = __builtin_fmaf(dx, s, a.x);
    a.y = __builtin_fmaf(dy, s, a.y);
    a.z = __builtin_fmaf(dz, s, a.z);
    j.x = __builtin_fmaf(__builtin_fmaf(-c, dx, ex), s, j.x);
    j.y = __builtin_fmaf(__builtin_fmaf(-c, dy, ey), s, j.y);
    j.z = __builtin_fmaf(__builtin_fmaf(-c, dz, ez), s, j.z);
}
__device__ __forceinline__ void field_log_halo(float k, float rc2, float wz, const float3 &x, const float3 &v, float3 &a, float3 &j)
{
    const float zw = wz * x.z, vw = wz * v.z;
    const float D = __builtin_fmaf(zw, x.z, __builtin_fmaf(x.y, x.y, __builtin_fmaf(x.x, x.x, rc2)));
    const float hd = __builtin_fmaf(zw, v.z, __builtin_fmaf(x.y, v.y, x.x * v.x));
    const float iD = __builtin_amdgcn_rcpf(D);
    const float g = k * iD;
    const float t = (2.f * hd) * iD;
    a.x = __builtin_fmaf(-g, x.x, a.x);
    a.y = __builtin_fmaf(-g, x.y, a.y);
    a.z = __builtin_fmaf(-g, zw, a.z);
    j.x = __builtin_fmaf(-g, __builtin_fmaf(-t, x.x, v.x), j.x);
    j.y = __builtin_fmaf(-g, __builtin_fmaf(-t, x.y, v.y), j.y);
    j.z = __builtin_fmaf(-g, __builtin_fmaf(-t, zw, vw), j.z);
}
__device__ __forceinline__ void field_miyamoto_nagai(float M, float la, float b2, const float3 &x, const float3 &v, float3 &a,
                                                     float3 &j)
{
    const float s2 = __builtin_fmaf(x.z, x.z, b2);
    const float is = __builtin_amdgcn_rsqf(s2);
    const float s = s2 * is;
    const float A = la + s;
    const float f = A * is;
    const float sd = (x.z * v.z) * is;
    const float fd = -((la * sd) * (is * is));
    const float D = __builtin_fmaf(A, A, __builtin_fmaf(x.y, x.y, x.x * x.x));
    const float hd = __builtin_fmaf(A, sd, __builtin_fmaf(x.y, v.y, x.x * v.x));
    const float iD = __builtin_amdgcn_rsqf(D);
    const float iD2 = iD * iD;
    const float mu = (M * iD) * iD2;
    const float c = (3.f * hd) * iD2;
    const float zf = x.z * f;
    const float zd = __builtin_fmaf(v.z, f, x.z * fd);
    a.x = __builtin_fmaf(-x.x, mu, a.x);
    a.y = __builtin_fmaf(-x.y, mu, a.y);
    a.z = __builtin_fmaf(-zf, mu, a.z);
    j.x = __builtin_fmaf(__builtin_fmaf(c, x.x, -v.x), mu, j.x);
    j.y = __builtin_fmaf(__builtin_fmaf(c, x.y, -v.y), mu, j.y);
    j.z = __builtin_fmaf(__builtin_fmaf(c, zf, -zd), mu, j.z);
}

// The system's components added to the sums of a group's rows, ascending component order; NONE is skipped.
template <int G>
__device__ __forceinline__ void field_add(const BatchField &f, const float3 (&xp)[G], const float3 (&vp)[G], float3 (&a1)[G],
                                          float3 (&j1)[G])
{
#pragma unroll
    for (int c = 0; c < NBODY_BATCH_FIELD_MAX_COMPONENTS; ++c) {
        const BatchFieldTerm &u = f.term[c];
        if (u.kind == NBODY_BATCH_FIELD_PLUMMER) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                field_plummer(u.c0, u.c1, xp[i], vp[i], a1[i], j1[i]);
        } else if (u.kind == NBODY_BATCH_FIELD_LOG_HALO) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                field_log_halo(u.c0, u.c1, u.c2, xp[i], vp[i], a1[i], j1[i]);
        } else if (u.kind == NBODY_BATCH_FIELD_MIYAMOTO_NAGAI) {
#pragma unroll
            for (int i = 0; i < G; ++i)
                field_miyamoto_nagai(u.c0, u.c1, u.c2, xp[i], vp[i], a1[i], j1[i]);
        }
    }
}

// massive_evaluate<RPL, GUARD, false> followed by the field: (a, j) at the state the columns hold, without the corrector.
constexpr int kOwnField = 5;
template <int RPL, bool GUARD>
__device__ __forceinline__ void field_evaluate(const float4 *sh, int n, int m, int tid, int T, float eps2, const BatchField &f,
                                               float3 (&a)[RPL], float3 (&jk)[RPL])
{
    constexpr int G = RPL < 2 ? RPL : 2;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {  // xyz only: ds_read_b96
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
            }
        }
        batch_forces_jerks<G, GUARD, false, kOwnField>(sh, m, xp, vp, eps2, a1, j1);
        field_add<G>(f, xp, vp, a1, j1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            a[g + i] = a1[i];
            jk[g + i] = j1[i];
        }
    }
}

// massive_evaluate_request<RPL, GUARD> with the field added between the column loop and the corrector: the criterion sees
// the field's accelerations and jerks at both ends of the step.
template <int RPL, bool GUARD>
__device__ __forceinline__ EvolveWant field_evaluate_request(const float4 *sh, int n, int m, int tid, int T, float eps2,
                                                             const BatchField &f, float4 *pos, float4 *vel, float3 (&a)[RPL],
                                                             float3 (&jk)[RPL], const EvolveSteps &e, const BatchEvolveArgs &p)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    EvolveWant want;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G], x[G], v[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = x[i] = v[i] = make_float3(0.f, 0.f, 0.f);
            if (r < n) {
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r + 1]);
                x[i] = *reinterpret_cast<const float3 *>(&pos[r]);
                v[i] = *reinterpret_cast<const float3 *>(&vel[r]);
            }
        }
        batch_forces_jerks<G, GUARD, false, kOwnField>(sh, m, xp, vp, eps2, a1, j1);
        field_add<G>(f, xp, vp, a1, j1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            hermite_correct(x[i].x, v[i].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, e.t);
            hermite_correct(x[i].y, v[i].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, e.t);
            hermite_correct(x[i].z, v[i].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, e.t);
            if (r < n) {  // x, y, z only: the mass words and the velocities' w stay as they are
                *reinterpret_cast<float3 *>(&pos[r]) = x[i];
                *reinterpret_cast<float3 *>(&vel[r]) = v[i];
            }
            float3 a0 = a[q], j0 = jk[q];
            renew_f32(a0);  // widened again below, one component at a time: the corrector's fp64 copies end here
            renew_f32(j0);
            renew_f32(a1[i]);
            renew_f32(j1[i]);
            a[q] = a1[i];
            jk[q] = j1[i];
            EvolveNorms s;
            evolve_norms(s, a0.x, a1[i].x, j0.x, j1[i].x, e);
            evolve_norms(s, a0.y, a1[i].y, j0.y, j1[i].y, e);
            evolve_norms(s, a0.z, a1[i].z, j0.z, j1[i].z, e);
            const double num = p.eta * (__builtin_sqrt(s.a1 * s.a2) + s.j1), den = __builtin_sqrt(s.j1 * s.a3) + s.a2;
            evolve_raise(want, r < n, num, den, p);
        }
    }
    return want;
}

// batch_hermite_adaptive_massive_kernel with the field: the same loop, level rule, tick arithmetic, state and counters, the
// same row groups and LDS layout.  massive == nullptr: no massive counts, every body is a column (m = n).  With m = 0 a row's
// accelerations and jerks are the field's alone.
// One row per lane is asked to stay at eight waves per SIMD (64 VGPRs), where the sibling is: the components' scalar registers
// press some of the loop's scalars into lanes of one more vector register otherwise.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(RPL == 1 ? 8 : 4, RPL == 1 ? 8 : 4))) void batch_hermite_field_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                   const int *counts, const int *massive,
                                                                   const BatchFieldTerm *terms, BatchEvolveState *state,
                                                                   int *counters, int max_bodies, BatchEvolveArgs p)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies
    __shared__ int red[16];         // the waves' levels
    const int n = counts[blockIdx.x];
    if (n <= 0)
        return;
    const int mc = massive ? massive[blockIdx.x] : n;
    const int m = uniform_i32(mc < n ? mc : n);
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    const BatchField f = field_load(terms);
    pos += (size_t)blockIdx.x * (size_t)max_bodies;
    vel += (size_t)blockIdx.x * (size_t)max_bodies;
    acc += (size_t)blockIdx.x * (size_t)max_bodies;
    jerk += (size_t)blockIdx.x * (size_t)max_bodies;
    float3 a[RPL], jk[RPL];
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, 0.f);
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!p.have_acc) {  // (a0, j0) at the current state, which the columns hold
        __syncthreads();
        field_evaluate<RPL, GUARD>(sh, n, m, tid, T, p.eps2, f, a, jk);
    }
    if (!p.have_level) {  // the first step: dt = eta_start |a| / |j|, compared as squares
        EvolveWant want;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
            const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
            evolve_raise(want, q * T + tid < n, p.eta_start2 * a2, j2, p);  // dt^2 = eta_start^2 |a|^2 / |j|^2
        }
        evolve_publish(red, want, tid);
    }
    __syncthreads();  // every lane is done reading before the first prediction rewrites the columns; red[] is complete
    if (!p.have_level) {
        const EvolveWant want = evolve_collect(red, T);
        level = want.level > p.levels ? p.levels : want.level;
        clamped += want.level > p.levels ? 1 : 0;
    }
    for (int run = 0; tick < p.target && run < p.budget && steps < p.max_steps; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n) {
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        const EvolveWant mine = field_evaluate_request<RPL, GUARD>(sh, n, m, tid, T, p.eps2, f, pos, vel, a, jk, e, p);
        evolve_publish(red, mine, tid);
        __syncthreads();
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick += 1ll << (p.levels - level);
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
    }
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
}

hipError_t launch_batch_field(const BatchLaunch &l, const BatchEvolveArgs &p)
{
    const int *massive = l.choice.kernel == BatchKernel::adaptive_massive ? l.massive : nullptr;
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_field_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts, massive,
                                   l.field, l.state, l.counters, l.max_bodies, p);
    });
}

// Phi(x_i) per body in fp64 (the header's "Potential"): one thread per slot, 0 beyond the counts.  Not the hot path.
__global__ __launch_bounds__(256) void batch_field_potential_kernel(const float4 *pos, const int *counts,
                                                                    const nbody_batch_field_component *comps, int n_components,
                                                                    int max_bodies, double *phi)
{
    const int s = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= max_bodies)
        return;
    const size_t slot = (size_t)s * (size_t)max_bodies + (size_t)i;
    double sum = 0.0;
    if (i < counts[s]) {
        const float4 xm = pos[slot];
        const double x = (double)xm.x, y = (double)xm.y, z = (double)xm.z;
        for (int c = 0; c < n_components; ++c) {
            const nbody_batch_field_component u = comps[(size_t)s * (size_t)n_components + c];
            const double p0 = (double)u.p[0], p1 = (double)u.p[1], p2 = (double)u.p[2];
            if (u.kind == NBODY_BATCH_FIELD_PLUMMER) {
                const double r2 = x * x + y * y + z * z + p1 * p1;
                sum += r2 > 0.0 ? -p0 / __builtin_sqrt(r2) : 0.0;
            } else if (u.kind == NBODY_BATCH_FIELD_LOG_HALO) {
                sum += 0.5 * (p0 * p0) * log(x * x + y * y + z * z / (p2 * p2) + p1 * p1);
            } else if (u.kind == NBODY_BATCH_FIELD_MIYAMOTO_NAGAI) {
                const double A = p1 + __builtin_sqrt(z * z + p2 * p2);
                sum += -p0 / __builtin_sqrt(x * x + y * y + A * A);
            }
        }
    }
    phi[slot] = sum;
}

// ---- tracer fates (include/nbody_batch_fate.h): massive counts together with a collision radius, radii or an escape radius.
// A test particle that touches a massive body or leaves the escape radius is removed -- frozen, with a fate -- and its system
// carries on; a collision among the massive bodies or a massive escaper stops the system as batch_hermite_stop_kernel does.

// BatchFateArgs, per launch; one kernel serves both kinds of radius: nbody_batch_launch.h.
constexpr int kFateHit = 1, kFateEscaped = 2;

// The cold path of a tracer that is removed, by its own lane only: the massive body of smallest r^2 + eps^2 among those
// within the pair's threshold (ties to the smallest index: the scan ascends and replaces on less-than only), with the
// evaluation's own chain on the columns LDS still holds, the separation and the relative speed at the row's predicted state,
// which it rereads from LDS with its radius: nothing is kept alive across the corrector for this.
__device__ __forceinline__ void fate_record(const float4 *sh, int m, int r, float eps2, bool hit, long long tick,
                                            const BatchFateArgs &fa)
{
    int target = -1;
    float sep = 0.f, speed = 0.f;
    if (hit) {
        const float4 xp = sh[2 * r], vp = sh[2 * r + 1];
        const float rr = vp.w;
        float best = __builtin_inff();
#pragma unroll 1
        for (int j = 0; j < m; ++j) {
            const float4 pj = sh[2 * j];
            const float dx = pj.x - xp.x, dy = pj.y - xp.y, dz = pj.z - xp.z;
            float r2 = __builtin_fmaf(dx, dx, eps2);
            r2 = __builtin_fmaf(dy, dy, r2);
            r2 = __builtin_fmaf(dz, dz, r2);
            if (r2 <= radii_threshold(rr, sh[2 * j + 1].w, eps2) && r2 < best) {
                best = r2;
                target = j;
            }
        }
        if (target >= 0) {
            const float4 pj = sh[2 * target], wj = sh[2 * target + 1];
            const float dx = pj.x - xp.x, dy = pj.y - xp.y, dz = pj.z - xp.z;
            const float ex = wj.x - vp.x, ey = wj.y - vp.y, ez = wj.z - vp.z;
            sep = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
            speed = __builtin_sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
        }
    }
    fa.fates[r] = BatchFate{tick, hit ? kFateHit : kFateEscaped, target, sep, speed};
}

// What one row found, after its group's column loop: the verdict per row group is (near2 & massive rows) | (near1 & tracer
// rows), both masks of the valid, live rows only -- a massive row walks its own column, a tracer row has none.  A massive
// row that collides or escapes sets its bit in *found (the system stops); for a tracer row that hits or escapes the result is
// kFateHit or kFateEscaped (it is dead from here on), otherwise 0.  x: the positions of the escape test.
__device__ __forceinline__ unsigned fate_examine(int m, int r, bool alive, unsigned long long near1, unsigned long long near2,
                                                 const float3 &x, const BatchStopArgs &sa, const BatchFateArgs &fa, int *found)
{
    const unsigned long long massive = __ballot(alive && r < m), tracer = __ballot(alive && r >= m);
    const unsigned long long touch = fa.collide ? (near2 & massive) | (near1 & tracer) : 0ull;
    const float d2 = __builtin_fmaf(x.z, x.z, __builtin_fmaf(x.y, x.y, x.x * x.x));
    const bool out = alive && d2 > sa.re2;
    *found |= ((touch & massive) != 0 ? kStopCollision : 0) | (__any(out && r < m) ? kStopEscape : 0);
    const bool hit = __builtin_amdgcn_inverse_ballot_w64(touch & tracer);  // the scalar mask as the lanes' condition
    return hit ? kFateHit : out && r >= m ? kFateEscaped : 0u;
}

// The rows' fates in one register per lane: bit q, row q is dead; bit 8 + q, it hit in the evaluation just made; bit 16 + q,
// it escaped there.  fate_note sets the bits of a row found; fate_flush, after the evaluation and before the barrier that
// precedes the next prediction, records the rows found and clears their upper bits: the cold path is kept out of the rows'
// loop, where the corrector needs every register.
__device__ __forceinline__ void fate_note(unsigned &dead, int q, unsigned what)
{
    dead |= what ? (1u | (what == kFateHit ? 1u << 8 : 1u << 16)) << q : 0u;
}
__device__ __forceinline__ void fate_flush(const float4 *sh, int m, int tid, int T, int rpl, float eps2, long long tick,
                                           const BatchFateArgs &fa, unsigned &dead)
{
    if (dead >> 8) {
        asm volatile("" : "+v"(tid));  // the rows' addresses are formed here, not carried through the steps from the kernel's top
        for (int q = 0; q < rpl; ++q)
            if ((dead >> (8 + q)) & 0x101u)
                fate_record(sh, m, q * T + tid, eps2, (dead >> (8 + q)) & 1u, tick, fa);
        dead &= 0xffu;
    }
}

// radii_evaluate with the column bound m and the rows' fates: a sibling (OWN = kOwnFate).  `dead` holds a bit per row of
// the lane; a dead row rides through the column loop and its result is dropped.
template <int RPL, bool GUARD>
__device__ __forceinline__ void fate_evaluate(const float4 *sh, int n, int m, int tid, int T, float eps2, float3 (&a)[RPL],
                                              float3 (&jk)[RPL], const BatchStopArgs &sa, const BatchFateArgs &fa,
                                              unsigned &dead, int *found)
{
    constexpr int G = RPL < 2 ? RPL : 2;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G];
        float rr[G];
        unsigned long long near1[G], near2[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = make_float3(0.f, 0.f, 0.f);
            rr[i] = 0.f;
            if (r < n) {
                const float4 w = sh[2 * r + 1];
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = make_float3(w.x, w.y, w.z);
                rr[i] = w.w;
            }
        }
        batch_forces_jerks<G, GUARD, true, kOwnFate, true>(sh, m, xp, vp, eps2, a1, j1, 0.f, near2, rr, near1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            const bool alive = r < n && !((dead >> q) & 1u);
            fate_note(dead, q, fate_examine(m, r, alive, near1[i], near2[i], xp[i], sa, fa, found));
            a[q] = a1[i];
            jk[q] = j1[i];
        }
    }
}

// radii_evaluate_request with the column bound m and the rows' fates.  A row that was dead before the step is neither
// corrected nor written and does not vote; a row found in this step is corrected and written, and does not vote.
template <int RPL, bool GUARD>
__device__ __forceinline__ EvolveWant fate_evaluate_request(const float4 *sh, int n, int m, int tid, int T, float eps2,
                                                            float4 *pos, float4 *vel, float3 (&a)[RPL], float3 (&jk)[RPL],
                                                            const EvolveSteps &e, const BatchEvolveArgs &p,
                                                            const BatchStopArgs &sa, const BatchFateArgs &fa, unsigned &dead,
                                                            int *found)
{
    constexpr int G = RPL < 2 ? RPL : 2;
    EvolveWant want;
#pragma unroll
    for (int g = 0; g < RPL; g += G) {
        float3 xp[G], vp[G], a1[G], j1[G], x[G], v[G];
        float rr[G];
        unsigned long long near1[G], near2[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int r = (g + i) * T + tid;
            xp[i] = vp[i] = x[i] = v[i] = make_float3(0.f, 0.f, 0.f);
            rr[i] = 0.f;
            if (r < n) {
                const float4 w = sh[2 * r + 1];
                xp[i] = *reinterpret_cast<const float3 *>(&sh[2 * r]);
                vp[i] = make_float3(w.x, w.y, w.z);
                rr[i] = w.w;
                x[i] = *reinterpret_cast<const float3 *>(&pos[r]);
                v[i] = *reinterpret_cast<const float3 *>(&vel[r]);
            }
        }
        batch_forces_jerks<G, GUARD, true, kOwnFate, true>(sh, m, xp, vp, eps2, a1, j1, 0.f, near2, rr, near1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int q = g + i, r = q * T + tid;
            const bool alive = r < n && !((dead >> q) & 1u);
            hermite_correct(x[i].x, v[i].x, a[q].x, a1[i].x, jk[q].x, j1[i].x, e.t);
            hermite_correct(x[i].y, v[i].y, a[q].y, a1[i].y, jk[q].y, j1[i].y, e.t);
            hermite_correct(x[i].z, v[i].z, a[q].z, a1[i].z, jk[q].z, j1[i].z, e.t);
            const unsigned gone = fate_examine(m, r, alive, near1[i], near2[i], x[i], sa, fa, found);
            fate_note(dead, q, gone);
            if (alive) {  // x, y, z only: the mass words and the velocities' w stay as they are
                *reinterpret_cast<float3 *>(&pos[r]) = x[i];
                *reinterpret_cast<float3 *>(&vel[r]) = v[i];
            }
            float3 a0 = a[q], j0 = jk[q];
            renew_f32(a0);  // widened again below, one component at a time: the corrector's fp64 copies end here
            renew_f32(j0);
            renew_f32(a1[i]);
            renew_f32(j1[i]);
            a[q] = a1[i];
            jk[q] = j1[i];
            EvolveNorms s;
            evolve_norms(s, a0.x, a1[i].x, j0.x, j1[i].x, e);
            evolve_norms(s, a0.y, a1[i].y, j0.y, j1[i].y, e);
            evolve_norms(s, a0.z, a1[i].z, j0.z, j1[i].z, e);
            const double num = p.eta * (__builtin_sqrt(s.a1 * s.a2) + s.j1), den = __builtin_sqrt(s.j1 * s.a3) + s.a2;
            evolve_raise(want, alive && !gone, num, den, p);
        }
    }
    return want;
}

// batch_hermite_adaptive_massive_kernel with the conditions of batch_hermite_stop_kernel / batch_hermite_radii_kernel and the
// tracers' fates: a sibling once more, so that those stay the code they are.  The same loop, LDS layout and workgroup shapes.
// A body's radius rides in sh[2 r + 1].w as in batch_hermite_radii_kernel.  Dead rows are known from the fate array, read at
// the launch's start, and kept as a bit per row in one register; they are not predicted, so their columns -- which nobody
// reads: they lie beyond m -- and their own predicted state stay the frozen state.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_fate_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                  const int *counts, const int *massive, BatchEvolveState *state,
                                                                  int *counters, int max_bodies, BatchEvolveArgs p,
                                                                  BatchStopArgs sa, BatchStopReport *report, BatchFateArgs fa)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies, and their radii
    __shared__ int red[16];         // the waves' levels
    __shared__ int red_stop[16];    // the waves' stopping conditions (massive rows only)
    __shared__ unsigned long long cold_best;  // the cold path's words
    __shared__ int cold_escaper;
    const int n = uniform_i32(counts[blockIdx.x]);
    if (n <= 0)
        return;
    const int mc = massive[blockIdx.x];
    const int m = uniform_i32(mc < n ? mc : n);
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    const bool frozen = uniform_i32(report[blockIdx.x].reason) != 0;
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (frozen || tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target && !frozen) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    pos += base;
    vel += base;
    acc += base;
    jerk += base;
    fa.fates += base;
    float3 a[RPL], jk[RPL];
    unsigned dead = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, fa.radii ? fa.radii[base + r] : fa.half_rc);
            dead |= fa.fates[r].fate != 0 ? 1u << q : 0u;
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    if (!p.have_acc) {  // (a0, j0) at the current state, which the columns hold
        __syncthreads();
        int found = 0;
        fate_evaluate<RPL, GUARD>(sh, n, m, tid, T, p.eps2, a, jk, sa, fa, dead, &found);
        fate_flush(sh, m, tid, T, RPL, p.eps2, tick, fa, dead);
        stop_publish(red_stop, found, tid);
    }
    if (!p.have_level) {  // the first step: dt = eta_start |a| / |j|, compared as squares; dead rows do not vote
        EvolveWant want;
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
            const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
            evolve_raise(want, q * T + tid < n && !((dead >> q) & 1u), p.eta_start2 * a2, j2, p);
        }
        evolve_publish(red, want, tid);
    }
    __syncthreads();  // every lane is done reading before the first prediction rewrites the columns; red[], red_stop[] are complete
    if (!p.have_level) {
        const EvolveWant want = evolve_collect(red, T);
        level = want.level > p.levels ? p.levels : want.level;
        clamped += want.level > p.levels ? 1 : 0;
    }
    int stop = 0;  // workgroup-uniform: the conditions the massive bodies met, which end the loop
    if (!p.have_acc)
        stop = stop_collect(red_stop, T);
    for (int run = 0; tick < p.target && run < p.budget && steps < p.max_steps && !stop; ++run) {
        const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
        for (int q = 0; q < RPL; ++q) {
            const int r = q * T + tid;
            if (r < n && !((dead >> q) & 1u)) {  // x, y, z only: the mass words and the radii stay
                const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                *reinterpret_cast<float3 *>(&sh[2 * r]) =
                    make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                    make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
            }
            renew_f32(a[q]);
            renew_f32(jk[q]);
        }
        __syncthreads();
        int found = 0;
        const long long after = tick + (1ll << (p.levels - level));  // the tick of a fate, as of a stop: the step's end
        const EvolveWant mine = fate_evaluate_request<RPL, GUARD>(sh, n, m, tid, T, p.eps2, pos, vel, a, jk, e, p, sa, fa, dead, &found);
        fate_flush(sh, m, tid, T, RPL, p.eps2, after, fa, dead);
        stop_publish(red_stop, found, tid);
        evolve_publish(red, mine, tid);
        __syncthreads();
        stop = stop_collect(red_stop, T);
        EvolveWant want = evolve_collect(red, T);
        clamped += want.level > p.levels ? 1 : 0;
        want.level = want.level > p.levels ? p.levels : want.level;
        tick = after;
        ++steps;
        min_level = level < min_level ? level : min_level;
        max_level = level > max_level ? level : max_level;
        if (want.level > level)
            level = want.level;
        else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
            --level;  // one level, on a tick the coarser step divides
    }
    int lane = tid;  // the rows' indices formed anew, as in batch_hermite_radii_kernel
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + lane;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target && !stop) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
    if (stop)  // among the massive bodies: the columns still hold the positions the conditions were examined at
        radii_stop_report(sh, pos, m, lane, T, RPL, p.eps2, sa, stop, tick, &report[blockIdx.x], cold_best, cold_escaper);
}

hipError_t launch_batch_fate(const BatchLaunch &l, const BatchEvolveArgs &p, const BatchStopArgs &sa, const BatchFateArgs &fa)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_fate_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts, l.massive,
                                   l.state, l.counters, l.max_bodies, p, sa, l.report, fa);
    });
}

// ---- accreting tracers (include/nbody_batch_accrete.h): a tracer that hits a massive body gives it its mass word.

// BatchAccreteArgs, per launch what each tracer gave and the systems' accretions: nbody_batch_launch.h.
constexpr int kFoundHit = 4;        // beside kStopCollision | kStopEscape in the waves' findings: a tracer hit at this evaluation
constexpr int kAccreteWords = NBODY_BATCH_MAX_BODIES / 32;  // a bit per row

// The rows of this lane that hit at the evaluation just made (bits 8 + q of `dead`, before fate_flush clears them) into the
// workgroup's bit map.  Cold: entered by a lane that found one.
__device__ __forceinline__ void accrete_mark(unsigned *hitmap, unsigned dead, int tid, int T, int rpl)
{
    asm volatile("" : "+v"(tid));
    for (int q = 0; q < rpl; ++q)
        if ((dead >> (8 + q)) & 1u) {
            const int r = q * T + tid;
            atomicOr(&hitmap[r >> 5], 1u << (r & 31));
        }
}

// The cold path of a system whose tracers hit and which did not stop (workgroup-uniform), after fate_flush and a barrier:
// lane 0 walks the bit map in ascending row index and merges each tracer that carries mass onto the target its fate names,
// in the state arrays and the radii array -- nbody_batch_merge.h's arithmetic, the target the survivor -- and writes given
// and the counter; it clears the map as it goes.  After a barrier, when a mass moved, the columns are refilled from the
// current state and radii as merge_absorb refills them, and a last barrier completes them.  Returns whether a mass moved,
// workgroup-uniform: if none did nothing was written and the columns are untouched.
__device__ __forceinline__ bool accrete_absorb(float4 *sh, float4 *pos, float4 *vel, float *rad, int n, int tid, int T, int rpl,
                                               const BatchFateArgs &fa, const BatchAccreteArgs &aa, size_t base,
                                               unsigned *hitmap, int &moved)
{
    asm volatile("" : "+v"(tid));  // the rows' addresses are formed here, not carried through the steps from the kernel's top
    if (tid == 0) {
        int count = 0;
        for (int w = 0; w < (n + 31) >> 5; ++w) {
            unsigned bits = hitmap[w];
            hitmap[w] = 0u;
            while (bits) {
                const int i = (w << 5) + __builtin_ctz(bits);
                bits &= bits - 1u;
                const int t = fa.fates[i].target;
                const float4 xi = pos[i];
                if (xi.w == 0.f || t < 0 || i >= n)  // nothing to give: the tracer is REMOVE's
                    continue;
                const float4 xt = pos[t], vt = vel[t], vi = vel[i];
                const double M = (double)xt.w + (double)xi.w;
                pos[t] = make_float4(merge_mean(xt.w, xt.x, xi.w, xi.x, M), merge_mean(xt.w, xt.y, xi.w, xi.y, M),
                                     merge_mean(xt.w, xt.z, xi.w, xi.z, M), xt.w + xi.w);
                vel[t] = make_float4(merge_mean(xt.w, vt.x, xi.w, vi.x, M), merge_mean(xt.w, vt.y, xi.w, vi.y, M),
                                     merge_mean(xt.w, vt.z, xi.w, vi.z, M), vt.w);
                pos[i].w = 0.f;
                if (rad)
                    rad[t] = merge_radius(rad[t], rad[i]);
                aa.given[base + i] = xi.w;
                ++count;
            }
        }
        if (count) {
            int sys = blockIdx.x;  // formed here, as in merge_absorb
            asm volatile("" : "+s"(sys));
            aa.accretions[sys] += count;
        }
        moved = count;
    }
    __syncthreads();  // the merged state is in the arrays, and every lane is done with the columns
    if (!uniform_i32(moved))
        return false;
    for (int q = 0; q < rpl; ++q) {
        const int r = q * T + tid;
        if (r < n) {
            const float4 w = vel[r];
            sh[2 * r] = pos[r];
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, rad ? rad[r] : fa.half_rc);
        }
    }
    __syncthreads();
    return true;
}

// batch_hermite_fate_kernel with the hit action ACCRETE of include/nbody_batch_accrete.h: a sibling again, so that the fate
// kernel stays the code it is.  The step is the fate kernel's -- the same column loop, LDS layout and workgroup shapes -- and
// the loop is batch_hermite_merge_kernel's: the evaluation at the current state and the first-step rule are one block that
// the outer loop enters again after an accretion.  A tracer hit at an evaluation sets kFoundHit beside the stopping
// conditions; when the massive bodies met none, accrete_absorb follows.  Launched only while collisions are watched.
template <int RPL, bool GUARD>
__global__ __launch_bounds__(1024) void batch_hermite_accrete_kernel(float4 *pos, float4 *vel, float4 *acc, float4 *jerk,
                                                                     const int *counts, const int *massive, BatchEvolveState *state,
                                                                     int *counters, int max_bodies, BatchEvolveArgs p,
                                                                     BatchStopArgs sa, BatchStopReport *report, BatchFateArgs fa,
                                                                     BatchAccreteArgs aa)
{
    extern __shared__ float4 sh[];  // 2 x max_bodies float4: the predicted state of the system's bodies, and their radii
    __shared__ int red[16];         // the waves' levels
    __shared__ int red_stop[16];    // the waves' stopping conditions (massive rows only) and kFoundHit
    __shared__ unsigned long long cold_best;  // the cold paths' words
    __shared__ int cold_escaper;
    __shared__ int cold_moved;
    __shared__ unsigned hitmap[kAccreteWords];  // the rows hit at the evaluation just made
    const int n = uniform_i32(counts[blockIdx.x]);
    if (n <= 0)
        return;
    const int mc = massive[blockIdx.x];
    const int m = uniform_i32(mc < n ? mc : n);
    const int tid = threadIdx.x, T = blockDim.x;
    const BatchEvolveState st0 = state[blockIdx.x];
    const bool frozen = uniform_i32(report[blockIdx.x].reason) != 0;
    long long tick = p.reset_tick ? 0 : uniform_i64(st0.tick);
    long long steps = p.new_call ? 0 : uniform_i64(st0.steps), clamped = p.new_call ? 0 : uniform_i64(st0.clamped);
    int level = uniform_i32(st0.level);
    int min_level = p.new_call ? kEvolveNoLevel : uniform_i32(st0.min_level);
    int max_level = p.new_call ? -1 : uniform_i32(st0.max_level);
    if (frozen || tick >= p.target || steps >= p.max_steps) {  // nothing to do in this launch
        if (tid == 0) {
            if (p.new_call)
                state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
            if (tick < p.target && !frozen) {
                atomicAdd(&counters[0], 1);
                atomicAdd(&counters[1], 1);
            }
        }
        return;
    }
    const size_t base = (size_t)blockIdx.x * (size_t)max_bodies;
    pos += base;
    vel += base;
    acc += base;
    jerk += base;
    fa.fates += base;
    for (int w = tid; w < kAccreteWords; w += T)  // a barrier lies before the first evaluation's marks
        hitmap[w] = 0u;
    float3 a[RPL], jk[RPL];
    unsigned dead = 0;
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + tid;
        a[q] = jk[q] = make_float3(0.f, 0.f, 0.f);
        if (r < n) {
            const float4 xm = pos[r], w = vel[r];
            sh[2 * r] = xm;
            sh[2 * r + 1] = make_float4(w.x, w.y, w.z, fa.radii ? fa.radii[base + r] : fa.half_rc);
            dead |= fa.fates[r].fate != 0 ? 1u << q : 0u;
            if (p.have_acc) {
                const float4 a0 = acc[r], j0 = jerk[r];
                a[q] = make_float3(a0.x, a0.y, a0.z);
                jk[q] = make_float3(j0.x, j0.y, j0.z);
            }
        }
    }
    int stop = 0;                 // workgroup-uniform: what the last evaluation found, kFoundHit included
    int run = 0;
    bool evaluate = !p.have_acc;  // (a0, j0) are to be evaluated at the current state, which the columns hold
    bool choose = !p.have_level;  // the level is to come from the first-step rule
    // The evaluation at the current state and the first-step rule, then the steps until the target, the budget, max_steps, a
    // condition or a hit; after a hit the accretion, and -- if a mass moved -- the same again.
    for (;;) {
        if (evaluate) {
            __syncthreads();
            int found = 0;
            fate_evaluate<RPL, GUARD>(sh, n, m, tid, T, p.eps2, a, jk, sa, fa, dead, &found);
            if ((dead >> 8) & 0xffu)
                accrete_mark(hitmap, dead, tid, T, RPL);
            found |= __any((dead >> 8) & 0xffu) ? kFoundHit : 0;  // wave-uniform, as the stop bits: lane 0 publishes
            fate_flush(sh, m, tid, T, RPL, p.eps2, tick, fa, dead);
            stop_publish(red_stop, found, tid);
        }
        if (choose) {  // dt = eta_start |a| / |j|, compared as squares; dead rows do not vote
            EvolveWant want;
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const double a2 = (double)a[q].x * (double)a[q].x + (double)a[q].y * (double)a[q].y + (double)a[q].z * (double)a[q].z;
                const double j2 = (double)jk[q].x * (double)jk[q].x + (double)jk[q].y * (double)jk[q].y + (double)jk[q].z * (double)jk[q].z;
                evolve_raise(want, q * T + tid < n && !((dead >> q) & 1u), p.eta_start2 * a2, j2, p);
            }
            evolve_publish(red, want, tid);
        }
        __syncthreads();  // every lane is done reading before a prediction rewrites the columns; red[], red_stop[] are complete
        if (choose) {     // never coarser than the tick allows (tick 0 allows every level)
            const EvolveWant want = evolve_collect(red, T);
            const int floor_level = merge_tick_level(tick, p.levels);
            level = want.level > p.levels ? p.levels : want.level;
            level = level < floor_level ? floor_level : level;
            clamped += want.level > p.levels ? 1 : 0;
        }
        if (evaluate)
            stop = stop_collect(red_stop, T);
        for (; tick < p.target && run < p.budget && steps < p.max_steps && !stop; ++run) {
            const EvolveSteps e = evolve_steps(p, level);
#pragma unroll
            for (int q = 0; q < RPL; ++q) {
                const int r = q * T + tid;
                if (r < n && !((dead >> q) & 1u)) {  // x, y, z only: the mass words and the radii stay
                    const float3 x = *reinterpret_cast<const float3 *>(&pos[r]), v = *reinterpret_cast<const float3 *>(&vel[r]);
                    *reinterpret_cast<float3 *>(&sh[2 * r]) =
                        make_float3(hermite_predict_x(x.x, v.x, a[q].x, jk[q].x, e.t), hermite_predict_x(x.y, v.y, a[q].y, jk[q].y, e.t),
                                    hermite_predict_x(x.z, v.z, a[q].z, jk[q].z, e.t));
                    *reinterpret_cast<float3 *>(&sh[2 * r + 1]) =
                        make_float3(hermite_predict_v(v.x, a[q].x, jk[q].x, e.t), hermite_predict_v(v.y, a[q].y, jk[q].y, e.t),
                                    hermite_predict_v(v.z, a[q].z, jk[q].z, e.t));
                }
                renew_f32(a[q]);
                renew_f32(jk[q]);
            }
            __syncthreads();
            int found = 0;
            const long long after = tick + (1ll << (p.levels - level));  // the tick of a fate, as of a stop: the step's end
            const EvolveWant mine = fate_evaluate_request<RPL, GUARD>(sh, n, m, tid, T, p.eps2, pos, vel, a, jk, e, p, sa, fa, dead, &found);
            if ((dead >> 8) & 0xffu)
                accrete_mark(hitmap, dead, tid, T, RPL);
            found |= __any((dead >> 8) & 0xffu) ? kFoundHit : 0;  // wave-uniform, as the stop bits: lane 0 publishes
            fate_flush(sh, m, tid, T, RPL, p.eps2, after, fa, dead);
            stop_publish(red_stop, found, tid);
            evolve_publish(red, mine, tid);
            __syncthreads();
            stop = stop_collect(red_stop, T);
            EvolveWant want = evolve_collect(red, T);
            clamped += want.level > p.levels ? 1 : 0;
            want.level = want.level > p.levels ? p.levels : want.level;
            tick = after;
            ++steps;
            min_level = level < min_level ? level : min_level;
            max_level = level > max_level ? level : max_level;
            if (want.level > level)
                level = want.level;
            else if (want.level < level && (tick & ((2ll << (p.levels - level)) - 1)) == 0)
                --level;  // one level, on a tick the coarser step divides
        }
        if (stop != kFoundHit)  // nothing found, or the massive bodies met a condition: a step that stops accretes nothing
            break;
        stop = 0;
        // every lane's corrected state and the fates of this evaluation lie before the last barrier
        evaluate = choose = accrete_absorb(sh, pos, vel, fa.radii ? fa.radii + base : nullptr, n, tid, T, RPL, fa, aa, base, hitmap,
                                           cold_moved);
    }
    stop &= kStopCollision | kStopEscape;
    int lane = tid;  // the rows' indices formed anew, as in batch_hermite_radii_kernel
    asm volatile("" : "+v"(lane));
#pragma unroll
    for (int q = 0; q < RPL; ++q) {
        const int r = q * T + lane;
        if (r < n) {
            acc[r] = make_float4(a[q].x, a[q].y, a[q].z, 0.f);
            jerk[r] = make_float4(jk[q].x, jk[q].y, jk[q].z, 0.f);
        }
    }
    if (tid == 0) {
        state[blockIdx.x] = BatchEvolveState{tick, steps, clamped, level, min_level, max_level, 0};
        if (tick < p.target && !stop) {
            atomicAdd(&counters[0], 1);
            if (steps >= p.max_steps)
                atomicAdd(&counters[1], 1);
        }
    }
    if (stop)  // among the massive bodies: the columns still hold the positions the conditions were examined at
        radii_stop_report(sh, pos, m, lane, T, RPL, p.eps2, sa, stop, tick, &report[blockIdx.x], cold_best, cold_escaper);
}

hipError_t launch_batch_accrete(const BatchLaunch &l, const BatchEvolveArgs &p, const BatchStopArgs &sa, const BatchFateArgs &fa,
                                const BatchAccreteArgs &aa)
{
    return with_shape(l.choice.rpl, l.choice.guard, [&](auto rpl, auto guard) {
        return launch_batch_kernel(batch_hermite_accrete_kernel<rpl(), guard()>, l, l.pos, l.vel, l.acc, l.jerk, l.counts,
                                   l.massive, l.state, l.counters, l.max_bodies, p, sa, l.report, fa, aa);
    });
}

}  // namespace

// ---- the entry points (nbody_batch_launch.h) -------------------------------------------------------------------------------

hipError_t launch_batch_evolve(const BatchLaunch &l, const BatchEvolveLaunch &a)
{
    if (l.choice.field)  // nbody_batch_field.h: the two families without conditions, through their sibling with the field
        return l.choice.kernel == BatchKernel::adaptive_massive || l.choice.kernel == BatchKernel::adaptive
                   ? launch_batch_field(l, a.p)
                   : hipErrorInvalidValue;
    switch (l.choice.kernel) {
    case BatchKernel::fate:  // nbody_batch_accrete.h: the accreting sibling where the choice says so
        return l.choice.accrete ? launch_batch_accrete(l, a.p, a.sa, a.fa, a.aa) : launch_batch_fate(l, a.p, a.sa, a.fa);
    case BatchKernel::radii: return launch_batch_radii(l, a.p, a.sa, a.ma, a.ra);
    case BatchKernel::adaptive_massive: return launch_batch_adaptive_massive(l, a.p);
    case BatchKernel::merge: return launch_batch_merge(l, a.p, a.sa, a.ma);
    case BatchKernel::stop:
    case BatchKernel::adaptive: return launch_batch_adaptive(l, a.p, a.sa);
    default: return hipErrorInvalidValue;  // a fixed-step family: batch_evolve_choice names none
    }
}

hipError_t launch_batch_steps(const BatchLaunch &l, bool kdk, int run, float dt, float eps2, bool acc_valid)
{
    switch (l.choice.kernel) {
    case BatchKernel::hermite_massive: return launch_batch_hermite_massive(l, run, dt, eps2, acc_valid ? 1 : 0);
    case BatchKernel::hermite: return launch_batch_hermite(l, run, dt, eps2, acc_valid ? 1 : 0);
    case BatchKernel::step_massive: return launch_batch_step_massive(l, kdk, run, dt, eps2, kdk && acc_valid ? 1 : 0);
    case BatchKernel::step: return launch_batch_step(l, kdk, run, dt, eps2, kdk && acc_valid ? 1 : 0);
    default: return hipErrorInvalidValue;  // an evolve family: batch_step_choice names none
    }
}

// One thread per slot, a row of workgroups per system.
hipError_t launch_batch_field_potential(const float4 *pos, const int *counts, const nbody_batch_field_component *comps,
                                        int n_components, int n_systems, int max_bodies, double *phi, hipStream_t stream)
{
    hipLaunchKernelGGL(batch_field_potential_kernel, dim3((unsigned)((max_bodies + 255) / 256), (unsigned)n_systems), dim3(256), 0,
                       stream, pos, counts, comps, n_components, max_bodies, phi);
    return hipGetLastError();
}

}  // namespace nbody
