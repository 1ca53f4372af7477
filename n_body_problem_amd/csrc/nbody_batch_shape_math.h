// nbody_batch_shape_math.h -- the arithmetic of nbody_batch_shape (include/nbody_batch_shape.h) that needs no GPU: the three
// records, the words of one body in the frame, r2e and the member decision, the addends of the tensor and of the final sums,
// the step of one lane over one body, the level-2 sum over the block partials, the cyclic Jacobi decomposition with its sort
// and signs, the update of the state with the convergence test, the whole iteration of one aperture with its final walk, and
// the system summary.  Plain C++17 without HIP, fp64 with +, -, x, / and sqrt alone: batch_shape_kernel
// (nbody_batch_analysis.hip) calls these with the image in LDS and one lane per block of 64 bodies, and a stand-alone driver
// (tests/batch_shape_driver.cpp) runs whole systems through the same functions, lane by lane for any workgroup shape, on the
// CPU, where tests/test_batch_shape_cpu.py compares every byte with tests/hermite_shape_ref.py.  Nothing here may be
// contracted: the build passes -ffp-contract=off.  Internal; the public surface is include/nbody_batch_shape.h.
#pragma once

#include "nbody_batch_surface_math.h"

namespace nbody {

constexpr int kShapeMaxApertures = 8;  // NBODY_BATCH_SHAPE_MAX_APERTURES
constexpr int kShapeConverged = 0, kShapeMax = 1, kShapeFew = 2, kShapeDegenerate = 3;  // NBODY_BATCH_SHAPE_CONVERGED ...
constexpr int kShapeMaxIterations = 64, kShapeLeastMembers = 4;
constexpr int kShapeBlock = 64;         // the bodies of one level-1 partial
constexpr int kShapeJacobiSweeps = 16;  // the most sweeps of one decomposition

// nbody_batch_shape_aperture's layout (nbody_batch_analysis.hip asserts it): 256 bytes.
struct BatchShapeAperture {
    int status, iterations;
    long long count;
    double radius, inner, q, s, change;
    double eigenvalues[3], axes[9];
    double weight, D[3], M[6], L[3];
};

// nbody_batch_shape_system's layout (nbody_batch_analysis.hip asserts it): 80 bytes.
struct BatchShapeSystem {
    int selected, unmeasured, apertures, reduced, converged, reserved;
    double total_weight, centre[3], velocity[3];
};

// nbody_batch_shape_body's layout (nbody_batch_analysis.hip asserts it): 8 bytes.
struct BatchShapeBody {
    unsigned inside;
    int reserved;
};

// ---- Apertures and frame -----------------------------------------------------------------------------------------------------
constexpr double kShapeLargest = __DBL_MAX__;

// A finite number: false for NaN and for either infinity, like radial_finite.
NBODY_HD inline bool shape_finite(double v) { return __builtin_fabs(v) <= kShapeLargest; }

// R R or Rin Rin: one fp64 product; a product that overflows becomes the largest finite value, as radial_edge2 does.
NBODY_HD inline double shape_square(double r)
{
    const double r2 = r * r;
    return r2 <= kShapeLargest ? r2 : kShapeLargest;
}

constexpr int kShapeFrameWords = 6;     // centre[3], velocity[3] of one system
constexpr int kShapeApertureWords = 4;  // radius, inner, out2, in2 of one aperture

// ---- One body ------------------------------------------------------------------------------------------------------------------
// What the image holds of a body: the position and mass words and the velocity words.  A body that is a member of nothing --
// one that does not take part, or an unmeasured one -- is held with x = NaN: the image needs no flag beside the words.
struct ShapePoint {
    float x, y, z, m, vx, vy, vz;
};

NBODY_HD inline bool shape_word_finite(float v) { return __builtin_fabsf(v) <= __FLT_MAX__; }

// Measured: all six words are finite.  The frame is finite, so the six differences are finite exactly then.
NBODY_HD inline bool shape_measured(const ShapePoint &p)
{
    return shape_word_finite(p.x) && shape_word_finite(p.y) && shape_word_finite(p.z) && shape_word_finite(p.vx) &&
           shape_word_finite(p.vy) && shape_word_finite(p.vz);
}

// The body as the image holds it.
NBODY_HD inline ShapePoint shape_image_point(const ShapePoint &p, bool eligible)
{
    ShapePoint out = p;
    if (!eligible)
        out.x = __builtin_nanf("");
    return out;
}
NBODY_HD inline bool shape_eligible(const ShapePoint &p) { return p.x == p.x; }

// w: the mass word or 1, widened.
NBODY_HD inline double shape_weight(const ShapePoint &p, int weight) { return weight == kGroupsWeightNumber ? 1.0 : (double)p.m; }

// The state of one aperture's iteration: e1, e2, e3 as rows and the two weights 1 / q^2 and 1 / s^2.
struct ShapeState {
    double e[9], w2, w3;
};
NBODY_HD inline ShapeState shape_identity()
{
    return ShapeState{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, 1.0, 1.0};
}

// r2e of a body at d under a state: the rotation with surface_along's parentheses, then (a'a' + w2 (b'b')) + w3 (c'c').
NBODY_HD inline double shape_r2e(const ShapeState &st, double dx, double dy, double dz)
{
    const double a = surface_along(st.e, dx, dy, dz), b = surface_along(st.e + 3, dx, dy, dz), c = surface_along(st.e + 6, dx, dy, dz);
    return (a * a + st.w2 * (b * b)) + st.w3 * (c * c);
}

// The member decision: measured, taking part and in2 < r2e <= out2.  A NaN r2e is a member of nothing.
NBODY_HD inline bool shape_member(bool eligible, double r2e, double in2, double out2) { return eligible && in2 < r2e && r2e <= out2; }

// ---- Level 1: the step of one lane over one body ---------------------------------------------------------------------------------
// The partial of one block: `N` fp64 sums and the member count.  A pass has 7 (T[6], W), the final walk 13 (weight, D[3],
// M[6], L[3]), total_weight 1.
constexpr int kShapePassWords = 7, kShapeFinalWords = 13;
template <int N>
struct ShapePartial {
    double v[N];
    int count;
};

// One body joins a pass's partial: T in the state's coordinates, (w (d_a d_b)) or (w (d_a d_b)) / r2e, and W.
NBODY_HD inline void shape_pass_step(ShapePartial<kShapePassWords> &a, const ShapePoint &p, const double *frame, const ShapeState &st,
                                     double in2, double out2, int weight, bool reduced)
{
    const double dx = (double)p.x - frame[0], dy = (double)p.y - frame[1], dz = (double)p.z - frame[2];
    const double r2e = shape_r2e(st, dx, dy, dz);
    if (!shape_member(shape_eligible(p), r2e, in2, out2))
        return;
    const double w = shape_weight(p, weight);
    double t[6] = {w * (dx * dx), w * (dy * dy), w * (dz * dz), w * (dx * dy), w * (dx * dz), w * (dy * dz)};
    if (reduced)
        for (int c = 0; c < 6; ++c)
            t[c] = t[c] / r2e;
    for (int c = 0; c < 6; ++c)
        a.v[c] += t[c];
    a.v[6] += w;
    a.count += 1;
}

// One body joins the final walk's partial; returns whether it is a member.  M is unreduced whatever the flag; L is radial's
// cross product.
NBODY_HD inline bool shape_final_step(ShapePartial<kShapeFinalWords> &a, const ShapePoint &p, const double *frame, const ShapeState &st,
                                      double in2, double out2, int weight)
{
    const double dx = (double)p.x - frame[0], dy = (double)p.y - frame[1], dz = (double)p.z - frame[2];
    const double r2e = shape_r2e(st, dx, dy, dz);
    if (!shape_member(shape_eligible(p), r2e, in2, out2))
        return false;
    const double ux = (double)p.vx - frame[3], uy = (double)p.vy - frame[4], uz = (double)p.vz - frame[5];
    const double w = shape_weight(p, weight);
    const double lx = dy * uz - dz * uy, ly = dz * ux - dx * uz, lz = dx * uy - dy * ux;
    a.v[0] += w;
    a.v[1] += w * dx;
    a.v[2] += w * dy;
    a.v[3] += w * dz;
    a.v[4] += w * (dx * dx);
    a.v[5] += w * (dy * dy);
    a.v[6] += w * (dz * dz);
    a.v[7] += w * (dx * dy);
    a.v[8] += w * (dx * dz);
    a.v[9] += w * (dy * dz);
    a.v[10] += w * lx;
    a.v[11] += w * ly;
    a.v[12] += w * lz;
    a.count += 1;
    return true;
}

// One body joins total_weight's partial: w of every measured body taking part.
NBODY_HD inline void shape_total_step(ShapePartial<1> &a, const ShapePoint &p, int weight)
{
    if (shape_eligible(p))
        a.v[0] += shape_weight(p, weight);
}

// The bodies of block k: 64 k ... min(64 k + 63, n - 1), in ascending index.
NBODY_HD inline int shape_blocks(int n) { return (n + kShapeBlock - 1) / kShapeBlock; }
NBODY_HD inline int shape_block_end(int k, int n) { return (k + 1) * kShapeBlock < n ? (k + 1) * kShapeBlock : n; }

// ---- Level 2: the block partials in ascending k, from +0.0 ---------------------------------------------------------------------
// get(k): the partial of block k.
template <int N, class Get>
NBODY_HD inline ShapePartial<N> shape_level2(Get get, int blocks)
{
    ShapePartial<N> total{};
    for (int k = 0; k < blocks; ++k) {
        const ShapePartial<N> p = get(k);
        for (int c = 0; c < N; ++c)
            total.v[c] += p.v[c];
        total.count += p.count;
    }
    return total;
}

// ---- Jacobi ----------------------------------------------------------------------------------------------------------------------
// One rotation of the pair (p, q) whose third index is r: app, aqq the diagonal words, apq the word it removes, arp and arq the
// other two off-diagonal words, v the eigenvector matrix by rows v[3 k + column].  A word that is negligible beside both
// diagonal words -- adding a hundred times its magnitude changes neither -- is set to 0 without a rotation.
NBODY_HD inline void shape_jacobi_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double *v, int p, int q)
{
    if (apq == 0.0)
        return;
    const double g = 100.0 * __builtin_fabs(apq), fp = __builtin_fabs(app), fq = __builtin_fabs(aqq);
    if (fp + g == fp && fq + g == fq) {
        apq = 0.0;
        return;
    }
    const double theta = (aqq - app) / (2.0 * apq);
    const double root = __builtin_sqrt(theta * theta + 1.0);
    const double t = theta < 0.0 ? -1.0 / (root - theta) : 1.0 / (theta + root);
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
    for (int k = 0; k < 3; ++k) {
        const double vp = v[3 * k + p], vq = v[3 * k + q];
        v[3 * k + p] = c * vp - s * vq;
        v[3 * k + q] = s * vp + c * vq;
    }
}

// What one decomposition gives: the eigenvalues sorted descending and e1, e2, e3 as rows.
struct ShapeEigen {
    double lambda[3], e[9];
};

// T[6] = xx, yy, zz, xy, xz, yz.  Sweeps over the pairs (0,1), (0,2), (1,2) until the three off-diagonal words are all 0 at the
// start of a sweep, kShapeJacobiSweeps at the most.  Then the sort lambda1 >= lambda2 >= lambda3 with ties to the lower
// original column, e1 and e2 with their component of largest magnitude positive (ties to the lower index), e3 = e1 x e2.
NBODY_HD inline ShapeEigen shape_jacobi(const double *T)
{
    double d0 = T[0], d1 = T[1], d2 = T[2], o01 = T[3], o02 = T[4], o12 = T[5];
    double v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < kShapeJacobiSweeps; ++sweep) {
        if (o01 == 0.0 && o02 == 0.0 && o12 == 0.0)
            break;
        shape_jacobi_rotate(d0, d1, o01, o02, o12, v, 0, 1);
        shape_jacobi_rotate(d0, d2, o02, o01, o12, v, 0, 2);
        shape_jacobi_rotate(d1, d2, o12, o01, o02, v, 1, 2);
    }
    const double d[3] = {d0, d1, d2};
    // The rank of column c: the columns that come before it.
    int at[3];
    for (int c = 0; c < 3; ++c) {
        int before = 0;
        for (int o = 0; o < 3; ++o)
            before += (d[o] > d[c] || (d[o] == d[c] && o < c)) ? 1 : 0;
        at[c] = before;
    }
    // NaN eigenvalues compare false with everything: keep the ranks a permutation.
    if (!(at[0] != at[1] && at[0] != at[2] && at[1] != at[2])) {
        at[0] = 0;
        at[1] = 1;
        at[2] = 2;
    }
    // Every index below is a constant once the loops are unrolled: the words stay in registers.
    ShapeEigen out;
    for (int r = 0; r < 3; ++r)
        out.lambda[r] = at[0] == r ? d[0] : (at[1] == r ? d[1] : d[2]);
    for (int r = 0; r < 2; ++r) {
        double *e = out.e + 3 * r;
        for (int k = 0; k < 3; ++k)
            e[k] = at[0] == r ? v[3 * k] : (at[1] == r ? v[3 * k + 1] : v[3 * k + 2]);
        double lead = e[0];
        if (__builtin_fabs(e[1]) > __builtin_fabs(lead))
            lead = e[1];
        if (__builtin_fabs(e[2]) > __builtin_fabs(lead))
            lead = e[2];
        if (lead < 0.0)
            for (int k = 0; k < 3; ++k)
                e[k] = -e[k];
    }
    const double *a = out.e, *b = out.e + 3;
    out.e[6] = a[1] * b[2] - a[2] * b[1];
    out.e[7] = a[2] * b[0] - a[0] * b[2];
    out.e[8] = a[0] * b[1] - a[1] * b[0];
    return out;
}

// ---- The iteration of one aperture -------------------------------------------------------------------------------------------------
// What the iteration carries from pass to pass beside the state.
struct ShapeProgress {
    ShapeState state;
    double q, s, change, lambda[3];
    int status, iterations;
    bool done;
};
NBODY_HD inline ShapeProgress shape_start() { return ShapeProgress{shape_identity(), 1.0, 1.0, 0.0, {0.0, 0.0, 0.0}, kShapeMax, 0, false}; }

// The end of pass k = g.iterations + 1, given the pass's totals (T[6], W and the member count): FEW, DEGENERATE, converged, MAX,
// or on to the next pass.
NBODY_HD inline void shape_update(ShapeProgress &g, const ShapePartial<kShapePassWords> &total, double tol, int max_iterations, int min_members)
{
    g.iterations += 1;
    if (total.count < min_members) {
        g.status = kShapeFew;
        g.done = true;
        return;
    }
    const ShapeEigen eig = shape_jacobi(total.v);
    const double l1 = eig.lambda[0], l2 = eig.lambda[1], l3 = eig.lambda[2];
    for (int c = 0; c < 3; ++c)
        g.lambda[c] = eig.lambda[c];
    const double w2 = l1 / l2, w3 = l1 / l3;
    if (l3 <= 0.0 || !shape_finite(w3) || !shape_finite(w2) || !(total.v[6] > 0.0)) {
        g.status = kShapeDegenerate;
        g.done = true;
        return;
    }
    const double q = __builtin_sqrt(l2 / l1), s = __builtin_sqrt(l3 / l1);
    const double dq = __builtin_fabs(q - g.q), ds = __builtin_fabs(s - g.s);
    const bool converged = dq <= tol * g.q && ds <= tol * g.s;
    const double cq = dq / g.q, cs = ds / g.s;
    g.change = cs > cq ? cs : cq;
    for (int c = 0; c < 9; ++c)
        g.state.e[c] = eig.e[c];
    g.state.w2 = w2;
    g.state.w3 = w3;
    g.q = q;
    g.s = s;
    if (converged) {
        g.status = kShapeConverged;
        g.done = true;
    } else if (g.iterations >= max_iterations) {
        g.status = kShapeMax;
        g.done = true;
    }
}

// The record of an aperture: how the iteration ended and the sums of the final walk.
NBODY_HD inline BatchShapeAperture shape_record(const ShapeProgress &g, double radius, double inner, const ShapePartial<kShapeFinalWords> &f)
{
    BatchShapeAperture r;
    r.status = g.status;
    r.iterations = g.iterations;
    r.count = f.count;
    r.radius = radius;
    r.inner = inner;
    r.q = g.q;
    r.s = g.s;
    r.change = g.change;
    for (int c = 0; c < 3; ++c)
        r.eigenvalues[c] = g.lambda[c];
    for (int c = 0; c < 9; ++c)
        r.axes[c] = g.state.e[c];
    r.weight = f.v[0];
    for (int c = 0; c < 3; ++c)
        r.D[c] = f.v[1 + c];
    for (int c = 0; c < 6; ++c)
        r.M[c] = f.v[4 + c];
    for (int c = 0; c < 3; ++c)
        r.L[c] = f.v[10 + c];
    return r;
}

// ---- The system summary ------------------------------------------------------------------------------------------------------------
NBODY_HD inline BatchShapeSystem shape_system(int selected, int unmeasured, int apertures, int reduced, int converged, double total,
                                              const double *frame)
{
    return BatchShapeSystem{selected, unmeasured, apertures, reduced, converged, 0, total, {frame[0], frame[1], frame[2]},
                            {frame[3], frame[4], frame[5]}};
}

// The per-body record: the membership bits.
NBODY_HD inline BatchShapeBody shape_body(unsigned inside) { return BatchShapeBody{inside, 0}; }

// Where the image holds body i: block k = i / 64 starts half a body late per block, so that the 64 lanes of a wave, lane k
// at body 64 k + j, read 16-byte words of 16 different bank groups (without the shift all 64 addresses are 2 KiB apart, on one).
NBODY_HD inline int shape_image_slot(int i) { return 2 * i + (i >> 6); }
NBODY_HD inline int shape_image_slots(int max_bodies) { return 2 * max_bodies + kShapeBlock; }
// Where the membership byte of body i is: four bytes later per block, so that the lanes' 32-bit words are 17 apart.
NBODY_HD inline int shape_inside_at(int i) { return i + 4 * (i >> 6); }
NBODY_HD inline int shape_inside_bytes(int max_bodies) { return (max_bodies + 4 * kShapeBlock + 15) / 16 * 16; }


// The workgroup: batch_shape's, kept at eight waves.  A wave works on one aperture and there are at most eight, so the sixteen
// waves of the largest capacity would leave eight idle after the image is built and halve every lane's registers, which the
// final walk's 13 sums beside the Jacobi words do not fit (the 1024-lane build spilled).  The rows of a lane are then RPL, or
// 2 RPL above 2048 bodies.
constexpr int kShapeMaxThreads = 512;
NBODY_HD inline int shape_threads(int batch_threads) { return batch_threads < kShapeMaxThreads ? batch_threads : kShapeMaxThreads; }
NBODY_HD inline int shape_rows(int rpl, int threads, int max_bodies)
{
    return rpl * ((max_bodies + rpl * threads - 1) / (rpl * threads));
}

}  // namespace nbody
