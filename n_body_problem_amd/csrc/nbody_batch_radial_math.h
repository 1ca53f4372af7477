// nbody_batch_radial_math.h -- the arithmetic of nbody_batch_radial_profile (include/nbody_batch_radial.h) that needs no GPU:
// the three records, the squared edge, the words of one body in the frame (d, u, s, rv, v2), the shell decision on squares,
// the body record, the terms of a member and the add step of every term group, the ascending walk of one walker over the
// image of a system, and which walker owns which shell and terms under either split.  Plain C++17 without HIP, fp64 with basic
// operations only: batch_radial_kernel (nbody_batch_analysis.hip) calls these with the image in LDS, and a stand-alone driver
// (tests/batch_radial_driver.cpp) runs whole systems through the same functions, lane by lane for any workgroup shape and
// either split, on the CPU, where tests/test_batch_radial_cpu.py compares every byte with tests/hermite_radial_ref.py.
// Nothing here may be contracted: the build passes -ffp-contract=off.  Internal; the public surface is
// include/nbody_batch_radial.h.
#pragma once

#include "nbody_batch_groups_math.h"

namespace nbody {

constexpr int kRadialMaxShells = 32;  // NBODY_BATCH_RADIAL_MAX_SHELLS
constexpr int kRadialBelow = -1, kRadialUnmeasured = -2, kRadialNotTaking = -3;  // NBODY_BATCH_RADIAL_BELOW ...
constexpr int kRadialSpherical = -1;

// nbody_batch_radial_shell's layout (nbody_batch_analysis.hip asserts it): 192 bytes.
struct BatchRadialShell {
    long long count;
    double weight, radius, vr1, vr2, vt2;
    double L[3], U[3], M[6], V[6];
};

// nbody_batch_radial_system's layout (nbody_batch_analysis.hip asserts it): 80 bytes.
struct BatchRadialSystem {
    int selected, below, above, unmeasured, shells, projected;
    double total_weight, centre[3], velocity[3];
};

// nbody_batch_radial_body's layout (nbody_batch_analysis.hip asserts it): 24 bytes.
struct BatchRadialBody {
    int shell, reserved;
    double radius, radial_velocity;
};

// ---- Edges and frame -------------------------------------------------------------------------------------------------------
constexpr double kRadialLargest = __DBL_MAX__;

// A finite number: false for NaN and for either infinity.  Stated as "within the largest finite value", an ordered <= against
// a finite value, like correlation_measured.
NBODY_HD inline bool radial_finite(double v) { return __builtin_fabs(v) <= kRadialLargest; }

// An edge is a finite number that is not negative.
NBODY_HD inline bool radial_edge_valid(double e) { return e >= 0.0 && e <= kRadialLargest; }

// e2 of one edge: one fp64 product.  A product that overflows becomes the largest finite value: every measured s is within it.
NBODY_HD inline double radial_edge2(double e)
{
    const double e2 = e * e;
    return e2 <= kRadialLargest ? e2 : kRadialLargest;
}

constexpr int kRadialFrameWords = 6;  // centre[3], velocity[3] of one system

// ---- One body ----------------------------------------------------------------------------------------------------------------
// What the image holds of a body: the position and mass words and the velocity words.
struct RadialPoint {
    float x, y, z, m, vx, vy, vz;
};

// The body in the frame, and the three words its shell is decided on.
struct RadialWords {
    double dx, dy, dz, ux, uy, uz, s, rv, v2;
};

// frame: centre[3], velocity[3].  projected: -1, or the axis that s and rv leave out; the two that remain in ascending order.
NBODY_HD inline RadialWords radial_words(const RadialPoint &p, const double *frame, int projected)
{
    RadialWords b;
    b.dx = (double)p.x - frame[0];
    b.dy = (double)p.y - frame[1];
    b.dz = (double)p.z - frame[2];
    b.ux = (double)p.vx - frame[3];
    b.uy = (double)p.vy - frame[4];
    b.uz = (double)p.vz - frame[5];
    const double xx = b.dx * b.dx, yy = b.dy * b.dy, zz = b.dz * b.dz;
    const double xu = b.dx * b.ux, yu = b.dy * b.uy, zu = b.dz * b.uz;
    if (projected == 0) {
        b.s = yy + zz;
        b.rv = yu + zu;
    } else if (projected == 1) {
        b.s = xx + zz;
        b.rv = xu + zu;
    } else if (projected == 2) {
        b.s = xx + yy;
        b.rv = xu + yu;
    } else {
        b.s = (xx + yy) + zz;
        b.rv = (xu + yu) + zu;
    }
    b.v2 = (b.ux * b.ux + b.uy * b.uy) + b.uz * b.uz;
    return b;
}

// w: the mass word or 1, widened.
NBODY_HD inline double radial_weight(const RadialPoint &p, int weight) { return weight == kGroupsWeightNumber ? 1.0 : (double)p.m; }

// Measured: s < +inf and v2 < +inf, false for +inf and for NaN.
NBODY_HD inline bool radial_measured(const RadialWords &b) { return b.s <= kRadialLargest && b.v2 <= kRadialLargest; }

// The shell of a body taking part: -2 unmeasured, -1 below, t in shell t, `shells` above.  e2 holds shells + 1 squared edges
// that do not descend.  The edges below s are counted: two that tie are passed together, so the shell between them stays empty.
NBODY_HD inline int radial_shell(const RadialWords &b, const double *e2, int shells)
{
    if (!radial_measured(b))
        return kRadialUnmeasured;
    int passed = 0;
    for (int t = 0; t <= shells; ++t)
        passed += b.s > e2[t] ? 1 : 0;
    return passed - 1;
}

// Whether a shell word is that of a measured body taking part (below, a shell, or above): total_weight's bodies.
NBODY_HD inline bool radial_counts_in_total(int shell) { return shell >= kRadialBelow; }

// r and vr of a body whose s > 0.
NBODY_HD inline double radial_r(const RadialWords &b) { return __builtin_sqrt(b.s); }
NBODY_HD inline double radial_vr(const RadialWords &b, double r) { return b.rv / r; }

// The body record: the radius of a measured body taking part and its radial velocity where the radius is > 0.
NBODY_HD inline BatchRadialBody radial_body(int shell, const RadialWords &b)
{
    BatchRadialBody out{shell, 0, 0.0, 0.0};
    if (radial_counts_in_total(shell)) {
        out.radius = radial_r(b);
        out.radial_velocity = out.radius > 0.0 ? radial_vr(b, out.radius) : 0.0;
    }
    return out;
}
NBODY_HD inline BatchRadialBody radial_body_absent() { return BatchRadialBody{kRadialNotTaking, 0, 0.0, 0.0}; }

// ---- The add step ------------------------------------------------------------------------------------------------------------
// The 23 sums and the count in six groups, the unit of the split walk: a walker adds the terms of its group alone.
constexpr int kRadialGroups = 6;
constexpr int kRadialGroupWeight = 0;    // count, weight, radius
constexpr int kRadialGroupVelocity = 1;  // vr1, vr2, vt2
constexpr int kRadialGroupL = 2, kRadialGroupU = 3, kRadialGroupM = 4, kRadialGroupV = 5;
constexpr int kRadialGroupAll = -1;      // the walker of a whole shell

template <int GROUP>
constexpr bool radial_has(int group) { return GROUP == kRadialGroupAll || GROUP == group; }

// One member joins the sums of GROUP: one add per term, the addend w * (...) with the parenthesis first.
template <int GROUP>
NBODY_HD inline void radial_add(BatchRadialShell &a, double w, const RadialWords &b)
{
    if constexpr (radial_has<GROUP>(kRadialGroupWeight) || radial_has<GROUP>(kRadialGroupVelocity)) {
        const double r = radial_r(b);
        if constexpr (radial_has<GROUP>(kRadialGroupWeight)) {
            a.count += 1;
            a.weight += w;
            a.radius += w * r;
        }
        if constexpr (radial_has<GROUP>(kRadialGroupVelocity)) {
            const double vr = radial_vr(b, r);
            const double vrvr = vr * vr;
            const double vt2 = __builtin_fmax(b.v2 - vrvr, 0.0);
            a.vr1 += w * vr;
            a.vr2 += w * vrvr;
            a.vt2 += w * vt2;
        }
    }
    if constexpr (radial_has<GROUP>(kRadialGroupL)) {
        const double lx = b.dy * b.uz - b.dz * b.uy, ly = b.dz * b.ux - b.dx * b.uz, lz = b.dx * b.uy - b.dy * b.ux;
        a.L[0] += w * lx;
        a.L[1] += w * ly;
        a.L[2] += w * lz;
    }
    if constexpr (radial_has<GROUP>(kRadialGroupU)) {
        a.U[0] += w * b.ux;
        a.U[1] += w * b.uy;
        a.U[2] += w * b.uz;
    }
    if constexpr (radial_has<GROUP>(kRadialGroupM)) {
        a.M[0] += w * (b.dx * b.dx);
        a.M[1] += w * (b.dy * b.dy);
        a.M[2] += w * (b.dz * b.dz);
        a.M[3] += w * (b.dx * b.dy);
        a.M[4] += w * (b.dx * b.dz);
        a.M[5] += w * (b.dy * b.dz);
    }
    if constexpr (radial_has<GROUP>(kRadialGroupV)) {
        a.V[0] += w * (b.ux * b.ux);
        a.V[1] += w * (b.uy * b.uy);
        a.V[2] += w * (b.uz * b.uz);
        a.V[3] += w * (b.ux * b.uy);
        a.V[4] += w * (b.ux * b.uz);
        a.V[5] += w * (b.uy * b.uz);
    }
}

// The walker's sums go to the shell's record: the words of GROUP and no others, so that six walkers fill one record.
template <int GROUP>
NBODY_HD inline void radial_store(BatchRadialShell *out, const BatchRadialShell &a)
{
    if constexpr (radial_has<GROUP>(kRadialGroupWeight)) {
        out->count = a.count;
        out->weight = a.weight;
        out->radius = a.radius;
    }
    if constexpr (radial_has<GROUP>(kRadialGroupVelocity)) {
        out->vr1 = a.vr1;
        out->vr2 = a.vr2;
        out->vt2 = a.vt2;
    }
    if constexpr (radial_has<GROUP>(kRadialGroupL)) {
        for (int c = 0; c < 3; ++c)
            out->L[c] = a.L[c];
    }
    if constexpr (radial_has<GROUP>(kRadialGroupU)) {
        for (int c = 0; c < 3; ++c)
            out->U[c] = a.U[c];
    }
    if constexpr (radial_has<GROUP>(kRadialGroupM)) {
        for (int c = 0; c < 6; ++c)
            out->M[c] = a.M[c];
    }
    if constexpr (radial_has<GROUP>(kRadialGroupV)) {
        for (int c = 0; c < 6; ++c)
            out->V[c] = a.V[c];
    }
}

// ---- The ascending walk --------------------------------------------------------------------------------------------------------
// One walker goes through the bodies j = 0 ... n - 1 of the image and adds the terms of GROUP where shell(j) is its shell t.
// With `totals` it also adds w of every measured body taking part into *total: the system's total_weight, one walker's task.
// Image: shell(j), the shell word of body j, and point(j), its RadialPoint.  out is the record of shell t.
template <int GROUP, class Image>
NBODY_HD inline void radial_walk(const Image &img, int n, int t, const double *frame, int projected, int weight, bool totals,
                                 BatchRadialShell *out, double *total)
{
    BatchRadialShell a{};
    double sum = 0.0;
    for (int j = 0; j < n; ++j) {
        const int sj = img.shell(j);
        const bool mine = sj == t, counted = totals && radial_counts_in_total(sj);
        if (!mine && !counted)
            continue;
        const RadialPoint p = img.point(j);
        const double w = radial_weight(p, weight);
        if (counted)
            sum += w;
        if (mine)
            radial_add<GROUP>(a, w, radial_words(p, frame, projected));
    }
    radial_store<GROUP>(out, a);
    if (totals)
        *total = sum;
}

// The walk of total_weight alone, for a call that asks for no shell records: the same adds in the same order.
template <class Image>
NBODY_HD inline void radial_walk_total(const Image &img, int n, int weight, double *total)
{
    double sum = 0.0;
    for (int j = 0; j < n; ++j)
        if (radial_counts_in_total(img.shell(j)))
            sum += radial_weight(img.point(j), weight);
    *total = sum;
}

// Which shell and terms walker w owns.  Split: kRadialMaxShells walkers per group, walker w has group w / 32 and shell w % 32,
// so that the lanes of one wave run at most two groups' code.  Whole: walker w has shell w and every term.  In either the
// walker of shell 0 that adds the weights also adds total_weight.
constexpr int kRadialWalkersSplit = kRadialGroups * kRadialMaxShells, kRadialWalkersWhole = kRadialMaxShells;
NBODY_HD inline int radial_walkers(bool split) { return split ? kRadialWalkersSplit : kRadialWalkersWhole; }

// Walker w of a system does its part, if it has one.  shells_out: the system's records, or NULL (then walker 0 adds
// total_weight and nothing else is done).  Every word of every record is written by exactly one walker.
template <class Image>
NBODY_HD inline void radial_walker(bool split, int w, const Image &img, int n, int shells, const double *frame, int projected, int weight,
                                   BatchRadialShell *shells_out, double *total)
{
    if (!shells_out) {
        if (w == 0)
            radial_walk_total(img, n, weight, total);
        return;
    }
    const int t = split ? w % kRadialMaxShells : w;
    if (t >= shells)
        return;
    const bool totals = w == 0;
    BatchRadialShell *out = shells_out + t;
    if (!split) {
        radial_walk<kRadialGroupAll>(img, n, t, frame, projected, weight, totals, out, total);
        return;
    }
    switch (w / kRadialMaxShells) {
    case kRadialGroupWeight: radial_walk<kRadialGroupWeight>(img, n, t, frame, projected, weight, totals, out, total); break;
    case kRadialGroupVelocity: radial_walk<kRadialGroupVelocity>(img, n, t, frame, projected, weight, false, out, total); break;
    case kRadialGroupL: radial_walk<kRadialGroupL>(img, n, t, frame, projected, weight, false, out, total); break;
    case kRadialGroupU: radial_walk<kRadialGroupU>(img, n, t, frame, projected, weight, false, out, total); break;
    case kRadialGroupM: radial_walk<kRadialGroupM>(img, n, t, frame, projected, weight, false, out, total); break;
    case kRadialGroupV: radial_walk<kRadialGroupV>(img, n, t, frame, projected, weight, false, out, total); break;
    default: break;
    }
}

// ---- Records -------------------------------------------------------------------------------------------------------------------
NBODY_HD inline BatchRadialSystem radial_system(int selected, int below, int above, int unmeasured, int shells, int projected, double total,
                                                const double *frame)
{
    return BatchRadialSystem{selected, below, above, unmeasured, shells, projected, total, {frame[0], frame[1], frame[2]},
                             {frame[3], frame[4], frame[5]}};
}

}  // namespace nbody
