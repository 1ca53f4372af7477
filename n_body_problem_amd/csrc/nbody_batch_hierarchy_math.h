// nbody_batch_hierarchy_math.h -- the fp64 arithmetic of nbody_batch_hierarchy (include/nbody_batch_hierarchy.h) that needs no
// GPU: the three records and their empty values, the merged state of a new node (nbody_batch_merge.h's arithmetic), the
// pair's elements and angular momentum (nbody_batch_pairs_elements.h's formulas), the perturbation scaling, the mutual
// inclination and the Mardling & Aarseth stability comparison.  Plain C++17 without HIP, like nbody_batch_members_math.h:
// batch_hierarchy_kernel (nbody_batch_analysis.hip) calls it once per candidate pair, and a stand-alone driver
// (tests/batch_hierarchy_driver.cpp) calls it on the CPU, where tests/test_batch_hierarchy_cpu.py checks it against closed
// forms.  Internal; the public surface is include/nbody_batch_hierarchy.h.
#pragma once

#include "nbody_batch_pairs_elements.h"

#include <cmath>
#include <limits>

namespace nbody {

constexpr int kHierarchyMaxLevels = 16;  // NBODY_BATCH_HIERARCHY_MAX_LEVELS

// nbody_batch_hierarchy_node's layout (nbody_batch_analysis.hip asserts it): 128 bytes.
struct BatchHierarchyNode {
    int child[2], parent, level, leaves, slot, stable, reserved;
    double mass, energy, semi_major_axis, eccentricity, inclination, separation, perturbation, mutual_inclination[2], h[3];
};

// nbody_batch_hierarchy_body's layout: 16 bytes.
struct BatchHierarchyBody {
    int parent, root, depth, reserved;
};

// nbody_batch_hierarchy_system's layout: 40 bytes.
struct BatchHierarchySystem {
    int nodes, roots, levels, converged, singles, binaries, triples, higher, unstable, reserved;
};

// Entries from the node count on; slots from the body count on; a system without leaves.
NBODY_HD inline BatchHierarchyNode hierarchy_empty_node()
{
    return BatchHierarchyNode{{-1, -1}, -1, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, {0.0, 0.0}, {0.0, 0.0, 0.0}};
}
NBODY_HD inline BatchHierarchyBody hierarchy_empty_body() { return BatchHierarchyBody{-1, -1, 0, 0}; }
NBODY_HD inline BatchHierarchySystem hierarchy_empty_system() { return BatchHierarchySystem{0, 0, 0, 1, 0, 0, 0, 0, 0, 0}; }

// One component of a node's state, the merged body of nbody_batch_merge.h: fp64 from the fp32 operands, rounded once;
// M = (double)m_i + (double)m_j, the arithmetic mean where M == 0.
NBODY_HD inline float hierarchy_merged(float mi, float ui, float mj, float uj, double M)
{
    if (M == 0.0)
        return (float)(0.5 * ((double)ui + (double)uj));
    return (float)(std::fma((double)mj, (double)uj, (double)mi * (double)ui) / M);
}

// perturbation = 2 g Q^3 / mu with Q = a (1 + e): the tidal force of the worst perturber at apocentre over the pair's own.
NBODY_HD inline double hierarchy_perturbation(float g, double a, double e, double mu)
{
    const double Q = a * (1.0 + e);
    return 2.0 * (double)g * (Q * Q * Q) / mu;
}

// The pair is accepted unless perturbation > tolerance: a NaN perturbation does not reject.
NBODY_HD inline bool hierarchy_accepts(double energy, double perturbation, double tolerance)
{
    return energy < 0.0 && !(perturbation > tolerance);
}

// acos(clamp(h . hc / (|h| |hc|))), 0 where a norm is 0.
NBODY_HD inline double hierarchy_mutual_inclination(const double *h, const double *hc)
{
    const double n = std::sqrt(h[0] * h[0] + h[1] * h[1] + h[2] * h[2]);
    const double nc = std::sqrt(hc[0] * hc[0] + hc[1] * hc[1] + hc[2] * hc[2]);
    if (!(n > 0.0) || !(nc > 0.0))
        return 0.0;
    double c = (h[0] * hc[0] + h[1] * hc[1] + h[2] * hc[2]) / (n * nc);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    return std::acos(c);
}

// Mardling & Aarseth (2001): 2.8 ((1 + q)(1 + e) / sqrt(1 - e))^(2/5) (1 - 0.3 i_mut / pi), q = m_o / m_c.
NBODY_HD inline double hierarchy_threshold(double q, double e, double imut)
{
    const double pi = 3.14159265358979323846;
    return 2.8 * std::pow((1.0 + q) * (1.0 + e) / std::sqrt(1.0 - e), 0.4) * (1.0 - 0.3 * imut / pi);
}

// The pericentre of the outer orbit over the inner semi-major axis.
NBODY_HD inline double hierarchy_ratio(double a, double e, double a_c) { return a * (1.0 - e) / a_c; }

// The composite child c passes where the ratio exceeds the threshold; a NaN on either side does not pass.
NBODY_HD inline bool hierarchy_child_passes(double a, double e, double a_c, double q, double imut)
{
    return hierarchy_ratio(a, e, a_c) > hierarchy_threshold(q, e, imut);
}

// The elements of the pair of roots i (the lower slot) and j from their fp32 states {x, y, z} and masses, by
// batch_pair_record's formulas, with mu = (double)m_j + (double)m_i; h = r x v, r = x_j - x_i, v = v_j - v_i in fp64.  Fills
// mass (the fp32 sum, widened), the five elements and h of rec; the caller fills the rest.
NBODY_HD inline void hierarchy_elements(const float *xi, const float *vi, float mi, const float *xj, const float *vj, float mj,
                                        BatchHierarchyNode &rec)
{
    const double mu = (double)mj + (double)mi;
    const BatchPairRecord p = batch_pair_record(0, 1, xi, vi, xj, vj, mu);
    const double rx = (double)xj[0] - (double)xi[0], ry = (double)xj[1] - (double)xi[1], rz = (double)xj[2] - (double)xi[2];
    const double vx = (double)vj[0] - (double)vi[0], vy = (double)vj[1] - (double)vi[1], vz = (double)vj[2] - (double)vi[2];
    rec.mass = (double)(mi + mj);
    rec.energy = p.energy;
    rec.semi_major_axis = p.semi_major_axis;
    rec.eccentricity = p.eccentricity;
    rec.inclination = p.inclination;
    rec.separation = p.separation;
    rec.h[0] = ry * vz - rz * vy;
    rec.h[1] = rz * vx - rx * vz;
    rec.h[2] = rx * vy - ry * vx;
}

}  // namespace nbody
