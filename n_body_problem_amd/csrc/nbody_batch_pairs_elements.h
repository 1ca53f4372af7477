// nbody_batch_pairs_elements.h -- the fp64 record of one pair of nbody_batch_pairs (include/nbody_batch_pairs.h, "The
// record"): differences, mu -> energy, semi-major axis, eccentricity, inclination and separation, with the header's special
// cases.  Plain C++17 without HIP, like nbody_sym_plan.h: batch_pairs_kernel (nbody_batch_analysis.hip) calls it once per row, and a
// stand-alone driver (tests/batch_pairs_driver.cpp) calls it on the CPU, where tests/test_batch_pairs_cpu.py checks it against
// closed forms.  Internal; the public surface is include/nbody_batch_pairs.h.
#pragma once

#include <cmath>
#include <limits>

#ifndef NBODY_HD
#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif
#endif

namespace nbody {

// nbody_batch_pair_record's layout (nbody_batch_analysis.hip asserts it): 48 bytes.
struct BatchPairRecord {
    int partner, mutual;
    double energy, semi_major_axis, eccentricity, inclination, separation;
};

// Rows without a partner and slots from the count on.
NBODY_HD inline BatchPairRecord batch_pair_empty() { return BatchPairRecord{-1, 0, 0.0, 0.0, 0.0, 0.0, 0.0}; }

// The record of row i = (xi, vi) with its partner j = (xj, vj): {x, y, z} each, the fp32 state.  mu is m_j + m_i in fp64, or
// m_j alone where row i is a test particle.  The pair is a candidate, so |r| > 0.
NBODY_HD inline BatchPairRecord batch_pair_record(int partner, int mutual, const float *xi, const float *vi, const float *xj,
                                                  const float *vj, double mu)
{
    const double rx = (double)xj[0] - (double)xi[0], ry = (double)xj[1] - (double)xi[1], rz = (double)xj[2] - (double)xi[2];
    const double vx = (double)vj[0] - (double)vi[0], vy = (double)vj[1] - (double)vi[1], vz = (double)vj[2] - (double)vi[2];
    const double inf = std::numeric_limits<double>::infinity();
    const double r = std::sqrt(rx * rx + ry * ry + rz * rz);
    const double v2 = vx * vx + vy * vy + vz * vz;
    BatchPairRecord rec;
    rec.partner = partner;
    rec.mutual = mutual;
    rec.separation = r;
    rec.energy = 0.5 * v2 - mu / r;
    // h = r x v
    const double hx = ry * vz - rz * vy, hy = rz * vx - rx * vz, hz = rx * vy - ry * vx;
    const double h = std::sqrt(hx * hx + hy * hy + hz * hz);
    double c = h > 0.0 ? hz / h : 1.0;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    if (mu == 0.0) {
        rec.semi_major_axis = 0.0;
        rec.eccentricity = inf;
    } else {
        rec.semi_major_axis = rec.energy == 0.0 ? inf : -mu / (2.0 * rec.energy);
        // the eccentricity vector (v x h) / mu - r / |r|
        const double ex = (vy * hz - vz * hy) / mu - rx / r;
        const double ey = (vz * hx - vx * hz) / mu - ry / r;
        const double ez = (vx * hy - vy * hx) / mu - rz / r;
        rec.eccentricity = std::sqrt(ex * ex + ey * ey + ez * ez);
    }
    rec.inclination = h > 0.0 ? std::acos(c) : 0.0;  // last: little else is live across it
    return rec;
}

}  // namespace nbody
