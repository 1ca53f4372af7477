// nbody_batch_members_math.h -- the arithmetic of nbody_batch_members (include/nbody_batch_members.h) that needs no GPU: the
// two records, the empty records, and the fp64 energy and decision of one row from its fp32 velocity, the frame's fp64
// velocity and the row's fp64 potential.  Plain C++17 without HIP, like nbody_batch_structure_math.h: batch_members_kernel
// (nbody_batch_analysis.hip) calls it per row and iteration, and a stand-alone driver (tests/batch_members_driver.cpp) calls it on the
// CPU, where tests/test_batch_members_cpu.py checks hand-picked rows.  Internal; the public surface is
// include/nbody_batch_members.h.
#pragma once

#ifndef NBODY_HD
#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif
#endif

namespace nbody {

constexpr int kMembersMaxIterations = 64;  // NBODY_BATCH_MEMBERS_MAX_ITERATIONS

// nbody_batch_member_body's layout (nbody_batch_analysis.hip asserts it): 24 bytes.
struct BatchMemberBody {
    double potential, energy;
    int member, removed_at;
};

// nbody_batch_member_system's layout (nbody_batch_analysis.hip asserts it): 88 bytes.
struct BatchMemberSystem {
    double bound_mass, centre[3], velocity[3], kinetic, potential;
    int members, sources, iterations, converged;
};

// Slots from the count on, and a system without bodies: no iteration was evaluated, which counts as converged.
NBODY_HD inline BatchMemberBody members_empty_body() { return BatchMemberBody{0.0, 0.0, 0, 0}; }
NBODY_HD inline BatchMemberSystem members_empty_system()
{
    return BatchMemberSystem{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0.0, 0.0, 0, 0, 0, 1};
}

// |v - V|^2 / 2 of one row in fp64 from its fp32 velocity: d = (double)v - V per component, 0.5 (dx dx + dy dy + dz dz).
NBODY_HD inline double members_kinetic(float vx, float vy, float vz, double Vx, double Vy, double Vz)
{
    const double dx = (double)vx - Vx, dy = (double)vy - Vy, dz = (double)vz - Vz;
    return 0.5 * (dx * dx + dy * dy + dz * dz);
}

// e = |v - V|^2 / 2 + phi.
NBODY_HD inline double members_energy(float vx, float vy, float vz, double Vx, double Vy, double Vz, double phi)
{
    return members_kinetic(vx, vy, vz, Vx, Vy, Vz) + phi;
}

// member_t = member_{t-1} && e < 0.  Strict: e = 0 (a lone body) and -0.0 are not negative, and neither is NaN.
NBODY_HD inline bool members_stays(bool member, double energy) { return member && energy < 0.0; }

}  // namespace nbody
