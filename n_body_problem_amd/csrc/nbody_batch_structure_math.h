// nbody_batch_structure_math.h -- the arithmetic of nbody_batch_structure (include/nbody_batch_structure.h) that needs no GPU:
// the two records, the sorted list of a row's eight smallest squared distances, the k-th of it, and the density of one body
// from its k-th distance and neighbour weight.  Plain C++17 without HIP, like nbody_batch_pairs_elements.h:
// batch_structure_kernel (nbody_batch_analysis.hip) calls it per pair and per row, and a stand-alone driver
// (tests/batch_structure_driver.cpp) calls it on the CPU, where tests/test_batch_structure_cpu.py checks it against std::sort
// and the formula.  Internal; the public surface is include/nbody_batch_structure.h.
#pragma once

#include <cmath>

#ifndef NBODY_HD
#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif
#endif

namespace nbody {

constexpr int kStructureMaxNeighbour = 8;  // NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR
constexpr int kStructureFractions = 8;     // NBODY_BATCH_STRUCTURE_FRACTIONS
constexpr double kFourPiOverThree = 4.1887902047863909846;

// nbody_batch_structure_body's layout (nbody_batch_analysis.hip asserts it): 40 bytes.
struct BatchStructureBody {
    double density, radius, enclosed;
    float neighbour_r2, neighbour_weight;
    int inside, reserved;
};

// nbody_batch_structure_system's layout (nbody_batch_analysis.hip asserts it): 120 bytes.
struct BatchStructureSystem {
    double centre[3], core_radius, core_density, total_weight;
    double lagrange[kStructureFractions];
    int estimated, reserved;
};

// Slots from the count on, and a system whose total weight is 0.
NBODY_HD inline BatchStructureBody structure_empty_body() { return BatchStructureBody{0.0, 0.0, 0.0, 0.f, 0.f, 0, 0}; }
NBODY_HD inline BatchStructureSystem structure_empty_system()
{
    return BatchStructureSystem{{0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0, 0};
}

// The sorted eight-smallest list: a is ascending and starts at +inf throughout; c (never NaN: +inf stands for "no neighbour
// pair") sinks to its place and the largest of the nine falls out.  Sixteen min / max, no branch, no index: the list stays
// in registers.  The result does not depend on the order the values come in.
NBODY_HD inline void structure_insert(float (&a)[kStructureMaxNeighbour], float c)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t < kStructureMaxNeighbour; ++t) {
        const float lo = fminf(a[t], c);
        c = fmaxf(a[t], c);
        a[t] = lo;
    }
}

// The k-th smallest, 1 <= k <= 8: the list is ascending, so it is the largest of the first k.  Taken with max, not with an
// index or a chain of selects, which the compiler turns into an index: either sends the list to scratch memory.
NBODY_HD inline float structure_kth(const float (&a)[kStructureMaxNeighbour], int k)
{
    float r = a[0];
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 1; t < kStructureMaxNeighbour; ++t)
        r = fmaxf(r, t < k ? a[t] : -__builtin_inff());
    return r;
}

// density = neighbour_weight / (4 pi / 3 r^3), r = sqrt((double)r2_k), in fp64; 0 where the row has fewer than k neighbours.
NBODY_HD inline double structure_density(float r2_k, float neighbour_weight)
{
    if (!(r2_k < __builtin_inff()))
        return 0.0;
    const double r = std::sqrt((double)r2_k);
    return (double)neighbour_weight / (kFourPiOverThree * (r * r * r));
}

}  // namespace nbody
