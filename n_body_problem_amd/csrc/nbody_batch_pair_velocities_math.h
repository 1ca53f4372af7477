// nbody_batch_pair_velocities_math.h -- the arithmetic of nbody_batch_pair_velocities (include/nbody_batch_pair_velocities.h)
// that needs no GPU: the two records, the terms of one pair, the bin of one pair among the edges of one pass, the step of one
// row over one column on the accumulators of the bins of one pass, the halving tree on the 64 row sums of a block, the
// ascending sum of the blocks, and the differencing into the system record.  Plain C++17 without HIP, on top of
// nbody_batch_correlation_math.h, whose examined-pair predicate, measured predicate, squared edge and (through
// nbody_batch_groups_math.h) r2 chain and `friends` predicate it reuses: batch_pair_velocities_kernel
// (nbody_batch_analysis.hip) calls these with the columns in LDS, and a stand-alone driver
// (tests/batch_pair_velocities_driver.cpp) runs whole systems through the same functions on the CPU, lane by lane for any
// workgroup shape and any number of bins per pass, where tests/test_batch_pair_velocities_cpu.py compares every byte with
// tests/hermite_pair_velocities_ref.py.  Nothing here may be contracted: the build passes -ffp-contract=off.  Internal; the
// public surface is include/nbody_batch_pair_velocities.h.
#pragma once

#include "nbody_batch_correlation_math.h"

namespace nbody {

constexpr int kPairVelocitiesMaxBins = 32;  // NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS
constexpr int kPairVelocitiesBlock = 64;    // rows per block of the pinned order
constexpr int kPairVelocitiesTerms = 9;     // weight, r1, r2, rv, vr1, vr2, vt2, v1, v2
#ifndef NBODY_BATCH_PAIR_VELOCITIES_PASS_BINS
#define NBODY_BATCH_PAIR_VELOCITIES_PASS_BINS 8
#endif
constexpr int kPairVelocitiesPassBins = NBODY_BATCH_PAIR_VELOCITIES_PASS_BINS;  // G of the kernel built; no record depends on it

// nbody_batch_pair_velocities_bin's layout (nbody_batch_analysis.hip asserts it): 96 bytes.
struct BatchPairVelocitiesBin {
    long long count, approaching, receding;
    double weight, r1, r2, rv, vr1, vr2, vt2, v1, v2;
};

// nbody_batch_pair_velocities_system's layout (nbody_batch_analysis.hip asserts it): 56 bytes.
struct BatchPairVelocitiesSystem {
    int rows, sources, both, bins, weight, reserved;
    long long pairs, below, above, unmeasured;
};

// The passes over the columns of a call with `bins` bins at G bins per pass, and the edges laid out for them: every pass reads
// G + 1 edges from t = pass * G on, the edges from `bins` on copies of edge `bins`, whose bins tie and hold nothing.
NBODY_HD inline int pair_velocities_passes(int bins, int g) { return (bins + g - 1) / g; }
NBODY_HD inline int pair_velocities_padded_edges(int bins, int g) { return pair_velocities_passes(bins, g) * g + 1; }

// ---- One body ----------------------------------------------------------------------------------------------------------------
// What the image holds of a body: the position and mass words and the three velocity words.
struct PairVelocityPoint {
    float x, y, z, m, vx, vy, vz;
};

// v2 of a pair is < +inf iff the six velocity words are finite: the differences of finite fp32 words and the sum of their three
// squares cannot overflow fp64, and a NaN or an infinite word makes its difference, its square and the sum a NaN or +inf.  So
// "v2 < +inf" is a property of the two bodies, decided once per body: every word within the largest finite value.
NBODY_HD inline bool pair_velocities_body_measured(const PairVelocityPoint &p)
{
    return __builtin_fabsf(p.vx) <= __FLT_MAX__ && __builtin_fabsf(p.vy) <= __FLT_MAX__ && __builtin_fabsf(p.vz) <= __FLT_MAX__;
}

// The flags of a body in the image: a source, a row, velocity words that can be measured.
constexpr int kPairVelocitiesSource = 1, kPairVelocitiesRow = 2, kPairVelocitiesMeasured = 4;
NBODY_HD inline int pair_velocities_flags(bool row, bool source, bool measured)
{
    return (source ? kPairVelocitiesSource : 0) | (row ? kPairVelocitiesRow : 0) | (measured ? kPairVelocitiesMeasured : 0);
}

// ---- One pair ----------------------------------------------------------------------------------------------------------------
// r2 of the pair as the bins see it: groups_r2, behind a NaN where the pair is not examined or its v2 is not measured; a NaN
// is within no edge, in no bin and not measured.
NBODY_HD inline float pair_velocities_r2(bool examined, bool v_measured, const PairVelocityPoint &pi, const PairVelocityPoint &pj)
{
    const float r2 = groups_r2(pi.x, pi.y, pi.z, pj.x, pj.y, pj.z);
    return examined && v_measured ? r2 : __builtin_nanf("");
}

// The bin of a pair among the G + 1 ascending squared edges of one pass: the edges the pair is not within are counted, so
// that two that tie are passed together.  -1: within the first edge; 0 ... G - 1: that bin of the pass; G: not within the
// last, or a NaN.
template <int G>
NBODY_HD inline int pair_velocities_bin(float r2, const float *e2)
{
    int passed = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int t = 0; t <= G; ++t)
        passed += groups_friends(r2, e2[t]) ? 0 : 1;
    return passed - 1;
}
template <int G>
NBODY_HD inline bool pair_velocities_member(int bin) { return bin >= 0 && bin < G; }

// ww: 1, or the product of the two mass words widened, exact in fp64.
NBODY_HD inline double pair_velocities_weight(const PairVelocityPoint &pi, const PairVelocityPoint &pj, int weight)
{
    return weight == kGroupsWeightNumber ? 1.0 : (double)pi.m * (double)pj.m;
}

// The nine addends of a member pair and the sign of rv.  fp64 from the widened words, in the order of the parentheses.
struct PairVelocityTerms {
    double w[kPairVelocitiesTerms];
    int approaching, receding;
};

NBODY_HD inline PairVelocityTerms pair_velocities_terms(const PairVelocityPoint &pi, const PairVelocityPoint &pj, int weight)
{
    const double dx = (double)pj.x - (double)pi.x, dy = (double)pj.y - (double)pi.y, dz = (double)pj.z - (double)pi.z;
    const double wx = (double)pj.vx - (double)pi.vx, wy = (double)pj.vy - (double)pi.vy, wz = (double)pj.vz - (double)pi.vz;
    const double s = (dx * dx + dy * dy) + dz * dz;
    const double rv = (dx * wx + dy * wy) + dz * wz;
    const double v2 = (wx * wx + wy * wy) + wz * wz;
    const double r = __builtin_sqrt(s);
    const double vr = rv / r;
    const double vrvr = vr * vr;
    const double vt2 = __builtin_fmax(v2 - vrvr, 0.0);
    const double v = __builtin_sqrt(v2);
    const double ww = pair_velocities_weight(pi, pj, weight);
    PairVelocityTerms t;
    t.w[0] = ww;
    t.w[1] = ww * r;
    t.w[2] = ww * s;
    t.w[3] = ww * rv;
    t.w[4] = ww * vr;
    t.w[5] = ww * vrvr;
    t.w[6] = ww * vt2;
    t.w[7] = ww * v;
    t.w[8] = ww * v2;
    t.approaching = rv < 0.0 ? 1 : 0;
    t.receding = rv > 0.0 ? 1 : 0;
    return t;
}

// ---- The accumulators of one pass --------------------------------------------------------------------------------------------
// The sums of one row over the G bins of a pass, cleared for every row; and the integers of a lane, which add up in any order
// and run on over its rows.
template <int G>
struct PairVelocitySums {
    double w[G][kPairVelocitiesTerms];
};
template <int G>
struct PairVelocityCounts {
    unsigned int count[G], approaching[G], receding[G];
};
// The cumulative counters of the system record, nbody_batch_correlation's: the pairs within the first edge, within the last,
// and the measured ones.
struct PairVelocitySystemCounts {
    unsigned int within_first, within_last, measured;
};

template <int G>
NBODY_HD inline void pair_velocities_clear(PairVelocitySums<G> &a)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int g = 0; g < G; ++g)
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (int k = 0; k < kPairVelocitiesTerms; ++k)
            a.w[g][k] = 0.0;
}
template <int G>
NBODY_HD inline void pair_velocities_clear(PairVelocityCounts<G> &c)
{
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int g = 0; g < G; ++g)
        c.count[g] = c.approaching[g] = c.receding[g] = 0;
}
NBODY_HD inline void pair_velocities_clear(PairVelocitySystemCounts &c) { c.within_first = c.within_last = c.measured = 0; }

// The system's counters take a pair: r2 is pair_velocities_r2's, first and last the squares of edge 0 and of edge `bins`.
NBODY_HD inline void pair_velocities_system_step(PairVelocitySystemCounts &c, float r2, float first, float last)
{
    c.within_first += groups_friends(r2, first) ? 1 : 0;
    c.within_last += groups_friends(r2, last) ? 1 : 0;
    c.measured += correlation_measured(r2) ? 1 : 0;
}

// A member of bin `bin` of the pass joins the sums of its row: one add per term.  The other bins of the pass take +0.0, which
// changes no bit of a sum that started at +0.0 (such a sum is never -0), so that no accumulator is copied or branched around
// and g never leaves the unrolled loop: the accumulators stay where they are.
template <int G>
NBODY_HD inline void pair_velocities_add(PairVelocitySums<G> &a, PairVelocityCounts<G> &c, int bin, const PairVelocityPoint &pi,
                                         const PairVelocityPoint &pj, int weight)
{
    const PairVelocityTerms t = pair_velocities_terms(pi, pj, weight);
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int g = 0; g < G; ++g) {
        const bool here = g == bin;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (int k = 0; k < kPairVelocitiesTerms; ++k)
            a.w[g][k] += here ? t.w[k] : 0.0;
        c.count[g] += here ? 1u : 0u;
        c.approaching[g] += here ? (unsigned int)t.approaching : 0u;
        c.receding[g] += here ? (unsigned int)t.receding : 0u;
    }
}

// Row i meets column j in one pass: the bin among the pass's edges, and the add where the pair is a member.  Returns r2 as the
// bins saw it, for the system's counters.
template <int G>
NBODY_HD inline float pair_velocities_step(PairVelocitySums<G> &a, PairVelocityCounts<G> &c, bool examined, bool v_measured,
                                           const PairVelocityPoint &pi, const PairVelocityPoint &pj, const float *e2, int weight)
{
    const float r2 = pair_velocities_r2(examined, v_measured, pi, pj);
    const int bin = pair_velocities_bin<G>(r2, e2);
    if (pair_velocities_member<G>(bin))
        pair_velocities_add<G>(a, c, bin, pi, pj, weight);
    return r2;
}

// ---- Blocks ------------------------------------------------------------------------------------------------------------------
// One step of the halving tree: p[l] = p[l] + p[l + off].  The device takes p[l + off] by a shuffle.
NBODY_HD inline double pair_velocities_tree_step(double mine, double other) { return mine + other; }

// The partial of one block from its 64 row sums, which it overwrites.
NBODY_HD inline double pair_velocities_tree(double *p)
{
    for (int off = kPairVelocitiesBlock / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l)
            p[l] = pair_velocities_tree_step(p[l], p[l + off]);
    return p[0];
}

NBODY_HD inline int pair_velocities_blocks(int n) { return (n + kPairVelocitiesBlock - 1) / kPairVelocitiesBlock; }

// The next `blocks` blocks in ascending order join the total, which starts at +0.0: partial k at partials[k * stride].
NBODY_HD inline double pair_velocities_total(double total, const double *partials, int stride, int blocks)
{
    for (int k = 0; k < blocks; ++k)
        total += partials[(long long)k * stride];
    return total;
}

// ---- Records -----------------------------------------------------------------------------------------------------------------
// A bin record is twelve words of eight bytes: three integers (count, approaching, receding), then the nine sums in the order
// of the terms.  One word of it from its total.
constexpr int kPairVelocitiesIntegers = 3, kPairVelocitiesWords = kPairVelocitiesIntegers + kPairVelocitiesTerms;
static_assert(sizeof(BatchPairVelocitiesBin) == 8 * kPairVelocitiesWords, "twelve words of eight bytes");
NBODY_HD inline void pair_velocities_store(BatchPairVelocitiesBin *out, int word, unsigned int total)
{
    const long long wide = (long long)total;
    __builtin_memcpy(reinterpret_cast<char *>(out) + 8 * word, &wide, 8);
}
NBODY_HD inline void pair_velocities_store(BatchPairVelocitiesBin *out, int word, double total)
{
    __builtin_memcpy(reinterpret_cast<char *>(out) + 8 * word, &total, 8);
}

// The record of one system from its totals, by nbody_batch_correlation's differencing.
NBODY_HD inline BatchPairVelocitiesSystem pair_velocities_system(int rows, int sources, int both, int bins, int weight,
                                                                 const PairVelocitySystemCounts &c)
{
    const long long pairs = correlation_pairs(rows, sources, both);
    return BatchPairVelocitiesSystem{rows,  sources, both, bins, weight, 0, pairs, correlation_below(c.within_first),
                                     correlation_above(c.measured, c.within_last), correlation_unmeasured(pairs, c.measured)};
}

}  // namespace nbody
