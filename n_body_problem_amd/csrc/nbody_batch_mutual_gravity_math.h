// nbody_batch_mutual_gravity_math.h -- the arithmetic of nbody_batch_mutual_gravity (include/nbody_batch_mutual_gravity.h) that
// needs no GPU: the two records, who is measured and in which set, the stable counting sort of the bodies by set (the rank of a
// body among the 64 of its chunk from the chunk's ballot, the prefix over the chunks' counts, the slot), the plan of row blocks,
// the step of one row over one column on its four accumulators, the nine addends of a row, and the words of an entry from the
// blocks' partials.  The halving tree and the ascending sum of the blocks are nbody_batch_pair_velocities_math.h's.  Plain
// C++17 without HIP: batch_mutual_gravity_kernel (nbody_batch_analysis.hip) calls these with the sorted columns in LDS, and a
// stand-alone driver (tests/batch_mutual_gravity_driver.cpp) runs whole systems through the same functions on the CPU, lane by
// lane for any workgroup shape, where tests/test_batch_mutual_gravity_cpu.py compares every byte with
// tests/hermite_mutual_gravity_ref.py.  Nothing here may be contracted: the build passes -ffp-contract=off.  Internal; the
// public surface is include/nbody_batch_mutual_gravity.h.
#pragma once

#include "nbody_batch_pair_velocities_math.h"

namespace nbody {

constexpr int kMutualGravityMaxSets = 8;    // NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS
constexpr int kMutualGravityNoSet = 255;    // NBODY_BATCH_MUTUAL_GRAVITY_NO_SET
constexpr int kMutualGravityBlock = kPairVelocitiesBlock;  // rows per block of the pinned order, bodies per chunk of the sort
constexpr int kMutualGravityTerms = 9;      // potential, force x y z, torque x y z, virial, power
constexpr int kMutualGravityMaxChunks = 64; // chunks of 64 bodies in the largest system (4096 bodies)

// nbody_batch_mutual_gravity_entry's layout (nbody_batch_analysis.hip asserts it): 80 bytes.
struct BatchMutualGravityEntry {
    long long pairs;
    double potential, force[3], torque[3], virial, power;
};

// nbody_batch_mutual_gravity_system's layout (nbody_batch_analysis.hip asserts it): 128 bytes.
struct BatchMutualGravitySystem {
    int sets, selected, left_out, unmeasured;
    long long pairs, coincident;
    int members[kMutualGravityMaxSets];
    double mass[kMutualGravityMaxSets];
};

// ---- One body ----------------------------------------------------------------------------------------------------------------
// Measured: all seven words finite (a NaN compares false).
NBODY_HD inline bool mutual_gravity_measured(float x, float y, float z, float m, float vx, float vy, float vz)
{
    return __builtin_fabsf(x) <= __FLT_MAX__ && __builtin_fabsf(y) <= __FLT_MAX__ && __builtin_fabsf(z) <= __FLT_MAX__ &&
           __builtin_fabsf(m) <= __FLT_MAX__ && __builtin_fabsf(vx) <= __FLT_MAX__ && __builtin_fabsf(vy) <= __FLT_MAX__ &&
           __builtin_fabsf(vz) <= __FLT_MAX__;
}

// A label the call takes: below `sets`, or "in no set".
NBODY_HD inline bool mutual_gravity_label_valid(int label, int sets) { return (label >= 0 && label < sets) || label == kMutualGravityNoSet; }
NBODY_HD inline bool mutual_gravity_labelled(int label, int sets) { return label >= 0 && label < sets; }

// The set of a body below the count, or -1: in no set, or unmeasured.
NBODY_HD inline int mutual_gravity_set(int label, int sets, bool measured) { return mutual_gravity_labelled(label, sets) && measured ? label : -1; }

// ---- The stable counting sort by set ----------------------------------------------------------------------------------------
// Chunk c is bodies 64 c ... 64 c + 63, one wave's lanes.  `mask` is the chunk's ballot of "my set is a": bit l is lane l's.
// The rank of lane `lane` among the chunk's members of the set: the members in the lanes below it.
NBODY_HD inline int mutual_gravity_chunk_rank(unsigned long long mask, int lane)
{
    return __builtin_popcountll(mask & ((1ull << lane) - 1ull));
}
NBODY_HD inline int mutual_gravity_chunk_count(unsigned long long mask) { return __builtin_popcountll(mask); }
NBODY_HD inline int mutual_gravity_chunks(int n) { return (n + kMutualGravityBlock - 1) / kMutualGravityBlock; }

// The prefix of one set over the chunks' counts, count[c * 8 + set]: offset[c * 8 + set] takes the members of the set in the
// chunks below c.  Returns the members of the set.
NBODY_HD inline int mutual_gravity_prefix(const int *count, int chunks, int set, int *offset)
{
    int running = 0;
    for (int c = 0; c < chunks; ++c) {
        offset[c * kMutualGravityMaxSets + set] = running;
        running += count[c * kMutualGravityMaxSets + set];
    }
    return running;
}

// Where the sets start in the sorted image, and where their row blocks start among the units of work: start[a] ... start[a + 1]
// are the slots of set a, unit_start[a] ... unit_start[a + 1] the units of its blocks.  Both arrays hold sets + 1 words.
NBODY_HD inline void mutual_gravity_starts(const int *members, int sets, int *start, int *unit_start)
{
    start[0] = unit_start[0] = 0;
    for (int a = 0; a < sets; ++a) {
        start[a + 1] = start[a] + members[a];
        unit_start[a + 1] = unit_start[a] + pair_velocities_blocks(members[a]);
    }
}

// The slot of a body: its set's start, the members in the chunks below, its rank in its chunk.  Ascending body index within a
// set, so the sort is the stable one.
NBODY_HD inline int mutual_gravity_slot(const int *start, const int *offset, int chunk, int set, int rank)
{
    return start[set] + offset[chunk * kMutualGravityMaxSets + set] + rank;
}

// The most units a system of max_bodies bodies in `sets` sets can have: every set may end in a ragged block.
NBODY_HD inline int mutual_gravity_max_units(int max_bodies, int sets) { return max_bodies / kMutualGravityBlock + sets; }

// The set whose blocks hold unit u (u below unit_start[sets]).
NBODY_HD inline int mutual_gravity_unit_set(const int *unit_start, int u)
{
    int a = 0;
    while (u >= unit_start[a + 1])
        ++a;
    return a;
}

// The whole sort of one system on the host, through the functions above: set[i] is mutual_gravity_set of body i (i < n);
// order[slot] takes the body of every slot, start and unit_start as mutual_gravity_starts leaves them, members[a] the count of
// set a.  count and offset are scratch of chunks x 8 words each.
inline void mutual_gravity_sort(const int *set, int n, int sets, int *count, int *offset, int *members, int *start, int *unit_start,
                                int *order)
{
    const int chunks = mutual_gravity_chunks(n);
    for (int c = 0; c < chunks; ++c)
        for (int a = 0; a < sets; ++a) {
            unsigned long long mask = 0;
            for (int lane = 0; lane < kMutualGravityBlock; ++lane)
                if (c * kMutualGravityBlock + lane < n && set[c * kMutualGravityBlock + lane] == a)
                    mask |= 1ull << lane;
            count[c * kMutualGravityMaxSets + a] = mutual_gravity_chunk_count(mask);
        }
    for (int a = 0; a < sets; ++a)
        members[a] = mutual_gravity_prefix(count, chunks, a, offset);
    mutual_gravity_starts(members, sets, start, unit_start);
    for (int c = 0; c < chunks; ++c)
        for (int a = 0; a < sets; ++a) {
            unsigned long long mask = 0;
            for (int lane = 0; lane < kMutualGravityBlock; ++lane)
                if (c * kMutualGravityBlock + lane < n && set[c * kMutualGravityBlock + lane] == a)
                    mask |= 1ull << lane;
            for (int lane = 0; lane < kMutualGravityBlock; ++lane)
                if (mask >> lane & 1ull)
                    order[mutual_gravity_slot(start, offset, c, a, mutual_gravity_chunk_rank(mask, lane))] = c * kMutualGravityBlock + lane;
        }
}

// ---- One pair ----------------------------------------------------------------------------------------------------------------
// A column as the image holds it, 16 bytes; a row as its lane holds it, widened; the four sums of a row over one source set.
struct MutualGravityColumn {
    float x, y, z, m;
};
struct MutualGravityRow {
    double x, y, z, mm, vx, vy, vz;
};
struct MutualGravitySums {
    double P, A[3];
};

NBODY_HD inline MutualGravityRow mutual_gravity_row(float x, float y, float z, float m, float vx, float vy, float vz)
{
    return MutualGravityRow{(double)x, (double)y, (double)z, (double)m, (double)vx, (double)vy, (double)vz};
}
NBODY_HD inline void mutual_gravity_clear(MutualGravitySums &a) { a.P = a.A[0] = a.A[1] = a.A[2] = 0.0; }
NBODY_HD inline double mutual_gravity_e2(float softening) { return (double)softening * (double)softening; }

// Row i meets column j: `examined` iff the row is a body of its set and j != i.  An examined pair with s2 == 0 is counted and
// adds nothing; any other pair that is not examined adds +0.0, which changes no bit of a sum that started at +0.0 (such a sum
// is never -0), so that no accumulator is branched around.
NBODY_HD inline void mutual_gravity_step(MutualGravitySums &a, unsigned int &coincident, bool examined, const MutualGravityRow &row,
                                         const MutualGravityColumn &col, double e2)
{
    const double dx = (double)col.x - row.x, dy = (double)col.y - row.y, dz = (double)col.z - row.z;
    const double s2 = ((dx * dx + dy * dy) + dz * dz) + e2;
    const bool apart = s2 != 0.0;
    const bool adds = examined && apart;
    const double r = __builtin_sqrt(apart ? s2 : 1.0);
    const double inv = 1.0 / r;
    const double mi = (double)col.m * inv;
    const double g = (mi * inv) * inv;
    coincident += examined && !apart ? 1u : 0u;
    a.P += adds ? mi : 0.0;
    a.A[0] += adds ? g * dx : 0.0;
    a.A[1] += adds ? g * dy : 0.0;
    a.A[2] += adds ? g * dz : 0.0;
}

// The nine addends of a row from its sums over one source set; a missing rank (`present` false) gives +0.0 nine times.
NBODY_HD inline void mutual_gravity_addends(bool present, const MutualGravityRow &row, const MutualGravitySums &a, const double *centre,
                                            const double *velocity, double *w)
{
    const double fx = row.mm * a.A[0], fy = row.mm * a.A[1], fz = row.mm * a.A[2];
    const double px = row.x - centre[0], py = row.y - centre[1], pz = row.z - centre[2];
    const double qx = row.vx - velocity[0], qy = row.vy - velocity[1], qz = row.vz - velocity[2];
    w[0] = present ? row.mm * a.P : 0.0;
    w[1] = present ? fx : 0.0;
    w[2] = present ? fy : 0.0;
    w[3] = present ? fz : 0.0;
    w[4] = present ? py * fz - pz * fy : 0.0;
    w[5] = present ? pz * fx - px * fz : 0.0;
    w[6] = present ? px * fy - py * fx : 0.0;
    w[7] = present ? (px * fx + py * fy) + pz * fz : 0.0;
    w[8] = present ? (qx * fx + qy * fy) + qz * fz : 0.0;
}

// ---- Records -----------------------------------------------------------------------------------------------------------------
// The examined pairs of entry (a, b).
NBODY_HD inline long long mutual_gravity_pairs(int members_a, int members_b, bool same)
{
    return (long long)members_a * (long long)members_b - (same ? (long long)members_a : 0ll);
}

// An entry is ten words of eight bytes: pairs, then the nine sums in the order of the addends.  Word 1 + k from the total of
// addend k: the potential is 0.0 - total, every other word the total itself.
static_assert(sizeof(BatchMutualGravityEntry) == 8 * (1 + kMutualGravityTerms), "ten words of eight bytes");
NBODY_HD inline void mutual_gravity_store(BatchMutualGravityEntry *out, int k, double total)
{
    const double word = k == 0 ? 0.0 - total : total;
    __builtin_memcpy(reinterpret_cast<char *>(out) + 8 * (1 + k), &word, 8);
}

// One word of an entry from the partials of its row blocks: partial of block q of the set, source set b, addend k at
// partials[((unit_start_a + q) * sets + b) * 9 + k], added in ascending q from +0.0.
NBODY_HD inline double mutual_gravity_total(const double *partials, int unit_start_a, int blocks_a, int sets, int b, int k)
{
    return pair_velocities_total(0.0, partials + ((long long)unit_start_a * sets + b) * kMutualGravityTerms + k, sets * kMutualGravityTerms,
                                 blocks_a);
}

// The mass of a set: its columns in ascending slot, which is ascending body index, one add each from +0.0.
NBODY_HD inline double mutual_gravity_mass(const MutualGravityColumn *cols, int first, int last)
{
    double mass = 0.0;
    for (int j = first; j < last; ++j)
        mass += (double)cols[j].m;
    return mass;
}

}  // namespace nbody
