// nbody_batch_groups_math.h -- the arithmetic of nbody_batch_groups (include/nbody_batch_groups.h) that needs no GPU: the
// three records and their empty values, the link predicate, the Link, Hook and Compress steps of one row on an array of
// labels, the fp64 sums of one group and the system summary.  Plain C++17 without HIP, like nbody_batch_members_math.h:
// batch_groups_kernel (nbody_batch_analysis.hip) calls these per row with the labels in LDS, and a stand-alone driver
// (tests/batch_groups_driver.cpp) runs whole systems through the same functions in sequential loops on the CPU, where
// tests/test_batch_groups_cpu.py compares them with a union-find.  Internal; the public surface is
// include/nbody_batch_groups.h.
#pragma once

#ifndef NBODY_HD
#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif
#endif

namespace nbody {

constexpr int kGroupsMaxSweeps = 64;  // NBODY_BATCH_GROUPS_MAX_SWEEPS
constexpr int kGroupsWeightMass = 0, kGroupsWeightNumber = 1;  // NBODY_BATCH_WEIGHT_MASS, NBODY_BATCH_WEIGHT_NUMBER

// The image of one body while the sweeps run: four words {x, y, z, label}, so that a column is one 16-byte read.  The labels
// are addressed through an int view of the image: label j is word 4 j + 3.
constexpr int kGroupsWords = 4, kGroupsLabelWord = 3;
NBODY_HD inline int groups_label_at(int j) { return kGroupsWords * j + kGroupsLabelWord; }

// nbody_batch_group_body's layout (nbody_batch_analysis.hip asserts it): 8 bytes.
struct BatchGroupBody {
    int group, size;
};

// nbody_batch_group_record's layout (nbody_batch_analysis.hip asserts it): 64 bytes.
struct BatchGroupRecord {
    double weight, centre[3], velocity[3];
    int count, sources;
};

// nbody_batch_group_system's layout (nbody_batch_analysis.hip asserts it): 32 bytes.
struct BatchGroupSystem {
    int groups, grouped, singles, largest, largest_count, sweeps, converged, reserved;
};

// Slots from the count on, slots that are no root, and a system without bodies (no sweep was run, which counts as converged).
NBODY_HD inline BatchGroupBody groups_empty_body() { return BatchGroupBody{-1, 0}; }
NBODY_HD inline BatchGroupRecord groups_empty_record() { return BatchGroupRecord{0.0, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, 0, 0}; }
NBODY_HD inline BatchGroupSystem groups_empty_system() { return BatchGroupSystem{0, 0, 0, -1, 0, 0, 1, 0}; }

// ---- Link ---------------------------------------------------------------------------------------------------------------
// r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) with d = x_j - x_i: bit-symmetric in i and j (d changes sign, its squares do not).
NBODY_HD inline float groups_r2(float xi, float yi, float zi, float xj, float yj, float zj)
{
    const float dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// Friends iff r2 <= b2.  False for NaN on either side; b2 = 0 links coincident bodies alone.
NBODY_HD inline bool groups_friends(float r2, float b2) { return r2 <= b2; }

// One column of row i's Link step: c <- min(c, L_j) if j is a friend.  The row's own column may pass through here as well:
// c starts at L_i, and the row's own label cannot lower it.
NBODY_HD inline int groups_link(int c, float xi, float yi, float zi, float xj, float yj, float zj, int label_j, float b2)
{
    const int low = label_j < c ? label_j : c;
    return groups_friends(groups_r2(xi, yi, zi, xj, yj, zj), b2) ? low : c;
}

// The sweep lowered row i's label.
NBODY_HD inline bool groups_lowered(int c, int label_i) { return c < label_i; }

// ---- Hook and Compress: words is the int view of the image, amin(int *address, int value) an integer min that commutes
// (an LDS atomic on the device, a plain min in a sequential loop) -------------------------------------------------------------
// Row i, whose Link step gave c < L_i: its root takes min(L[root], c), and the row takes c.  Where the row is its own root the
// two are one min; where it is not, no other row writes the row's label (hooks aim at roots alone).
template <class AtomicMin>
NBODY_HD inline void groups_hook(int *words, int i, int label_i, int c, AtomicMin amin)
{
    amin(words + groups_label_at(label_i), c);
    if (label_i != i)
        words[groups_label_at(i)] = c;
}

// One pass of Compress for row i: what L_i becomes, L[L_i].  The caller writes it after every row has read.
NBODY_HD inline int groups_compress(const int *words, int i) { return words[groups_label_at(words[groups_label_at(i)])]; }

// ---- Records --------------------------------------------------------------------------------------------------------------
// w_j: the mass word of a source (j < m), 0 for a test particle -- a select, so that the word is not read into the result --
// or 1 for every body.
NBODY_HD inline float groups_weight(int weight, float mass_word, bool source)
{
    return weight == kGroupsWeightNumber ? 1.f : (source ? mass_word : 0.f);
}

// The sums of one group, formed member by member in ascending index.  Each product of two floats is exact in fp64.
struct GroupSums {
    double w = 0.0, wx = 0.0, wy = 0.0, wz = 0.0, wu = 0.0, wv = 0.0, ww = 0.0;
    int count = 0, sources = 0;
};

// Column j with its weight and position: added if it carries the row's label.  A column outside the group adds +0.0, which
// leaves every sum's bits as they are (no sum is ever -0.0: they start at +0.0, and x + (-x) is +0.0), so a loop over all
// columns and a loop over the members alone give the same bits.
NBODY_HD inline void groups_add_position(GroupSums &s, bool same, bool source, float w, float x, float y, float z)
{
    const double dw = (double)w;
    s.w += same ? dw : 0.0;
    s.wx += same ? dw * (double)x : 0.0;
    s.wy += same ? dw * (double)y : 0.0;
    s.wz += same ? dw * (double)z : 0.0;
    s.count += same ? 1 : 0;
    s.sources += same && source ? 1 : 0;
}

NBODY_HD inline void groups_add_velocity(GroupSums &s, bool same, float w, float u, float v, float ww)
{
    const double dw = (double)w;
    s.wu += same ? dw * (double)u : 0.0;
    s.wv += same ? dw * (double)v : 0.0;
    s.ww += same ? dw * (double)ww : 0.0;
}

// The record of a group from its sums: one fp64 division per component, 0 where the weight is 0.
NBODY_HD inline BatchGroupRecord groups_record(const GroupSums &s)
{
    const bool none = s.w == 0.0;
    return BatchGroupRecord{s.w,
                            {none ? 0.0 : s.wx / s.w, none ? 0.0 : s.wy / s.w, none ? 0.0 : s.wz / s.w},
                            {none ? 0.0 : s.wu / s.w, none ? 0.0 : s.wv / s.w, none ? 0.0 : s.ww / s.w},
                            s.count, s.sources};
}

// ---- The system summary from the roots ------------------------------------------------------------------------------------
// The largest group is the largest key: the count above the root's complement, so that ties go to the lower root.  Counts and
// roots stay below 2^13 (4096 bodies at most), the key below 2^26.  No root: key -1.
constexpr int kGroupsKeyShift = 13, kGroupsKeyNone = -1;
NBODY_HD inline int groups_key(int count, int root) { return (count << kGroupsKeyShift) | ((1 << kGroupsKeyShift) - 1 - root); }
NBODY_HD inline int groups_key_count(int key) { return key < 0 ? 0 : key >> kGroupsKeyShift; }
NBODY_HD inline int groups_key_root(int key) { return key < 0 ? -1 : (1 << kGroupsKeyShift) - 1 - (key & ((1 << kGroupsKeyShift) - 1)); }

// What the roots add up to: integers, so the order of the additions does not matter.
struct GroupTally {
    int groups = 0, grouped = 0, singles = 0, key = kGroupsKeyNone;
};

NBODY_HD inline void groups_tally_root(GroupTally &t, int count, int root, int min_members)
{
    t.groups += count >= min_members ? 1 : 0;
    t.grouped += count >= min_members ? count : 0;
    t.singles += count == 1 ? 1 : 0;
    const int key = groups_key(count, root);
    t.key = key > t.key ? key : t.key;
}

NBODY_HD inline BatchGroupSystem groups_summary(const GroupTally &t, int sweeps, int converged)
{
    return BatchGroupSystem{t.groups, t.grouped, t.singles, groups_key_root(t.key), groups_key_count(t.key), sweeps, converged, 0};
}

}  // namespace nbody
