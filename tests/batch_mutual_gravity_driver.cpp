// Runs whole systems through the arithmetic of csrc/nbody_batch_mutual_gravity_math.h (include/nbody_batch_mutual_gravity.h)
// on the CPU for tests/test_batch_mutual_gravity_cpu.py: the functions batch_mutual_gravity_kernel calls, here lane by lane in
// sequential loops, for any workgroup shape.
// Commands on stdin:
//   system N SETS T -> then one line "eps cx cy cz vx vy vz" (eps an fp32 word as its 32 bits in decimal, the frame's fp64
//                    words as their 64 bits), then N lines "x y z m vx vy vz label", every fp32 word as its 32 bits in decimal,
//                    the label 0 ... 255.  T threads, a multiple of 64.  Prints  sets selected left_out unmeasured pairs
//                    coincident members[8] mass[8]  and then one line per entry (a, b), a first: pairs and the nine sums, every
//                    fp64 word as its 64 bits in decimal.
//   sort N SETS   -> then one line of N sets (-1: none).  Prints the body of every slot, then start[0 ... SETS], then
//                    unit_start[0 ... SETS].
//   layout        -> sizes and offsets of the two records
//   limits        -> the limits, the block, the terms, the most chunks, and the most units of 4096 bodies in 8 sets
#include "nbody_batch_mutual_gravity_math.h"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static float float_of(unsigned int bits)
{
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
}

static double double_of(unsigned long long bits)
{
    double d;
    std::memcpy(&d, &bits, sizeof d);
    return d;
}

static unsigned long long bits_of(double d)
{
    unsigned long long w;
    std::memcpy(&w, &d, sizeof w);
    return w;
}

struct Body {
    float x, y, z, m, vx, vy, vz;
    int label;
};

static void run(int n, int sets, int T, float eps, const double *centre, const double *velocity, const std::vector<Body> &body)
{
    const int waves = T / kMutualGravityBlock, chunks = mutual_gravity_chunks(n);
    // who is in which set
    std::vector<int> set((size_t)(n > 0 ? n : 1), -1);
    int selected = 0, left_out = 0, unmeasured = 0;
    for (int i = 0; i < n; ++i) {
        const Body &b = body[(size_t)i];
        const bool labelled = mutual_gravity_labelled(b.label, sets);
        set[(size_t)i] = mutual_gravity_set(b.label, sets, mutual_gravity_measured(b.x, b.y, b.z, b.m, b.vx, b.vy, b.vz));
        selected += set[(size_t)i] >= 0 ? 1 : 0;
        left_out += !labelled ? 1 : 0;
        unmeasured += labelled && set[(size_t)i] < 0 ? 1 : 0;
    }
    // the sort
    std::vector<int> count((size_t)(chunks > 0 ? chunks : 1) * kMutualGravityMaxSets), offset(count.size(), -1), order((size_t)(n > 0 ? n : 1), -1);
    int members[kMutualGravityMaxSets], start[kMutualGravityMaxSets + 1], unit_start[kMutualGravityMaxSets + 1];
    mutual_gravity_sort(set.data(), n, sets, count.data(), offset.data(), members, start, unit_start, order.data());
    std::vector<MutualGravityColumn> cols((size_t)(selected > 0 ? selected : 1));
    for (int slot = 0; slot < selected; ++slot) {
        const Body &b = body[(size_t)order[(size_t)slot]];
        cols[(size_t)slot] = MutualGravityColumn{b.x, b.y, b.z, b.m};
    }
    // the units, round the waves
    const double e2 = mutual_gravity_e2(eps);
    const int units = unit_start[sets];
    std::vector<double> partials((size_t)mutual_gravity_max_units(n, sets) * sets * kMutualGravityTerms, -1.0);  // one never written would show
    unsigned long long coincident = 0;
    for (int wave = 0; wave < waves; ++wave)
        for (int u = wave; u < units; u += waves) {
            const int a = mutual_gravity_unit_set(unit_start, u);
            for (int b = 0; b < sets; ++b) {
                double w[kMutualGravityTerms][kMutualGravityBlock];
                for (int lane = 0; lane < kMutualGravityBlock; ++lane) {
                    const int rank = (u - unit_start[a]) * kMutualGravityBlock + lane, slot = start[a] + rank;
                    const bool present = rank < members[a];
                    MutualGravityRow row = mutual_gravity_row(0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
                    if (present) {
                        const Body &me = body[(size_t)order[(size_t)slot]];
                        row = mutual_gravity_row(cols[(size_t)slot].x, cols[(size_t)slot].y, cols[(size_t)slot].z, cols[(size_t)slot].m, me.vx,
                                                 me.vy, me.vz);
                    }
                    MutualGravitySums sums;
                    mutual_gravity_clear(sums);
                    unsigned int met = 0;
                    for (int j = start[b]; j < start[b + 1]; ++j)
                        mutual_gravity_step(sums, met, present && j != slot, row, cols[(size_t)j], e2);
                    coincident += met;
                    double mine[kMutualGravityTerms];
                    mutual_gravity_addends(present, row, sums, centre, velocity, mine);
                    for (int k = 0; k < kMutualGravityTerms; ++k)
                        w[k][lane] = mine[k];
                }
                for (int k = 0; k < kMutualGravityTerms; ++k)
                    partials[((size_t)u * sets + b) * kMutualGravityTerms + k] = pair_velocities_tree(w[k]);
            }
        }
    // the records
    BatchMutualGravitySystem s{};
    s.sets = sets;
    s.selected = selected;
    s.left_out = left_out;
    s.unmeasured = unmeasured;
    s.coincident = (long long)coincident;
    std::vector<BatchMutualGravityEntry> out((size_t)(sets * sets));
    for (int a = 0; a < sets; ++a) {
        s.members[a] = members[a];
        s.mass[a] = mutual_gravity_mass(cols.data(), start[a], start[a + 1]);
        for (int b = 0; b < sets; ++b) {
            BatchMutualGravityEntry &e = out[(size_t)(a * sets + b)];
            e.pairs = mutual_gravity_pairs(members[a], members[b], a == b);
            s.pairs += e.pairs;
            for (int k = 0; k < kMutualGravityTerms; ++k)
                mutual_gravity_store(&e, k, mutual_gravity_total(partials.data(), unit_start[a], unit_start[a + 1] - unit_start[a], sets, b, k));
        }
    }
    std::printf("%d %d %d %d %lld %lld", s.sets, s.selected, s.left_out, s.unmeasured, s.pairs, s.coincident);
    for (int a = 0; a < kMutualGravityMaxSets; ++a)
        std::printf(" %d", s.members[a]);
    for (int a = 0; a < kMutualGravityMaxSets; ++a)
        std::printf(" %llu", bits_of(s.mass[a]));
    std::printf("\n");
    for (const BatchMutualGravityEntry &e : out)
        std::printf("%lld %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", e.pairs, bits_of(e.potential), bits_of(e.force[0]), bits_of(e.force[1]),
                    bits_of(e.force[2]), bits_of(e.torque[0]), bits_of(e.torque[1]), bits_of(e.torque[2]), bits_of(e.virial), bits_of(e.power));
}

static int run_system(std::istringstream &in)
{
    int n = 0, sets = 0, T = 0;
    in >> n >> sets >> T;
    if (n < 0 || n > kMutualGravityMaxChunks * kMutualGravityBlock || sets < 1 || sets > kMutualGravityMaxSets || T < kMutualGravityBlock ||
        T % kMutualGravityBlock) {
        std::fprintf(stderr, "system: bad N, SETS or T\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream frame_line(line);
    unsigned int eps_bits = 0;
    unsigned long long f[6] = {0, 0, 0, 0, 0, 0};
    frame_line >> eps_bits;
    for (unsigned long long &w : f)
        frame_line >> w;
    const double centre[3] = {double_of(f[0]), double_of(f[1]), double_of(f[2])}, velocity[3] = {double_of(f[3]), double_of(f[4]), double_of(f[5])};
    std::vector<Body> body((size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        unsigned int w[7] = {0, 0, 0, 0, 0, 0, 0};
        for (unsigned int &x : w)
            words >> x;
        int label = kMutualGravityNoSet;
        words >> label;
        if (!mutual_gravity_label_valid(label, sets)) {
            std::fprintf(stderr, "system: bad label\n");
            return 2;
        }
        body[(size_t)i] = Body{float_of(w[0]), float_of(w[1]), float_of(w[2]), float_of(w[3]), float_of(w[4]), float_of(w[5]), float_of(w[6]), label};
    }
    run(n, sets, T, float_of(eps_bits), centre, velocity, body);
    return 0;
}

static int run_sort(std::istringstream &in)
{
    int n = 0, sets = 0;
    in >> n >> sets;
    if (n < 0 || n > kMutualGravityMaxChunks * kMutualGravityBlock || sets < 1 || sets > kMutualGravityMaxSets) {
        std::fprintf(stderr, "sort: bad N or SETS\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream words(line);
    std::vector<int> set((size_t)(n > 0 ? n : 1), -1);
    int chosen = 0;
    for (int i = 0; i < n; ++i) {
        words >> set[(size_t)i];
        if (set[(size_t)i] >= sets) {
            std::fprintf(stderr, "sort: bad set\n");
            return 2;
        }
        chosen += set[(size_t)i] >= 0 ? 1 : 0;
    }
    const int chunks = mutual_gravity_chunks(n);
    std::vector<int> count((size_t)(chunks > 0 ? chunks : 1) * kMutualGravityMaxSets), offset(count.size(), -1), order((size_t)(n > 0 ? n : 1), -1);
    int members[kMutualGravityMaxSets], start[kMutualGravityMaxSets + 1], unit_start[kMutualGravityMaxSets + 1];
    mutual_gravity_sort(set.data(), n, sets, count.data(), offset.data(), members, start, unit_start, order.data());
    for (int slot = 0; slot < chosen; ++slot)
        std::printf("%d ", order[(size_t)slot]);
    std::printf("\n");
    for (int a = 0; a <= sets; ++a)
        std::printf("%d ", start[a]);
    std::printf("\n");
    for (int a = 0; a <= sets; ++a)
        std::printf("%d ", unit_start[a]);
    std::printf("\n");
    return 0;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "system") {
            if (const int status = run_system(in))
                return status;
        } else if (word == "sort") {
            if (const int status = run_sort(in))
                return status;
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchMutualGravityEntry), offsetof(BatchMutualGravityEntry, pairs),
                        offsetof(BatchMutualGravityEntry, potential), offsetof(BatchMutualGravityEntry, force), offsetof(BatchMutualGravityEntry, torque),
                        offsetof(BatchMutualGravityEntry, virial), offsetof(BatchMutualGravityEntry, power));
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchMutualGravitySystem), offsetof(BatchMutualGravitySystem, sets),
                        offsetof(BatchMutualGravitySystem, selected), offsetof(BatchMutualGravitySystem, left_out),
                        offsetof(BatchMutualGravitySystem, unmeasured), offsetof(BatchMutualGravitySystem, pairs),
                        offsetof(BatchMutualGravitySystem, coincident), offsetof(BatchMutualGravitySystem, members),
                        offsetof(BatchMutualGravitySystem, mass));
        } else if (word == "limits") {
            std::printf("%d %d %d %d %d %d\n", kMutualGravityMaxSets, kMutualGravityNoSet, kMutualGravityBlock, kMutualGravityTerms,
                        kMutualGravityMaxChunks, mutual_gravity_max_units(4096, 8));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
