// Runs whole systems through the arithmetic of csrc/nbody_batch_groups_math.h (include/nbody_batch_groups.h) on the CPU for
// tests/test_batch_groups_cpu.py: the functions batch_groups_kernel calls per row, here in sequential loops with every read of
// a step before its writes.  Commands on stdin:
//   system N M WEIGHT MIN_MEMBERS MAX_SWEEPS B -> then N lines "x y z mass vx vy vz" (read as double, narrowed to float; B too,
//                                                 and b2 = B * B in float).  Prints
//                                                   sweeps converged groups grouped singles largest largest_count reserved
//                                                   the N labels
//                                                   the N sizes
//                                                   roots
//                                                   and per root "root weight cx cy cz vx vy vz count sources" (%.17g)
//   layout                                     -> sizes of the three records and the offsets of their fields
//   empty                                      -> the empty body, group and system records, and the limit
#include "nbody_batch_groups_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static float word_as_float(int w)
{
    float f;
    std::memcpy(&f, &w, sizeof f);
    return f;
}

static int float_as_word(float f)
{
    int w;
    std::memcpy(&w, &f, sizeof w);
    return w;
}

static void run_system(std::istringstream &in)
{
    int n = 0, m = 0, weight = 0, min_members = 2, max_sweeps = kGroupsMaxSweeps;
    std::string bs;
    in >> n >> m >> weight >> min_members >> max_sweeps >> bs;
    const float b = (float)std::strtod(bs.c_str(), nullptr);
    const float b2 = b * b;
    m = m < n ? m : n;
    std::vector<int> words((size_t)kGroupsWords * (size_t)(n > 0 ? n : 1));  // the image {x, y, z, label}
    std::vector<float> mass(n), vx(n), vy(n), vz(n);
    for (int i = 0; i < n; ++i) {
        std::string line, w[7];
        std::getline(std::cin, line);
        std::istringstream row(line);
        for (std::string &s : w)
            row >> s;
        for (int c = 0; c < 3; ++c)
            words[kGroupsWords * i + c] = float_as_word((float)std::strtod(w[c].c_str(), nullptr));
        words[groups_label_at(i)] = i;
        mass[i] = (float)std::strtod(w[3].c_str(), nullptr);
        vx[i] = (float)std::strtod(w[4].c_str(), nullptr);
        vy[i] = (float)std::strtod(w[5].c_str(), nullptr);
        vz[i] = (float)std::strtod(w[6].c_str(), nullptr);
    }
    const auto X = [&](int i, int c) { return word_as_float(words[kGroupsWords * i + c]); };
    const auto plain_min = [](int *address, int value) {
        if (value < *address)
            *address = value;
    };
    int sweeps = 0, converged = 1;
    std::vector<int> c(n), label(n), next(n);
    if (n > 0) {
        for (int t = 1;; ++t) {
            bool lowered = false;
            for (int i = 0; i < n; ++i) {  // Link: reads alone
                label[i] = words[groups_label_at(i)];
                c[i] = label[i];
                for (int j = 0; j < n; ++j)
                    c[i] = groups_link(c[i], X(i, 0), X(i, 1), X(i, 2), X(j, 0), X(j, 1), X(j, 2), words[groups_label_at(j)], b2);
                lowered = lowered || groups_lowered(c[i], label[i]);
            }
            sweeps = t;
            converged = lowered ? 0 : 1;
            if (!lowered)
                break;
            for (int i = 0; i < n; ++i)  // Hook: label[] was read before any write
                if (groups_lowered(c[i], label[i]))
                    groups_hook(words.data(), i, label[i], c[i], plain_min);
            for (;;) {  // Compress: every row reads, then every row writes
                bool moved = false;
                for (int i = 0; i < n; ++i) {
                    const int now = words[groups_label_at(i)];
                    next[i] = groups_compress(words.data(), now);
                    moved = moved || next[i] != now;
                }
                for (int i = 0; i < n; ++i)
                    words[groups_label_at(i)] = next[i];
                if (!moved)
                    break;
            }
            if (t >= max_sweeps)
                break;
        }
    }
    for (int i = 0; i < n; ++i)
        label[i] = words[groups_label_at(i)];
    std::vector<GroupSums> sum(n);
    GroupTally tally;
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) {
            const float w = groups_weight(weight, mass[j], j < m);
            groups_add_position(sum[i], label[j] == label[i], j < m, w, X(j, 0), X(j, 1), X(j, 2));
            groups_add_velocity(sum[i], label[j] == label[i], w, vx[j], vy[j], vz[j]);
        }
        if (label[i] == i)
            groups_tally_root(tally, sum[i].count, i, min_members);
    }
    const BatchGroupSystem s = groups_summary(tally, sweeps, converged);
    std::printf("%d %d %d %d %d %d %d %d\n", s.sweeps, s.converged, s.groups, s.grouped, s.singles, s.largest, s.largest_count, s.reserved);
    for (int i = 0; i < n; ++i)
        std::printf("%d ", label[i]);
    std::printf("\n");
    for (int i = 0; i < n; ++i)
        std::printf("%d ", sum[i].count);
    std::printf("\n");
    int roots = 0;
    for (int i = 0; i < n; ++i)
        roots += label[i] == i;
    std::printf("%d\n", roots);
    for (int i = 0; i < n; ++i) {
        if (label[i] != i)
            continue;
        const BatchGroupRecord r = groups_record(sum[i]);
        std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", i, r.weight, r.centre[0], r.centre[1], r.centre[2],
                    r.velocity[0], r.velocity[1], r.velocity[2], r.count, r.sources);
    }
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
            run_system(in);
        } else if (word == "layout") {
            std::printf("%zu %zu %zu  %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchGroupBody),
                        offsetof(BatchGroupBody, group), offsetof(BatchGroupBody, size), sizeof(BatchGroupRecord),
                        offsetof(BatchGroupRecord, weight), offsetof(BatchGroupRecord, centre), offsetof(BatchGroupRecord, velocity),
                        offsetof(BatchGroupRecord, count), offsetof(BatchGroupRecord, sources), sizeof(BatchGroupSystem),
                        offsetof(BatchGroupSystem, groups), offsetof(BatchGroupSystem, grouped), offsetof(BatchGroupSystem, singles),
                        offsetof(BatchGroupSystem, largest), offsetof(BatchGroupSystem, largest_count),
                        offsetof(BatchGroupSystem, sweeps), offsetof(BatchGroupSystem, converged), offsetof(BatchGroupSystem, reserved));
        } else if (word == "empty") {
            const BatchGroupBody b = groups_empty_body();
            const BatchGroupRecord r = groups_empty_record();
            const BatchGroupSystem s = groups_empty_system();
            double sum = r.weight;
            for (int c = 0; c < 3; ++c)
                sum += r.centre[c] + r.velocity[c];
            std::printf("%d %d  %g %d %d  %d %d %d %d %d %d %d %d  %d\n", b.group, b.size, sum, r.count, r.sources, s.groups, s.grouped,
                        s.singles, s.largest, s.largest_count, s.sweeps, s.converged, s.reserved, kGroupsMaxSweeps);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
