// Runs whole systems through the arithmetic of csrc/nbody_batch_radial_math.h (include/nbody_batch_radial.h) on the CPU for
// tests/test_batch_radial_cpu.py: the functions batch_radial_kernel calls, in the kernel's two phases and for the kernel's
// assignment of rows and walkers to lanes -- a workgroup of T lanes (a multiple of 64) with RPL rows per lane at
// r = q * T + tid, and walker w = tid, tid + T, ... of either split.
// Commands on stdin:
//   system N SLOTS T RPL SPLIT SHELLS PROJECTED WEIGHT WANT -> then one line of SHELLS + 1 edges, one line of the frame
//                    (centre[3], velocity[3]) and N lines "x y z m vx vy vz take" (numbers read as double by strtod, so that
//                    hexadecimal floats, nan and inf are read; the body's words are narrowed to float).  SPLIT 1: one walker
//                    per (shell, term group); 0: one per shell.  WANT 0: no shell records are asked for.  Prints three lines
//                    of hexadecimal bytes: the system record; the SHELLS shell records (empty without WANT); the SLOTS body
//                    records.  Every shell record starts out as a pattern that no walker writes, so that a word nobody wrote
//                    shows.
//   layout        -> the sizes of the three records and the offsets of their fields
#include "nbody_batch_radial_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

static double read_double(std::istream &in)
{
    std::string w;
    in >> w;
    return std::strtod(w.c_str(), nullptr);
}

static void print_bytes(const void *data, size_t bytes)
{
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t k = 0; k < bytes; ++k)
        std::printf("%02x", p[k]);
    std::printf("\n");
}

// The image as the kernel keeps it: the bodies' words and one shell byte each.
struct Image {
    const std::vector<RadialPoint> *points;
    const std::vector<signed char> *shells;
    int shell(int j) const { return (*shells)[(size_t)j]; }
    RadialPoint point(int j) const { return (*points)[(size_t)j]; }
};

static int run_system(std::istringstream &in)
{
    int n = 0, slots = 0, T = 0, rpl = 0, split = 0, shells = 0, projected = 0, weight = 0, want = 0;
    in >> n >> slots >> T >> rpl >> split >> shells >> projected >> weight >> want;
    if (n < 0 || n > slots || T < 64 || T % 64 || rpl < 1 || rpl * T < slots || shells < 1 || shells > kRadialMaxShells ||
        projected < kRadialSpherical || projected > 2 || (weight != kGroupsWeightMass && weight != kGroupsWeightNumber)) {
        std::fprintf(stderr, "system: bad arguments\n");
        return 2;
    }
    std::string line;
    std::getline(std::cin, line);
    std::istringstream edge_words(line);
    std::vector<double> e2((size_t)shells + 1);
    for (double &e : e2) {
        const double edge = read_double(edge_words);
        if (!radial_edge_valid(edge)) {
            std::fprintf(stderr, "system: bad edge\n");
            return 2;
        }
        e = radial_edge2(edge);
    }
    std::getline(std::cin, line);
    std::istringstream frame_words(line);
    double frame[kRadialFrameWords];
    for (double &f : frame)
        f = read_double(frame_words);
    std::vector<RadialPoint> points((size_t)(n > 0 ? n : 1));
    std::vector<char> take((size_t)(n > 0 ? n : 1), 1);
    for (int i = 0; i < n; ++i) {
        std::getline(std::cin, line);
        std::istringstream words(line);
        RadialPoint &p = points[(size_t)i];
        p.x = (float)read_double(words);
        p.y = (float)read_double(words);
        p.z = (float)read_double(words);
        p.m = (float)read_double(words);
        p.vx = (float)read_double(words);
        p.vy = (float)read_double(words);
        p.vz = (float)read_double(words);
        int t = 1;
        words >> t;
        take[(size_t)i] = t != 0;
    }
    // Phase 1: the lanes in any order -- here descending, to make the point -- every row its shell byte and its body record.
    std::vector<signed char> shell_of((size_t)(n > 0 ? n : 1), 0);
    std::vector<BatchRadialBody> bodies((size_t)slots);
    int tally[4] = {0, 0, 0, 0};
    for (int tid = T - 1; tid >= 0; --tid)
        for (int q = 0; q < rpl; ++q) {
            const int r = q * T + tid;
            BatchRadialBody record = radial_body_absent();
            if (r < n) {
                int sh = kRadialNotTaking;
                if (take[(size_t)r]) {
                    const RadialWords b = radial_words(points[(size_t)r], frame, projected);
                    sh = radial_shell(b, e2.data(), shells);
                    tally[0] += 1;
                    tally[1] += sh == kRadialBelow ? 1 : 0;
                    tally[2] += sh == shells ? 1 : 0;
                    tally[3] += sh == kRadialUnmeasured ? 1 : 0;
                    record = radial_body(sh, b);
                }
                shell_of[(size_t)r] = (signed char)sh;
            }
            if (r < slots)
                bodies[(size_t)r] = record;
        }
    // Phase 2: the walkers of every lane, the lanes descending again; lane 0's first walker adds total_weight.
    std::vector<BatchRadialShell> records((size_t)shells);
    std::memset(records.data(), 0xAB, sizeof(BatchRadialShell) * records.size());
    const Image image{&points, &shell_of};
    double total_of_lane0 = 0.0;
    for (int tid = T - 1; tid >= 0; --tid) {
        double total = 0.0;
        for (int w = tid; w < radial_walkers(split != 0); w += T)
            radial_walker(split != 0, w, image, n, shells, frame, projected, weight, want ? records.data() : nullptr, &total);
        if (tid == 0)
            total_of_lane0 = total;
    }
    const BatchRadialSystem s = radial_system(tally[0], tally[1], tally[2], tally[3], shells, projected, total_of_lane0, frame);
    print_bytes(&s, sizeof s);
    print_bytes(records.data(), want ? sizeof(BatchRadialShell) * records.size() : 0);
    print_bytes(bodies.data(), sizeof(BatchRadialBody) * bodies.size());
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
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchRadialShell), offsetof(BatchRadialShell, count),
                        offsetof(BatchRadialShell, weight), offsetof(BatchRadialShell, radius), offsetof(BatchRadialShell, vr1),
                        offsetof(BatchRadialShell, vr2), offsetof(BatchRadialShell, vt2), offsetof(BatchRadialShell, L),
                        offsetof(BatchRadialShell, U), offsetof(BatchRadialShell, M), offsetof(BatchRadialShell, V));
            std::printf(" %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(BatchRadialSystem), offsetof(BatchRadialSystem, selected),
                        offsetof(BatchRadialSystem, below), offsetof(BatchRadialSystem, above), offsetof(BatchRadialSystem, unmeasured),
                        offsetof(BatchRadialSystem, shells), offsetof(BatchRadialSystem, projected),
                        offsetof(BatchRadialSystem, total_weight), offsetof(BatchRadialSystem, centre),
                        offsetof(BatchRadialSystem, velocity));
            std::printf(" %zu %zu %zu %zu %zu\n", sizeof(BatchRadialBody), offsetof(BatchRadialBody, shell),
                        offsetof(BatchRadialBody, reserved), offsetof(BatchRadialBody, radius), offsetof(BatchRadialBody, radial_velocity));
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
