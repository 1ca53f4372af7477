// Checks the arithmetic of csrc/nbody_batch_members_math.h (include/nbody_batch_members.h) on the CPU for
// tests/test_batch_members_cpu.py.  One command per line on stdin, one line of output each:
//   energy vx vy vz Vx Vy Vz phi -> members_kinetic and members_energy of the row (%.17g): the velocity is read as float, the
//                                   frame and the potential as double
//   stays MEMBER e               -> members_stays(MEMBER != 0, e): 0 or 1 (e as strtod reads it: nan, -0.0, inf)
//   layout                       -> sizes of the two records and the offsets of their fields
//   empty                        -> the empty body record and the empty system record
#include "nbody_batch_members_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace nbody;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word;
        if (!(in >> word))
            continue;
        if (word == "energy") {
            std::string w[7];
            for (std::string &s : w)
                in >> s;
            const float vx = std::strtof(w[0].c_str(), nullptr), vy = std::strtof(w[1].c_str(), nullptr), vz = std::strtof(w[2].c_str(), nullptr);
            const double Vx = std::strtod(w[3].c_str(), nullptr), Vy = std::strtod(w[4].c_str(), nullptr), Vz = std::strtod(w[5].c_str(), nullptr);
            const double phi = std::strtod(w[6].c_str(), nullptr);
            std::printf("%.17g %.17g\n", members_kinetic(vx, vy, vz, Vx, Vy, Vz), members_energy(vx, vy, vz, Vx, Vy, Vz, phi));
        } else if (word == "stays") {
            int member = 0;
            std::string e;
            in >> member >> e;
            std::printf("%d\n", members_stays(member != 0, std::strtod(e.c_str(), nullptr)) ? 1 : 0);
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(BatchMemberBody),
                        offsetof(BatchMemberBody, potential), offsetof(BatchMemberBody, energy), offsetof(BatchMemberBody, member),
                        offsetof(BatchMemberBody, removed_at), sizeof(BatchMemberSystem), offsetof(BatchMemberSystem, bound_mass),
                        offsetof(BatchMemberSystem, centre), offsetof(BatchMemberSystem, velocity), offsetof(BatchMemberSystem, kinetic),
                        offsetof(BatchMemberSystem, potential), offsetof(BatchMemberSystem, members), offsetof(BatchMemberSystem, sources),
                        offsetof(BatchMemberSystem, iterations), offsetof(BatchMemberSystem, converged));
        } else if (word == "empty") {
            const BatchMemberBody b = members_empty_body();
            const BatchMemberSystem s = members_empty_system();
            double sum = s.bound_mass + s.kinetic + s.potential;
            for (int c = 0; c < 3; ++c)
                sum += s.centre[c] + s.velocity[c];
            std::printf("%g %g %d %d  %g %d %d %d %d %d\n", b.potential, b.energy, b.member, b.removed_at, sum, s.members, s.sources,
                        s.iterations, s.converged, kMembersMaxIterations);
        } else {
            std::fprintf(stderr, "unknown command %s\n", word.c_str());
            return 2;
        }
    }
    return 0;
}
