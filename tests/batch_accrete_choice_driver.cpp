// Prints what csrc/nbody_batch_choice.h chooses with a hit action (include/nbody_batch_accrete.h) as text for
// tests/test_batch_accrete_cpu.py.  One command per line on stdin, one line of output each:
//   integrator massive_set radii_set collision_radius escape_radius collision_action tracer_action hit_action max_bodies softening
//       -> fates|accreting|family is fate|accrete|rows per lane|threads|guard|dynamic LDS bytes|status:message (0: when not refused)
#include "nbody_batch_choice.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

using namespace nbody;

static float number(std::istream &in)
{
    std::string s;
    in >> s;
    return std::strtof(s.c_str(), nullptr);
}

int main()
{
    BatchConfig c;
    while (std::cin >> c.integrator) {
        int massive, radii, max_bodies;
        std::cin >> massive >> radii;
        c.massive_set = massive != 0;
        c.radii_set = radii != 0;
        c.collision_radius = number(std::cin);
        c.escape_radius = number(std::cin);
        std::cin >> c.collision_action >> c.tracer_action >> c.hit_action >> max_bodies;
        const float softening = number(std::cin);
        const BatchMode m = batch_mode(c);
        const BatchChoice k = batch_evolve_choice(c, max_bodies, softening);
        std::printf("%d|%d|%d|%d|%d|%d|%d|%zu|%d:%s\n", (int)m.fates, (int)m.accreting, (int)(k.kernel == BatchKernel::fate),
                    (int)k.accrete, k.rpl, k.threads, (int)k.guard, k.lds, batch_refusal_status(k.refusal),
                    batch_refusal_message(k.refusal));
    }
    return 0;
}
