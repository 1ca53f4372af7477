// Prints the choices of csrc/nbody_batch_choice.h as text for tests/test_batch_choice_cpu.py.  One command per line on stdin,
// one line of output each (numbers as text: 0, 1e-9, 0.01, inf, nan):
//   step|evolve integrator massive_set radii_set collision_radius escape_radius collision_action tracer_action max_bodies softening
//       -> family|rows per lane|threads|guard|dynamic LDS bytes|none, or none|0|0|0|0|status:message when the call is refused
//   args levels n_intervals dt_max eta eta_start softening   -> the message nbody_batch_evolve_on reports, or none
//   mode massive_set radii_set collision_radius escape_radius collision_action tracer_action -> collisions|stopping|merging|fates
#include "nbody_batch_choice.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

using namespace nbody;

static const char *name(BatchKernel k)
{
    switch (k) {
    case BatchKernel::step: return "step";
    case BatchKernel::step_massive: return "step_massive";
    case BatchKernel::hermite: return "hermite";
    case BatchKernel::hermite_massive: return "hermite_massive";
    case BatchKernel::adaptive: return "adaptive";
    case BatchKernel::stop: return "stop";
    case BatchKernel::merge: return "merge";
    case BatchKernel::radii: return "radii";
    case BatchKernel::adaptive_massive: return "adaptive_massive";
    case BatchKernel::fate: return "fate";
    }
    return "unknown";
}

static float number(std::istream &in)
{
    std::string s;
    in >> s;
    return std::strtof(s.c_str(), nullptr);
}

static BatchConfig config(std::istream &in, bool with_integrator)
{
    BatchConfig c;
    int massive, radii;
    if (with_integrator)
        in >> c.integrator;
    in >> massive >> radii;
    c.massive_set = massive != 0;
    c.radii_set = radii != 0;
    c.collision_radius = number(in);
    c.escape_radius = number(in);
    in >> c.collision_action >> c.tracer_action;
    return c;
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "step" || cmd == "evolve") {
            const BatchConfig c = config(std::cin, true);
            int max_bodies;
            std::cin >> max_bodies;
            const float softening = number(std::cin);
            const BatchChoice k = cmd == "step" ? batch_step_choice(c, max_bodies, softening) : batch_evolve_choice(c, max_bodies, softening);
            if (k.refusal != BatchRefusal::none)
                std::printf("none|0|0|0|0|%d:%s\n", batch_refusal_status(k.refusal), batch_refusal_message(k.refusal));
            else
                std::printf("%s|%d|%d|%d|%zu|none\n", name(k.kernel), k.rpl, k.threads, (int)k.guard, k.lds);
        } else if (cmd == "args") {
            int levels;
            long long n_intervals;
            std::cin >> levels >> n_intervals;
            const float dt_max = number(std::cin), eta = number(std::cin), eta_start = number(std::cin), softening = number(std::cin);
            const char *msg = batch_evolve_args_error(levels, n_intervals, dt_max, eta, eta_start, softening);
            std::printf("%s\n", msg ? msg : "none");
        } else if (cmd == "mode") {
            const BatchMode m = batch_mode(config(std::cin, false));
            std::printf("%d|%d|%d|%d\n", (int)m.collisions, (int)m.stopping, (int)m.merging, (int)m.fates);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
