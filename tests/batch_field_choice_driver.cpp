// Prints what csrc/nbody_batch_choice.h chooses with an external field (include/nbody_batch_field.h) as text for
// tests/test_batch_field_cpu.py.  One command per line on stdin, one line of output each (numbers as text: 0, 1e-9, inf, nan):
//   step|evolve field_set integrator massive_set radii_set collision_radius escape_radius collision_action tracer_action max_bodies softening
//       -> the line tests/batch_choice_driver.cpp prints for the same settings, then |field (0 or 1)
//   component kind p0 p1 p2   -> the message batch_field_component_error returns, or none
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
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "step" || cmd == "evolve") {
            BatchConfig c;
            int field, massive, radii, max_bodies;
            std::cin >> field >> c.integrator >> massive >> radii;
            c.field_set = field != 0;
            c.massive_set = massive != 0;
            c.radii_set = radii != 0;
            c.collision_radius = number(std::cin);
            c.escape_radius = number(std::cin);
            std::cin >> c.collision_action >> c.tracer_action >> max_bodies;
            const float softening = number(std::cin);
            const BatchChoice k = cmd == "step" ? batch_step_choice(c, max_bodies, softening) : batch_evolve_choice(c, max_bodies, softening);
            static const char *const names[] = {"step",  "step_massive", "hermite", "hermite_massive",  "adaptive",
                                                "stop",  "merge",        "radii",   "adaptive_massive", "fate"};
            const char *family = names[(int)k.kernel];
            if (k.refusal != BatchRefusal::none)
                std::printf("none|0|0|0|0|%d:%s|%d\n", batch_refusal_status(k.refusal), batch_refusal_message(k.refusal), (int)k.field);
            else
                std::printf("%s|%d|%d|%d|%zu|none|%d\n", family, k.rpl, k.threads, (int)k.guard, k.lds, (int)k.field);
        } else if (cmd == "component") {
            int kind;
            std::cin >> kind;
            const float p[3] = {number(std::cin), number(std::cin), number(std::cin)};
            const char *msg = batch_field_component_error(kind, p);
            std::printf("%s\n", msg ? msg : "none");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
