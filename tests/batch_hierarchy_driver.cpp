// Checks the arithmetic of csrc/nbody_batch_hierarchy_math.h (include/nbody_batch_hierarchy.h) on the CPU for
// tests/test_batch_hierarchy_cpu.py.  One command per line on stdin, one line of output each (%.17g):
//   elements xi(3) vi(3) mi xj(3) vj(3) mj -> mass energy a e inclination separation hx hy hz of the pair (the state read as float)
//   merged mi ui mj uj                     -> hierarchy_merged (the operands read as float)
//   perturbation g a e mu                  -> hierarchy_perturbation (g read as float)
//   accepts energy perturbation tolerance  -> hierarchy_accepts: 0 or 1
//   threshold q e imut                     -> hierarchy_threshold
//   passes a e a_c q imut                  -> hierarchy_ratio and hierarchy_child_passes
//   imut hx hy hz cx cy cz                 -> hierarchy_mutual_inclination
//   layout                                 -> sizes of the three records and the offsets of their fields
//   empty                                  -> the empty records
#include "nbody_batch_hierarchy_math.h"

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace nbody;

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string word, w;
        if (!(in >> word))
            continue;
        std::vector<double> a;
        while (in >> w)
            a.push_back(std::strtod(w.c_str(), nullptr));
        if (word == "elements" && a.size() == 14) {
            float f[14];
            for (int k = 0; k < 14; ++k)
                f[k] = (float)a[k];
            BatchHierarchyNode rec = hierarchy_empty_node();
            hierarchy_elements(f, f + 3, f[6], f + 7, f + 10, f[13], rec);
            std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", rec.mass, rec.energy, rec.semi_major_axis,
                        rec.eccentricity, rec.inclination, rec.separation, rec.h[0], rec.h[1], rec.h[2]);
        } else if (word == "merged" && a.size() == 4) {
            const float mi = (float)a[0], ui = (float)a[1], mj = (float)a[2], uj = (float)a[3];
            std::printf("%.17g\n", (double)hierarchy_merged(mi, ui, mj, uj, (double)mi + (double)mj));
        } else if (word == "perturbation" && a.size() == 4) {
            std::printf("%.17g\n", hierarchy_perturbation((float)a[0], a[1], a[2], a[3]));
        } else if (word == "accepts" && a.size() == 3) {
            std::printf("%d\n", hierarchy_accepts(a[0], a[1], a[2]) ? 1 : 0);
        } else if (word == "threshold" && a.size() == 3) {
            std::printf("%.17g\n", hierarchy_threshold(a[0], a[1], a[2]));
        } else if (word == "passes" && a.size() == 5) {
            std::printf("%.17g %d\n", hierarchy_ratio(a[0], a[1], a[2]), hierarchy_child_passes(a[0], a[1], a[2], a[3], a[4]) ? 1 : 0);
        } else if (word == "imut" && a.size() == 6) {
            std::printf("%.17g\n", hierarchy_mutual_inclination(a.data(), a.data() + 3));
        } else if (word == "layout") {
            std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu  %zu %zu %zu %zu\n",
                        sizeof(BatchHierarchyNode), offsetof(BatchHierarchyNode, child), offsetof(BatchHierarchyNode, parent),
                        offsetof(BatchHierarchyNode, level), offsetof(BatchHierarchyNode, leaves), offsetof(BatchHierarchyNode, slot),
                        offsetof(BatchHierarchyNode, stable), offsetof(BatchHierarchyNode, mass), offsetof(BatchHierarchyNode, energy),
                        offsetof(BatchHierarchyNode, semi_major_axis), offsetof(BatchHierarchyNode, eccentricity),
                        offsetof(BatchHierarchyNode, inclination), offsetof(BatchHierarchyNode, separation),
                        offsetof(BatchHierarchyNode, perturbation), offsetof(BatchHierarchyNode, mutual_inclination),
                        offsetof(BatchHierarchyNode, h), sizeof(BatchHierarchyBody), offsetof(BatchHierarchyBody, parent),
                        offsetof(BatchHierarchyBody, root), offsetof(BatchHierarchyBody, depth), sizeof(BatchHierarchySystem),
                        offsetof(BatchHierarchySystem, nodes), offsetof(BatchHierarchySystem, singles),
                        offsetof(BatchHierarchySystem, unstable));
        } else if (word == "empty") {
            const BatchHierarchyNode n = hierarchy_empty_node();
            const BatchHierarchyBody b = hierarchy_empty_body();
            const BatchHierarchySystem s = hierarchy_empty_system();
            const double sum = n.mass + n.energy + n.semi_major_axis + n.eccentricity + n.inclination + n.separation + n.perturbation +
                               n.mutual_inclination[0] + n.mutual_inclination[1] + n.h[0] + n.h[1] + n.h[2];
            std::printf("%d %d %d %d %d %d %d %g  %d %d %d  %d %d %d %d %d %d %d %d %d %d\n", n.child[0], n.child[1], n.parent,
                        n.level, n.leaves, n.slot, n.stable, sum, b.parent, b.root, b.depth, s.nodes, s.roots, s.levels, s.converged,
                        s.singles, s.binaries, s.triples, s.higher, s.unstable, kHierarchyMaxLevels);
        } else {
            std::fprintf(stderr, "unknown command %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
