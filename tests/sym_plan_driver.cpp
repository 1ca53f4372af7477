// Prints pair-once launch plans (csrc/nbody_sym_plan.h) as text for tests/test_sym_plan_cpu.py.  One command per line on stdin:
//   plan n_total split_len n_splits strip_len row_lo row_count group_splits group_lo group_count first count complement sum_parts
//   sides S                             -- sym_rows_side(R, C, S) for every R, then every C: S x S digits
//   strip n_splits split_len setting    -- sym_strip_len
#include "nbody_sym_plan.h"

#include <cstdio>
#include <iostream>
#include <string>

using namespace nbody;

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "plan") {
            SymPlanRequest q;
            int complement = 0;
            std::cin >> q.n_total >> q.split_len >> q.n_splits >> q.strip_len >> q.row_lo >> q.row_count >> q.group_splits >>
                q.group_lo >> q.group_count >> q.first >> q.count >> complement >> q.sum_parts;
            q.complement = complement != 0;
            const SymHostPlan plan = sym_build_plan(q);
            std::printf("plan %zu %zu %zu %d\n", plan.parts.size(), plan.row_entries, plan.col_entries,
                        sym_row_slots(q.n_splits, q.strip_len));
            for (const SymPlanPart &p : plan.parts) {
                std::printf("part %d %d %d %d %lld %lld %zu %zu\nstrips", p.g0, p.g1, p.split_lo, p.split_hi, (long long)p.b0,
                            (long long)p.rows, p.row_off, p.col_off);
                for (const SymStrip &s : p.strips)
                    std::printf(" %d %d %d %d", s.R, s.C0, s.count, s.slot);
                std::printf("\ndiag");
                for (const SymDiag &d : p.diag)
                    std::printf(" %d %d", d.R, d.C);
                std::printf("\n");
            }
        } else if (cmd == "sides") {
            int S = 0;
            std::cin >> S;
            for (int R = 0; R < S; ++R)
                for (int C = 0; C < S; ++C)
                    std::putchar(sym_rows_side(R, C, S) ? '1' : '0');
            std::printf("\n");
        } else if (cmd == "strip") {
            int n_splits = 0, split_len = 0, setting = 0;
            std::cin >> n_splits >> split_len >> setting;
            std::printf("%d\n", sym_strip_len(n_splits, split_len, setting));
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
