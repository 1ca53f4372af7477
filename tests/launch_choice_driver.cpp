// Prints the launch choices of csrc/nbody_launch_choice.h as text for tests/test_launch_choice_cpu.py.  One command per line on
// stdin (eps, eps_pp, equal_mass: 0 or 1), one line of output each:
//   sym split_len eps eps_pp packed strip_len
//       -> tile kernel|threads|dynamic LDS bytes|serves the diagonal|reads the flags|diagonal kernel|threads|dynamic LDS bytes
//   force blocking split_len eps eps_pp                                  -> kernel|threads|rows per workgroup
//   pick setting split_len row_count split_count cu_count equal_mass     -> blocking|own_split_mass
//   packed rows_per_lane equal_mass                                      -> SymArgs::packed
//   split n_total                                                        -> one-sided split length|pair-once split length
//   graph graph_replay pair_once sum_parts n_total split_len eps eps_pp rows_per_lane equal_mass -> replay wanted
#include "nbody_launch_choice.h"

#include <cstdio>
#include <iostream>
#include <string>

using namespace nbody;

static const char *tf(int v) { return v ? "true" : "false"; }

// the kernel with its template arguments as the source spells them: force_sym_kernel<4, false, 2, 1>
static std::string name(const SymChoice &k)
{
    char s[96];
    const int *t = k.targ;
    switch (k.family) {
    case SymFamily::force_sym_quarter_kernel: std::snprintf(s, sizeof s, "force_sym_quarter_kernel<%d, %d>", t[0], t[1]); break;
    case SymFamily::force_sym_kernel: std::snprintf(s, sizeof s, "force_sym_kernel<%d, %s, %d, %d>", t[0], tf(t[1]), t[2], t[3]); break;
    case SymFamily::force_sym_general_kernel:
        std::snprintf(s, sizeof s, "force_sym_general_kernel<%d, %s, %s, %s>", t[0], tf(t[1]), tf(t[2]), tf(t[3]));
        break;
    default: return "none";
    }
    return s;
}

static std::string name(const ForceChoice &k)
{
    char s[96];
    const int *t = k.targ;
    switch (k.family) {
    case ForceFamily::force_kernel: std::snprintf(s, sizeof s, "force_kernel<%d, %s, %s>", t[0], tf(t[1]), tf(t[2])); break;
    case ForceFamily::force_kernel_r4: std::snprintf(s, sizeof s, "force_kernel_r4<%s>", tf(t[0])); break;
    case ForceFamily::force_kernel_r4pk: std::snprintf(s, sizeof s, "force_kernel_r4pk<%s, %s>", tf(t[0]), tf(t[1])); break;
    case ForceFamily::force_kernel_r4pk_w1: std::snprintf(s, sizeof s, "force_kernel_r4pk_w1<%s, %d, %s>", tf(t[0]), t[1], tf(t[2])); break;
    default: return "none";
    }
    return s;
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "sym") {
            int split_len, eps, pps, packed, strip_len;
            std::cin >> split_len >> eps >> pps >> packed >> strip_len;
            const SymChoice t = sym_tile_choice(split_len, eps, pps, packed, strip_len);
            const SymChoice d = sym_diag_choice(split_len, eps, pps, packed);
            std::printf("%s|%d|%zu|%d|%d|%s|%d|%zu\n", name(t).c_str(), t.threads(), t.lds, (int)t.serves_diag(), (int)t.reads_flags(),
                        name(d).c_str(), d.threads(), d.lds);
        } else if (cmd == "force") {
            int blocking, split_len, eps, pps;
            std::cin >> blocking >> split_len >> eps >> pps;
            const ForceChoice k = force_choice(blocking, split_len, 0, 0, 0, eps, pps, true);
            std::printf("%s|%d|%d\n", name(k).c_str(), k.threads, k.rows_per_block);
        } else if (cmd == "pick") {
            int setting, split_len, split_count, cu_count, equal_mass;
            long long row_count;
            std::cin >> setting >> split_len >> row_count >> split_count >> cu_count >> equal_mass;
            const ForceChoice k = force_choice(setting, split_len, row_count, split_count, cu_count, true, false, equal_mass);
            std::printf("%d|%d\n", k.rows_per_lane, (int)k.own_split_mass);
        } else if (cmd == "packed") {
            int rows_per_lane, equal_mass;
            std::cin >> rows_per_lane >> equal_mass;
            std::printf("%d\n", sym_packed(rows_per_lane, equal_mass));
        } else if (cmd == "split") {
            long long n;
            std::cin >> n;
            std::printf("%lld|%lld\n", (long long)default_split_len(n), (long long)pair_once_split_len(n));
        } else if (cmd == "graph") {
            int graph_replay, pair_once, sum_parts, split_len, eps, pps, rows_per_lane, equal_mass;
            long long n_total;
            std::cin >> graph_replay >> pair_once >> sum_parts >> n_total >> split_len >> eps >> pps >> rows_per_lane >> equal_mass;
            const SymChoice t = sym_tile_choice(split_len, eps, pps, sym_packed(rows_per_lane, equal_mass), 1);
            std::printf("%d\n", (int)graph_replay_wanted(graph_replay, pair_once, sum_parts, n_total, t));
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
