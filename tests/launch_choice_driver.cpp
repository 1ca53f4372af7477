// Prints the launch choices of csrc/nbody_launch_choice.h as text for tests/test_launch_choice_cpu.py.  One command per line on
// stdin (eps, eps_pp, equal_mass: 0 or 1), one line of output each:
//   sym split_len eps eps_pp packed strip_len
//       -> tile kernel|threads|dynamic LDS bytes|serves the diagonal|reads the flags|diagonal kernel|threads|dynamic LDS bytes
//   force blocking split_len eps eps_pp                                  -> kernel|threads|rows per workgroup
//   pick setting split_len row_count split_count cu_count equal_mass     -> blocking|own_split_mass
//   packed rows_per_lane equal_mass                                      -> SymArgs::packed
//   split n_total                                                        -> one-sided split length|pair-once split length
//   graph graph_replay pair_once sum_parts n_total split_len eps eps_pp rows_per_lane equal_mass -> replay wanted
//   finish op pair_once n_total split_len row_lo row_count sum_parts strip_setting summed         -> kernel|threads|combine in front
//       op: update, prepare or kick; the state is the one a force call for every column leaves (csrc/nbody_sym_plan.h: its
//       last summation part), summed: nbody_sym_reduce or nbody_sym_rowsum has run since
//   choice op pair_once whole one_part_unsummed n_splits strip_len row_count                      -> the same, finish_choice's own inputs
#include "nbody_launch_choice.h"
#include "nbody_sym_plan.h"

#include <algorithm>
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

static std::string name(const FinishChoice &k)
{
    char s[96];
    switch (k.family) {
    case FinishFamily::update_kernel: std::snprintf(s, sizeof s, "update_kernel<%d>", k.targ); break;
    case FinishFamily::update_sym_kernel: std::snprintf(s, sizeof s, "update_sym_kernel<%d>", k.targ); break;
    case FinishFamily::sym_finish_update_kernel: std::snprintf(s, sizeof s, "sym_finish_update_kernel<%d>", k.targ); break;
    case FinishFamily::kdk_kick_kernel: std::snprintf(s, sizeof s, "kdk_kick_kernel<%d>", k.targ); break;
    default: return "none";
    }
    return s;
}

// finish_choice on the state nbody_capi_step.hip derives it from: the geometry of nbody_create_shard and nbody_set_force_mode
// and the last part of the plan of a force call for every column
static FinishChoice finish_of(const std::string &op, bool pair_once, int64_t n_total, int split_len, int64_t row_lo, int64_t row_count,
                              int sum_parts, int strip_setting, bool summed)
{
    const int n_splits = (int)((n_total + split_len - 1) / split_len);
    const FinishOp what = op == "update" ? FinishOp::update : op == "prepare" ? FinishOp::prepare : FinishOp::kick;
    const bool whole = row_lo == 0 && row_count == n_total;
    if (!pair_once)
        return finish_choice(what, false, whole, false, n_splits, 1, row_count);
    const int gs = std::max(1, (n_splits + kSymGroups - 1) / kSymGroups);
    const int split_lo = (int)(row_lo / split_len), split_hi = (int)((row_lo + row_count + split_len - 1) / split_len);
    SymPlanRequest q;
    q.n_total = n_total, q.split_len = split_len, q.n_splits = n_splits;
    q.strip_len = sym_strip_len(n_splits, split_len, strip_setting);
    q.row_lo = row_lo, q.row_count = row_count;
    q.group_splits = gs, q.group_lo = split_lo / gs, q.group_count = (split_hi + gs - 1) / gs - q.group_lo;
    q.first = 0, q.count = n_splits, q.complement = false, q.sum_parts = sum_parts;
    const SymHostPlan plan = sym_build_plan(q);
    const SymPlanPart &last = plan.parts.back();
    const bool one_part_unsummed = !summed && last.g1 - last.g0 == q.group_count && last.row_off == 0 && last.col_off == 0;
    return finish_choice(what, true, whole, one_part_unsummed, n_splits, q.strip_len, row_count);
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
        } else if (cmd == "choice") {
            std::string op;
            int pair_once, whole, one_part, n_splits, strip_len;
            long long row_count;
            std::cin >> op >> pair_once >> whole >> one_part >> n_splits >> strip_len >> row_count;
            const FinishOp what = op == "update" ? FinishOp::update : op == "prepare" ? FinishOp::prepare : FinishOp::kick;
            const FinishChoice k = finish_choice(what, pair_once, whole, one_part, n_splits, strip_len, row_count);
            std::printf("%s|%d|%d\n", name(k).c_str(), k.threads, (int)k.combine);
        } else if (cmd == "finish") {
            std::string op;
            int pair_once, split_len, sum_parts, strip_setting, summed;
            long long n_total, row_lo, row_count;
            std::cin >> op >> pair_once >> n_total >> split_len >> row_lo >> row_count >> sum_parts >> strip_setting >> summed;
            if (op != "update" && op != "prepare" && op != "kick") {
                std::fprintf(stderr, "unknown finish %s\n", op.c_str());
                return 1;
            }
            const FinishChoice k = finish_of(op, pair_once, n_total, split_len, row_lo, row_count, sum_parts, strip_setting, summed);
            std::printf("%s|%d|%d\n", name(k).c_str(), k.threads, (int)k.combine);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    return 0;
}
