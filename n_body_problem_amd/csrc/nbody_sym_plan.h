// nbody_sym_plan.h -- the launch plan of the pair-once mode: which strips and diagonal tiles a force call launches, in which
// order, cut into which summation parts, and where each part's partial sums go.  Plain C++17 without HIP: the kernels
// (nbody_kernels.h includes this file) and the C ABI (nbody_capi_step.hip) share the geometry below, and a CPU test
// (tests/test_sym_plan_cpu.py) checks the plan without a GPU.  Internal; the public surface is include/nbody.h.
#pragma once
#include "../../include/nbody.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define NBODY_HD __host__ __device__
#else
#define NBODY_HD
#endif

namespace nbody {

// Pair-once kernel (nbody_symmetric.hip): one workgroup per ordered pair of splits (R, C), R's bodies as rows (one
// context's own rows), C's bodies as columns; each unordered pair {R, C} is computed once, by the owner of the side
// sym_rows_side() names.
constexpr int kSymGroups = 8;  // the canonical summation: 8 groups of ceil(n_splits / 8) splits, see sym_finalize

// True when the tile of the unordered split pair {R, C} (R != C) is computed with R's bodies as rows: the "forward
// half" of the ring of S splits, so every split is the row side of (S - 1) / 2 tiles -- equal work for every rank that
// owns equally many splits.  A pure function of (R, C, S): the summation kernels use it to know which partial sums exist.
NBODY_HD inline bool sym_rows_side(int R, int C, int S)
{
    int d = C - R;
    if (d < 0)
        d += S;
    if (d == 0)
        return false;
    if (2 * d != S)
        return 2 * d < S;
    const int lo = R < C ? R : C;  // S even, opposite splits: alternate
    return ((lo & 1) == 0) == (R == lo);
}

// Strips (round 4).  A workgroup takes `strip_len` = K consecutive column splits of one row split -- the splits C with equal
// C / K that form a tile with R (K = 1: every tile alone, rounds 1-3) -- and keeps the rows' sums in registers across them: one
// row-side partial sum per (row, strip) instead of per (row, tile).  The strip that holds column split C is slot
// sym_row_slot(R, C) of the row split's array: the blocks of K splits are counted along the ring from the block of R + 1 (K = 1:
// the ring distance of the tile, the layout of rounds 1-3); slot 0 is the diagonal tile.  Blocks are absolute (C / K), the
// number of splits is a multiple of 8 K, so a strip never straddles a summation group or a rank's column chunk: which sums
// exist and in which order they are added is a function of (n_total, split_len) only, as before.
NBODY_HD inline int sym_row_slot(int R, int C, int S, int K)
{
    int j = C / K - ((R + 1) % S) / K;
    if (j < 0)
        j += S / K;
    return j + 1;
}
NBODY_HD inline int sym_row_slots(int S, int K) { return K == 1 ? S / 2 + 1 : S / (2 * K) + 3; }

// Strips from the 2048-body splits on -- N >= 2^20, where the partial sums are gigabytes: a tile workgroup takes four
// consecutive column splits of its row split and keeps the rows' sums in registers across them: a quarter of the row-side
// partial sums (N = 2^20: 0.8 instead of 3.2 GB per pass; the column side keeps its 3.2 GB -- halving that as well takes a
// workgroup that owns a whole CU, measured 7 % slower: profiles/r04_ab_whole_cu_workgroup.txt).  The blocks of four are absolute
// and the number of splits must be a multiple of 8 x 4, so no strip straddles a summation group or a rank's column chunk and
// which sums exist stays a function of (n_total, split_len) alone; other split counts keep single tiles.
// Automatic (setting 0): strips of FOUR column splits from 1024 splits on (N >= 2^21), of TWO below (N = 2^20).  A strip is one
// workgroup, and a rank of eight's share of an N = 2^20 pass is only 4088 strips of four on 768 workgroup slots -- 5.3 rounds of
// 3.5 ms, six in practice: 21.6 ms against 18.7 ms with single tiles and 20.0 ms with strips of two, while one GPU runs strips of
// two and of four equally fast (146.2 ms; profiles/r04_shard_rate.txt).  A function of (n_total, split_len) only, like the split
// length: the strips define the order of the row-side sums.
inline int sym_strip_len(int n_splits, int split_len, int setting)
{
    const int want = setting ? setting : (split_len >= 2048 ? (n_splits >= 1024 ? 4 : 2) : 1);
    return want > 1 && n_splits % (kSymGroups * want) == 0 && split_len == 2048 ? want : 1;
}

struct SymStrip { int R, C0, count, slot; };  // row split R, column splits C0 ... C0 + count - 1; the layout of int4
struct SymDiag { int R, C; };                  // the diagonal tile (R, R); the layout of int2

// A part: a run of whole row groups whose tiles go in one launch and whose partial sums are added up as soon as that launch
// is over.
struct SymPlanPart {
    int g0 = 0, g1 = 0;              // row groups [g0, g1)
    int split_lo = 0, split_hi = 0;  // = row splits [split_lo, split_hi)
    int64_t b0 = 0, rows = 0;        // = rows [b0, b0 + rows) of the context
    size_t row_off = 0, col_off = 0; // where the part's [sym_row_slots][rows] and [splits][n_splits/2][split_len] arrays start
                                     // in the row-side / column-side partial sums, in 12-byte entries
    std::vector<SymStrip> strips;    // in launch order
    std::vector<SymDiag> diag;       // single tiles only: the diagonal tiles' own launch
};

struct SymHostPlan {
    std::vector<SymPlanPart> parts;
    size_t row_entries = 0, col_entries = 0;  // the partial-sum arrays the plan needs (the whole pass, or two parts of it)
};

// What a plan depends on: the context's geometry and the column range of one force call.
struct SymPlanRequest {
    int64_t n_total = 0;
    int split_len = 0, n_splits = 0, strip_len = 1;
    int64_t row_lo = 0, row_count = 0;  // the context's rows: whole splits
    int group_splits = 1, group_lo = 0, group_count = 0;
    int first = 0, count = 0;           // column splits [first, first + count) ...
    bool complement = false;            // ... or every other one
    int sum_parts = 0;                  // nbody_set_summation_parts: 0 = automatic
    bool selected(int C) const { return (C >= first && C < first + count) != complement; }
};

// The strips with a row split in [r_lo, r_hi), in launch order.
inline std::vector<SymStrip> sym_list_rows(const SymPlanRequest &q, int r_lo, int r_hi)
{
    const int S = q.n_splits, SL = q.strip_len;
    // Launch order = L2 locality (speed only; every tile has its own outputs).  The tile of row split R and ring
    // distance d has column split (R + d) mod S.  Blocks of 8 row splits x 8 distances touch 23 splits' bodies
    // instead of 128; workgroups are dealt round-robin to the MI355X's 8 XCDs, so block k's tiles
    // take the launch slots congruent to k mod 8 and meet in one XCD's L2.
    constexpr int B = 8;
    std::vector<std::vector<SymStrip>> per_xcd(8);
    const int n_blocks = S / SL;  // SL = 1: a "block" is one column split, a strip one tile, its slot the ring distance
    // the half ring and the two blocks past it, never a block twice (S = 2 would meet its one other split again)
    const int n_walk = std::min(n_blocks / 2 + 2, n_blocks);
    int k = 0;
    for (int Rb = r_lo; Rb < r_hi; Rb += B)
        for (int jb = 0; jb < n_walk; jb += B, ++k)
            for (int R = Rb; R < std::min(Rb + B, r_hi); ++R)
                for (int j = jb; j < std::min(jb + B, n_walk); ++j) {
                    const int J = (((R + 1) % S) / SL + j) % n_blocks;  // the j-th block along the ring from R + 1
                    int C0 = -1, cnt = 0;
                    for (int C = J * SL; C < (J + 1) * SL; ++C)
                        if (q.selected(C) && sym_rows_side(R, C, S)) {
                            if (cnt == 0)
                                C0 = C;
                            ++cnt;
                        }
                    if (cnt > 0)
                        per_xcd[(size_t)k % per_xcd.size()].push_back({R, C0, cnt, sym_row_slot(R, C0, S, SL)});
                }
    // Strips: the DIAGONAL tiles ride in the tile launch, as full squares of the hand-scheduled loops that keep their
    // row side (slot 0) -- 512 one-tile workgroups more for the launch's tail at N = 2^20 instead of a compiler-scheduled
    // launch beside it (0.4 % more pair evaluations; profiles/r04_strips_ab.txt)
    if (SL > 1)
        for (int R = r_lo; R < r_hi; ++R)
            if (q.selected(R))
                per_xcd[(size_t)R % per_xcd.size()].push_back({R, R, 1, 0});
    // whole strips first, the shorter ones of the band's edges behind them, longest first (the launch's tail is made
    // of ever shorter workgroups: three-tile strips, then two, then one -- 145.4 against 145.9 ms per N = 2^20 step
    // with the short ones in list order, profiles/r04_strips_ab.txt) -- inside each XCD's sequence, so that a block's
    // strips keep meeting in one L2 (a partition of the interleaved list shifted the launch slots: 4.6 instead of 1.4 GB
    // of fabric reads per N = 2^20 pass)
    for (auto &seq : per_xcd)
        std::stable_sort(seq.begin(), seq.end(), [](const SymStrip &x, const SymStrip &y) { return x.count > y.count; });
    std::vector<SymStrip> strips;
    for (size_t j = 0, more = 1; more; ++j) {
        more = 0;
        for (auto &seq : per_xcd)
            if (j < seq.size()) {
                strips.push_back(seq[j]);
                more = 1;
            }
    }
    return strips;
}

// The plan of one force call: the context's strips (and diagonal tiles) with a column split in the range asked for, cut into
// summation parts.
inline SymHostPlan sym_build_plan(const SymPlanRequest &q)
{
    const int S = q.n_splits, L = q.split_len, SL = q.strip_len;
    const int own_lo = (int)(q.row_lo / L), own_hi = (int)((q.row_lo + q.row_count + L - 1) / L);
    const bool whole = q.row_lo == 0 && q.row_count == q.n_total && !q.complement && q.first == 0 && q.count == S;
    // Summation parts (one context that owns every row, all columns in one call, a system large enough for several
    // launches): the canonical order is by row groups, so a part's sums can be formed as soon as its launch is over,
    // on the auxiliary stream beside the next part's tiles, and nothing about the result changes.  What stays behind
    // the force pass is the last part's share of the summation and the combination.  2 parts = 7 groups + 1 (one
    // extra launch tail, the arrays hold the whole pass); 4 or 8 equal parts keep two parts' arrays.
    const int n_groups = (S + q.group_splits - 1) / q.group_splits;
    int K = q.sum_parts;
    if (K == 0) {  // automatic: one launch is the fastest (profiles/r02_summation_parts_eight_rows.txt); more only for memory
        // the column side and the row side (a strip's rows are summed in registers: 1 / strip_len of the entries)
        const double pass_bytes = 6.0 * (double)q.n_total * (double)q.n_total / (double)L * (1.0 + 1.0 / (double)SL);
        // 4 parts of 3 + 3 + 1 + 1 groups hold two slots of three groups = 3/4 of the pass; 8 equal parts a quarter
        K = pass_bytes <= (double)NBODY_PARTIAL_SUM_BUDGET_BYTES ? 1 : 0.75 * pass_bytes <= (double)NBODY_PARTIAL_SUM_BUDGET_BYTES ? 4 : 8;
    }
    // below 32768 tiles (N = 2^18) an extra launch costs more than the summation it hides: the automatic choice takes
    // one part there (an explicit nbody_set_summation_parts is honoured at every size)
    const int64_t min_tiles = q.sum_parts == 0 ? 32768 : 0;
    if (!whole || (int64_t)S * S / 2 < min_tiles || n_groups < 2)
        K = 1;
    else if (K > 2 && n_groups % K != 0)
        K = 2;
    SymHostPlan plan;
    for (int p = 0; p < K; ++p) {
        SymPlanPart part;
        if (K == 1) {
            part.g0 = q.group_lo;
            part.g1 = q.group_lo + q.group_count;
        } else if (K == 2) {
            part.g0 = p ? n_groups - 1 : 0;
            part.g1 = p ? n_groups : n_groups - 1;
        } else if (K == 4 && n_groups == 8) {
            // 3 + 3 + 1 + 1 groups: what stays behind the force pass is the LAST part's summation (its partial sums are
            // read back at HBM speed: 0.2 GB per group and per million bodies^2 / split_len), so the last part is one
            // group, not two -- update_ms 0.50 -> 0.3 ms at N = 2^20 -- and the two slots hold three groups each
            static const int cut[5] = {0, 3, 6, 7, 8};
            part.g0 = cut[p];
            part.g1 = cut[p + 1];
        } else {
            part.g0 = p * (n_groups / K);
            part.g1 = (p + 1) * (n_groups / K);
        }
        part.split_lo = std::max(own_lo, part.g0 * q.group_splits);
        part.split_hi = std::min(own_hi, part.g1 * q.group_splits);
        part.b0 = (int64_t)part.split_lo * L - q.row_lo;
        part.rows = std::min<int64_t>((int64_t)part.split_hi * L, q.row_lo + q.row_count) - (int64_t)part.split_lo * L;
        const size_t row_need = (size_t)sym_row_slots(S, SL) * (size_t)part.rows;
        const size_t col_need = (size_t)(part.split_hi - part.split_lo) * (size_t)(S / 2) * (size_t)L;
        if (K > 2) {  // two slots used in turn
            plan.row_entries = std::max(plan.row_entries, 2 * row_need);
            plan.col_entries = std::max(plan.col_entries, 2 * col_need);
        } else {
            part.row_off = plan.row_entries;
            part.col_off = plan.col_entries;
            plan.row_entries += row_need;
            plan.col_entries += col_need;
        }
        part.strips = sym_list_rows(q, part.split_lo, part.split_hi);
        for (int R = part.split_lo; R < part.split_hi && SL == 1; ++R)
            if (q.selected(R))
                part.diag.push_back({R, R});
        plan.parts.push_back(std::move(part));
    }
    if (K > 2)
        for (int p = 0; p < K; ++p) {
            plan.parts[(size_t)p].row_off = (p & 1) * (plan.row_entries / 2);
            plan.parts[(size_t)p].col_off = (p & 1) * (plan.col_entries / 2);
        }
    return plan;
}

}  // namespace nbody
