// nbody_launch_choice.h -- which force kernel a configuration runs and with what launch shape, which kernel finishes the step,
// the split-length rules and the automatic graph-replay rule: pure functions of their arguments.  Plain C++17 without HIP, like nbody_sym_plan.h (which tiles, in
// which order): the launchers (nbody_kernels.hip, nbody_symmetric.hip) look the chosen kernel up in their tables, the C ABI
// (nbody_capi_step.hip) reads what its sequencing needs, and a CPU test (tests/test_launch_choice_cpu.py) checks every choice without
// a GPU.  Internal; the public surface is include/nbody.h.
#pragma once
#include <cstddef>
#include <cstdint>

namespace nbody {

constexpr int kTile = 256;  // bodies per LDS tile == threads per workgroup (reference BLOCK_SIZE, kernel.cu:65)

// ---- split lengths -------------------------------------------------------------------------------------------------------

inline int64_t default_split_len(int64_t n_total)
{
    // Columns per partial sum.  A function of n_total ONLY: split boundaries define the summation order, so
    // they must not depend on the sharding.  n_total/128 rounded up to whole 256-body tiles, at most 8192
    // (32 LDS tiles): 128 splits up to 2^20 bodies (79 at the reference's 20 000), n_total/8192 beyond.
    // Many short splits keep the grid fine-grained -- at N = 65 536 a 256-column split measured 20 % faster
    // than a 4096-column one, and 8 ranks sharing N = 2^20 still get 128 row tiles x 128 splits each -- at
    // the price of 16 B x n_splits per row of partial sums (2 GiB at N = 2^20, ~0.4 % of the step time).
    if (n_total <= 0)
        return kTile;
    // Small systems (one-wave workgroups of 256 rows x one split, section "small systems" of DESIGN.md): the pass takes
    // ceil(waves / 1024) rounds on the chip's 1024 SIMDs, so 256-column splits leave the reference's own size -- 20 225 bodies:
    // 80 x 80 = 6400 waves, 6.25 per SIMD -- waiting for the SIMDs that got seven (profiles/r03_pmc_small_n_one_sided.txt: 83 % of
    // the large kernel's VALU share).  Where that decomposition needs three rounds or more the split length (a multiple of 64)
    // is the one (a multiple of 64 from 256 to 512: the one-wave kernel stages such a split whole) that minimises rounds x
    // length, rounds = ceil(rows-of-256 x splits / 1024), among the lengths that leave at least four rounds (four waves per
    // SIMD to hide each other's latencies): 20 225 and 20 000 bodies get 64 splits of 320 columns -- 5120 waves, five per SIMD,
    // 5 x 320 = 1600 columns per SIMD instead of 7 x 256 = 1792; measured 100.4 against 108.3 us per force pass, 0.108 against
    // 0.116 ms per step (profiles/r04_small_n_split.txt).  256 stays wherever nothing is strictly better (shorter splits were
    // tried: the partial sums they add cost the update more than the pass gains).  Still a function of n_total only.
    constexpr int64_t kOneWaveKernelBodies = 32768;  // below it a one-sided workgroup is one wave (force_kernel_r4pk_w1)
    const int64_t rb = (n_total + kTile - 1) / kTile;
    if (n_total < kOneWaveKernelBodies && rb * rb > 2048) {
        auto rounds = [&](int64_t L) { return ((n_total + L - 1) / L * rb + 1023) / 1024; };
        int64_t best = kTile;
        for (int64_t L = kTile + 64; L <= 2 * kTile; L += 64)
            if (rounds(L) >= 4 && rounds(L) * L < rounds(best) * best)
                best = L;
        return best;
    }
    int64_t len = (n_total + 127) / 128;
    len = (len + kTile - 1) / kTile * kTile;
    return len > 8192 ? 8192 : len;
}

inline int64_t pair_once_split_len(int64_t n_total)
{
    // 1024 = the eight-row kernel's rows per pass with two waves (four-row kernel: four waves): shorter splits idle waves,
    // longer ones coarsen the grid (N = 131072 on one GPU 3.6 / 4.6 / 6.2 ms with 1024 / 2048 / 512).  One pass writes
    // n_total^2 / split_len partial sums of 12 bytes into the two arrays: from N = 2^20 on the splits are 2048 bodies -- half
    // the partial sums (6.4 GB per pass at N = 2^20, held in 4 summation parts of which two exist at a time: 3.2 GB) and
    // 2.2 % less time per step than 1024-body splits in 8 parts at the same memory (156.0 against 159.5 ms, one GPU; one
    // rank of 8: 19.7 against 20.0 ms; profiles/r02_split_len_auto_parts_sustained.txt, r02_shard_rate_eight_rows_split_len.txt);
    // at N = 524288 one rank of 8 would lose 5 % to 2048 (a quarter of the tiles per rank), so 1024 stays below 2^20.
    // The length doubles again where 16-byte entries (round 1's layout: the bound is kept) would pass 150 GB: 4096 from
    // N = 2^23 (N = 2^22: 2048, 103 GB per pass, 26 GB held).  A function of n_total only: split boundaries define the
    // summation order.
    // Below that the splits shrink with the system (more, smaller tiles to fill the chip; one or two waves per workgroup):
    // 256 bodies up to 65 535, 512 up to 131 071 -- measured per size with the round-3 kernels, one GPU
    // (profiles/r03_split_len_mid_range.txt: N = 49 152: 0.436 / 0.479 / 0.544 ms per step with 256 / 512 / 1024; 65 536:
    // 0.722 / 0.715 / 0.840; 98 304: 1.582 / 1.524 / 1.591; 131 072: 2.79 / 2.66 / 2.62).  768 is no length for the tile
    // kernels (two waves cover 512 rows per pass: the second pass would run half empty and the equal-mass loops are off
    // where a pass is partial -- N = 196 608 ran at 8.88 ms per step with it, 5.79 with 1024).
    const double pairs16 = 16.0 * (double)n_total * (double)n_total;
    if (n_total < 65536)
        return kTile;
    if (n_total < 131072)
        return 2 * kTile;
    int64_t len;
    len = n_total >= ((int64_t)1 << 20) ? 2048 : 1024;
    while (len < 4096 && pairs16 / (double)len > 150e9)
        len *= 2;
    return len;
}

// ---- the pair-once mode --------------------------------------------------------------------------------------------------

// SymArgs::packed of a context's rows-per-lane setting (nbody_set_rows_per_lane)
inline int sym_packed(int rows_per_lane, bool equal_mass_path)
{
    int packed = rows_per_lane == 4 ? 1 : rows_per_lane == 2 ? 2 : rows_per_lane == 1 ? 0 : 3;
    if (packed >= 2 && !equal_mass_path)
        packed = 3;  // no tile can take the equal-mass loop
    return packed;
}

// A kernel family is named after its kernel; targ holds that kernel's template arguments in the order of its declaration:
// force_sym_quarter_kernel<LOOP, NH>, force_sym_kernel<W, GUARD, ROWS8, MODE>, force_sym_general_kernel<W, DIAG, GUARD, PPS>.
enum class SymFamily { none, force_sym_quarter_kernel, force_sym_kernel, force_sym_general_kernel };

struct SymChoice {
    SymFamily family = SymFamily::none;  // none: nothing to launch
    int targ[4] = {0, 0, 0, 0};
    int waves = 0;   // per workgroup
    size_t lds = 0;  // dynamic LDS bytes
    int threads() const { return 64 * waves; }
    // the quarter-tile kernel computes the diagonal tiles in the same launch: no diagonal launch, nothing beside the tiles
    bool serves_diag() const { return family == SymFamily::force_sym_quarter_kernel; }
    // ... and reads the masses itself; every other tile launch has the equal-mass flags (launch_split_mass) in front
    bool reads_flags() const { return family != SymFamily::force_sym_quarter_kernel; }
};

constexpr size_t kSymStageBytesPerWave = 2048;  // nbody_symmetric.hip: kSymStageFloatsPerWave floats

// the column-group stage, three column-sum arrays, and the per-wave eps_j^2 stage of the per-particle-softening variant
inline size_t sym_lds_bytes(int waves, int split_len)
{
    return (size_t)waves * kSymStageBytesPerWave + (size_t)split_len * 12 + (size_t)waves * 128 * sizeof(float);
}

inline SymChoice sym_choice(SymFamily family, int t0, int t1, int t2, int t3, int split_len)
{
    SymChoice k;
    k.family = family;
    k.targ[0] = t0, k.targ[1] = t1, k.targ[2] = t2, k.targ[3] = t3;
    const bool quarter = family == SymFamily::force_sym_quarter_kernel;
    k.waves = quarter ? 4 * t1 : t0;  // the quarter-tile kernel: four waves per 256 bodies of the split, its LDS is static
    k.lds = quarter ? 0 : sym_lds_bytes(k.waves, split_len);
    return k;
}

// The launch of the tiles (R != C) of a pair-once force call.  packed: SymArgs::packed; strip_len: sym_strip_len().
inline SymChoice sym_tile_choice(int split_len, bool eps, bool eps_pp, int packed, int strip_len)
{
    using F = SymFamily;
    const int L = split_len;
    // Small systems (256- and 512-body splits, the packed loops; not per-particle softening with eps = 0, where a pair may meet
    // at r^2 = 0 unguarded, and not per-particle softening at all with 512-body splits: eight waves per tile, per-particle
    // softening keeps the eight-row loops (S10 / S12) of force_sym_kernel there): the tiles AND the diagonal tiles are served
    // by force_sym_quarter_kernel in ONE launch, which needs no split_mass flags.
    if (packed >= 2 && ((L == 512 && !eps_pp) || (L == 256 && !(eps_pp && !eps))))
        return sym_choice(F::force_sym_quarter_kernel, eps_pp ? 1 : eps ? 0 : 2, L / 256, 0, 0, L);
    // MODE of force_sym_kernel: 1 = one pass covers the split, the rows stay in registers across a strip; 2 = the kernels that
    // cannot keep a strip's rows in registers add its tiles' row sums in memory (strips exist with 2048-body splits only)
    const int in_memory = strip_len > 1 ? 2 : 0;
    // eight rows per lane for the equal-mass tiles (packed == 2): half the waves per split, 512 rows each
    // (512-body splits, one wave per workgroup, measured 0.8 % slower than the four-row loop at N = 131072: multiples of
    // 1024 only)
    const int w8 = L % 2048 == 0 ? 4 : L % 1024 == 0 ? 2 : 1;  // whole passes of 512 rows per wave
    if (packed >= 2 && eps_pp && eps && L % 512 == 0)  // per-particle softening: the eight-row loop S10
        return sym_choice(F::force_sym_kernel, w8, false, 3, L == 512 * w8 ? 1 : 0, L);
    if (packed >= 2 && !eps_pp && eps && L % 1024 == 0) {
        if (packed == 3)  // both eight-row loops; for arbitrary masses too (three waves per SIMD)
            return sym_choice(F::force_sym_kernel, w8, false, 2, L == 512 * w8 ? 1 : 0, L);
        return sym_choice(F::force_sym_kernel, w8, false, 1, in_memory, L);
    }
    // waves per tile workgroup: W x 256 rows per pass must not exceed the split
    const int W = L >= 1024 ? 4 : L >= 512 ? 2 : 1;
    // per-particle softening: the four-row loop S11 with eps > 0; with eps = 0 a particle may have eps_i = 0 too and the guarded,
    // compiler-scheduled kernel runs (NBODY_SYM_PACKED=0 / rows_per_lane 4: that kernel always -- A/B, tests)
    if (eps_pp && eps && packed >= 2)
        return sym_choice(F::force_sym_kernel, W, false, 4, in_memory, L);
    if (eps_pp)
        return sym_choice(F::force_sym_general_kernel, W, false, !eps, true, L);
    return sym_choice(F::force_sym_kernel, W, !eps, 0, in_memory, L);
}

// The launch of the diagonal tiles: none where the tile launch serves them.
inline SymChoice sym_diag_choice(int split_len, bool eps, bool eps_pp, int packed)
{
    if (sym_tile_choice(split_len, eps, eps_pp, packed, 1).serves_diag())
        return SymChoice();
    // A diagonal workgroup must fit where a tile workgroup leaves: beside the two-wave tile kernels of 1024-body splits
    // (three waves of ~165 registers per SIMD) a four-wave diagonal workgroup found room only in the launch's tail -- at N = 131 072
    // the diagonal launch ended 85 us after the tiles and was the step's critical path (profiles/r04_diagonal_tiles.txt).
    const int W = split_len > 1024 ? 4 : split_len >= 512 ? 2 : 1;
    return sym_choice(SymFamily::force_sym_general_kernel, W, true, !eps, eps_pp, split_len);
}

// ---- the one-sided mode --------------------------------------------------------------------------------------------------

// force_kernel<RPL, GUARD, PPS>, force_kernel_r4<GUARD>, force_kernel_r4pk<GUARD, PPS>, force_kernel_r4pk_w1<GUARD, QT, PPS>
enum class ForceFamily { none, force_kernel, force_kernel_r4, force_kernel_r4pk, force_kernel_r4pk_w1 };

struct ForceChoice {
    int rows_per_lane = 0;  // the blocking: the setting, or the automatic one
    ForceFamily family = ForceFamily::none;  // none: no such blocking
    int targ[3] = {0, 0, 0};
    int rows_per_block = 0, threads = 0;
    bool own_split_mass = false;  // ForceArgs::own_split_mass: no launch_split_mass in front
};

// setting: nbody_set_rows_per_lane (0 = automatic; row_count, split_count and cu_count matter to that alone): 4 = the
// hand-allocated kernel (default), 41 = the same with one wave per workgroup (small systems), 40 = one row per instruction, 1/2/8
// and -4 = the compiler-allocated template.  GUARD is on when eps = 0 -- with per-particle softening too: a particle may have eps = 0.
inline ForceChoice force_choice(int setting, int split_len, int64_t row_count, int split_count, int cu_count, bool eps, bool eps_pp,
                                bool equal_mass_path)
{
    using F = ForceFamily;
    ForceChoice k;
    auto kernel = [&](F family, int t0, int t1, int t2, int rows_per_block, int threads) {
        k.family = family;
        k.targ[0] = t0, k.targ[1] = t1, k.targ[2] = t2;
        k.rows_per_block = rows_per_block, k.threads = threads;
        return k;
    };
    // Largest register blocking that still fills the chip evenly; 4 rows per lane (the hand-allocated kernel) is fastest
    // once there are enough workgroups.  With short splits (<= 512 columns: one or two LDS tiles per workgroup) a
    // workgroup is over quickly and what counts is how evenly the last ones spread: measured at the reference's N = 20 225
    // (split 256) 1 row per lane 0.145 ms, 2: 0.152, 4: 0.156; from N = 32 768 on 4 wins (tools/small_n.py).  Speed only:
    // each row's sum is the same FMA chain whatever the blocking.
    // Too few 1024-row workgroups: the same packed loop with one wave (256 rows) per workgroup -- at every size below (N =
    // 4096 ... 20 225: 29 / 34 / 59 / 78 / 121 us per step against 42 / 38 / 73 / 89 / 137 with the compiler-allocated one-row
    // kernel, profiles/r03_small_n_blocking*.txt).  Per-particle softening: the same two kernels with the softening term in
    // the loop (N = 20 225: 0.165 ms per step with the compiler-allocated one-row kernel it used to take).
    const int64_t blocks4 = (row_count + (int64_t)kTile * 4 - 1) / ((int64_t)kTile * 4) * split_count;
    k.rows_per_lane = setting ? setting : blocks4 >= (split_len <= 512 ? 10LL : 4LL) * cu_count ? 4 : 41;
    // the one-wave kernel forms the equal-mass flag of a split of up to 512 columns itself, from the columns it has staged: no launch
    // in front.  The flag covers the split's split_len columns, one at or beyond n_total counting as mass 0 (split_mass_kernel's
    // rule: the flag must not depend on who forms it) -- so not the rest of the 256-column tile staged for a split of 64, 128 or 192
    k.own_split_mass = k.rows_per_lane == 41 && split_len <= 2 * kTile && equal_mass_path;
    switch (k.rows_per_lane) {
    case 4: return kernel(F::force_kernel_r4pk, !eps, eps_pp, 0, kTile * 4, kTile);  // packed fp32; per-particle softening: its own loop
    case 41:  // packed, one wave per workgroup; QT: splits of up to 512 columns are staged whole (64 QT columns, QT >= 4)
        return kernel(F::force_kernel_r4pk_w1, !eps, split_len > 2 * kTile ? 0 : split_len > kTile ? (split_len + 63) / 64 : 4, eps_pp,
                      kTile, 64);
    case 40:  // one row per instruction
        return eps_pp ? kernel(F::force_kernel, 4, !eps, true, kTile * 4, kTile) : kernel(F::force_kernel_r4, !eps, 0, 0, kTile * 4, kTile);
    case 1: case 2: case 8: return kernel(F::force_kernel, k.rows_per_lane, !eps, eps_pp, kTile * k.rows_per_lane, kTile);
    case -4: return kernel(F::force_kernel, 4, !eps, eps_pp, kTile * 4, kTile);
    default: return k;
    }
}

// ---- the finish: partial sums into velocities and positions ------------------------------------------------------------------

// What a step runs behind its force pass.  update_kernel<BLOCK> and update_sym_kernel<BLOCK> (nbody_kernels.hip: the kick-drift
// from the one-sided partial sums / from the pair-once group sums, which sym_group_sums has completed in front),
// sym_finish_update_kernel<MODE> (nbody_symmetric.hip: column sums, row sums, combination and MODE 0 the kick-drift, 1 the
// closing half kick, 2 the acceleration alone, in one launch), kdk_kick_kernel<MODE> (0 the acceleration alone, 1 with the
// closing half kick) -- in the pair-once mode behind sym_combine_kernel (`combine`), which hands it one "split".
enum class FinishOp { update, prepare, kick };  // nbody_update, nbody_kdk_prepare, nbody_kdk_kick
enum class FinishFamily { none, update_kernel, update_sym_kernel, sym_finish_update_kernel, kdk_kick_kernel };

struct FinishChoice {
    FinishFamily family = FinishFamily::none;
    int targ = 0;          // BLOCK of the update kernels, MODE of the others
    int threads = 0;       // per workgroup
    bool combine = false;  // sym_combine_kernel in front (after whatever group sums are missing)
    bool fused() const { return family == FinishFamily::sym_finish_update_kernel; }
};

constexpr int kFusedFinishMaxSplits = 320;

// few rows: one wave per workgroup, so that every CU gets some (20 225 rows: 317 workgroups instead of 80)
inline int update_threads(int64_t row_count) { return row_count < 256 * (int64_t)kTile ? 64 : kTile; }

// pair_once: the force mode; whole: the context owns every row; one_part_unsummed: the last force call left its tiles in ONE
// summation part that holds every group of the context, at the start of both partial-sum arrays, and neither nbody_sym_reduce
// nor nbody_sym_rowsum has run since; strip_len: sym_strip_len() (pair-once mode).
// Small and mid-size pair-once systems (every row, the tiles in one part, nothing summed yet, up to 320 splits of single tiles):
// ONE finishing kernel forms the column sums, the row sums and their combination and ends in the update / the half kick (up to
// 320 splits: -4 % per step at N = 32 768, nothing from 131 072 on, profiles/r03_ab_fused_finish.txt; the bits are the same
// either way).
inline FinishChoice finish_choice(FinishOp op, bool pair_once, bool whole, bool one_part_unsummed, int n_splits, int strip_len,
                                  int64_t row_count)
{
    using F = FinishFamily;
    FinishChoice k;
    if (pair_once && whole && one_part_unsummed && n_splits <= kFusedFinishMaxSplits && strip_len == 1) {
        k.family = F::sym_finish_update_kernel;
        k.targ = op == FinishOp::update ? 0 : op == FinishOp::kick ? 1 : 2;
        k.threads = 256;
        return k;
    }
    if (op == FinishOp::update) {  // pair-once: the combination of the group sums rides in the update kernel
        k.family = pair_once ? F::update_sym_kernel : F::update_kernel;
        k.targ = k.threads = update_threads(row_count);
        return k;
    }
    k.family = F::kdk_kick_kernel;
    k.targ = op == FinishOp::kick ? 1 : 0;
    k.threads = kTile;
    k.combine = pair_once;
    return k;
}

// ---- graph replay --------------------------------------------------------------------------------------------------------

// Measured (tools/graph_ab.py, profiles/r02_graph_replay_ab.txt): a graph launch costs ~10 us more than three kernels
// enqueued back to back, so the one-sided step (flags, forces, update) is FASTER eager at every size (N = 256: 29 against
// 40 us per step; N = 20 225: 143 against 153); the pair-once step is seven launches on two streams with events between
// them, and there the replay wins up to a few ten thousand bodies (N = 4096: 96 against 114 us; N = 20 225: 169 against
// 190; N = 65 536: 801 against 788).  Automatic = pair-once mode, at most this many bodies, and a step of more than two kernels.
constexpr int64_t kGraphAutoBodies = 32768;

// graph_replay: nbody_set_graph_replay (-1: automatic); tiles: the context's sym_tile_choice()
inline bool graph_replay_wanted(int graph_replay, bool pair_once, int sum_parts, int64_t n_total, const SymChoice &tiles)
{
    // (round 4: where the tile launch serves the diagonal tiles too -- one part -- a pair-once step is two
    // kernels on one stream, and those are faster enqueued eagerly as well: N = 1024: 12.5 against 18.5 us per step, 20 225:
    // 85.9 against 91.4, profiles/r04_pair_once_small_n.txt)
    const bool two_kernels = pair_once && sum_parts <= 1 && tiles.serves_diag();  // (kick-drift-kick: three, fused finish)
    return graph_replay == 1 || (graph_replay == -1 && pair_once && n_total <= kGraphAutoBodies && !two_kernels);
}

}  // namespace nbody
