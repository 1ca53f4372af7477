// nbody_capi_step.hip -- the C ABI of include/nbody.h, the step: force mode and split geometry, the pair-once plans and the
// partial-sum buffers, the force calls, the summation calls, the update and the kick-drift-kick calls, and nbody_step ...
// nbody_step_n_on with graph replay.  Host side of the reference's per-frame step bracket (kernel.cu:1225-1242).
#include "nbody_ctx.h"
#include "nbody_kernels.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

using namespace nbody;

// The cached plans and their device lists go; whatever was enqueued on them has finished (the callers wait first).
static void free_sym_tiles(nbody_ctx *c)
{
    c->sym_plans.clear();
    c->pending = nullptr;
    c->step_graph.reset();
}

// The kernel that finishes nbody_update, nbody_kdk_prepare or nbody_kdk_kick: finish_choice (nbody_launch_choice.h) on the
// context's state.
static FinishChoice finish_of(const nbody_ctx *c, FinishOp op)
{
    const bool pair_once = c->force_mode == NBODY_FORCE_SYMMETRIC;
    const bool whole = c->row_lo == 0 && c->row_count == c->n_total;
    const bool one_part_unsummed = pair_once && c->pending && !c->sym_reduced && !c->sym_rows_summed &&
                                   c->pending->g1 - c->pending->g0 == c->group_count && c->pending->row_off == 0 &&
                                   c->pending->col_off == 0;
    return finish_choice(op, pair_once, whole, one_part_unsummed, c->n_splits, c->strip_len, c->row_count);
}

// Partial sums consumed or forgotten: the next force call starts a new step (and recomputes the equal-mass flags).
static void clear_split_done(nbody_ctx *c)
{
    std::fill(c->split_done.begin(), c->split_done.end(), 0);
    c->flags_valid = false;
}

extern "C" {

// ---- the step -------------------------------------------------------------------------------

// A context that owns every row may change its split length while no partial sums are pending (NBODY_FORCE_AUTO: the two
// force modes want different ones): everything sized or indexed by splits is released and rebuilt by the next force call.
static int resplit(nbody_ctx *c, int64_t split_len)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = sync_streams(c))
        return rc;
    free_sym_tiles(c);
    c->partials.release();
    c->col_partials.release();
    c->split_len = split_len;
    c->n_splits = (int)((c->n_total + split_len - 1) / split_len);
    c->split_done.assign((size_t)c->n_splits, 0);
    c->flags_valid = false;
    c->split_mass.release();
    HIP_TRY(c, c->split_mass.ensure((size_t)std::max(1, c->n_splits)));
    c->force_mode = NBODY_FORCE_ONE_SIDED;  // the pair-once geometry (groups of splits) is set up again by the caller
    c->sym_reduced = c->sym_rows_summed = false;
    c->acc_valid = false;
    return NBODY_OK;
}

static int sym_strip_len(const nbody_ctx *c) { return nbody::sym_strip_len(c->n_splits, (int)c->split_len, c->strip_setting); }

int nbody_set_force_mode(nbody_ctx *c, int mode)
{
    if (!c || (mode != NBODY_FORCE_ONE_SIDED && mode != NBODY_FORCE_SYMMETRIC && mode != NBODY_FORCE_AUTO))
        return fail(c, NBODY_ERR_INVALID, "nbody_set_force_mode: unknown mode");
    if (mode == NBODY_FORCE_AUTO) {  // the faster mode for this body count, with the split length that mode wants
        if (c->row_lo != 0 || c->row_count != c->n_total)
            return fail(c, NBODY_ERR_INVALID, "nbody_set_force_mode: NBODY_FORCE_AUTO needs a context that owns every row (the "
                                              "split length of a shard is part of the sharding)");
        mode = c->n_total >= NBODY_PAIR_ONCE_MIN_BODIES ? NBODY_FORCE_SYMMETRIC : NBODY_FORCE_ONE_SIDED;
        const int64_t want = mode == NBODY_FORCE_SYMMETRIC ? nbody_pair_once_split_len(c->n_total) : nbody_default_split_len(c->n_total);
        if (want != c->split_len) {
            int rc = resplit(c, want);
            if (rc != NBODY_OK)
                return rc;
        }
    }
    if (mode == NBODY_FORCE_SYMMETRIC && c->force_mode != NBODY_FORCE_SYMMETRIC) {
        if (c->split_len < 256 || c->split_len > 4096 || c->split_len % kTile != 0)
            return fail(c, NBODY_ERR_INVALID,
                        "nbody_set_force_mode: the pair-once mode needs 256 <= split_len <= 4096, a multiple of 256 (create the context with "
                        "split_len = nbody_pair_once_split_len(n_total))");
        // the canonical summation: kSymGroups groups of ceil(n_splits / kSymGroups) splits; a context owns whole groups
        const int gs = std::max(1, (c->n_splits + kSymGroups - 1) / kSymGroups);
        const int split_lo = (int)(c->row_lo / c->split_len);
        const int split_hi = (int)((c->row_lo + c->row_count + c->split_len - 1) / c->split_len);
        const int64_t row_hi = c->row_lo + c->row_count;
        if (c->row_count && row_hi % c->split_len != 0 && row_hi != c->n_total)
            return fail(c, NBODY_ERR_INVALID, "nbody_set_force_mode: in the pair-once mode a context's rows must end on a split "
                                              "boundary or at n_total (a tile's row side is a whole split)");
        if (c->row_count && (split_lo % gs != 0 || (split_hi % gs != 0 && split_hi != c->n_splits)))
            return fail(c, NBODY_ERR_INVALID,
                        "nbody_set_force_mode: in the pair-once mode a context's rows must be whole groups of " +
                            std::to_string(gs) + " splits (n_splits / 8, rounded up)");
        c->group_splits = gs;
        c->group_lo = split_lo / gs;
        c->group_count = c->row_count ? (split_hi + gs - 1) / gs - c->group_lo : 0;
        c->strip_len = sym_strip_len(c);
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->sym_acc.ensure((size_t)c->row_count));
        HIP_TRY(c, c->rowsum.ensure((size_t)kSymGroups * (size_t)c->row_count));
        while (c->ev_tiles.size() < (size_t)kSymGroups) {
            OwnedEvent a, b;
            HIP_TRY(c, hipEventCreateWithFlags(&a.h, hipEventDisableTiming));
            HIP_TRY(c, hipEventCreateWithFlags(&b.h, hipEventDisableTiming));
            c->ev_tiles.push_back(std::move(a));
            c->ev_red.push_back(std::move(b));
        }
        if (!c->colparts) {
            HIP_TRY(c, c->colparts_own.ensure((size_t)kSymGroups * (size_t)c->n_total));
            c->colparts = c->colparts_own.ptr;
        }
        c->sym_reduced = c->sym_rows_summed = false;
    }
    c->force_mode = mode;
    clear_split_done(c);
    c->acc_valid = false;
    c->step_graph.reset();
    return NBODY_OK;
}

int nbody_set_strip_len(nbody_ctx *c, int len)
{
    if (!c || !(len == 0 || len == 1 || len == 2 || len == 4 || len == 8))
        return fail(c, NBODY_ERR_INVALID, "nbody_set_strip_len: expected 0 (automatic), 1, 2, 4 or 8");
    if (c->strip_setting != len) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (int rc = sync_streams(c))
            return rc;
        free_sym_tiles(c);  // the cached plans carry the strips
        clear_split_done(c);
    }
    c->strip_setting = len;
    if (c->force_mode == NBODY_FORCE_SYMMETRIC)
        c->strip_len = sym_strip_len(c);
    c->acc_valid = false;
    return NBODY_OK;
}

int nbody_sym_set_colparts(nbody_ctx *c, float *d_buf)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->step_graph.reset();
    if (d_buf) {
        c->colparts = reinterpret_cast<float4 *>(d_buf);
    } else {
        if (!c->colparts_own.ptr && c->n_total) {
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, c->colparts_own.ensure((size_t)kSymGroups * (size_t)c->n_total));
        }
        c->colparts = c->colparts_own.ptr;
    }
    c->sym_reduced = c->sym_rows_summed = false;
    return NBODY_OK;
}

int nbody_sym_groups(const nbody_ctx *c, int64_t *group_lo, int64_t *group_count, int64_t *group_splits)
{
    if (!c || c->force_mode != NBODY_FORCE_SYMMETRIC)
        return NBODY_ERR_INVALID;
    if (group_lo) *group_lo = c->group_lo;
    if (group_count) *group_count = c->group_count;
    if (group_splits) *group_splits = c->group_splits;
    return NBODY_OK;
}

static int all_splits_done(nbody_ctx *c, const char *who);

int nbody_sym_reduce(nbody_ctx *c)
{
    if (!c || c->force_mode != NBODY_FORCE_SYMMETRIC)
        return fail(c, NBODY_ERR_INVALID, "nbody_sym_reduce: the context is not in the pair-once mode");
    int rc = all_splits_done(c, "nbody_sym_reduce");
    if (rc != NBODY_OK)
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->pending)
        return fail(c, NBODY_ERR_STATE, "nbody_sym_reduce: no force call since the last update");
    // the groups of the last part; the earlier parts' sums were formed beside the tile launches
    const nbody_ctx::SymPart &p = *c->pending;
    HIP_TRY(c, launch_sym_colparts(c->col_partials.ptr + p.col_off, c->colparts, (int)c->n_total, (int)c->split_len, c->n_splits,
                                   p.split_lo, c->group_splits, p.g0, p.g1 - p.g0, c->stream));
    c->sym_reduced = true;
    return NBODY_OK;
}

// The row-side sums of the last part's rows (every earlier part's were formed beside the tile launches).  They need this
// context's own partial sums only, so a sharded host runs them while the column-side sums are on the wire:
// forces -> nbody_sym_reduce -> [start the exchange] -> nbody_sym_rowsum -> [exchange lands] -> nbody_update.
static int sym_rowsum_on(nbody_ctx *c, hipStream_t stream)
{
    if (!c || c->force_mode != NBODY_FORCE_SYMMETRIC)
        return fail(c, NBODY_ERR_INVALID, "nbody_sym_rowsum: the context is not in the pair-once mode");
    int rc = all_splits_done(c, "nbody_sym_rowsum");
    if (rc != NBODY_OK)
        return rc;
    if (!c->pending)
        return fail(c, NBODY_ERR_STATE, "nbody_sym_rowsum: no force call since the last update");
    if (c->sym_rows_summed)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const nbody_ctx::SymPart &p = *c->pending;
    HIP_TRY(c, launch_sym_rowsum(reinterpret_cast<const float3 *>(c->partials.ptr) + p.row_off, c->rowsum.ptr + p.b0,
                                 (int)(c->row_lo + p.b0), (int)p.rows, (int)c->split_len, c->n_splits, c->group_splits,
                                 (int)c->row_count, c->strip_len, stream));
    c->sym_rows_summed = true;
    return NBODY_OK;
}

int nbody_sym_rowsum(nbody_ctx *c) { return sym_rowsum_on(c, c ? c->stream : nullptr); }

// Pair-once mode: what is still missing of the group sums -- the column-side sums of the last part (unless nbody_sym_reduce
// has run: a shard exchanges them first) and the row-side sums of its rows.  After it rowsum[g][b] and colparts[g][b] hold
// every group's two halves for the context's rows.
static int sym_group_sums(nbody_ctx *c, const char *who)
{
    if (!c->sym_reduced) {
        if (c->row_lo != 0 || c->row_count != c->n_total)
            return fail(c, NBODY_ERR_STATE, std::string(who) + ": pair-once mode on a shard: call nbody_sym_reduce and exchange "
                                                                 "the column sums first");
        // One context, both halves still to do (a pass launched in one part: with strips the whole summation stands behind the
        // force pass): the row-side sums on the auxiliary stream BESIDE the column-side sums -- two HBM-bound walks over
        // different arrays, 0.6 + 0.7 ms one after the other at N = 2^20.
        if (!c->sym_rows_summed) {
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
            HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
            int rc = sym_rowsum_on(c, c->aux_stream);
            if (rc == NBODY_OK)
                rc = nbody_sym_reduce(c);
            if (rc != NBODY_OK)
                return rc;
            HIP_TRY(c, hipEventRecord(c->ev_join, c->aux_stream));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
            c->sym_reduced = c->sym_rows_summed = false;
            return NBODY_OK;
        }
        int rc = nbody_sym_reduce(c);
        if (rc != NBODY_OK)
            return rc;
    }
    int rc = nbody_sym_rowsum(c);
    if (rc != NBODY_OK)
        return rc;
    c->sym_reduced = c->sym_rows_summed = false;
    return NBODY_OK;
}

// The partial sums the update kernels add up: the [n_splits][row_count] array of the one-sided kernel, or, in the
// pair-once mode, the one "split" sym_combine produces from the row sums and the (exchanged) column sums.
static int summed_partials(nbody_ctx *c, const char *who, const float4 **partials, int *n_splits)
{
    int rc = all_splits_done(c, who);
    if (rc != NBODY_OK)
        return rc;
    if (c->force_mode != NBODY_FORCE_SYMMETRIC) {
        *partials = c->partials.ptr;
        *n_splits = c->n_splits;
        return NBODY_OK;
    }
    rc = sym_group_sums(c, who);
    if (rc != NBODY_OK)
        return rc;
    const int n_groups = (c->n_splits + c->group_splits - 1) / c->group_splits;
    HIP_TRY(c, launch_sym_combine(c->rowsum.ptr, c->colparts, c->sym_acc.ptr, (int)c->row_lo, (int)c->row_count, (int)c->n_total, n_groups,
                                  c->stream));
    *partials = c->sym_acc.ptr;
    *n_splits = 1;
    return NBODY_OK;
}

int nbody_set_summation_parts(nbody_ctx *c, int parts)
{
    if (!c || !(parts == 0 || parts == 1 || parts == 2 || parts == 4 || parts == 8))
        return fail(c, NBODY_ERR_INVALID, "nbody_set_summation_parts: expected 0 (default), 1, 2, 4 or 8");
    if (c->sum_parts != parts) {
        HIP_TRY(c, hipSetDevice(c->device));
        if (int rc = sync_streams(c))
            return rc;
        free_sym_tiles(c);  // the cached plans carry the cut into parts
        clear_split_done(c);
    }
    c->sum_parts = parts;
    c->acc_valid = false;
    return NBODY_OK;
}

int nbody_set_early_summation(nbody_ctx *c, int on) { return nbody_set_summation_parts(c, on ? 0 : 1); }

int64_t nbody_partial_sum_bytes(const nbody_ctx *c)
{
    return c ? (int64_t)(c->partials.capacity * sizeof(float4) + c->col_partials.capacity * sizeof(float3)) : 0;
}

// The partial-sum array of the one-sided mode (a mode switch may need a larger one).
static int ensure_partials(nbody_ctx *c)
{
    const size_t entries = (size_t)c->n_splits * (size_t)c->row_count;  // [n_splits][rows] float4
    if (entries <= c->partials.capacity)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->step_graph.reset();  // a captured step would keep launching on the array freed here
    if (c->partials.ptr)
        if (int rc = sync_streams(c))
            return rc;
    if (c->partials.ensure(entries) != hipSuccess)
        return fail(c, NBODY_ERR_ALLOC, "partial sums: hipMalloc of " + std::to_string(sizeof(float4) * entries >> 20) +
                                            " MiB failed (a longer split_len needs less)");
    return NBODY_OK;
}

// The two partial-sum arrays of the pair-once mode, in 12-byte entries: what the plan of a force call needs (the whole pass,
// or two parts of it).  They only grow.
static int ensure_sym_buffers(nbody_ctx *c, size_t row_entries, size_t col_entries)
{
    const size_t row_f4 = (row_entries * sizeof(float3) + sizeof(float4) - 1) / sizeof(float4);
    if (row_f4 <= c->partials.capacity && col_entries <= c->col_partials.capacity)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    c->step_graph.reset();  // a captured step would keep launching on the arrays freed here
    if (int rc = sync_streams(c))
        return rc;
    if (c->partials.ensure(row_f4) != hipSuccess)
        return fail(c, NBODY_ERR_ALLOC, "row-side partial sums: hipMalloc of " + std::to_string(sizeof(float4) * row_f4 >> 20) +
                                            " MiB failed (more summation parts or a longer split_len need less)");
    if (c->col_partials.ensure(col_entries) != hipSuccess)
        return fail(c, NBODY_ERR_ALLOC, "column-side partial sums: hipMalloc of " +
                                            std::to_string(sizeof(float3) * col_entries >> 20) +
                                            " MiB failed (more summation parts or a longer split_len need less)");
    return NBODY_OK;
}

// The equal-mass flags once per step, by its first force call: a later call for other columns (the complement launch on a
// second stream, the ring's chunks) would rewrite the same values under the kernels that read them
static int ensure_split_flags(nbody_ctx *c, const float4 *pos)
{
    if (c->flags_valid) {
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_flags, 0));  // written on the stream of the step's first call
        return NBODY_OK;
    }
    HIP_TRY(c, launch_split_mass(pos, c->split_mass.ptr, (int)c->n_total, (int)c->split_len, c->equal_mass_path, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_flags, c->stream));
    c->flags_valid = true;
    return NBODY_OK;
}

static void mark_splits_done(nbody_ctx *c, int first, int count, bool complement)
{
    for (int s = 0; s < c->n_splits; ++s)
        if ((s >= first && s < first + count) != complement)
            c->split_done[(size_t)s] = 1;
}

static_assert(sizeof(SymStrip) == sizeof(int4) && std::is_standard_layout<SymStrip>::value, "strips go to the device as int4");
static_assert(sizeof(SymDiag) == sizeof(int2) && std::is_standard_layout<SymDiag>::value, "diagonal tiles go to the device as int2");

// The plan of this context's force calls for one column range: built by the first such call (nbody_sym_plan.h) and uploaded
// in one step -- ONE allocation holds every part's strips, then every part's diagonal tiles; nothing stays allocated when
// that fails.
static int sym_plan_for(nbody_ctx *c, int first, int count, bool complement, const nbody_ctx::SymPlan **out)
{
    const auto key = std::make_tuple(first, count, complement);
    auto it = c->sym_plans.find(key);
    if (it == c->sym_plans.end()) {
        const SymHostPlan host = sym_build_plan({c->n_total, (int)c->split_len, c->n_splits, c->strip_len, c->row_lo, c->row_count,
                                                 c->group_splits, c->group_lo, c->group_count, first, count, complement, c->sum_parts});
        std::vector<char> bytes;
        auto append = [&](const auto &v) { bytes.insert(bytes.end(), (const char *)v.data(), (const char *)(v.data() + v.size())); };
        for (const SymPlanPart &hp : host.parts)
            append(hp.strips);
        const size_t diag_bytes = bytes.size();
        for (const SymPlanPart &hp : host.parts)
            append(hp.diag);
        nbody_ctx::SymPlan plan;
        HIP_TRY(c, hipSetDevice(c->device));
        if (!bytes.empty()) {
            HIP_TRY(c, plan.lists.ensure(bytes.size()));
            const hipError_t e = hipMemcpy(plan.lists.ptr, bytes.data(), bytes.size(), hipMemcpyHostToDevice);
            if (e != hipSuccess)
                return fail(c, NBODY_ERR_DEVICE, std::string("hipMemcpy(pair-once plan): ") + hipGetErrorString(e));
        }
        const int4 *tiles = reinterpret_cast<const int4 *>(plan.lists.ptr);
        const int2 *diag = reinterpret_cast<const int2 *>(plan.lists.ptr + diag_bytes);
        for (const SymPlanPart &hp : host.parts) {
            const int n_tiles = (int)hp.strips.size(), n_diag = (int)hp.diag.size();
            plan.parts.push_back({hp.g0, hp.g1, hp.split_lo, hp.b0, hp.rows, n_tiles ? tiles : nullptr, n_diag ? diag : nullptr,
                                  n_tiles, n_diag, hp.row_off, hp.col_off});
            tiles += n_tiles;
            diag += n_diag;
        }
        plan.row_entries = host.row_entries;
        plan.col_entries = host.col_entries;
        it = c->sym_plans.emplace(key, std::move(plan)).first;
    }
    *out = &it->second;
    return NBODY_OK;
}

// Pair-once mode: this context's tiles with a column split in the range asked for, in the parts of the range's plan.
static int sym_forces(nbody_ctx *c, const float4 *pos, int first, int count, bool complement, float softening, const char *who)
{
    const int S = c->n_splits, L = (int)c->split_len;
    const bool whole = c->row_lo == 0 && c->row_count == c->n_total && !complement && first == 0 && count == S;
    if (!whole && c->pending && c->pending->g1 - c->pending->g0 != c->group_count)
        for (int sp = 0; sp < S; ++sp)
            if (c->split_done[(size_t)sp])
                return fail(c, NBODY_ERR_STATE, std::string(who) + ": a column range after a call for all columns in several "
                                                                    "summation parts: the earlier parts are already summed");
    const int SL = c->strip_len;
    if (SL > 1 && (first % SL != 0 || ((first + count) % SL != 0 && first + count != S)))
        return fail(c, NBODY_ERR_INVALID, std::string(who) + ": with strips of " + std::to_string(SL) + " column splits a column "
                                                              "range must start and end on a multiple of that many splits");
    const nbody_ctx::SymPlan *found = nullptr;
    if (int rc = sym_plan_for(c, first, count, complement, &found))
        return rc;
    const nbody_ctx::SymPlan &plan = *found;
    {
        int rc = ensure_sym_buffers(c, plan.row_entries, plan.col_entries);
        if (rc != NBODY_OK)
            return rc;
    }
    const int K = (int)plan.parts.size();
    SymArgs sa;
    sa.pos = pos;
    sa.n_total = (int)c->n_total;
    sa.split_len = L;
    sa.eps2 = softening * softening;
    sa.eps_pp = c->eps_pp;
    sa.split_mass = c->split_mass.ptr;
    // 3 (default): packed two-columns-per-step loops, eight rows per lane on every tile of splits of whole 1024 bodies -- one
    // kernel holds the equal-mass loop (S8) and the loop for arbitrary masses (S9), allocated for three waves per SIMD, which
    // costs the equal-mass loop 0.1 % against its own four-waves kernel (144.33 / 144.39 against 144.17 / 144.19 ms per
    // N = 2^20 pass, profiles/r03_ab_packed3_equal_mass.txt) and gives every tile with arbitrary masses the eight-row loop
    // (164.0 against 176.2 ms with the four-row loop, profiles/r03_ab_general_mass_eight_rows.txt).  The other arrangements
    // stay reachable through nbody_set_rows_per_lane for A/B measurement in one process: 2 = round 2's (equal-mass tiles eight
    // rows in a four-waves kernel, the others four rows), 4 = four rows per lane everywhere, 1 = the one-column loops.
    sa.packed = sym_packed(c->rows_per_lane, c->equal_mass_path);
    sa.equal_mass_path = c->equal_mass_path ? 1 : 0;
    const SymChoice tiles = sym_tile_choice(L, sa.eps2 > 0.f, sa.eps_pp != nullptr, sa.packed, c->strip_len);
    auto part_args = [&](const nbody_ctx::SymPart &p) {
        sa.row_partials = reinterpret_cast<float3 *>(c->partials.ptr) + p.row_off;
        sa.col_partials = c->col_partials.ptr + p.col_off;
        sa.tiles = p.tiles;
        sa.n_tiles = p.n_tiles;
        sa.strip_len = c->strip_len;
        sa.diag_tiles = p.diag;
        sa.n_diag = p.n_diag;
        sa.row_lo = (int)(c->row_lo + p.b0);
        sa.row_count = (int)p.rows;
    };
    HIP_TRY(c, hipSetDevice(c->device));
    if (tiles.reads_flags())
        if (int rc = ensure_split_flags(c, sa.pos))
            return rc;
    // The auxiliary stream, beside the tile launches: a part's diagonal tiles (pairs inside one split; their own slot of
    // the row-side array: 0.56 ms at N = 2^20 that no longer stands between the tiles and the summation), and, once the
    // part's tile launch is over, its column-side sums per group and the row-side sums of its rows.  With two slots the
    // diagonal tiles of part p + 2 follow the sums of part p on this stream, and the tile launch of part p + 2 waits for
    // them (they ran beside part p + 1's tiles).
    // (small systems, one part: the tile launch serves the diagonal tiles and nothing runs beside it -- no fork, no join:
    // an eagerly enqueued step at N = 1024 took 29 us with them against 18.5 us replayed as a graph)
    const bool aux_idle = tiles.serves_diag() && K == 1;
    if (!aux_idle) {
        HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_fork, 0));
    }
    auto diag_launch = [&](int p) -> int {
        if (aux_idle)
            return NBODY_OK;
        part_args(plan.parts[(size_t)p]);
        TimedLaunch t(c, &c->ev_aux, &c->aux_ms, &c->aux_launches, c->aux_stream, true);  // reported separately
        HIP_TRY(c, launch_forces_symmetric_diag(sa, c->aux_stream));
        return NBODY_OK;
    };
    for (int p = 0; p < std::min(K, 2); ++p)
        if (int rc = diag_launch(p))
            return rc;
    // Two parts (7 groups + 1): the last part's tiles go on a stream of the LOWEST priority that does not wait for the first
    // part's -- the dispatcher serves the first part's workgroups while it has any and fills their tail with the second
    // part's, so the extra launch costs no tail, and the first part's summation (7/8 of it) runs beside the second part's
    // tiles instead of behind the pass.
    if (K == 2 && !c->tail_stream) {
        int least = 0, greatest = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->tail_stream.h, hipStreamNonBlocking, least));
    }
    for (int p = 0; p < K; ++p) {
        const nbody_ctx::SymPart &part = plan.parts[(size_t)p];
        hipStream_t ts = K == 2 && p == 1 ? c->tail_stream.h : c->stream;
        if (ts != c->stream)
            HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_fork, 0));  // the positions and the equal-mass flags are in place
        if (K > 2 && p >= 2)
            HIP_TRY(c, hipStreamWaitEvent(ts, c->ev_red[(size_t)p - 2], 0));
        part_args(part);
        {
            TimedLaunch t(c, &c->ev_force, &c->force_ms, &c->force_launches, ts, true);  // the dominant kernel alone
            HIP_TRY(c, launch_forces_symmetric(sa, ts));
        }
        if (p == K - 1) {
            if (ts != c->stream) {  // the last part's sums are formed on the context's stream
                HIP_TRY(c, hipEventRecord(c->ev_tiles[(size_t)p], ts));
                HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_tiles[(size_t)p], 0));
            }
            break;
        }
        HIP_TRY(c, hipEventRecord(c->ev_tiles[(size_t)p], ts));
        HIP_TRY(c, hipStreamWaitEvent(c->aux_stream, c->ev_tiles[(size_t)p], 0));
        {
            TimedLaunch t(c, &c->ev_aux, &c->aux_ms, &c->aux_launches, c->aux_stream, true);  // overlapped, like the diagonal
            HIP_TRY(c, launch_sym_colparts(c->col_partials.ptr + part.col_off, c->colparts, (int)c->n_total, L, S, part.split_lo,
                                           c->group_splits, part.g0, part.g1 - part.g0, c->aux_stream));
            HIP_TRY(c, launch_sym_rowsum(reinterpret_cast<const float3 *>(c->partials.ptr) + part.row_off, c->rowsum.ptr + part.b0,
                                         (int)(c->row_lo + part.b0), (int)part.rows, L, S, c->group_splits, (int)c->row_count,
                                         c->strip_len, c->aux_stream));
        }
        HIP_TRY(c, hipEventRecord(c->ev_red[(size_t)p], c->aux_stream));
        if (p + 2 < K)
            if (int rc = diag_launch(p + 2))
                return rc;
    }
    if (!aux_idle) {
        HIP_TRY(c, hipEventRecord(c->ev_join, c->aux_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    }
    c->pending = &plan.parts.back();
    mark_splits_done(c, first, count, complement);
    c->sym_reduced = c->sym_rows_summed = false;
    return NBODY_OK;
}

// One-sided mode: every row of this context against the column splits asked for, in one launch.
static int one_sided_forces(nbody_ctx *c, const float4 *pos, int first, int count, bool complement, float softening)
{
    {
        int rc = ensure_partials(c);
        if (rc != NBODY_OK)
            return rc;
    }
    ForceArgs a;
    a.split_mass = c->split_mass.ptr;
    a.pos = pos;
    a.partials = c->partials.ptr;
    a.row_lo = (int)c->row_lo;
    a.row_count = (int)c->row_count;
    a.n_total = (int)c->n_total;
    a.split_len = (int)c->split_len;
    a.eps2 = softening * softening;
    a.eps_pp = c->eps_pp;
    if (complement) {  // every split except [first, first+count)
        a.split_first = 0;
        a.split_count = c->n_splits - count;
        a.skip_first = first;
        a.skip_count = count;
    } else {
        a.split_first = first;
        a.split_count = count;
        a.skip_first = c->n_splits;  // never reached
        a.skip_count = 0;
    }
    if (a.split_count <= 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const ForceChoice k = force_choice(c->rows_per_lane, a.split_len, c->row_count, a.split_count, c->cu_count, a.eps2 > 0.f,
                                       a.eps_pp != nullptr, c->equal_mass_path);
    a.own_split_mass = k.own_split_mass;
    if (!a.own_split_mass)
        if (int rc = ensure_split_flags(c, a.pos))
            return rc;
    {
        TimedLaunch t(c, &c->ev_force, &c->force_ms, &c->force_launches);
        HIP_TRY(c, launch_forces(a, k, c->stream));
    }
    mark_splits_done(c, first, count, complement);
    return NBODY_OK;
}

static int forces_impl(nbody_ctx *c, const float *d_pos, int64_t col_lo, int64_t col_count, float softening,
                       bool complement, const char *who)
{
    if (!c || (!d_pos && c->n_total))
        return fail(c, NBODY_ERR_INVALID, std::string(who) + ": NULL argument");
    if (!(softening >= 0.f) || !std::isfinite(softening))
        return fail(c, NBODY_ERR_INVALID, std::string(who) + ": softening must be finite and >= 0");
    if (softening > 0.f && softening < NBODY_MIN_SOFTENING)
        return fail(c, NBODY_ERR_INVALID, std::string(who) + ": 0 < softening < 1e-9 would overflow fp32 (eps^-3 x mass in the "
                                                             "self pair); use 0 (zero-distance pairs then contribute nothing)");
    if (col_lo < 0 || col_count < 0 || col_lo + col_count > c->n_total || col_lo % c->split_len != 0 ||
        ((col_lo + col_count) % c->split_len != 0 && col_lo + col_count != c->n_total))
        return fail(c, NBODY_ERR_INVALID, std::string(who) + ": column range must be split-aligned and inside [0,n_total]");
    if (c->row_count == 0 || c->n_total == 0)
        return NBODY_OK;
    const int first = (int)(col_lo / c->split_len);
    const int count = (int)((col_count + c->split_len - 1) / c->split_len);
    if (complement ? count == c->n_splits : count == 0)
        return NBODY_OK;  // no column selected
    const float4 *pos = reinterpret_cast<const float4 *>(d_pos);
    if (c->force_mode == NBODY_FORCE_SYMMETRIC)
        return sym_forces(c, pos, first, count, complement, softening, who);
    return one_sided_forces(c, pos, first, count, complement, softening);
}

int nbody_forces(nbody_ctx *c, const float *d_pos, int64_t col_lo, int64_t col_count, float softening)
{
    return forces_impl(c, d_pos, col_lo, col_count, softening, false, "nbody_forces");
}

int nbody_forces_complement(nbody_ctx *c, const float *d_pos, int64_t col_lo, int64_t col_count, float softening)
{
    return forces_impl(c, d_pos, col_lo, col_count, softening, true, "nbody_forces_complement");
}

int nbody_update(nbody_ctx *c, float *d_pos, float *d_vel, float dt)
{
    if (!c || ((!d_pos || !d_vel) && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_update: NULL argument");
    if (!std::isfinite(dt))
        return fail(c, NBODY_ERR_INVALID, "nbody_update: dt must be finite");
    if (c->row_count == 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    {
        TimedLaunch t(c, &c->ev_update, &c->update_ms, &c->update_launches);
        // Small and mid-size systems (every row, the tiles in one part, nothing summed yet): one finishing kernel instead of
        // column sums + row sums + update (finish_choice; the bits are the same either way).
        const FinishChoice k = finish_of(c, FinishOp::update);
        if (k.fused()) {
            int rc = all_splits_done(c, "nbody_update");
            if (rc != NBODY_OK)
                return rc;
            HIP_TRY(c, launch_sym_finish_update(reinterpret_cast<const float3 *>(c->partials.ptr), c->col_partials.ptr,
                                                reinterpret_cast<float4 *>(d_pos), reinterpret_cast<float4 *>(d_vel), (int)c->n_total,
                                                (int)c->split_len, c->n_splits, c->group_splits, dt, c->stream));
        } else if (k.family == FinishFamily::update_sym_kernel) {  // the combination of the group sums rides in the update kernel
            int rc = all_splits_done(c, "nbody_update");
            if (rc == NBODY_OK)
                rc = sym_group_sums(c, "nbody_update");
            if (rc != NBODY_OK)
                return rc;
            const int n_groups = (c->n_splits + c->group_splits - 1) / c->group_splits;
            HIP_TRY(c, launch_update_sym(reinterpret_cast<float4 *>(d_pos), reinterpret_cast<float4 *>(d_vel), c->rowsum.ptr, c->colparts,
                                         (int)c->row_lo, (int)c->row_count, (int)c->n_total, n_groups, dt, c->stream));
        } else {
            const float4 *partials;
            int n_splits;
            int rc = summed_partials(c, "nbody_update", &partials, &n_splits);
            if (rc != NBODY_OK)
                return rc;
            HIP_TRY(c, launch_update(reinterpret_cast<float4 *>(d_pos), reinterpret_cast<float4 *>(d_vel), partials,
                                     (int)c->row_lo, (int)c->row_count, n_splits, dt, c->stream));
        }
    }
    clear_split_done(c);
    return NBODY_OK;
}

// ---- kick-drift-kick (velocity Verlet) with cached accelerations ----------------------------------------------

static int all_splits_done(nbody_ctx *c, const char *who)
{
    for (int s = 0; s < c->n_splits; ++s)
        if (!c->split_done[(size_t)s])
            return fail(c, NBODY_ERR_STATE, std::string(who) + ": split " + std::to_string(s) +
                                                " has no partial sums (call nbody_forces for every column range first)");
    return NBODY_OK;
}

static int ensure_acc(nbody_ctx *c)
{
    if (!c->acc.ptr && c->row_count) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->acc.ensure((size_t)c->row_count));
    }
    return NBODY_OK;
}

int nbody_invalidate_forces(nbody_ctx *c)
{
    if (!c)
        return NBODY_ERR_INVALID;
    c->acc_valid = false;
    clear_split_done(c);  // partial sums of other positions are no partial sums
    return NBODY_OK;
}

int nbody_kdk_prepare(nbody_ctx *c)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if (c->row_count == 0) {
        c->acc_valid = true;
        return NBODY_OK;
    }
    if (finish_of(c, FinishOp::prepare).fused()) {  // one kernel instead of column sums + row sums + combination + copy (the same bits)
        int rc = all_splits_done(c, "nbody_kdk_prepare");
        if (rc == NBODY_OK)
            rc = ensure_acc(c);
        if (rc != NBODY_OK)
            return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, launch_sym_finish_kick(reinterpret_cast<const float3 *>(c->partials.ptr), c->col_partials.ptr, c->acc.ptr, nullptr,
                                          (int)c->n_total, (int)c->split_len, c->n_splits, c->group_splits, 0.f, false, c->stream));
        clear_split_done(c);
        c->acc_valid = true;
        return NBODY_OK;
    }
    const float4 *partials;
    int n_splits;
    int rc = summed_partials(c, "nbody_kdk_prepare", &partials, &n_splits);
    if (rc == NBODY_OK)
        rc = ensure_acc(c);
    if (rc != NBODY_OK)
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, launch_kdk_reduce(c->acc.ptr, partials, (int)c->row_count, n_splits, c->stream));
    clear_split_done(c);
    c->acc_valid = true;
    return NBODY_OK;
}

int nbody_kdk_kick_drift(nbody_ctx *c, float *d_pos, float *d_vel, float dt)
{
    if (!c || ((!d_pos || !d_vel) && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_kdk_kick_drift: NULL argument");
    if (!std::isfinite(dt))
        return fail(c, NBODY_ERR_INVALID, "nbody_kdk_kick_drift: dt must be finite");
    if (!c->acc_valid)
        return fail(c, NBODY_ERR_STATE, "nbody_kdk_kick_drift: no cached accelerations (nbody_forces + nbody_kdk_prepare first)");
    if (c->row_count == 0)
        return NBODY_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    {
        TimedLaunch t(c, &c->ev_update, &c->update_ms, &c->update_launches);
        HIP_TRY(c, launch_kdk_kick_drift(reinterpret_cast<float4 *>(d_pos), reinterpret_cast<float4 *>(d_vel), c->acc.ptr,
                                         (int)c->row_lo, (int)c->row_count, dt, c->stream));
    }
    c->acc_valid = false;  // the positions moved: a kick must follow
    return NBODY_OK;
}

int nbody_kdk_kick(nbody_ctx *c, float *d_vel, float dt)
{
    if (!c || (!d_vel && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_kdk_kick: NULL argument");
    if (!std::isfinite(dt))
        return fail(c, NBODY_ERR_INVALID, "nbody_kdk_kick: dt must be finite");
    if (c->row_count == 0) {
        c->acc_valid = true;
        return NBODY_OK;
    }
    int rc = ensure_acc(c);
    if (rc != NBODY_OK)
        return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    {
        TimedLaunch t(c, &c->ev_update, &c->update_ms, &c->update_launches);
        if (finish_of(c, FinishOp::kick).fused()) {
            rc = all_splits_done(c, "nbody_kdk_kick");
            if (rc != NBODY_OK)
                return rc;
            HIP_TRY(c, launch_sym_finish_kick(reinterpret_cast<const float3 *>(c->partials.ptr), c->col_partials.ptr, c->acc.ptr,
                                              reinterpret_cast<float4 *>(d_vel), (int)c->n_total, (int)c->split_len, c->n_splits,
                                              c->group_splits, dt, true, c->stream));
        } else {
            const float4 *partials;
            int n_splits;
            rc = summed_partials(c, "nbody_kdk_kick", &partials, &n_splits);
            if (rc != NBODY_OK)
                return rc;
            HIP_TRY(c, launch_kdk_kick(reinterpret_cast<float4 *>(d_vel), c->acc.ptr, partials, (int)c->row_count, n_splits, dt,
                                       c->stream));
        }
    }
    clear_split_done(c);
    c->acc_valid = true;
    return NBODY_OK;
}

int nbody_step_async(nbody_ctx *c, float *d_pos, float *d_vel, const float *d_masses, float dt, float softening)
{
    if (!c)
        return NBODY_ERR_INVALID;
    if ((!d_pos && c->n_total) || (!d_vel && c->row_count))
        return fail(c, NBODY_ERR_INVALID, "nbody_step: NULL positions or velocities");
    if (d_masses) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, launch_scatter_mass(reinterpret_cast<float4 *>(d_pos), d_masses, (int)c->n_total, c->stream));
        c->acc_valid = false;
    }
    if (c->n_total == 0)
        return NBODY_OK;
    int rc;
    if (c->integrator == NBODY_INTEGRATOR_KDK) {
        if (c->row_lo != 0 || c->row_count != c->n_total)
            return fail(c, NBODY_ERR_INVALID, "nbody_step: a sharded context drives kick-drift-kick through nbody_kdk_* "
                                              "(the drift must be exchanged before the forces)");
        if (!c->acc_valid) {
            rc = nbody_forces(c, d_pos, 0, c->n_total, softening);
            if (rc == NBODY_OK)
                rc = nbody_kdk_prepare(c);
            if (rc != NBODY_OK)
                return rc;
        }
        rc = nbody_kdk_kick_drift(c, d_pos, d_vel, dt);
        if (rc == NBODY_OK)
            rc = nbody_forces(c, d_pos, 0, c->n_total, softening);
        if (rc == NBODY_OK)
            rc = nbody_kdk_kick(c, d_vel, dt);
        return rc;
    }
    rc = nbody_forces(c, d_pos, 0, c->n_total, softening);
    if (rc != NBODY_OK)
        return rc;
    return nbody_update(c, d_pos, d_vel, dt);
}

int nbody_step(nbody_ctx *c, float *d_pos, float *d_vel, const float *d_masses, float dt, float softening)
{
    int rc = nbody_step_async(c, d_pos, d_vel, d_masses, dt, softening);
    return rc == NBODY_OK ? nbody_sync(c) : rc;
}

int nbody_step_n(nbody_ctx *c, int k, float dt, float softening)
{
    if (!c || k < 0)
        return fail(c, NBODY_ERR_INVALID, "nbody_step_n: bad argument");
    if ((c->n_total && !c->pos.ptr) || (c->row_count && !c->vel.ptr))
        return fail(c, NBODY_ERR_STATE, "nbody_step_n: call nbody_set_positions and nbody_set_velocities first");
    return nbody_step_n_on(c, reinterpret_cast<float *>(c->pos.ptr), reinterpret_cast<float *>(c->vel.ptr), k, dt, softening);
}

// k steps on the given buffers, one synchronisation at the end.  The first step runs eagerly (it may allocate: partial
// sums, tile lists, and in the kick-drift-kick mode it computes the initial accelerations); from the second on, when the
// system is small, ONE step is captured from the stream into a HIP graph and the graph is launched k - 1 times: the same
// kernels with the same arguments in the same order, so the same bits, without the per-launch host work and with the
// dependencies resolved on the device.
int nbody_step_n_on(nbody_ctx *c, float *d_pos, float *d_vel, int k, float dt, float softening)
{
    if (!c || k < 0)
        return fail(c, NBODY_ERR_INVALID, "nbody_step_n: bad argument");
    const bool whole = c->row_lo == 0 && c->row_count == c->n_total;
    const bool want = graph_replay_wanted(c->graph_replay, c->force_mode == NBODY_FORCE_SYMMETRIC, c->sum_parts, c->n_total,
                                          sym_tile_choice((int)c->split_len, softening * softening > 0.f, c->eps_pp != nullptr,
                                                          sym_packed(c->rows_per_lane, c->equal_mass_path), c->strip_len));
    const bool use_graph = want && whole && !c->timing && k >= 3 && c->n_total > 0;
    int s = 0;
    if (use_graph) {
        int rc = nbody_step_async(c, d_pos, d_vel, nullptr, dt, softening);  // eager: allocations, caches, first forces
        if (rc != NBODY_OK)
            return rc;
        ++s;
        nbody_ctx::GraphKey key;
        key.pos = d_pos; key.vel = d_vel; key.eps_pp = c->eps_pp; key.stream = nullptr;
        key.dt = dt; key.softening = softening;
        key.force_mode = c->force_mode; key.integrator = c->integrator; key.rows_per_lane = c->rows_per_lane;
        key.equal_mass = c->equal_mass_path;
        HIP_TRY(c, hipSetDevice(c->device));
        // The graph lives on the context's own stream (the caller's may be the legacy default stream, which cannot be
        // captured); events order it behind the eager step and the caller's stream behind it.
        hipStream_t user = c->stream;
        if (user != c->own_stream) {
            HIP_TRY(c, hipEventRecord(c->ev_graph_in, user));
            HIP_TRY(c, hipStreamWaitEvent(c->own_stream, c->ev_graph_in, 0));
        }
        if (!c->step_graph || !(c->graph_key == key)) {
            c->step_graph.reset();
            hipGraph_t graph = nullptr;
            HIP_TRY(c, hipStreamBeginCapture(c->own_stream, hipStreamCaptureModeThreadLocal));
            c->stream = c->own_stream;
            rc = nbody_step_async(c, d_pos, d_vel, nullptr, dt, softening);
            c->stream = user;
            hipError_t e = hipStreamEndCapture(c->own_stream, &graph);
            if (rc != NBODY_OK || e != hipSuccess || !graph) {
                if (graph)
                    (void)hipGraphDestroy(graph);
                return rc != NBODY_OK ? rc : fail(c, NBODY_ERR_DEVICE, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
            }
            e = hipGraphInstantiate(&c->step_graph.h, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (e != hipSuccess) {
                c->step_graph.h = nullptr;
                return fail(c, NBODY_ERR_DEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
            }
            c->graph_key = key;
        }
        for (; s < k; ++s)
            HIP_TRY(c, hipGraphLaunch(c->step_graph, c->own_stream));
        if (user != c->own_stream) {
            HIP_TRY(c, hipEventRecord(c->ev_graph_out, c->own_stream));
            HIP_TRY(c, hipStreamWaitEvent(user, c->ev_graph_out, 0));
        }
        return nbody_sync(c);
    }
    for (; s < k; ++s) {
        int rc = nbody_step_async(c, d_pos, d_vel, nullptr, dt, softening);
        if (rc != NBODY_OK)
            return rc;
    }
    return nbody_sync(c);
}

}  // extern "C"
