// nbody_ctx.h -- the context of a single system (include/nbody.h, nbody_create ...), as the three host sources behind its C ABI
// see it: nbody_capi.hip (lifecycle, owned buffers, plain setters, timing, diagnostics), nbody_capi_step.hip (force sequencing,
// updates, step and graph replay) and nbody_capi_order.hip (body order).  Internal: nothing here crosses the C ABI.
//
// Ownership: whatever the context allocates on the device is a member that frees itself (nbody_device_owned.h), so
// nbody_destroy waits for the context's streams and deletes it.  The streams are declared first and so destroyed last.
#pragma once

#include "../../include/nbody.h"
#include "nbody_device_owned.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <string>
#include <tuple>
#include <vector>

typedef std::vector<std::pair<nbody::OwnedEvent, nbody::OwnedEvent>> EventPairs;  // start and stop of timed launches

struct nbody_ctx {
    nbody::OwnedStream own_stream;
    nbody::OwnedStream aux_stream;   // pair-once mode: the diagonal-tile launch runs here, beside the tile launch
    nbody::OwnedStream tail_stream;  // pair-once mode, two summation parts: the LAST part's tiles, lowest priority, beside the first's
    hipStream_t stream = nullptr;    // the stream work is enqueued on (own_stream or the caller's)
    int device = 0;
    int64_t n_total = 0, row_lo = 0, row_count = 0, split_len = 0;
    int n_splits = 0;
    int rows_per_lane = 0;  // 0 = pick per launch
    bool equal_mass_path = true;  // splits whose bodies share one mass take the inner loop without mass multiplies
    int sum_parts = 0;  // pair-once mode, one context: launches the row groups are cut into (nbody_set_summation_parts)
    int force_mode = NBODY_FORCE_ONE_SIDED;
    int strip_setting = 0;  // nbody_set_strip_len: 0 = automatic
    int strip_len = 1;      // pair-once mode: column splits a tile workgroup takes with the rows' sums kept in registers (SymArgs)
    int integrator = NBODY_INTEGRATOR_KICK_DRIFT;
    nbody::DeviceArray<float4> acc;  // kick-drift-kick mode: accelerations of the own rows at the current positions
    bool acc_valid = false;
    const float *eps_pp = nullptr;  // per-particle softening lengths in use, n_total floats (borrowed or eps_own), or NULL
    nbody::DeviceArray<float> eps_own;  // the copy nbody_upload_particle_softening made
    // pair-once mode (nbody_symmetric.hip)
    // One force call = one or more parts: a part is a run of whole row groups whose tiles go in one launch and whose partial
    // sums are added up (on the auxiliary stream, beside the next part's tiles) as soon as that launch is over.  With more than
    // two parts the partial sums live in two buffer slots used in turn: the arrays hold two parts, not the whole pass.
    struct SymPart {  // what the launches and the summation calls read of a part of the plan (SymPlanPart, nbody_sym_plan.h)
        int g0 = 0, g1 = 0;              // row groups [g0, g1)
        int split_lo = 0;                // their first own row split
        int64_t b0 = 0, rows = 0;        // = rows [b0, b0 + rows) of this context
        const int4 *tiles = nullptr;     // strips {R, first C, count, slot}
        const int2 *diag = nullptr;
        int n_tiles = 0, n_diag = 0;
        size_t row_off = 0, col_off = 0;  // where its arrays start in partials / col_partials, in 12-byte entries
    };
    struct SymPlan {
        std::vector<SymPart> parts;
        size_t row_entries = 0, col_entries = 0;
        nbody::DeviceArray<char> lists;  // every part's strips, then every part's diagonal tiles
    };
    std::map<std::tuple<int, int, bool>, SymPlan> sym_plans;  // per column range asked for
    const SymPart *pending = nullptr;  // the part of the last force call whose sums are still to be formed (the last one)
    std::vector<nbody::OwnedEvent> ev_tiles, ev_red;  // per part: tile launch over / its sums formed (the slot is free again)
    nbody::DeviceArray<float3> col_partials;  // column-side partial sums, see SymArgs; sized by the plan (ensure_sym_buffers)
    float4 *colparts = nullptr;      // [kSymGroups][n_total] in use: the caller's (nbody_sym_set_colparts) or colparts_own
    nbody::DeviceArray<float4> colparts_own;
    nbody::DeviceArray<float4> sym_acc;    // [row_count]: the summed accelerations the update kernels read as one split
    nbody::DeviceArray<float4> rowsum;     // [kSymGroups][row_count]: row-side sums per column group (launch_sym_rowsum)
    nbody::DeviceArray<float> split_mass;  // [n_splits]: the one mass of each split's bodies or NaN (pair-once tiles' fast path)
    bool sym_reduced = false;        // nbody_sym_reduce has run since the last forces
    bool sym_rows_summed = false;    // ... and nbody_sym_rowsum (the row-side sums of the last part)
    int group_splits = 1, group_lo = 0, group_count = 0;
    int cu_count = 256;
    // nbody_step_n on small systems: one step captured into a HIP graph and replayed (the inner loop is launch-bound).
    // The captured step bakes in every device pointer the launches take (partial sums, tile lists, exchange buffer): whatever
    // frees or replaces one of them resets the graph first, and the next nbody_step_n captures a new one.
    nbody::OwnedGraphExec step_graph;
    struct GraphKey {
        const void *pos = nullptr, *vel = nullptr, *eps_pp = nullptr, *stream = nullptr;
        float dt = 0.f, softening = 0.f;
        int force_mode = -1, integrator = -1, rows_per_lane = 0;
        bool equal_mass = false;
        bool operator==(const GraphKey &o) const
        {
            return pos == o.pos && vel == o.vel && eps_pp == o.eps_pp && stream == o.stream && dt == o.dt &&
                   softening == o.softening && force_mode == o.force_mode && integrator == o.integrator &&
                   rows_per_lane == o.rows_per_lane && equal_mass == o.equal_mass;
        }
    } graph_key;
    int graph_replay = -1;  // -1: automatic (systems of at most kGraphAutoBodies bodies), 0: off, 1: on
    nbody::OwnedEvent ev_fork, ev_join, ev_graph_in, ev_graph_out;
    nbody::OwnedEvent ev_flags;  // the step's equal-mass flags have been written (a later force call may run on another stream)
    bool flags_valid = false;    // split_mass holds the flags of the positions of this step (launch_split_mass has run since the
                                 // partial sums were last consumed or forgotten)
    nbody::DeviceArray<float4> partials;  // [n_splits][row_count]  (the reference's gravity_sum_array, kernel.cu:1148);
                                          // pair-once mode: [n_splits / 2 + 1][row_count].  Allocated at the first force call.
    nbody::DeviceArray<float4> pos;         // owned position buffer (n_total), optional
    nbody::DeviceArray<float4> vel;         // owned velocity buffer (row_count), optional
    nbody::DeviceArray<double> reduce_dev;  // per-block partials of the diagnostics kernels
    std::vector<double> reduce_host;
    std::vector<unsigned char> split_done;  // which splits nbody_forces has produced since the last update
    bool timing = false;
    EventPairs ev_force, ev_update, ev_aux;  // launches not yet added to the totals
    std::vector<nbody::OwnedEvent> ev_pool;
    double force_ms = 0, update_ms = 0, aux_ms = 0;  // aux: what the pair-once mode runs on the auxiliary stream BESIDE the
                                                      // tile launches (diagonal tiles, early summation)
    int64_t force_launches = 0, update_launches = 0, aux_launches = 0;
    // body order on the device (nbody_order.hip): the last permutation nbody_order_compute produced, the sort's scratch and
    // the buffer in-place gathers go through.  Allocated by the first use.
    nbody::DeviceArray<unsigned> order_perm;  // [n_total]: slot k <- body order_perm[k]; the identity beyond the n of the last compute
    int64_t order_n = -1;                     // that n, or -1: no permutation yet
    nbody::DeviceArray<char> order_scratch, order_tmp;
    std::string err;
};

// Internal to the library: the names below are not exported, so its dynamic symbols stay those of the C ABI.
#pragma GCC visibility push(hidden)

namespace nbody {

// The message of a failed call, kept in the context or, without one, per thread for nbody_last_error(NULL); returns status.
int fail(nbody_ctx *c, int status, const std::string &msg);

// Waits for the caller's, the own and the auxiliary stream: whatever was enqueued may read an array that is about to be freed.
int sync_streams(nbody_ctx *c);

// Timing (nbody_capi.hip): an event from the pool or a new one; and the finished launches at the head of a list added to the
// totals, their events back in the pool (all of them, waiting for each stop event, when `wait`).
hipError_t get_event(nbody_ctx *c, OwnedEvent *e);
int drain(nbody_ctx *c, EventPairs &l, double &ms, int64_t &n, bool wait);

// Brackets the launches of its scope with a pair of events on their stream while timing is on.
struct TimedLaunch {
    nbody_ctx *c;
    EventPairs *list;
    double *ms;
    int64_t *count;
    hipStream_t stream;
    OwnedEvent a, b;
    TimedLaunch(nbody_ctx *ctx, EventPairs *l, double *total_ms, int64_t *launches, hipStream_t on = nullptr, bool other = false)
        : c(ctx), list(l), ms(total_ms), count(launches), stream(other ? on : ctx->stream)
    {
        if (!c->timing)
            return;
        if (list->size() >= 64)
            (void)drain(c, *list, *ms, *count, false);
        if (get_event(c, &a) != hipSuccess || get_event(c, &b) != hipSuccess) {
            if (a)
                c->ev_pool.push_back(std::move(a));
            return;
        }
        (void)hipEventRecord(a, stream);
    }
    ~TimedLaunch()
    {
        if (a && b) {
            (void)hipEventRecord(b, stream);
            list->emplace_back(std::move(a), std::move(b));
        }
    }
};

}  // namespace nbody

#pragma GCC visibility pop

#define HIP_TRY(c, call)                                                                                   \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return nbody::fail((c), e_ == hipErrorOutOfMemory ? NBODY_ERR_ALLOC : NBODY_ERR_DEVICE,        \
                               std::string(#call) + ": " + hipGetErrorString(e_));                         \
    } while (0)
