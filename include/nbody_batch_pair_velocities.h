/* nbody_batch_pair_velocities.h -- the pair velocity statistics of batched ensembles: for every system and each of up to 32
 * bins of separation, fp64 sums over the ordered pairs (row, source) of the bin: their number, how many approach and recede,
 * and the weighted sums of separation, radial velocity, its square, the tangential and the whole relative velocity.  This is
 * what the mean pairwise radial velocity v12(r), the pairwise dispersions along and across the separation, the velocity
 * structure functions S1(r) and S2(r) and the least-squares expansion rate sum(d.w) / sum(d.d) of an association or a stream
 * are made of.  nbody_batch_correlation counts the same pairs; this sums over them, in an order pinned below.
 * Included by nbody.h (inside its extern "C") after nbody_batch_shape.h; additive to ABI version 5, no new status.
 *
 * Rows and sources.  rows and sources are two host pointers to n_systems x max_bodies bytes each, or NULL, exactly those of
 *   nbody_batch_correlation.h: body i of system s is a row iff i < min(counts[s], max_bodies) and rows is NULL or
 *   rows[s * max_bodies + i] != 0; it is a source under the same rule with sources.  A NULL mask selects every body below the
 *   count.  Only bodies below the count take part, whatever the massive counts are.
 * Pairs.  An ordered pair (i, j) is examined iff rows[i], sources[j] and j != i.  With both masks NULL, or both equal, every
 *   unordered pair is examined twice, as (i, j) and as (j, i).
 * Distance.  r2 is groups_r2, the fp32 chain of nbody_batch_groups.h, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 * Edges.  edges holds bins + 1 fp32 values, 1 <= bins <= NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS (32), every value finite and
 *   >= 0, strictly ascending.  per_system == 0: one set for all systems; per_system != 0: n_systems x (bins + 1) values, the
 *   set of system s at s * (bins + 1).  e2[t] = edges[t] * edges[t] is one fp32 product on the host; a product that overflows
 *   is taken as the largest finite fp32 value.  Squares may tie: a tied bin holds nothing.
 * Bins.  A pair is within edge t iff r2 <= e2[t].  Bin t holds the measured pairs with e2[t] < r2 <= e2[t + 1].  The bin of a
 *   pair is decided in fp32 by the code nbody_batch_correlation runs.
 * Unmeasured.  An examined pair is unmeasured iff !(r2 < +inf) (a NaN or infinite coordinate, nbody_batch_correlation's rule)
 *   or !(v2 < +inf), v2 below: a NaN or infinite velocity word of either body (v2 of finite words cannot overflow fp64, so
 *   this is a property of the two bodies).  below: the measured pairs within edge 0.  above: the measured pairs not within
 *   the last edge.  The identity
 *     below + sum of count + above + unmeasured == pairs == rows * sources - both
 *   holds exactly.  On a state with finite velocities the system words and the per-bin counts are the same integers that
 *   nbody_batch_correlation returns.
 * Weight.  weight is NBODY_BATCH_WEIGHT_NUMBER (ww = 1) or NBODY_BATCH_WEIGHT_MASS (ww = (double)m_i * (double)m_j, exact in
 *   fp64), m the fourth position word.
 * Terms of a member pair.  A member of bin t is an examined, measured pair of that bin.  Everything is fp64, basic operations
 *   only, nothing contracted, in the order of the parentheses, from the fp32 words widened; the fourth velocity word is not
 *   read:
 *     d_a = (double)x_j,a - (double)x_i,a      w_a = (double)v_j,a - (double)v_i,a      (a = x, y, z)
 *     s  = (dx dx + dy dy) + dz dz      rv = (dx wx + dy wy) + dz wz      v2 = (wx wx + wy wy) + wz wz
 *     r  = sqrt(s)      vr = rv / r      vt2 = fmax(v2 - vr vr, 0)      v = sqrt(v2)
 *   A member has fp32 r2 > e2[t] >= 0, so some fp32 coordinate differs, so s > 0 and r > 0.
 * Records.
 *   Per bin, nbody_batch_pair_velocities_bin, 96 bytes: count (offset 0) the members; approaching (8) those with rv < 0;
 *     receding (16) those with rv > 0; then the sums over the members of weight (24) ww; r1 (32) ww r; r2 (40) ww s; rv (48)
 *     ww rv; vr1 (56) ww vr; vr2 (64) ww (vr vr); vt2 (72) ww vt2; v1 (80) ww v; v2 (88) ww v2.  The addend is formed as
 *     written: the parenthesis first, then the product with ww.  An empty bin reads 0 everywhere.
 *   Per system, nbody_batch_pair_velocities_system, 56 bytes: rows (0), sources (4), both (8), bins (12) as
 *     nbody_batch_correlation_system; weight (16) as given; reserved (20) 0; pairs (24); below (32); above (40);
 *     unmeasured (48).
 *   systems_out is a host pointer to n_systems records.  bins_out is a host pointer to n_systems x bins records, bin t of
 *   system s at s * bins + t, or NULL.  NULL skips that copy; the system records are the same bits either way.
 * The pinned order.  Three levels, defined on body indices alone.
 *   Row sums.  For row i, bin t and each of the nine sums: start at +0.0 and add the addends of the members (i, j) of bin t
 *     in ascending j, one fp64 add per member.  A body that is not a row, or is at or beyond the count, has row sums of +0.0.
 *   Blocks.  Block k is rows 64 k ... 64 k + 63.  Its partial is the halving tree over p[l] = rowsum(64 k + l): for
 *     off = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + off] for l < off.  The result is p[0].
 *   Blocks in ascending order.  total = 0; total += partial_k for k = 0, 1, ...
 *   Adding +0.0 changes no bit and no sum can be -0, so a bin record depends on the system's state, masks, weight and edges
 *   alone.
 *   r1, vr1, vr2, vt2 and v1 pass through the device's fp64 square root and division; weight, r2, rv, v2 and the integers
 *   are made of +, -, x and comparisons alone and are the same bits wherever IEEE arithmetic is.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more, and freed in nbody_batch_destroy.
 * Bit invariance.  A system's records depend on its state, its masks, the weight and its edges alone: the same bits in any
 *   slot, n_systems, max_bodies, workgroup shape and number of passes over the columns.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, edges or systems_out; bins outside 1 ... 32; a weight that is not 0 or 1; an edge that is negative, NaN or
 *   infinite; edges that are not strictly ascending (the message names the system and the edge).  All are refused before any
 *   device work.
 * Out of scope: per-body (per-row) profiles, more than 32 bins in one call, projected separations, a triangular walk for the
 *   auto case, pairs across systems, device-side outputs, and the external field. */
#ifndef NBODY_AMD_BATCH_PAIR_VELOCITIES_H
#define NBODY_AMD_BATCH_PAIR_VELOCITIES_H

#define NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS 32

typedef struct nbody_batch_pair_velocities_bin {
    long long count;        /* offset  0: the members of the bin */
    long long approaching;  /* offset  8: members with rv < 0 */
    long long receding;     /* offset 16: members with rv > 0 */
    double weight;          /* offset 24: sum of ww */
    double r1;              /* offset 32: sum of ww r */
    double r2;              /* offset 40: sum of ww s */
    double rv;              /* offset 48: sum of ww rv */
    double vr1;             /* offset 56: sum of ww vr */
    double vr2;             /* offset 64: sum of ww (vr vr) */
    double vt2;             /* offset 72: sum of ww vt2 */
    double v1;              /* offset 80: sum of ww v */
    double v2;              /* offset 88: sum of ww v2 */
} nbody_batch_pair_velocities_bin;  /* 96 bytes */

typedef struct nbody_batch_pair_velocities_system {
    int rows;              /* offset  0: the selected rows below the count */
    int sources;           /* offset  4: the selected sources below the count */
    int both;              /* offset  8: bodies below the count that are a row and a source */
    int bins;              /* offset 12: as given */
    int weight;            /* offset 16: as given */
    int reserved;          /* offset 20: 0 */
    long long pairs;       /* offset 24: the examined pairs, rows * sources - both */
    long long below;       /* offset 32: measured pairs within edge 0 */
    long long above;       /* offset 40: measured pairs not within the last edge */
    long long unmeasured;  /* offset 48: pairs whose r2 or v2 is not < +inf */
} nbody_batch_pair_velocities_system;  /* 56 bytes */

typedef char nbody_batch_pair_velocities_bin_is_96_bytes[sizeof(nbody_batch_pair_velocities_bin) == 96 ? 1 : -1];
typedef char nbody_batch_pair_velocities_system_is_56_bytes[sizeof(nbody_batch_pair_velocities_system) == 56 ? 1 : -1];

int nbody_batch_pair_velocities(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities, int bins,
                                const float *edges, int per_system, const unsigned char *rows, const unsigned char *sources,
                                int weight, nbody_batch_pair_velocities_system *systems_out,
                                nbody_batch_pair_velocities_bin *bins_out);

#endif /* NBODY_AMD_BATCH_PAIR_VELOCITIES_H */
