/* nbody_batch_correlation.h -- the pair-separation counts of batched ensembles: for every system the number of ordered pairs
 * (row, source) whose separation falls into each of up to 32 bins.  This is what the two-point correlation function xi(r), the
 * correlation integral C(r) with its slope (the correlation dimension), and the DD, DR and RR counts of the Landy-Szalay
 * estimator are made of; with two different masks it is a cross-count: tracers around planets, the stars of one cluster
 * around those of another, stream stars around subhaloes.  nbody_batch_neighbours gives the count within one radius per call
 * and nbody_batch_span one mean separation; this is the whole curve.  The result is a set of integers.
 * Included by nbody.h (inside its extern "C") after nbody_batch_neighbours.h; additive to ABI version 5, no new status.
 *
 * Rows and sources.  rows and sources are two host pointers to n_systems x max_bodies bytes each, like sources of
 *   nbody_batch_neighbours, or NULL.  Body i of system s is a row iff i < min(counts[s], max_bodies) and rows is NULL or
 *   rows[s * max_bodies + i] != 0; it is a source under the same rule with sources.  A NULL mask selects every body below the
 *   count.  Only bodies below the count take part, whatever the massive counts (nbody_batch_massive.h) are: this is geometry.
 *   Removed tracers and merged bodies are seen as the state holds them.
 * Pairs.  An ordered pair (i, j) is examined iff rows[i], sources[j] and j != i.  With both masks NULL, or both equal, every
 *   unordered pair is examined twice, as (i, j) and as (j, i), and every count is even: r2 is bit-symmetric.
 * Distance.  r2 is groups_r2, the fp32 chain of nbody_batch_groups.h, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 *   There is no softening.
 * Edges.  edges holds bins + 1 fp32 values, 1 <= bins <= NBODY_BATCH_CORRELATION_MAX_BINS (32).  Every value is finite and
 *   >= 0, and the values are strictly ascending.  per_system == 0: edges is a host pointer to one set of bins + 1 values for
 *   all systems; per_system != 0: to n_systems x (bins + 1) values, the set of system s at s * (bins + 1).
 *   e2[t] = edges[t] * edges[t] is one fp32 product on the host, the product nbody_batch_groups and nbody_batch_neighbours use
 *   for their radius; a product that overflows is taken as the largest finite fp32 value, which every measured r2 is within.
 *   Squares may tie (two adjacent tiny edges whose products round to the same value): a tied bin counts nothing.
 * Bins.  A pair is within edge t iff groups_friends(r2, e2[t]), that is r2 <= e2[t].  Bin t holds the pairs within edge t + 1
 *   and not within edge t: bins are half-open on the left, (edge t, edge t + 1].  The cumulative count at any edge is exactly
 *   what nbody_batch_neighbours' within sums to over the rows at that radius, and exactly nbody_batch_groups' link predicate.
 * Counts.  below: the examined pairs within edge 0; with edge 0 = 0 these are the coincident pairs.  unmeasured: the examined
 *   pairs whose r2 is not < +inf (a NaN or infinite coordinate).  above: everything else, the measured pairs not within the
 *   last edge.  The identity
 *     below + sum of counts + above + unmeasured == pairs == rows * sources - both
 *   holds exactly.
 * Records.
 *   Per system, nbody_batch_correlation_system, 48 bytes: rows (offset 0) the selected rows below the count; sources (4) the
 *     selected sources below the count; both (8) the bodies below the count that are a row and a source; bins (12) as given;
 *     pairs (16) the examined pairs; below (24), above (32), unmeasured (40).
 *   systems_out is a host pointer to n_systems records.  counts_out is a host pointer to n_systems x bins unsigned int, bin t
 *   of system s at s * bins + t, or NULL; the largest possible count is 4096 * 4095.  NULL skips that copy; the system
 *   records are the same bits either way.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more bins, and freed in nbody_batch_destroy.
 * Bit invariance.  A system's record and counts depend on its state, its masks and its edges alone: the same bits in any slot,
 *   n_systems and max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm, edges
 *   or systems_out; bins outside 1 ... 32; an edge that is negative, NaN or infinite; edges that are not strictly ascending
 *   (the message names the system and the edge).  All are refused before any device work.
 * Out of scope: weighted counts (mass products, velocity differences: floating-point sums whose order would have to be
 *   pinned), per-body count profiles, more than 32 bins in one call, a triangular walk for the auto case, softened or periodic
 *   distances, pairs across systems, device-side outputs, and changing the state. */
#ifndef NBODY_AMD_BATCH_CORRELATION_H
#define NBODY_AMD_BATCH_CORRELATION_H

#define NBODY_BATCH_CORRELATION_MAX_BINS 32

typedef struct nbody_batch_correlation_system {
    int rows;              /* offset  0: the selected rows below the count */
    int sources;           /* offset  4: the selected sources below the count */
    int both;              /* offset  8: bodies below the count that are a row and a source */
    int bins;              /* offset 12: as given */
    long long pairs;       /* offset 16: the examined pairs, rows * sources - both */
    long long below;       /* offset 24: pairs within edge 0 */
    long long above;       /* offset 32: measured pairs not within the last edge */
    long long unmeasured;  /* offset 40: pairs whose r2 is not < +inf */
} nbody_batch_correlation_system;  /* 48 bytes */

typedef char nbody_batch_correlation_system_is_48_bytes[sizeof(nbody_batch_correlation_system) == 48 ? 1 : -1];
typedef char nbody_batch_correlation_system_pairs_at_16[(sizeof(int) == 4 && sizeof(long long) == 8) ? 1 : -1];

int nbody_batch_correlation(nbody_batch *b, const float *d_positions_xyzm, int bins, const float *edges, int per_system,
                            const unsigned char *rows, const unsigned char *sources,
                            nbody_batch_correlation_system *systems_out, unsigned int *counts_out);

#endif /* NBODY_AMD_BATCH_CORRELATION_H */
