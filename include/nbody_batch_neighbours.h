/* nbody_batch_neighbours.h -- the nearest-neighbour lists of batched ensembles: for every body of every system the indices and
 * squared distances of its k nearest sources, and the number of sources within a radius.  It does what three headers left
 * out of scope: the "neighbour lists" of nbody_batch_pairs.h, "the neighbours' indices" of nbody_batch_structure.h (which keeps
 * a row's eight smallest squared distances and forgets whose they were) and the "k-nearest-neighbour lists" of
 * nbody_batch_span.h (which reports one nearest).  A local velocity dispersion, a phase-space density, the perturbers of a
 * binary, the candidates of a neighbour scheme, the nearest massive bodies of every tracer and the bodies within a radius all
 * start from these lists, and none needs the state on the host.
 * Included by nbody.h (inside its extern "C") after nbody_batch_span.h; additive to ABI version 5, no new status.
 *
 * Rows.  The rows are all i < min(counts[s], max_bodies) of system s, whatever the massive counts (nbody_batch_massive.h)
 *   are: this is geometry, as in nbody_batch_span.h.  Removed tracers and merged bodies are seen as the state holds them.
 * Sources.  The columns are the sources: every body j < count when sources is NULL, otherwise the bodies with
 *   sources[s * max_bodies + j] != 0; sources is a host pointer to n_systems x max_bodies bytes, like subset of
 *   nbody_batch_span and initial of nbody_batch_members.  Rows are never restricted: an unselected body still gets the list of
 *   its nearest sources.  With the massive bodies as sources the lists are the nearest planets of every planetesimal.
 * Distance.  r2 is the fp32 chain of nbody_batch_groups.h, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 *   It is bit-symmetric in i and j and never -0.  There is no softening.
 * Candidates.  Column j is a candidate of row i iff j != i, j is a source, and r2 < +inf.  A coincident body (r2 == 0) is a
 *   neighbour: this differs from nbody_batch_structure, which counts no pair at distance 0.  A NaN or infinite r2 is not a
 *   candidate.
 * Order.  Candidates are ordered by r2, ties go to the lower j.  The order is total, so a row's list is a set of integers
 *   that does not depend on the schedule, the slot, n_systems or max_bodies.
 * Lists.  1 <= k <= NBODY_BATCH_NEIGHBOURS_MAX (8).  Row i's list holds its found(i) = min(k, candidates) smallest candidates
 *   in that order: index[t] and r2[t] for t < found.  Slots from found on hold index -1 and r2 +inf.  Rows from the count on
 *   hold the same in every slot, with found = 0 and within = 0.  index_out and r2_out are host pointers to
 *   n_systems x max_bodies x k words each, the list of row i of system s at (s * max_bodies + i) * k; both or neither may be
 *   NULL.
 * Within.  within(i) is the number of candidates with r2 <= b2, where b2 = radii[s] * radii[s] is one fp32 product of the
 *   per-system radius: the predicate and the product of nbody_batch_groups.  radii is a host pointer to n_systems values, or
 *   NULL: within is then 0 for every row.  It counts all candidates, not only the listed ones.
 * Records.
 *   Per system, nbody_batch_neighbour_system: bodies is the number of rows; sources the number of selected bodies below the
 *     count; listed the rows with found >= 1; complete the rows with found == k; mutual the rows i with found >= 1 whose
 *     nearest j has found(j) >= 1 and whose own nearest is i; reserved is 0; mean_nearest is the fp64 sum, in ascending i,
 *     of sqrt((double)r2[0]) over the listed rows, each term the correctly rounded fp64 square root, divided by listed in
 *     one division, and 0 when listed is 0; mean_kth is the same over r2[k - 1] of the complete rows, divided by complete.
 *   Per body, nbody_batch_neighbour_body: {found, within}.
 *   systems_out is a host pointer to n_systems records.  bodies_out is a host pointer to n_systems x max_bodies records laid
 *   out like the positions, or NULL.  NULL skips that copy; the system records are the same bits either way.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for a larger k, and freed in nbody_batch_destroy.
 * Bit invariance.  A system's records and lists depend on its state, its sources, its radius and k alone: the same bits in
 *   any slot, n_systems and max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm or
 *   systems_out; k outside 1 ... 8; exactly one of index_out and r2_out NULL; a radius that is negative or NaN.  All are
 *   refused before any device work.
 * Out of scope: k > 8, neighbours in velocity or phase space, softened distances, lists across systems, device-side outputs,
 *   a shorter-list instantiation for small k, and changing the state. */
#ifndef NBODY_AMD_BATCH_NEIGHBOURS_H
#define NBODY_AMD_BATCH_NEIGHBOURS_H

#define NBODY_BATCH_NEIGHBOURS_MAX 8

typedef struct nbody_batch_neighbour_system {
    int bodies;           /* the rows: min(counts[s], max_bodies) */
    int sources;          /* the selected bodies below the count */
    int listed;           /* rows with found >= 1 */
    int complete;         /* rows with found == k */
    int mutual;           /* listed rows whose nearest body's nearest is the row itself */
    int reserved;         /* 0 */
    double mean_nearest;  /* mean of sqrt((double)r2[0]) over the listed rows; 0 without one */
    double mean_kth;      /* mean of sqrt((double)r2[k - 1]) over the complete rows; 0 without one */
} nbody_batch_neighbour_system;  /* 40 bytes */

typedef struct nbody_batch_neighbour_body {
    int found;   /* min(k, candidates) */
    int within;  /* candidates with r2 <= b2; 0 without radii */
} nbody_batch_neighbour_body;    /* 8 bytes */

int nbody_batch_neighbours(nbody_batch *b, const float *d_positions_xyzm, int k, const float *radii,
                           const unsigned char *sources, nbody_batch_neighbour_system *systems_out,
                           nbody_batch_neighbour_body *bodies_out, int *index_out, float *r2_out);

#endif /* NBODY_AMD_BATCH_NEIGHBOURS_H */
