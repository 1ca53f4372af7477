/* nbody_batch_span.h -- the spanning trees of batched ensembles: the Euclidean minimum spanning tree (MST) of every system,
 * or of a subset of its bodies.  nbody_batch_groups gives the pieces of a system at one linking length; the tree gives them
 * at every length at once (cutting its edges longer than b leaves exactly the friends-of-friends groups at b), and it is what
 * the Q parameter of Cartwright & Whitworth (2004) and the mass-segregation ratio of Allison et al. (2009) are made of.  The
 * latter is an ensemble of small trees over subsets of one cluster: B copies of the cluster, one subset mask per system, one
 * launch.
 * Included by nbody.h (inside its extern "C") after nbody_batch_groups.h; additive to ABI version 5, no new status.
 *
 * Bodies.  The rows are all i < counts[s] of system s, whatever the massive counts (nbody_batch_massive.h) are: this is
 *   geometry, as in nbody_batch_groups.h.  A body is selected when subset is NULL or subset[s * max_bodies + i] != 0; subset is
 *   a host pointer to n_systems x max_bodies bytes, like initial of nbody_batch_members.  The tree spans the selected bodies;
 *   selected is their number.
 * Length.  r2 is the fp32 chain of nbody_batch_groups.h, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)).
 *   It is bit-symmetric in i and j and never -0.  There is no softening.
 * Order.  The edge between i < j has the 64-bit key K = (bits(r2) << 24) | (i << 12) | j.  r2 is non-negative, so its bits order
 *   as its value does; ties in length go to the lower i, then to the lower j.  K is a strict total order, so the minimum
 *   spanning tree is unique, and the result is that tree: it does not depend on the algorithm or the schedule that found it.
 *   The keys are compared as integers throughout.  A non-finite coordinate still has integer keys, so the launch stays bounded
 *   and deterministic; the tree then has no meaning.
 * Rounds.  Every selected body starts as a component of its own, named by its index.  One round is the following steps, all
 *   reads before any write:
 *   Each component takes the minimum K over the edges with exactly one end in it.
 *   A component c whose edge leads to component o records the edge and hooks under o when o's minimum is a different edge,
 *     does the same when o's minimum is the same edge and c > o, and does nothing when o's minimum is the same edge and c < o.
 *   Compress.  L_i <- L[L_i] for all selected rows at once, repeated until a pass changes nothing: every label is a root.
 *   rounds is the number of rounds run until one component is left; 0 for selected <= 1.  It is a function of the state and
 *   the subset alone: every step above is.  Every component has an edge that leaves it while another component exists, a
 *   component hooks at most once per round, and of two components that chose the same edge one hooks, so a round at least
 *   halves the components: rounds is at most 12 for 4096 bodies.  NBODY_BATCH_SPAN_MAX_ROUNDS (13) bounds the loop all the
 *   same.  Every component is absorbed exactly once, with the edge it recorded.
 * Records.
 *   Per system, nbody_batch_span_system: edges is selected - 1, or 0 for selected <= 1; selected; rounds; reserved is 0;
 *     total_length is the fp64 sum of sqrt((double)r2) over the edges in ascending K, each term the correctly rounded fp64
 *     square root; longest is the last of those terms (0 without edges); mean_separation as below.
 *   Per slot, nbody_batch_span_edge: slot e holds the e-th edge in ascending K, with i < j; slots from edges on hold
 *     {-1, -1, 0, 0}.
 *   Per body, nbody_batch_span_body: degree is the number of tree edges at the body; nearest is the selected body with the
 *     lowest K to it, which is the first round's row result and always a tree neighbour.  An unselected body, a slot from the
 *     count on, or a lone selected body has {0, -1}.
 *   systems_out is a host pointer to n_systems records.  edges_out and bodies_out are host pointers to n_systems x max_bodies
 *   records laid out like the positions, or NULL: NULL skips that copy; the system records are the same bits either way.
 * Separations (separations = 1).  Row i sums (double)sqrtf(r2_ij) over the selected j != i in ascending j, sqrtf the correctly
 *   rounded fp32 square root; the rows are summed in ascending i in fp64; mean_separation is that sum over
 *   selected (selected - 1), one fp64 division.  It is 0 with separations = 0 or selected < 2.  It costs one more pass over
 *   the columns and runs only when asked for.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use and
 *   freed in nbody_batch_destroy.
 * Bit invariance.  A system's records depend on its state and its subset alone: the same bits in any slot, n_systems and
 *   max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm or
 *   systems_out; separations other than 0 or 1.  All are refused before any device work.
 * Out of scope: weighted or projected (2-D) trees, trees across systems, k-nearest-neighbour lists, and changing the
 *   state. */
#ifndef NBODY_AMD_BATCH_SPAN_H
#define NBODY_AMD_BATCH_SPAN_H

#define NBODY_BATCH_SPAN_MAX_ROUNDS 13

typedef struct nbody_batch_span_system {
    int edges;               /* selected - 1, or 0 for selected <= 1 */
    int selected;            /* the selected bodies */
    int rounds;              /* rounds run until one component was left */
    int reserved;            /* 0 */
    double total_length;     /* sum of sqrt((double)r2) over the edges in ascending K */
    double longest;          /* the last of those terms; 0 without edges */
    double mean_separation;  /* mean fp32 distance over the ordered selected pairs; 0 unless asked for */
} nbody_batch_span_system;   /* 40 bytes */

typedef struct nbody_batch_span_edge {
    int i, j;      /* i < j; -1, -1 from edges on */
    float r2;      /* the squared length; 0 from edges on */
    int reserved;  /* 0 */
} nbody_batch_span_edge;     /* 16 bytes */

typedef struct nbody_batch_span_body {
    int degree;   /* tree edges at the body */
    int nearest;  /* the selected body with the lowest K to it; -1 where there is none */
} nbody_batch_span_body;     /* 8 bytes */

int nbody_batch_span(nbody_batch *b, const float *d_positions_xyzm, const unsigned char *subset, int separations,
                     nbody_batch_span_system *systems_out, nbody_batch_span_edge *edges_out, nbody_batch_span_body *bodies_out);

#endif /* NBODY_AMD_BATCH_SPAN_H */
