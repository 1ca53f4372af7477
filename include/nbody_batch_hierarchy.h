/* nbody_batch_hierarchy.h -- hierarchies of batched ensembles: the nested bound pairs of every system, found on the device by
 * a sibling of the pairs kernel.  What a small-N scattering run ends as is a hierarchy such as [[0 1] 2] 3: Fewbody-style
 * codes find it by pairing the most bound mutual pairs, replacing each pair by its centre of mass, and pairing again.  This
 * call does that per system in one launch, judges every pair by the tide of its worst perturber and every nested pair by the
 * stability criterion of Mardling & Aarseth (2001), and counts singles, binaries, triples and higher multiples.
 * Included by nbody.h (inside its extern "C") after nbody_batch_members.h; additive to ABI version 5, no new status.
 *
 * Leaves and slots.  The leaves are the bodies j < m: m = counts[s], or with massive counts set (nbody_batch_massive.h)
 *   m = min(massive[s], counts[s]).  Test particles take no part: their per-body record reads "single, no parent", and they
 *   are counted in nothing.  Every root (a node without a parent) lives in a slot: a leaf lives in its own index, a new node
 *   in the lower of its two children's slots, so a node's slot is its smallest leaf index; the other child's slot is dead
 *   from then on.  Removed tracers and merged bodies are seen as the state holds them, as in nbody_batch_pairs.
 * Level t = 1, 2, ... over the live roots, while two or more roots live:
 *   Walk 1, the partner.  Every live root looks for a partner among the other live roots with the fp32 search of
 *     nbody_batch_pairs.h: the same operation order, mu = m_j + m_i, r2 == 0 is no candidate, ties go to the lower slot, a
 *     NaN or +inf eps is never chosen.  Dead slots are never candidates and never rows: a dead slot's mass word in LDS is
 *     NaN, so its mu and eps are NaN and the search's own comparison never takes it, without a branch.
 *   Candidate pairs.  Two live roots i < j (slots) that choose each other and whose fp64 energy is < 0.  The record is
 *     nbody_batch_pairs.h's, from the two fp32 root states, mu = m_j + m_i in fp64.
 *   Walk 2, the perturbation.  For every candidate pair, with the new node's fp32 state X (below):
 *     g = max over live roots k not in {i, j} of s_k, s_k = (m_k inv)(inv inv), inv = rsq(r2), r2 the fmaf chain of walk 1
 *     on d = x_k - X; g is kept in fp32 in ascending k (a later s replaces g where s > g) and is 0 with no other root.
 *     perturbation = 2 (double)g Q^3 / mu, Q = a (1 + e), in fp64: the tidal force of the worst perturber at apocentre over
 *     the pair's own.  The pair is accepted unless perturbation > tidal_tolerance; +inf accepts every candidate.
 *   New nodes.  Every accepted pair becomes a node, all of them at once, in ascending lower slot.  Node k of system s
 *     (counted over all levels, in creation order) has the id counts[s] + k; a leaf's id is its index.
 *   The node's state is the merged body of nbody_batch_merge.h, exactly: the mass is the fp32 sum; position and velocity per
 *     component are fma(m_j, u_j, m_i u_i) / (m_i + m_j) in fp64, rounded once to fp32; with m_i + m_j == 0 the arithmetic
 *     mean.  The state arrays in global memory are never written.
 *   Stability.  For each composite child c with semi-major axis a_c and angular momentum h_c, and the other child o:
 *     q = m_o / m_c; i_mut = acos(clamp(h . h_c / (|h| |h_c|))), 0 where a norm is 0; the child passes if
 *     a (1 - e) / a_c > 2.8 ((1 + q)(1 + e) / sqrt(1 - e))^(2/5) (1 - 0.3 i_mut / pi), all in fp64.
 *     stable is 1 if every composite child passes and is itself stable.  A node of two leaves is stable.
 *   End.  The loop ends after a level that made no node (converged = 1), when fewer than two roots live (converged = 1: a
 *     system of one leaf evaluates no level), and after max_levels levels (converged = 0 if the last level still made a node
 *     and two or more roots live).
 * Records.  nodes_out: n_systems x max_bodies records laid out like the positions; entry k of a system is node k; the entries
 *   from the node count on are all zero, except that child and parent are -1.  child[0] is the lower slot's id.
 *   bodies_out: per slot i < counts[s] its parent node (or -1), root (the id of its top ancestor; its own index if it has
 *   none) and depth (nodes between it and the root, inclusive of the root; 0 for a single); beyond the count {-1, -1, 0, 0}.
 *   systems_out: nodes, roots (live roots at the end, leaves only), levels (levels evaluated), converged, singles, binaries,
 *   triples, higher (roots with 1, 2, 3, >= 4 leaves), unstable (roots with stable == 0).  A system without leaves is all
 *   zero with converged = 1.  All three are host pointers; nodes_out and bodies_out may be NULL: they skip 128 and 16 bytes
 *   per slot, and the system records keep the same bits.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it, like nbody_batch_members.
 *   It forgets nothing: a nbody_batch_evolve_on after it is bit for bit the nbody_batch_evolve_on without it.  The device
 *   buffers belong to the handle; they are allocated on first use and freed in nbody_batch_destroy.
 * A system's records depend on that system alone: its slot, n_systems, max_bodies and the other systems change no bit.  That
 *   is why ids count from counts[s] and not from max_bodies.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; a NULL state pointer or NULL
 *   systems_out; max_levels outside 1 ... 16; a NaN or negative tolerance.  All are refused before any device work.
 * Out of scope: softened elements, test particles as leaves or satellites, re-pairing a dissolved node, secular (Kozai)
 *   criteria, and changing the state. */
#ifndef NBODY_AMD_BATCH_HIERARCHY_H
#define NBODY_AMD_BATCH_HIERARCHY_H

#define NBODY_BATCH_HIERARCHY_MAX_LEVELS 16

typedef struct nbody_batch_hierarchy_node {
    int child[2];           /* ids; child[0] is the lower slot's */
    int parent;             /* id, or -1 for a root */
    int level;              /* the level that made the node */
    int leaves;             /* leaves below the node */
    int slot;               /* smallest leaf index */
    int stable;
    int reserved;
    double mass;            /* the fp32 node mass, widened */
    double energy;          /* the pair's elements, as nbody_batch_pair_record's */
    double semi_major_axis;
    double eccentricity;
    double inclination;
    double separation;
    double perturbation;    /* 2 g Q^3 / mu */
    double mutual_inclination[2]; /* per child; 0 for a leaf child */
    double h[3];            /* r x v of the pair */
} nbody_batch_hierarchy_node; /* 128 bytes */

typedef struct nbody_batch_hierarchy_body {
    int parent;   /* node id, or -1 */
    int root;     /* id of its top ancestor; its own index if it has none */
    int depth;    /* nodes between it and the root, inclusive of the root; 0 for a single */
    int reserved;
} nbody_batch_hierarchy_body; /* 16 bytes */

typedef struct nbody_batch_hierarchy_system {
    int nodes, roots;     /* nodes made; live roots at the end (leaves only) */
    int levels, converged;
    int singles, binaries, triples, higher; /* roots with 1, 2, 3, >= 4 leaves */
    int unstable;         /* roots with stable == 0 */
    int reserved;
} nbody_batch_hierarchy_system; /* 40 bytes */

int nbody_batch_hierarchy(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities, double tidal_tolerance,
                          int max_levels, nbody_batch_hierarchy_system *systems_out, nbody_batch_hierarchy_node *nodes_out,
                          nbody_batch_hierarchy_body *bodies_out);

#endif /* NBODY_AMD_BATCH_HIERARCHY_H */
