/* nbody_batch_pairs.h -- bound pairs of batched ensembles: every body's partner and the orbital elements of the pair, found
 * on the device by a sibling of the force kernels.  What a scattering experiment, a planetesimal sweep or a small cluster is
 * run for: which two bodies are bound at the end and with what semi-major axis and eccentricity, which planet a tracer
 * orbits, how many binaries have formed.
 * Included by nbody.h (inside its extern "C") after nbody_batch_field.h; additive to ABI version 5, no new status.
 *
 * The partner.  For every body i < counts[s] of every system the partner is the candidate column j with the smallest
 *   specific two-body energy eps_ij = v_ij^2 / 2 - mu_ij / r_ij, G = 1 as everywhere else, no softening.
 * Candidates.  Without massive counts (nbody_batch_massive.h) all j < counts[s]; with massive counts set
 *   j < min(massive[s], counts[s]): test particles are rows, never columns, as in the force kernels.  j == i is never a
 *   candidate, and a pair whose fp32 squared distance is 0 is never a candidate (the self pair is one of those).
 * The mass.  mu_ij = m_j + m_i when row i is itself a massive body or no massive counts are set; mu_ij = m_j when row i is a
 *   test particle: its mass word exerts no force, so it binds nothing.
 * The search runs in fp32, every fmaf one fused operation, nothing else contracted, rsq the hardware reciprocal square root
 *   (v_rsq_f32), the columns in ascending j:
 *     d = x_j - x_i, w = v_j - v_i (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx));  v2 = fmaf(wz, wz, fmaf(wy, wy, wx wx));
 *     inv = rsq(r2);  mu = m_j + m_i (the m_i of a test particle counts as 0: mu = m_j + 0);  eps = fmaf(-mu, inv, 0.5f * v2).
 *   The running best starts at +inf with partner -1; a candidate with r2 > 0 replaces it where eps < best.  So the smaller
 *   energy wins, ties go to the lower j, a candidate whose eps is +inf or NaN is never chosen, and a row with no candidate
 *   gets partner -1.
 * The record of the chosen pair is computed in fp64 from the fp32 state: r = x_j - x_i and v = v_j - v_i formed in fp64,
 *   mu = m_j + m_i in fp64 (m_j alone for a test particle), h = r x v, and
 *     energy          = v^2 / 2 - mu / |r|
 *     semi_major_axis = -mu / (2 energy): negative for a hyperbolic pair, +inf at energy == 0
 *     eccentricity    = |(v x h) / mu - r / |r||: the eccentricity vector, not 1 + 2 eps h^2 / mu^2, which loses everything
 *                       near e = 0
 *     inclination     = acos(h_z / |h|) in radians, against the z axis; 0 where |h| == 0
 *     separation      = |r|
 *   Where mu == 0: semi_major_axis = 0 and eccentricity = +inf.
 * Mutual pairs and binaries.  mutual is 1 where partner[partner[i]] == i, else 0.  A system's binaries are its mutual pairs
 *   with energy < 0, counted once (i < j).  Rows with partner -1, and slots from the count on, read the empty record
 *   {-1, 0, 0, 0, 0, 0, 0}.
 * What the call sees.  Removed tracers (nbody_batch_fate.h) and merged bodies (nbody_batch_merge.h) are seen as the state
 *   holds them: frozen tracers are ordinary rows, and the counts are the live ones.  nbody_batch_pairs reads the caller's
 *   buffers as nbody_batch_energy does, on the handle's stream after the queued work, and waits for it: synchronous.
 *   records_out is a host pointer to n_systems x max_bodies records laid out like the positions.
 *   nbody_batch_pairs_binaries writes n_systems counts of the last nbody_batch_pairs call; before any call it returns
 *   NBODY_ERR_STATE with a message.  A NULL handle or argument: NBODY_ERR_INVALID, and nbody_batch_last_error names the function.
 * The call forgets nothing: the cached accelerations, jerks, levels, stops, fates and logs are untouched, so a
 *   nbody_batch_evolve_on after it is bit for bit the nbody_batch_evolve_on without it.  The records live in a device buffer
 *   the handle owns, allocated on first use.
 * A system's records are functions of that system alone: its slot, n_systems, max_bodies and the other systems change no bit.
 * Out of scope: softened elements, triples and hierarchies, neighbour lists, and a search among test particles. */
#ifndef NBODY_AMD_BATCH_PAIRS_H
#define NBODY_AMD_BATCH_PAIRS_H

typedef struct nbody_batch_pair_record {
    int partner;            /* the column j, or -1 */
    int mutual;             /* 1 where partner[partner[i]] == i */
    double energy;          /* v^2 / 2 - mu / |r| */
    double semi_major_axis; /* -mu / (2 energy) */
    double eccentricity;
    double inclination;     /* radians */
    double separation;      /* |r| */
} nbody_batch_pair_record; /* 48 bytes */

int nbody_batch_pairs(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities_xyzw,
                      nbody_batch_pair_record *records_out);
int nbody_batch_pairs_binaries(nbody_batch *b, int64_t *count_out);

#endif /* NBODY_AMD_BATCH_PAIRS_H */
