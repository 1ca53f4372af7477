/* nbody_batch_gravity.h -- gravity at points: the acceleration, the potential and the tidal tensor that the bodies of every
 * system of a batch exert at that system's own bodies or at sample points given by the caller.  This is the
 * get_gravity_at_point / get_potential_at_point pair of AMUSE's gravitational-dynamics interface (what a bridge scheme kicks
 * another code's particles with), the potential and acceleration maps of a system, and the tides a sub-cluster or a binary
 * feels.  nbody_batch_members gives a per-body potential as a by-product and the step kernels keep their accelerations to
 * themselves; this is the sibling that hands out both, with the tidal tensor, anywhere.
 * Included by nbody.h (inside its extern "C") after nbody_batch_hierarchy.h; additive to ABI version 5, no new status.
 *
 * Sources.  The sources are the bodies j < m of system s: with massive counts set (nbody_batch_massive.h)
 *   m = min(massive[s], counts[s]), otherwise m = counts[s], exactly as in nbody_batch_members.  Test particles are never
 *   sources and their mass words are not read.
 * Points mode (d_points_xyzw != NULL).  d_points_xyzw is a device array of n_systems x n_points x 4 floats {x, y, z, ignored};
 *   n_points lies in [1, NBODY_BATCH_GRAVITY_MAX_POINTS]; host_point_counts holds n_systems values in [0, n_points], and NULL
 *   means every system has n_points.  Row p < point_counts[s] of system s is a point that feels all m sources.  The outputs hold
 *   n_points entries per system.
 * Own-bodies mode (d_points_xyzw == NULL; then n_points must be 0 and host_point_counts NULL).  The rows are the bodies
 *   i < counts[s], test particles included, and the outputs hold max_bodies entries per system.  Source j == i is skipped by
 *   index, as nbody_batch_members does it (inv = 0 for that column).
 * Pair term.  All fp32, every fmaf one fused operation, nothing else contracted:
 *     d = x_j - x (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps2)));  inv = rsq(r2), where at eps = 0
 *     an r2 below 2^-84 gives inv = 0, so that a source at zero distance adds nothing to any output;
 *     mi = m_j * inv;  inv2 = inv * inv;  s = mi * inv2.
 *   This is the r2, inv and s of the step kernels, operation for operation.
 * Acceleration.  a = fmaf(d, s, a) per component: one fp32 chain per component in ascending j, starting at +0 -- the chain of
 *   the step kernels, so that a kick_drift step of dt = 1 from rest leaves these bits in the velocities.
 * Potential.  nbody_batch_members' rule: sum += (double)mi in ascending j in fp64, potential = 0.0 - sum.
 * Tidal tensor.  Computed only when tidal_out != NULL.  tidal_out holds six floats per row, {xx, xy, xz, yy, yz, zz}, laid out
 *   like the records.  T_ab = d a_a / d x_b = sum_j m_j (3 d_a d_b (r^2 + eps^2)^-5/2 - delta_ab (r^2 + eps^2)^-3/2), the exact
 *   derivative of the softened acceleration; its trace is -3 eps^2 sum_j m_j (r^2 + eps^2)^-5/2, zero without softening.  In
 *   fp32:  u = (3.f * s) * inv2;  p_a = u * d_a;  six chains t_ab = fmaf(p_a, d_b, t_ab) for a <= b and one chain tr = tr + s,
 *   all in ascending j from +0; after the loop t_xx, t_yy and t_zz each become t - tr.
 * Records beyond the rows.  Rows from point_counts[s] (points mode) or counts[s] (own-bodies mode) on read the empty record,
 *   all zero, and six zeros in tidal_out.  A system with m = 0 gives +0 everywhere.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  records_out and tidal_out
 *   are host pointers to n_systems x n_points (points mode) or n_systems x max_bodies (own-bodies mode) entries.  The device
 *   buffers belong to the handle: they are allocated on first use, grown when a call needs more, and freed in
 *   nbody_batch_destroy.  The call forgets nothing: the cached accelerations, jerks, levels, stops, fates and logs are
 *   untouched, so a nbody_batch_evolve_on after it is bit for bit the nbody_batch_evolve_on without it.
 * Bit invariance.  A row's three outputs depend on that system's sources, eps and the row's coordinates alone: not on the
 *   row's index, n_points, the point counts, the slot, n_systems, max_bodies or the launch shape.  In own-bodies mode a row
 *   that is a source skips itself and nothing else: a test particle's row is bit for bit the point at its position.
 * Softening.  nbody_batch_energy's rule: finite, 0 or >= NBODY_MIN_SOFTENING.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm or
 *   NULL records_out; n_points outside its range; n_points or host_point_counts given without points; a point count outside
 *   [0, n_points]; a bad softening.  All are refused before any device work.
 * Out of scope: the external field of nbody_batch_field.h (nbody_batch_field_potential has its potential), jerks,
 *   device-side outputs, and a frame other than the state's. */
#ifndef NBODY_AMD_BATCH_GRAVITY_H
#define NBODY_AMD_BATCH_GRAVITY_H

#define NBODY_BATCH_GRAVITY_MAX_POINTS 1048576 /* per system */

typedef struct nbody_batch_gravity_record {
    float acceleration[3];  /* G = 1 */
    float reserved;         /* 0 */
    double potential;       /* <= 0 */
} nbody_batch_gravity_record; /* 24 bytes */

int nbody_batch_gravity(nbody_batch *b, const float *d_positions_xyzm,
                        const float *d_points_xyzw, int64_t n_points, const int64_t *host_point_counts,
                        float softening, nbody_batch_gravity_record *records_out, float *tidal_out);

#endif /* NBODY_AMD_BATCH_GRAVITY_H */
