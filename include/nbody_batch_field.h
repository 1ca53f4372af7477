/* nbody_batch_field.h -- external fields for Hermite batches: an analytic background potential next to the pair sum, as the
 * direct-summation codes carry one (phiGRAPE's Plummer, Miyamoto-Nagai and logarithmic-halo terms): tidal streams in a
 * galactic potential, clusters dissolving in one, ring particles around an extended primary.
 * Included by nbody.h (inside its extern "C") after nbody_batch_accrete.h; additive to ABI version 5, no new status.
 *
 * The field.  Every system has a static field centred on the coordinate origin, the sum of up to
 *   NBODY_BATCH_FIELD_MAX_COMPONENTS = 4 components, G = 1 as everywhere else.  nbody_batch_field_set takes
 *   host[s * n_components + c], component c of system s, n_components in [1, 4] (NULL switches the field off, which is the
 *   default); nbody_batch_field_read returns the components as they were set and their number (NBODY_ERR_STATE with a
 *   message when off).  The handle owns the values.  nbody_batch_field_set forgets what nbody_batch_massive_set forgets --
 *   the cached accelerations and jerks, the evolve level, the stops, and an interrupted nbody_batch_evolve_on call -- with
 *   NULL too; new states and nbody_batch_set_counts leave the field alone.
 * Refused with NBODY_ERR_INVALID and a message that names the function, the system, the component and the value, before
 *   any device work: a NULL handle, an unknown kind, a parameter outside its domain (below), n_components outside [1, 4]
 *   with a non-NULL pointer.  A refused call changes nothing.
 * Components.  x = (x, y, z) and v are the PREDICTED state of the row, the one the pair sum is evaluated at; a and j are
 *   the row's fp32 sums.  Accelerations and jerks are the exact derivatives of Phi, j = da/dt along v.  Everything below is
 *   fp32, every fmaf one fused operation, nothing else contracted; rsq is v_rsq_f32 and rcp is v_rcp_f32.  Squares of
 *   parameters and 1 / q^2 are formed once per nbody_batch_field_set on the host in fp32 (the quotient correctly rounded).
 *   NBODY_BATCH_FIELD_NONE (0): skipped -- not added as zero; p is ignored.
 *   NBODY_BATCH_FIELD_PLUMMER (1), p = (M, b, -): Phi = -M / sqrt(|x|^2 + b^2).  M finite and >= 0; b finite, and 0 or
 *     >= NBODY_MIN_SOFTENING.  The column interaction's own instruction sequence (nbody.h, the batch's pair term) for a
 *     column of mass M at rest at the origin, with b^2 in place of eps^2:
 *       d = 0 - x, e = 0 - v (per component);  r2 = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, b b)));
 *       b b == 0: r2 below 2^-84 becomes +inf (the guard of a zero-distance pair: the term then adds exactly 0);
 *       inv = rsq(r2), inv2 = inv inv, s = (M inv) inv2, rv = fmaf(dz, ez, fmaf(dy, ey, dx ex)), c = (3 rv) inv2;
 *       a = fmaf(d, s, a), j = fmaf(fmaf(-c, d, e), s, j).
 *     So a test particle in PLUMMER(M, b) runs bit for bit as it runs beside a body of mass M fixed at the origin with the
 *     softening b.
 *   NBODY_BATCH_FIELD_LOG_HALO (2), p = (v0, rc, q): w = (1, 1, 1 / q^2), D = sum w x^2 + rc^2, Phi = v0^2 ln(D) / 2,
 *     a = -v0^2 w x / D, j = -v0^2 (w v / D - w x Ddot / D^2), Ddot = 2 sum w x v.  v0 >= 0, rc > 0, q > 0, all finite.
 *       k = v0 v0, wz = 1 / (q q);  zw = wz z, vw = wz vz;  D = fmaf(zw, z, fmaf(y, y, fmaf(x, x, rc rc)));
 *       hd = fmaf(zw, vz, fmaf(y, vy, x vx));  iD = rcp(D), g = k iD, t = (2 hd) iD;
 *       a = fmaf(-g, (x, y, zw), a);  j = fmaf(-g, fmaf(-t, (x, y, zw), (vx, vy, vw)), j).
 *   NBODY_BATCH_FIELD_MIYAMOTO_NAGAI (3), p = (M, a, b): s = sqrt(z^2 + b^2), A = a + s, D = x^2 + y^2 + A^2,
 *     Phi = -M / sqrt(D), a = -M (x, y, z A / s) D^-3/2 and j its derivative along v.  M >= 0, a >= 0, b > 0, all finite.
 *       s2 = fmaf(z, z, b b), is = rsq(s2), s = s2 is, A = a + s, f = A is, sd = (z vz) is, fd = -((a sd) (is is));
 *       D = fmaf(A, A, fmaf(y, y, x x)), hd = fmaf(A, sd, fmaf(y, vy, x vx));
 *       iD = rsq(D), iD2 = iD iD, mu = (M iD) iD2, c = (3 hd) iD2;  zf = z f, zd = fmaf(vz, f, z fd);
 *       a = fmaf(-(x, y, zf), mu, a);  j = fmaf(fmaf(c, (x, y, zf), -(vx, vy, zd)), mu, j).
 * Order.  The field's terms are added to the row's sums after the column loop and before the corrector, in ascending
 *   component order, and so before the first-step rule and Aarseth's criterion too: the field counts in the time step.  A
 *   system whose components are all NONE takes exactly the run it takes with the field off, bit for bit.
 * Test particles are rows like any other; the field reads no mass word and feels every row, massive or not.
 * Potential.  nbody_batch_field_potential fills host_phi, n_systems x max_bodies values laid out like the positions, with
 *   Phi(x_i) of the positions d_positions_xyzm holds, in fp64 from the fp32 positions and parameters (squares and 1 / q^2
 *   formed in fp64; a PLUMMER term with b = 0 at |x| = 0 counts 0, as a zero-distance pair does); 0 beyond the counts and
 *   everywhere while the field is off.  Synchronous.  nbody_batch_energy stays exactly what it is: the pair energy.
 * Scope.  nbody_batch_evolve_on takes the field with NBODY_INTEGRATOR_HERMITE, with or without massive counts
 *   (nbody_batch_massive.h), through a sibling of its kernel with the same workgroup shape and LDS layout; levels = 0 gives
 *   fixed steps.  Everything nbody_batch_evolve.h promises holds: the exact tick axis, independence of
 *   nbody_batch_evolve_launch_steps, evolve(a) followed by evolve(b) is evolve(a + b), resumption after max_steps, and
 *   results that are functions of the system alone.  Refused with NBODY_ERR_INVALID and a message while a field is set:
 *   nbody_batch_evolve_on together with a collision radius, an escape radius, radii, the collision action MERGE or the
 *   tracer action REMOVE where it would act; and nbody_batch_step_n_* for every integrator (evolve with levels = 0 takes
 *   fixed steps).  Off (the default, or after NULL) every entry point launches exactly what it launches without this header.
 * Out of scope: fields in the condition, fate and accrete kernels; KDK and kick-drift; off-centre, moving, rotating or
 *   time-dependent fields; further profiles such as Hernquist, NFW or a tidal tensor. */
#ifndef NBODY_AMD_BATCH_FIELD_H
#define NBODY_AMD_BATCH_FIELD_H

#define NBODY_BATCH_FIELD_MAX_COMPONENTS 4

enum {
    NBODY_BATCH_FIELD_NONE = 0,
    NBODY_BATCH_FIELD_PLUMMER = 1,
    NBODY_BATCH_FIELD_LOG_HALO = 2,
    NBODY_BATCH_FIELD_MIYAMOTO_NAGAI = 3
};

typedef struct nbody_batch_field_component {
    int kind;   /* NBODY_BATCH_FIELD_* */
    float p[3]; /* PLUMMER (M, b, -), LOG_HALO (v0, rc, q), MIYAMOTO_NAGAI (M, a, b) */
} nbody_batch_field_component; /* 16 bytes */

int nbody_batch_field_set(nbody_batch *b, const nbody_batch_field_component *host, int n_components);
int nbody_batch_field_read(nbody_batch *b, nbody_batch_field_component *host, int *n_components);
int nbody_batch_field_potential(nbody_batch *b, const float *d_positions_xyzm, double *host_phi);

#endif /* NBODY_AMD_BATCH_FIELD_H */
