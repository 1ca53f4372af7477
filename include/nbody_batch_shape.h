/* nbody_batch_shape.h -- the shapes of batched ensembles: for every system and each of up to 8 apertures the ellipsoid that the
 * iterated moment tensor converges to (Dubinski & Carlberg 1991, Allgood et al. 2006, Zemp et al. 2011) -- its axis ratios q
 * and s, its axes, what lies inside it and how the iteration went.  nbody_batch_radial gives the second moments of spherical
 * shells, which bias every axis ratio towards 1, and left iterative ellipsoidal shells out of scope; nbody_batch_surface takes
 * a view from the caller.  This finds the direction.  Included by nbody.h (inside its extern "C") after nbody_batch_surface.h;
 * additive to ABI version 5, no new status.
 *
 * Bodies.  nbody_batch_radial.h's rule: body i of system s takes part iff i < min(counts[s], max_bodies) and subset is NULL or
 *   subset[s * max_bodies + i] != 0 (a host pointer to n_systems x max_bodies bytes).  The massive counts play no part.
 * Weight.  NBODY_BATCH_WEIGHT_MASS (0): w is the mass word.  NBODY_BATCH_WEIGHT_NUMBER (1): w = 1.  Either is widened to fp64.
 * Frame.  centre and velocity are host pointers to n_systems x 3 doubles each, or NULL for zeros; every value is finite.
 *     d_k = (double)x_k - c_k,   u_k = (double)v_k - v0_k   (k = x, y, z)
 *   A body taking part is unmeasured iff any of its six words (x, y, z, vx, vy, vz) is not finite.  It is then a member of
 *   nothing.
 * Arithmetic.  Everything is fp64 with +, -, x, / and sqrt alone, nothing contracted: every operation below is one rounded
 *   operation, in the order the parentheses give.
 * Apertures.  1 <= apertures <= NBODY_BATCH_SHAPE_MAX_APERTURES (8).  radii[a] is finite and > 0.  inner may be NULL for
 *   zeros; otherwise inner[a] is finite and 0 <= inner[a] < radii[a]: an ellipsoidal shell, which Zemp et al. recommend for a
 *   local shape.  per_system == 0: one set of `apertures` values for all systems; per_system != 0: n_systems sets, that of
 *   system s at s * apertures.  The apertures need not be ordered and are independent of each other.  out2 = R R and
 *   in2 = Rin Rin are one fp64 product each, on the host; a product that overflows is taken as the largest finite double.
 * The iteration of one aperture.  The state is three row vectors e1, e2, e3 (major, middle, minor) and two weights w2 = 1 / q^2
 *   and w3 = 1 / s^2.  It starts as the identity with w2 = w3 = 1, so the first pass is the sphere.  The major axis is kept at R
 *   (Allgood et al.).  Pass k = 1, 2, ...:
 *   1. a' = (e1_x d_x + e1_y d_y) + e1_z d_z, and likewise b' with e2 and c' with e3 (nbody_batch_surface.h's parentheses);
 *        r2e = (a'a' + w2 (b'b')) + w3 (c'c').
 *      The body is a member iff it is measured and in2 < r2e <= out2.  So a member always has r2e > 0.
 *   2. The tensor T[6] (xx, yy, zz, xy, xz, yz) in the state's coordinates, not the rotated ones, over the members: the
 *      unreduced addend is w (d_a d_b), the reduced addend (w (d_a d_b)) / r2e; `reduced` != 0 chooses the latter.  Also the
 *      member count and the weight W = sum of w.
 *   3. Fewer members than min_members (>= 4): stop, status FEW; the state of the previous pass is kept.
 *   4. T is decomposed by a cyclic Jacobi iteration on the words d0, d1, d2 (diagonal) and o01, o02, o12, with V = identity:
 *      a sweep rotates the pairs in the order (0,1), (0,2), (1,2); sweeps are made until all three off-diagonal words are 0 at
 *      the start of a sweep, 16 at the most.  The rotation of (p, q) with third index r: nothing if a_pq == 0; if
 *      |a_pp| + g == |a_pp| and |a_qq| + g == |a_qq| with g = 100 |a_pq|, a_pq = 0 and nothing else; otherwise
 *        theta = (a_qq - a_pp) / (2 a_pq),   root = sqrt(theta theta + 1),
 *        t = theta < 0 ? -1 / (root - theta) : 1 / (theta + root),   c = 1 / sqrt(t t + 1),   s = t c,   h = t a_pq,
 *        a_pp = a_pp - h,   a_qq = a_qq + h,   a_pq = 0,
 *        a_rp = c a_rp - s a_rq,   a_rq = s a_rp + c a_rq   (both from the old words),
 *        V_kp = c V_kp - s V_kq,   V_kq = s V_kp + c V_kq   (k = 0, 1, 2, both from the old words).
 *      The eigenvalues are sorted lambda1 >= lambda2 >= lambda3, ties to the lower original column; e1 and e2 are the columns
 *      of V of lambda1 and lambda2, each with its component of largest magnitude positive, ties to the lower index;
 *      e3 = e1 x e2, so the triple is right-handed.  If lambda3 <= 0, or lambda1 / lambda3 or lambda1 / lambda2 is not finite,
 *      or W is not > 0: stop, status DEGENERATE; the previous state is kept and the eigenvalues are recorded all the same.  A
 *      razor-thin disc ends here and says so.
 *   5. w2 = lambda1 / lambda2, w3 = lambda1 / lambda3, q = sqrt(lambda2 / lambda1), s = sqrt(lambda3 / lambda1).  Converged
 *      iff |q - q_prev| <= tol q_prev && |s - s_prev| <= tol s_prev, with q_prev = s_prev = 1 before pass 1; otherwise on to the
 *      next pass, up to max_iterations (1 ... 64), which gives status MAX.  change is the larger of |q - q_prev| / q_prev and
 *      |s - s_prev| / s_prev.  With the unreduced tensor an unchanged member set converges by construction.
 *   After the last pass one more walk runs under the final state: count, weight = sum of w, D[3] = sum of w d_a,
 *   M[6] = sum of w (d_a d_b), unreduced whatever the flag, L[3] = sum of w (d x u) with nbody_batch_radial.h's cross product,
 *   and each body's membership bit.
 * The pinned order.  Every sum is two-level.  Level 1: the partial of block k is the sum over that block's members, bodies
 *   64 k ... 64 k + 63, in ascending index, from +0.0, one fp64 add per member and term.  Level 2: the total is the sum of the
 *   block partials in ascending k, from +0.0.  An addend is formed as written, the parenthesis first.  A record therefore
 *   depends on the system's state, mask, frame and apertures alone: the same bits in any slot, n_systems, max_bodies and
 *   workgroup shape.  Adding +0.0 for a non-member is the same bits as skipping it.  For n <= 64 this order is
 *   nbody_batch_radial_profile's.  The order is not plain ascending index because the iteration walks the system up to 65
 *   times: a serial chain 4096 adds deep per term and pass is what the two-level order avoids -- 64 lanes walk 64 blocks at
 *   once and one chain of 64 adds closes each term.
 * Records.
 *   Per aperture, nbody_batch_shape_aperture, 256 bytes: status (offset 0) 0 converged, 1 MAX, 2 FEW, 3 DEGENERATE;
 *     iterations (4) the passes made; count (8) the members of the final walk; radius (16) and inner (24) as given; q (32) and
 *     s (40) the axis ratios; change (48); eigenvalues[3] (56) as sorted, of the last decomposition, 0 if there was none;
 *     axes[9] (80) e1, e2, e3 as rows, which is nbody_batch_surface_map's axes layout; weight (152), D[3] (160), M[6] (184),
 *     L[3] (232) the sums of the final walk.
 *   Per system, nbody_batch_shape_system, 80 bytes: selected (0) the bodies taking part; unmeasured (4); apertures (8) and
 *     reduced (12) as given; converged (16) the number of apertures with status 0; reserved (20) 0; total_weight (24) the sum
 *     of w over the measured bodies taking part, in the two-level order; centre[3] (32) and velocity[3] (56) as used.
 *   Per body, nbody_batch_shape_body, 8 bytes, optional: inside (0) whose bit a is set iff the body is a member of aperture
 *     a's final ellipsoid; reserved (4) 0.  Slots from the count on, and bodies not taking part, read 0.
 *   systems_out is a host pointer to n_systems records; apertures_out to n_systems x apertures records, aperture a of system s
 *   at s * apertures + a, or NULL; bodies_out to n_systems x max_bodies records, or NULL.  NULL skips that copy, and the other
 *   records are the same bits either way.
 *   The division and the square root are the device's.  q, s, change, eigenvalues and axes pass through them, and through the
 *   members they choose every other word of an aperture does: weight, D, M, L, total_weight are made of +, - and x alone
 *   given the members.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use and
 *   freed in nbody_batch_destroy.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, radii or systems_out; apertures outside 1 ... 8; a radius that is not finite or not > 0; an inner radius that
 *   is negative, not finite or >= its radius (the message names the system and the aperture); a weight that is not 0 or 1; a
 *   tol that is not finite or negative; max_iterations outside 1 ... 64; min_members < 4; a centre or velocity that is not
 *   finite.  All are refused before any device work.
 * Out of scope: keeping the volume or the middle axis instead of the major one (either needs a cube root), recentring during
 *   the iteration (pass nbody_batch_structure's centre), shapes of velocity space, more than 8 apertures in one call, shapes
 *   across systems, device-side outputs, and the single-system context. */
#ifndef NBODY_AMD_BATCH_SHAPE_H
#define NBODY_AMD_BATCH_SHAPE_H

#define NBODY_BATCH_SHAPE_MAX_APERTURES 8
#define NBODY_BATCH_SHAPE_MAX_ITERATIONS 64
#define NBODY_BATCH_SHAPE_CONVERGED 0   /* both ratios changed by at most tol in the last pass */
#define NBODY_BATCH_SHAPE_MAX 1         /* max_iterations passes were made */
#define NBODY_BATCH_SHAPE_FEW 2         /* a pass found fewer than min_members members */
#define NBODY_BATCH_SHAPE_DEGENERATE 3  /* a pass's tensor has no three positive eigenvalues */

typedef struct nbody_batch_shape_aperture {
    int status;             /* offset   0: NBODY_BATCH_SHAPE_CONVERGED ... _DEGENERATE */
    int iterations;         /* offset   4: the passes made */
    long long count;        /* offset   8: the members of the final walk */
    double radius;          /* offset  16: as given */
    double inner;           /* offset  24: as given, 0 without `inner` */
    double q;               /* offset  32: middle over major */
    double s;               /* offset  40: minor over major */
    double change;          /* offset  48: the larger relative change of q and s in the last pass that updated them */
    double eigenvalues[3];  /* offset  56: as sorted */
    double axes[9];         /* offset  80: e1, e2, e3 as rows */
    double weight;          /* offset 152: sum of w */
    double D[3];            /* offset 160: sum of w d */
    double M[6];            /* offset 184: sum of w (d_a d_b): xx, yy, zz, xy, xz, yz */
    double L[3];            /* offset 232: sum of w (d x u) */
} nbody_batch_shape_aperture;  /* 256 bytes */

typedef struct nbody_batch_shape_system {
    int selected;         /* offset  0: the bodies taking part */
    int unmeasured;       /* offset  4: those with a word that is not finite */
    int apertures;        /* offset  8: as given */
    int reduced;          /* offset 12: 1 or 0, as given */
    int converged;        /* offset 16: the apertures with status 0 */
    int reserved;         /* offset 20: 0 */
    double total_weight;  /* offset 24: sum of w over the measured bodies taking part */
    double centre[3];     /* offset 32: as used */
    double velocity[3];   /* offset 56: as used */
} nbody_batch_shape_system;  /* 80 bytes */

typedef struct nbody_batch_shape_body {
    unsigned int inside;  /* offset 0: bit a: a member of aperture a's final ellipsoid */
    int reserved;         /* offset 4: 0 */
} nbody_batch_shape_body;  /* 8 bytes */

typedef char nbody_batch_shape_aperture_is_256_bytes[sizeof(nbody_batch_shape_aperture) == 256 ? 1 : -1];
typedef char nbody_batch_shape_system_is_80_bytes[sizeof(nbody_batch_shape_system) == 80 ? 1 : -1];
typedef char nbody_batch_shape_body_is_8_bytes[sizeof(nbody_batch_shape_body) == 8 ? 1 : -1];

int nbody_batch_shape(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities,
                      int apertures, const double *radii, /* apertures values, or n_systems sets of them */
                      const double *inner,                /* like radii, or NULL for zeros */
                      int per_system,
                      const double *centre,         /* n_systems x 3 values, or NULL for zeros */
                      const double *velocity,       /* n_systems x 3 values, or NULL for zeros */
                      int weight,                   /* NBODY_BATCH_WEIGHT_MASS or _NUMBER */
                      int reduced,                  /* != 0: the reduced tensor */
                      double tol, int max_iterations, int min_members,
                      const unsigned char *subset,  /* n_systems x max_bodies bytes, or NULL */
                      nbody_batch_shape_system *systems_out,
                      nbody_batch_shape_aperture *apertures_out,  /* n_systems x apertures, or NULL */
                      nbody_batch_shape_body *bodies_out);        /* n_systems x max_bodies, or NULL */

#endif /* NBODY_AMD_BATCH_SHAPE_H */
