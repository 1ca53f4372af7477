/* nbody_batch_radial.h -- the radial profiles of batched ensembles: for every system the bodies binned into up to 32 shells
 * about a centre, and per shell the sums that the density, the mean radial velocity, the radial and tangential velocity
 * dispersions, the anisotropy, the rotation and the shape of the shell are made of.  nbody_batch_structure gives Lagrangian
 * radii and nbody_batch_correlation counts pairs around bodies; this is how a cluster is built as a function of radius.
 * nbody_batch_correlation left weighted counts out of scope because their summation order would have to be pinned: this
 * header pins it.  Included by nbody.h (inside its extern "C") after nbody_batch_approaches.h; additive to ABI version 5, no
 * new status.
 *
 * Bodies.  Body i of system s takes part iff i < min(counts[s], max_bodies) and subset is NULL or subset[s * max_bodies + i]
 *   != 0 (a host pointer to n_systems x max_bodies bytes).  The massive counts (nbody_batch_massive.h) play no part, as in
 *   nbody_batch_structure.  Removed tracers and merged bodies are seen as the state holds them.
 * Weight.  NBODY_BATCH_WEIGHT_MASS (0, nbody_batch_structure.h): w is the mass word.  NBODY_BATCH_WEIGHT_NUMBER (1): w = 1.
 *   Either is widened to fp64.
 * Frame.  centre and velocity are host pointers to n_systems x 3 doubles each, or NULL for zeros; every value is finite.
 * Arithmetic.  Everything is fp64, basic operations only, nothing contracted: every product and every sum below is one
 *   rounded operation, in the order the parentheses give.
 *     d_a = (double)x_a - c_a,   u_a = (double)v_a - v0_a   (a = x, y, z)
 *     projected == -1 (spherical):  s = (dx dx + dy dy) + dz dz,   rv = (dx ux + dy uy) + dz uz
 *     projected == p in 0, 1, 2:    s = da da + db db,             rv = da ua + db ub
 *       with a < b the two axes that are not p: the cylindrical radius about axis p and the radial velocity in the plane.
 *     v2 = (ux ux + uy uy) + uz uz, in either geometry.
 * Shells.  edges holds shells + 1 doubles, 1 <= shells <= NBODY_BATCH_RADIAL_MAX_SHELLS (32); every edge is finite and >= 0
 *   and the edges are strictly ascending.  per_system == 0: one set for all systems; per_system != 0: n_systems sets, that of
 *   system s at s * (shells + 1).  e2[t] = edges[t] * edges[t] is one fp64 product on the host; a product that overflows is
 *   taken as the largest finite double.  A body taking part is
 *     unmeasured  iff !(s < +inf) || !(v2 < +inf)   (a NaN or infinite coordinate or velocity),
 *     below       iff otherwise s <= e2[0],
 *     in shell t  iff otherwise e2[t] < s <= e2[t + 1]: shells are half-open on the left, (edge t, edge t + 1],
 *     above       iff otherwise, s > e2[shells].
 *   The decision is made on squares: no square root, no division; on inputs whose s is exact it is exact on any hardware.
 *   Squares that tie give an empty shell.  The identity
 *     below + sum of count + above + unmeasured == selected
 *   holds exactly.
 * Terms of a member.  s > e2[t] >= 0, so r > 0.
 *     r = sqrt(s),   vr = rv / r,   vt2 = fmax(v2 - vr vr, 0)
 *     Lx = dy uz - dz uy,   Ly = dz ux - dx uz,   Lz = dx uy - dy ux   (the 3-D cross product in either geometry)
 * Records.
 *   Per shell, nbody_batch_radial_shell, 192 bytes: count (offset 0, the members); weight (8) sum of w; radius (16) sum of
 *     w r; vr1 (24) sum of w vr; vr2 (32) sum of w (vr vr); vt2 (40) sum of w vt2; L[3] (48) sum of w L_a; U[3] (72) sum of
 *     w u_a; M[6] (96) sum of w (d_a d_b) in the order xx, yy, zz, xy, xz, yz; V[6] (144) sum of w (u_a u_b) in that order.
 *   The pinned order.  Every sum of a shell runs over that shell's members in ascending body index, from 0, one fp64 add per
 *     member and term; the addend is formed as written, the parenthesis first and then the product with w.  A shell record
 *     therefore depends on the system's state, mask, frame and edges alone: the same bits in any slot, n_systems, max_bodies
 *     and workgroup shape.  An empty shell reads 0 everywhere.
 *   Per system, nbody_batch_radial_system, 80 bytes: selected (0) the bodies taking part; below (4), above (8), unmeasured
 *     (12); shells (16) and projected (20) as given; total_weight (24) the sum of w over the measured bodies taking part
 *     (below and above included), in ascending index; centre[3] (32) and velocity[3] (56) as used.
 *   Per body, nbody_batch_radial_body, 24 bytes, optional: shell (0) the shell index, -1 below, `shells` above, -2
 *     unmeasured, -3 not taking part; reserved (4) 0; radius (8) sqrt(s) of a measured body taking part, else 0;
 *     radial_velocity (16) rv / radius where that radius is > 0, else 0.  Slots from the count on hold -3 and zeros.
 *   systems_out is a host pointer to n_systems records; shells_out to n_systems x shells records, shell t of system s at
 *   s * shells + t, or NULL; bodies_out to n_systems x max_bodies records, or NULL.  NULL skips that copy, and the other
 *   records are the same bits either way.
 *   The square root and the division are the device's.  radius, vr1, vr2 and vt2 of a shell and the two doubles of a body
 *   pass through them; every other word is made of +, - and x alone and is the same on any IEEE hardware.  On an MI355X
 *   these six were observed bit-equal to a reference with correctly rounded roots and quotients on every case of the test
 *   suite; nothing here relies on that, and the tests hold them to a derived bound.
 *   In a projection only the two axes kept decide whether a body is measured: a body whose coordinate along the axis left out
 *   is NaN or infinite is a member like any other, and L and M of its shell carry that coordinate.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more shells, and freed in nbody_batch_destroy.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, edges or systems_out; shells outside 1 ... 32; an edge that is negative, NaN or infinite; edges that are not
 *   strictly ascending (the message names the system and the edge); a weight that is not 0 or 1; projected outside -1 ... 2; a
 *   centre or velocity that is not finite.  All are refused before any device work.
 * Out of scope: potentials and energies per shell (compose with nbody_batch_members and nbody_batch_gravity), iterative
 *   ellipsoidal shells, shells at equal weight on the device (nbody_batch_structure's Lagrangian radii make such edges), more
 *   than 32 shells in one call, profiles across systems, device-side outputs, and recentring the state. */
#ifndef NBODY_AMD_BATCH_RADIAL_H
#define NBODY_AMD_BATCH_RADIAL_H

#define NBODY_BATCH_RADIAL_MAX_SHELLS 32
#define NBODY_BATCH_RADIAL_BELOW (-1)        /* a body's shell word: within the first edge */
#define NBODY_BATCH_RADIAL_UNMEASURED (-2)   /* s or v2 is not < +inf */
#define NBODY_BATCH_RADIAL_NOT_TAKING (-3)   /* masked out, or a slot from the count on */

typedef struct nbody_batch_radial_shell {
    long long count;  /* offset   0: the members */
    double weight;    /* offset   8: sum of w */
    double radius;    /* offset  16: sum of w r */
    double vr1;       /* offset  24: sum of w vr */
    double vr2;       /* offset  32: sum of w (vr vr) */
    double vt2;       /* offset  40: sum of w vt2 */
    double L[3];      /* offset  48: sum of w (d x u) */
    double U[3];      /* offset  72: sum of w u */
    double M[6];      /* offset  96: sum of w (d_a d_b): xx, yy, zz, xy, xz, yz */
    double V[6];      /* offset 144: sum of w (u_a u_b), the same order */
} nbody_batch_radial_shell;  /* 192 bytes */

typedef struct nbody_batch_radial_system {
    int selected;         /* offset  0: the bodies taking part */
    int below;            /* offset  4: those within the first edge */
    int above;            /* offset  8: those beyond the last edge */
    int unmeasured;       /* offset 12: those whose s or v2 is not < +inf */
    int shells;           /* offset 16: as given */
    int projected;        /* offset 20: as given; -1 for spherical */
    double total_weight;  /* offset 24: sum of w over the measured bodies taking part, in ascending index */
    double centre[3];     /* offset 32: as used */
    double velocity[3];   /* offset 56: as used */
} nbody_batch_radial_system;  /* 80 bytes */

typedef struct nbody_batch_radial_body {
    int shell;               /* offset  0: the shell, or -1 below, `shells` above, -2 unmeasured, -3 not taking part */
    int reserved;            /* offset  4: 0 */
    double radius;           /* offset  8: sqrt(s), or 0 */
    double radial_velocity;  /* offset 16: rv / radius, or 0 */
} nbody_batch_radial_body;  /* 24 bytes */

typedef char nbody_batch_radial_shell_is_192_bytes[sizeof(nbody_batch_radial_shell) == 192 ? 1 : -1];
typedef char nbody_batch_radial_system_is_80_bytes[sizeof(nbody_batch_radial_system) == 80 ? 1 : -1];
typedef char nbody_batch_radial_body_is_24_bytes[sizeof(nbody_batch_radial_body) == 24 ? 1 : -1];

int nbody_batch_radial_profile(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities,
                               int shells, const double *edges, /* shells + 1 values, or n_systems sets of them */
                               int per_system,
                               const double *centre,         /* n_systems x 3 values, or NULL for zeros */
                               const double *velocity,       /* n_systems x 3 values, or NULL for zeros */
                               int weight,                   /* NBODY_BATCH_WEIGHT_MASS or _NUMBER */
                               int projected,                /* -1, or the axis 0, 1 or 2 that is dropped */
                               const unsigned char *subset,  /* n_systems x max_bodies bytes, or NULL */
                               nbody_batch_radial_system *systems_out,
                               nbody_batch_radial_shell *shells_out,   /* n_systems x shells, or NULL */
                               nbody_batch_radial_body *bodies_out);   /* n_systems x max_bodies, or NULL */

#endif /* NBODY_AMD_BATCH_RADIAL_H */
