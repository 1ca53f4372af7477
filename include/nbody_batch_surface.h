/* nbody_batch_surface.h -- the surface maps of batched ensembles: for every system the bodies binned into a grid of up to 64 x
 * 64 cells in a plane of the caller's choice, and per cell the sums that the surface density, the line-of-sight velocity and
 * its dispersion (the first two moments of a mock observation), the velocity in the plane and the depth along the line of
 * sight are made of.  nbody_batch_radial bins a system in one dimension about a centre; this bins it in two, as seen from a
 * direction: what the system looks like.  Included by nbody.h (inside its extern "C") after nbody_batch_radial.h; additive to
 * ABI version 5, no new status.
 *
 * Bodies.  Body i of system s takes part iff i < min(counts[s], max_bodies) and subset is NULL or subset[s * max_bodies + i]
 *   != 0 (a host pointer to n_systems x max_bodies bytes): nbody_batch_radial.h's rule.  The massive counts play no part.
 * Weight.  NBODY_BATCH_WEIGHT_MASS (0, nbody_batch_structure.h): w is the mass word.  NBODY_BATCH_WEIGHT_NUMBER (1): w = 1.
 *   Either is widened to fp64.
 * Frame.  centre and velocity are host pointers to n_systems x 3 doubles each, or NULL for zeros; every value is finite.
 * View.  axes is a host pointer to n_systems x 9 doubles, three row vectors per system: A (the map's first axis), B (its
 *   second) and Q (the line of sight), or NULL for the identity: A = x, B = y, Q = z.  Every value is finite; nothing else is
 *   checked: orthonormality is the caller's business, and a view that shears or scales is applied as given.
 * Arithmetic.  Everything is fp64, basic operations only, nothing contracted: every product and every sum below is one
 *   rounded operation, in the order the parentheses give.  No word passes through a square root or a division, so every word
 *   is the same on any IEEE hardware.
 *     d_k = (double)x_k - c_k,   u_k = (double)v_k - v0_k   (k = x, y, z)
 *     a  = (A_x d_x + A_y d_y) + A_z d_z,   b  = (B_x d_x + B_y d_y) + B_z d_z,   q  = (Q_x d_x + Q_y d_y) + Q_z d_z
 *     ua = (A_x u_x + A_y u_y) + A_z u_z,   ub = (B_x u_x + B_y u_y) + B_z u_z,   uq = (Q_x u_x + Q_y u_y) + Q_z u_z
 * Grid.  columns x rows cells, 1 <= columns, rows <= NBODY_BATCH_SURFACE_MAX_SIDE (64).  edges_a holds columns + 1 doubles
 *   and edges_b rows + 1; every edge is finite and each set is strictly ascending.  per_system == 0: one set of each for all
 *   systems; per_system != 0: n_systems sets of each, those of system s at s * (columns + 1) and s * (rows + 1).  A body
 *   taking part is
 *     unmeasured    iff any of a, b, q, ua, ub, uq is not finite (NaN or an infinity),
 *     outside       iff otherwise a < ea[0] || a >= ea[columns] || b < eb[0] || b >= eb[rows],
 *     in cell (i, j) iff otherwise, with ea[i] <= a < ea[i + 1] and eb[j] <= b < eb[j + 1]: cells are half-open on the right,
 *                   numpy.histogram2d's rule except that the last edge is not closed.  The cell index is j * columns + i.
 *   The identity
 *     outside + sum of count + unmeasured == selected
 *   holds exactly.
 * Records.
 *   Per cell, nbody_batch_surface_cell, 64 bytes: count (offset 0, the members); weight (8) sum of w; v1 (16) sum of w uq;
 *     v2 (24) sum of w (uq uq); pa (32) sum of w ua; pb (40) sum of w ub; z1 (48) sum of w q; z2 (56) sum of w (q q).
 *   The pinned order.  Every sum of a cell runs over that cell's members in ascending body index, one fp64 add per member and
 *     term; the addend is formed as written, the parenthesis first and then the product with w.  A cell record therefore
 *     depends on the system's state, mask, frame, view and edges alone: the same bits in any slot, n_systems, max_bodies and
 *     workgroup shape.  An empty cell reads 0 everywhere.
 *   Per system, nbody_batch_surface_system, 88 bytes: selected (0) the bodies taking part; outside (4); unmeasured (8);
 *     columns (12) and rows (16) as given; occupied (20) the cells with count > 0; peak (24) the cell with the largest count,
 *     ties to the lower index, -1 if there is none; peak_count (28) that cell's count, 0 if there is none; total_weight (32)
 *     the sum of w over the measured bodies taking part, outside bodies included, in ascending index: with the same mask and
 *     weight nbody_batch_radial_profile's total_weight, bit for bit, on finite states; centre[3] (40) and velocity[3] (64) as
 *     used.
 *   Per body, nbody_batch_surface_body, 24 bytes, optional: cell (0) the cell index, -1 outside, -2 unmeasured, -3 not taking
 *     part; reserved (4) 0; a (8) and b (16) the rotated coordinates of a measured body taking part, else 0.  Slots from the
 *     count on hold -3 and zeros.
 *   systems_out is a host pointer to n_systems records; cells_out to n_systems x rows x columns records, cell (i, j) of
 *   system s at (s * rows + j) * columns + i, or NULL; bodies_out to n_systems x max_bodies records, or NULL.  NULL skips
 *   that copy, and the other records are the same bits either way.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more cells, and freed in nbody_batch_destroy.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, edges_a, edges_b or systems_out; columns or rows outside 1 ... 64; an edge that is NaN or infinite; edges
 *   that are not strictly ascending (the message names the axis, the system and the edge); a weight that is not 0 or 1; a
 *   centre, velocity or axes value that is not finite.  All are refused before any device work.
 * Out of scope: perspective, smoothing kernels and cloud-in-cell deposit, 3-D meshes, position-velocity diagrams, more than
 *   64 x 64 cells, maps across systems, device-side outputs, and anything for the single-system context. */
#ifndef NBODY_AMD_BATCH_SURFACE_H
#define NBODY_AMD_BATCH_SURFACE_H

#define NBODY_BATCH_SURFACE_MAX_SIDE 64
#define NBODY_BATCH_SURFACE_OUTSIDE (-1)      /* a body's cell word: measured, beyond the grid */
#define NBODY_BATCH_SURFACE_UNMEASURED (-2)   /* one of a, b, q, ua, ub, uq is not finite */
#define NBODY_BATCH_SURFACE_NOT_TAKING (-3)   /* masked out, or a slot from the count on */

typedef struct nbody_batch_surface_cell {
    long long count;  /* offset  0: the members */
    double weight;    /* offset  8: sum of w */
    double v1;        /* offset 16: sum of w uq */
    double v2;        /* offset 24: sum of w (uq uq) */
    double pa;        /* offset 32: sum of w ua */
    double pb;        /* offset 40: sum of w ub */
    double z1;        /* offset 48: sum of w q */
    double z2;        /* offset 56: sum of w (q q) */
} nbody_batch_surface_cell;  /* 64 bytes */

typedef struct nbody_batch_surface_system {
    int selected;         /* offset  0: the bodies taking part */
    int outside;          /* offset  4: those beyond the grid */
    int unmeasured;       /* offset  8: those with a word that is not finite */
    int columns;          /* offset 12: as given */
    int rows;             /* offset 16: as given */
    int occupied;         /* offset 20: the cells with count > 0 */
    int peak;             /* offset 24: the cell with the largest count, ties to the lower index; -1 if there is none */
    int peak_count;       /* offset 28: that cell's count */
    double total_weight;  /* offset 32: sum of w over the measured bodies taking part, in ascending index */
    double centre[3];     /* offset 40: as used */
    double velocity[3];   /* offset 64: as used */
} nbody_batch_surface_system;  /* 88 bytes */

typedef struct nbody_batch_surface_body {
    int cell;      /* offset  0: the cell, or -1 outside, -2 unmeasured, -3 not taking part */
    int reserved;  /* offset  4: 0 */
    double a;      /* offset  8: the rotated first coordinate, or 0 */
    double b;      /* offset 16: the rotated second coordinate, or 0 */
} nbody_batch_surface_body;  /* 24 bytes */

typedef char nbody_batch_surface_cell_is_64_bytes[sizeof(nbody_batch_surface_cell) == 64 ? 1 : -1];
typedef char nbody_batch_surface_system_is_88_bytes[sizeof(nbody_batch_surface_system) == 88 ? 1 : -1];
typedef char nbody_batch_surface_body_is_24_bytes[sizeof(nbody_batch_surface_body) == 24 ? 1 : -1];

int nbody_batch_surface_map(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities,
                            int columns, int rows,
                            const double *edges_a,        /* columns + 1 values, or n_systems sets of them */
                            const double *edges_b,        /* rows + 1 values, or n_systems sets of them */
                            int per_system,
                            const double *centre,         /* n_systems x 3 values, or NULL for zeros */
                            const double *velocity,       /* n_systems x 3 values, or NULL for zeros */
                            const double *axes,           /* n_systems x 9 values (A, B, Q), or NULL for the identity */
                            int weight,                   /* NBODY_BATCH_WEIGHT_MASS or _NUMBER */
                            const unsigned char *subset,  /* n_systems x max_bodies bytes, or NULL */
                            nbody_batch_surface_system *systems_out,
                            nbody_batch_surface_cell *cells_out,    /* n_systems x rows x columns, or NULL */
                            nbody_batch_surface_body *bodies_out);  /* n_systems x max_bodies, or NULL */

#endif /* NBODY_AMD_BATCH_SURFACE_H */
