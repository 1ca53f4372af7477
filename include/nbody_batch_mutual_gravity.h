/* nbody_batch_mutual_gravity.h -- the mutual gravity of labelled sets of batched ensembles: for every system and every ordered
 * pair (a, b) of up to 8 disjoint sets of its bodies, what set b does to set a: the potential energy between them, the net
 * force, the torque and the Clausius virial about a centre, and the power in a frame, as fp64 sums over the pairs (i in a,
 * j in b) in an order pinned below.  This is what the binding energy left between two clusters after a fly-by, the torque and
 * the drag of a stream on its progenitor, the rate at which planets heat a disc and the torque between a bar and a halo are
 * made of.  nbody_batch_energy gives one number per system and nbody_batch_members one potential per body from all sources;
 * this resolves the same pair term by who acts on whom.
 * Included by nbody.h (inside its extern "C") after nbody_batch_pair_velocities.h; additive to ABI version 5, no new status.
 *
 * Sets.  labels is a host pointer to n_systems x max_bodies bytes: body i of system s is in set labels[s * max_bodies + i] if
 *   that byte is below sets, and in no set if it is NBODY_BATCH_MUTUAL_GRAVITY_NO_SET (255); no other value is taken.
 *   1 <= sets <= NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS (8).  Only bodies below the count min(counts[s], max_bodies) take part,
 *   whatever the massive counts are; bytes from the count on are checked like the others and read by nothing.
 * Unmeasured.  A labelled body below the count is unmeasured iff any of its seven words x, y, z, m, vx, vy, vz is a NaN or
 *   infinite.  It is taken out of every set, counted in `unmeasured` and read by nothing else: a property of the body, not of a
 *   pair.  A body in no set may hold anything.  The fourth velocity word is not read.
 * Finite by construction.  After that every fp64 word below is finite for a centre and a velocity within the fp32 range:
 *   widened fp32 words cannot overflow fp64 through these products.  |d| < 2^129 and e2 < 2^256, so s2 < 2^260; a pair that
 *   adds has s2 >= 2^-298 (the smallest difference of two fp32 words is 2^-149), so inv <= 2^149, mi < 2^277, g < 2^575,
 *   |g d| < 2^704, a row sum over at most 4096 members < 2^716, |f| < 2^844, and with |p|, |q| < 2^130 every addend is below
 *   2^976 and every sum of at most 4096 of them below 2^988.
 * Pair term.  Row i in set a, source j in set b, j != i.  Everything is fp64, basic operations only, nothing contracted, in the
 *   order of the parentheses, from the fp32 words widened:
 *     d_c = (double)x_j,c - (double)x_i,c  (c = x, y, z)      e2 = (double)softening * (double)softening
 *     s2 = ((dx dx + dy dy) + dz dz) + e2
 *   If s2 == 0 (only possible at softening = 0 with a coincident pair) the pair counts in `pairs` and in `coincident` and adds
 *   nothing.  Otherwise
 *     r = sqrt(s2)      inv = 1.0 / r      mi = (double)m_j * inv      g = (mi * inv) * inv.
 * Row sums.  For row i and each source set b, four sums from +0.0 over the members j of b in ascending j, one add per member:
 *     P_b += mi      A_b,c += g * d_c.
 * Row addends.  With mm = (double)m_i, f_c = mm * A_b,c, p_c = (double)x_i,c - centre_c and q_c = (double)v_i,c - velocity_c:
 *     potential: mm * P_b      force_c: f_c      torque_x: p_y f_z - p_z f_y (and cyclic: torque_y = p_z f_x - p_x f_z,
 *     torque_z = p_x f_y - p_y f_x)      virial: (p_x f_x + p_y f_y) + p_z f_z      power: (q_x f_x + q_y f_y) + q_z f_z.
 * The pinned order over rows, defined on body indices alone.  The rows of set a are ranked 0 ... n_a - 1 in ascending body
 *   index.  Block k of set a is its ranks 64 k ... 64 k + 63.  A block's partial of each of the nine sums is the halving tree
 *   of nbody_batch_pair_velocities.h over p[l] = addend of rank 64 k + l, a missing rank +0.0: for off = 32, 16, 8, 4, 2, 1:
 *   p[l] = p[l] + p[l + off] for l < off; the result is p[0].  The record word is the blocks' partials added in ascending k
 *   from +0.0: total = 0; total += partial_k.  The potential word is 0.0 - total.
 * Records.
 *   Per ordered pair of sets, nbody_batch_mutual_gravity_entry, 80 bytes, set b acting on set a: pairs (offset 0) the examined
 *     pairs (i in a, j in b, j != i); potential (8) sum_i m_i sum_j -m_j / r; force[3] (16) sum_i m_i a_i<-b, the net force of
 *     b on a; torque[3] (40) sum_i p_i x (m_i a_i<-b); virial (64) sum_i p_i . (m_i a_i<-b); power (72) sum_i q_i . (m_i
 *     a_i<-b), the rate at which b does work on a.  Entry (a, b) of system s sits at (s * sets + a) * sets + b.  An entry with
 *     an empty set reads 0 everywhere.
 *   Per system, nbody_batch_mutual_gravity_system, 128 bytes: sets (0) as given; selected (4) bodies below the count that are
 *     in a set; left_out (8) bodies below the count that are in no set; unmeasured (12); pairs (16); coincident (24) the
 *     examined pairs with s2 == 0; members[8] (32) the bodies of each set; mass[8] (64) the sum of (double)m_i over each set in
 *     ascending body index from +0.0, one add per member.  Words of sets from `sets` on read 0.
 *   Three identities hold exactly: selected + left_out + unmeasured == min(counts[s], max_bodies);
 *     entry.pairs == members[a] * members[b] - (a == b) * members[a]; the system's pairs is the sum of its entries' pairs.
 *   systems_out is a host pointer to n_systems records.  matrix_out is a host pointer to n_systems x sets x sets entries, or
 *   NULL.  NULL skips that copy; the system records are the same bits either way.
 * Frames.  centre and velocity are host pointers to n_systems x 3 doubles, or NULL for zeros: the point torque and virial are
 *   taken about, and the frame the power is measured in.  potential and force do not read them.
 * Bit invariance.  An entry depends on the state, the labels of its two sets, the softening, centre and velocity alone: the
 *   same bits in any slot, n_systems, max_bodies, workgroup shape and launch plan.  Renaming the sets permutes the entries byte
 *   for byte.  Every floating word of an entry passes through the device's fp64 square root and division, which are the
 *   correctly rounded ones; the integers and mass[] are the same bits wherever IEEE arithmetic is.
 * The call is synchronous: it runs on the handle's stream after the queued work and waits for it.  It forgets nothing: the
 *   cached accelerations, jerks, levels, stops, fates and logs are untouched, so a nbody_batch_evolve_on after it is bit for
 *   bit the nbody_batch_evolve_on without it.  The device buffers belong to the handle; they are allocated on first use, grown
 *   when a later call asks for more, and freed in nbody_batch_destroy.
 * Errors.  NBODY_ERR_INVALID, and nbody_batch_last_error names the function, for: a NULL handle; NULL d_positions_xyzm,
 *   d_velocities, labels or systems_out; sets outside 1 ... 8; a label >= sets that is not 255 (the message names the system
 *   and the body); a softening that is not finite, or neither 0 nor >= NBODY_MIN_SOFTENING; a NaN or infinite centre or
 *   velocity word.  All are refused before any device work.
 * Out of scope: tensors, a per-body breakdown, more than 8 sets, overlapping sets, the external field, pairs across systems and
 *   device-side outputs. */
#ifndef NBODY_AMD_BATCH_MUTUAL_GRAVITY_H
#define NBODY_AMD_BATCH_MUTUAL_GRAVITY_H

#define NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS 8
#define NBODY_BATCH_MUTUAL_GRAVITY_NO_SET 255

typedef struct nbody_batch_mutual_gravity_entry {
    long long pairs;   /* offset  0: the examined pairs (i in a, j in b, j != i) */
    double potential;  /* offset  8: sum_i m_i sum_j -m_j / r */
    double force[3];   /* offset 16: the net force of b on a */
    double torque[3];  /* offset 40: about the centre */
    double virial;     /* offset 64: sum_i p_i . (m_i a_i<-b) */
    double power;      /* offset 72: sum_i q_i . (m_i a_i<-b) */
} nbody_batch_mutual_gravity_entry;  /* 80 bytes */

typedef struct nbody_batch_mutual_gravity_system {
    int sets;              /* offset   0: as given */
    int selected;          /* offset   4: bodies below the count that are in a set */
    int left_out;          /* offset   8: bodies below the count that are in no set */
    int unmeasured;        /* offset  12: labelled bodies below the count with a NaN or infinite word */
    long long pairs;       /* offset  16: the sum of the entries' pairs */
    long long coincident;  /* offset  24: examined pairs with s2 == 0 */
    int members[8];        /* offset  32: the bodies of each set */
    double mass[8];        /* offset  64: the sum of (double)m_i over each set, ascending body index */
} nbody_batch_mutual_gravity_system;  /* 128 bytes */

typedef char nbody_batch_mutual_gravity_entry_is_80_bytes[sizeof(nbody_batch_mutual_gravity_entry) == 80 ? 1 : -1];
typedef char nbody_batch_mutual_gravity_system_is_128_bytes[sizeof(nbody_batch_mutual_gravity_system) == 128 ? 1 : -1];

int nbody_batch_mutual_gravity(nbody_batch *b, const float *d_positions_xyzm, const float *d_velocities, int sets,
                               const unsigned char *labels, float softening, const double *centre, const double *velocity,
                               nbody_batch_mutual_gravity_system *systems_out, nbody_batch_mutual_gravity_entry *matrix_out);

#endif /* NBODY_AMD_BATCH_MUTUAL_GRAVITY_H */
