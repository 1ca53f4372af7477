"""Inputs, the fp64 reference, the tolerance and the table of cases of the single-system energy and momentum tests (no HIP,
no GPU): energy_kernel<PPS, GUARD> pair by pair, its kinetic half and momentum_kernel row by row.

One pair per call.  Every mass word is 0 except M_R = 1.7 on row r and M_C = 2.3 on column c.  Every other term of every
row's chain is fma(0, inv, s) with a finite inv -- s itself -- so energy() holds the terms (r, c) and (c, r) alone:
    potential = -1/2 [r owned] M_R M_C / sqrt(d^2 + E) - 1/2 [c owned] M_C M_R / sqrt(d^2 + E),
in fp64 from the fp32 inputs, "owned" = the row lies in the context's rows, E as force_pair_ref.softening2 (eps^2 from the fp32
softening, plus eps_r^2 + eps_c^2 with per-particle softening); d^2 + E = 0 gives 0 (the guard of eps = 0).  A shard that owns
one of the two bodies separates the two directions: a dropped or doubled direction is a factor of two.  The two masses differ,
so (r, c) and (c, r) are different calls.

Configuration.  `configuration(n)`: force_pair_ref.configuration(n) -- body n - 3 lies exactly on body 7 -- with body ORIGIN
moved to (0, 0, 0) exactly; below 16 bodies pair_matrix_ref's lattice alone, its last body at the origin.
`softening_lengths(n)`: force_pair_ref's, which hold zeros (every fifth body and the coincident pair).

Tolerance per term:    tol = K u |term|,    u = 2^-24,
K from energy_tile's operations, counted as force_pair_ref counts its own (v_rsq_f32 is documented to 1 ulp = 2 u):
  * d_c = x_c - x_r: 1 u.  r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, E))): each square carries 2 u, E = eps * eps carries 1 u, a
    sum of positive parts carries the largest of them, and three roundings: 2 + 3 = 5 u.  inv = rsq(r2): 2.5 + 2 = 4.5 u.
  * s = fma(m_c, inv, 0): one rounding, 5.5 u.  (double)s, the fp64 sum across tiles, -0.5 m_r phi and the fp64 reduction
    over rows add roundings of 2^-53, which the count leaves out as it leaves out the second-order terms.   K_ENERGY = 5.5
  * per-particle softening: E = fl(fma(e_r, e_r, eps2) + fl(e_c e_c)): eps2 carries 1 u, the fma one more on its sum (2 u),
    e_c^2 1 u, the addition 1 u: 3 u instead of 1 u in the first addend, so r2 carries 3 + 3 = 6 u, inv 3 + 2 = 5 u, the
    fma 6 u.                                                                                             K_ENERGY_PPS = 6.0
  * guarded (eps = 0): a compare and a select on r2, no rounding; E = 0 is exact.  The same K.
(An estimate of "about 6 u, and 6.5 u" was made for these loops before the count was written out; the count is half a u
below it and is what the tests use.)  No margin, nothing fitted to the kernel's output.  `numpy_term` restates the loop in
numpy fp32 with the rsq moved by up to 1 ulp; the CPU test holds it under the tolerance.

Special entries: a lone lit body gives exactly 0.0 (a leaked self term would be m^2 / eps); the coincident pair with softening
gives the full term -m_r m_c / sqrt(E) -- exclusion is by index, not by distance --, without any (eps = 0, both lengths 0)
exactly 0 by the guard; the all-dark system exactly 0.0.

Kinetic energy and momentum (`kinetic_inputs`): hashed masses and velocities, the fourth velocity word 1e30 (it must not
enter); numpy fp64 over the owned rows; tolerance (row_count + 8) 2^-53 sum |term|: a few roundings per term (the products
of two floats are exact in fp64) plus the summation, whatever its order.

`CASES`: whole contexts and shards whose first row is no multiple of the 256-body tile, each with eps in {1e-2, 0} crossed
with per-particle softening off and on -- the four template variants; `probes(case)` the (r, c) pairs of a case."""
import numpy as np

import force_pair_ref as fp
import pair_matrix_ref as pm

U = pm.U
M_R = float(np.float32(1.7))
M_C = float(np.float32(2.3))
EPS = fp.EPS
K_ENERGY = 5.5
K_ENERGY_PPS = 6.0
ORIGIN = 129                       # the body moved to (0, 0, 0), from 16 bodies on
HASHED_PAIRS = 200
EDGES = (0, 1, 63, 64, 255, 256, 257, 511, 512, 1023, 1024, 1025, 1279, 1280)
KINETIC_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)
FOURTH_WORD = 1e30
TILE = 256
ROWS_PER_WORKGROUP = 1024          # energy_kernel: four rows per lane, 256 lanes


def k_of(pps):
    return K_ENERGY_PPS if pps else K_ENERGY


def has_coincident_pair(n):
    return n >= 16


def origin_body(n):
    return min(ORIGIN, n - 4) if has_coincident_pair(n) else n - 1


def configuration(n):
    """(n, 3) float32."""
    x = fp.configuration(n) if has_coincident_pair(n) else pm.configuration(n)[0].copy()
    x[origin_body(n)] = 0.0
    return x


def softening_lengths(n):
    if has_coincident_pair(n):
        return fp.softening_lengths(n)
    e = (0.004 + 0.016 * pm._hash01(np.arange(n), 91)).astype(np.float32)
    e[::5] = 0.0
    return e


def pair_terms(x, rows, cols, eps, eps_pp=None):
    """m_r m_c / sqrt(d^2 + E) of the pairs (rows[k], cols[k]), fp64 from the fp32 inputs; 0 where d^2 + E = 0."""
    x = np.asarray(x, np.float32).astype(np.float64)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    d = x[cols] - x[rows]
    E = float(np.float32(eps)) ** 2
    if eps_pp is not None:
        e = np.asarray(eps_pp, np.float32).astype(np.float64)
        E = E + e[rows] ** 2 + e[cols] ** 2
    r2 = (d * d).sum(-1) + E
    ok = r2 > 0.0
    return np.where(ok, M_R * M_C / np.sqrt(np.where(ok, r2, 1.0)), 0.0)


def owned(i, row_lo, row_count):
    i = np.asarray(i, np.int64)
    return ((i >= row_lo) & (i < row_lo + row_count)).astype(np.float64)


def expected_potential(x, rows, cols, eps, eps_pp, row_lo, row_count):
    """(potential, tolerance) of the calls with M_R on rows[k] and M_C on cols[k]."""
    t = pair_terms(x, rows, cols, eps, eps_pp)
    share = 0.5 * (owned(rows, row_lo, row_count) + owned(cols, row_lo, row_count))
    return -share * t, k_of(eps_pp is not None) * U * share * t


def numpy_term(x, rows, cols, eps, eps_pp=None, wobble=0):
    """What a correct energy_tile contributes for row rows[k] and column cols[k] alone, as the kernel weighs it: the fp64
    product of M_R and the fp32 s = fma(M_C, inv, 0).  wobble in {-1, 0, 1} moves the rsq by that many ulps."""
    f, fma, rsq = pm._f, pm._fma, pm._rsq
    x = f(x)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    d = x[cols] - x[rows]
    eps2 = np.float32(eps) * np.float32(eps)
    if eps_pp is None:
        E = eps2
    else:
        e = f(eps_pp)
        E = fma(e[rows], e[rows], eps2) + e[cols] * e[cols]
    r2 = fma(d[..., 2], d[..., 2], fma(d[..., 1], d[..., 1], fma(d[..., 0], d[..., 0], E)))
    if not float(np.float32(eps)) > 0.0:
        r2 = np.where(r2 >= np.float32(2.0 ** -84), r2, np.float32(np.inf)).astype(np.float32)
    inv = rsq(r2, np.broadcast_to(np.asarray(wobble), r2.shape))
    s = fma(np.float32(M_C), inv, np.float32(0.0))
    return M_R * s.astype(np.float64)


# ---- kinetic energy and momentum -------------------------------------------------------------------------------------------

def kinetic_inputs(n):
    """(mass (n,), vel (n, 4)) float32: masses hashed in [0.5, 2), velocities in [-1, 1), the fourth word 1e30."""
    i = np.arange(n)
    mass = (0.5 + 1.5 * pm._hash01(i, 61)).astype(np.float32)
    vel = np.full((n, 4), FOURTH_WORD, np.float32)
    vel[:, :3] = np.stack([2.0 * pm._hash01(i, 62 + c) - 1.0 for c in range(3)], axis=1)
    return mass, vel


def expected_kinetic(mass, vel, row_lo, row_count):
    """((kinetic, px, py, pz, mass), their tolerances) over the owned rows, fp64."""
    m = np.asarray(mass, np.float32).astype(np.float64)[row_lo:row_lo + row_count]
    v = np.asarray(vel, np.float32).astype(np.float64)[row_lo:row_lo + row_count, :3]
    terms = np.concatenate([(0.5 * m * (v * v).sum(-1))[:, None], m[:, None] * v, m[:, None]], axis=1)
    return terms.sum(0), (row_count + 8) * 2.0 ** -53 * np.abs(terms).sum(0)


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------

VARIANTS = [(EPS, False), (0.0, False), (EPS, True), (0.0, True)]      # energy_kernel<PPS, GUARD>: every instantiation


def kernel_of(eps, pps):
    return f"energy_kernel<{'true' if pps else 'false'}, {'false' if eps > 0 else 'true'}>"


def _cases():
    shapes = [("whole_1500", 1500, 0, 0, 1500, "a workgroup's rows past 1024, a ragged last tile"),
              ("shard_320_2600", 2600, 320, 320, 1100, "a shard start that is no tile multiple; self tiles misaligned; two workgroups"),
              ("shard_1920_2600", 2600, 320, 1920, 680, "the last shard; the ragged tail on both sides"),
              ("whole_1", 1, 0, 0, 1, "the degenerate sizes"), ("whole_2", 2, 0, 0, 2, "the degenerate sizes")]
    out = []
    for name, n, L, lo, cnt, reaches in shapes:
        for eps, pps in VARIANTS:
            tag = ("soft" if eps > 0 else "guard") + ("_pps" if pps else "")
            out.append({"name": f"{name}_{tag}", "n": n, "split_len": L, "row_lo": lo, "row_count": cnt, "eps": eps, "pps": pps,
                        "kernel": kernel_of(eps, pps), "reaches": reaches})
    return out


CASES = _cases()


def edge_bodies(case):
    n, lo, cnt = case["n"], case["row_lo"], case["row_count"]
    e = set(EDGES) | {n - 2, n - 1, lo - 1, lo, lo + cnt - 1, lo + cnt, origin_body(n)}
    if has_coincident_pair(n):
        e |= {fp.COINCIDENT, fp.coincident_row(n)}
    return sorted(i for i in e if 0 <= i < n)


def probes(case):
    """(rows, cols) int64: every ordered pair of edge bodies, then HASHED_PAIRS hashed pairs (none with r = c, none twice)."""
    n = case["n"]
    e = edge_bodies(case)
    pairs = [(r, c) for r in e for c in e if r != c]
    seen = set(pairs)
    k = 0
    while n > len(e) and len(pairs) < len(e) * (len(e) - 1) + HASHED_PAIRS:
        r, c = int(pm._hash01(k, 31) * n), int(pm._hash01(k, 32) * n)
        k += 1
        if r != c and (r, c) not in seen:
            seen.add((r, c))
            pairs.append((r, c))
    p = np.array(pairs, np.int64).reshape(-1, 2)
    return p[:, 0], p[:, 1]
