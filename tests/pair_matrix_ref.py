"""Inputs, the one-source fp64 reference and the checker of the pair-matrix tests (no HIP, no GPU).

The idea.  Take B copies of one configuration of n bodies and give copy s a mass word on column c_s alone.  Then row i of
system s moves under exactly one pair term, (i, c_s), and one launch of a batch kernel returns the whole n x n matrix of
terms: which loop iteration a wrong entry belongs to is read off its (system, row).  The source feels nothing and drifts
uniformly, so the fp64 reference of a system is a test particle about one moving source, vectorised over rows and sources.

Configuration.  `configuration(n, seed)`: n sites of a cubic lattice of side ceil(cbrt(n)) that fills a cube of edge EXTENT
with its lower corner at OFFSET on every axis (no coordinate near zero, see K_round), each site moved by at most JITTER of
the spacing per axis; every separation lies in `separation_bounds(n)`.  Velocities are a linear field about the cube's
centre plus a bulk motion and a hashed part, v = SIGMA A (x - x_c) + v_b + 0.02 hash: speeds of order 0.1 to 1 (1.8 in the
corners), and the relative velocity of a pair is about SIGMA A d -- close pairs do not fly through each other in one long
step, and every pair has a jerk worth measuring, h |e| / r of order 0.1.  All from an integer hash; the fourth velocity
word is 7.  The source's mass word is `probe_mass(n)`, the largest power of two with h^2 m <= MASS_FACTOR r_min^3: heavy
enough for the jerk of the farthest rows to show, while the closest rows are thrown about their source within the step.

Schemes, as include/nbody.h, include/nbody_batch_evolve.h, oracle/ and hermite_ref.py state them, in fp64 from the fp32
inputs, the softening squared from the fp32 softening:
    kick-drift   v1 = v + a(x) h;  x1 = x + v1 h
    KDK          v' = v + a(x) h/2;  x1 = x + v' h;  v1 = v' + a(x1) h/2          (fresh handle: a(x) evaluated first)
    Hermite      xp = x + h (v + h/2 (a0 + h/3 j0));  vp = v + h (a0 + h/2 j0);  (a1, j1) = F(xp, vp)
                 v1 = v + h/2 ((a0 + a1) + h/6 (j0 - j1));  x1 = x + h/2 ((v + v1) + h/6 (a0 - a1))     (fresh handle)
with the source at x_s + v_s h (and v_s) wherever the scheme evaluates after a drift.  eps = 0: a pair at zero distance
(the self pair, a coincident pair) contributes nothing.  `one_step(..., variant=)` also gives the *drift* (term removed)
and, for Hermite, the *jerkless* step (j0 = j1 = 0).

Tolerance.  For every entry (system, row) and each of the six components of its new state,

    tol = K_term u |ref - drift| + K_round u |ref|,        u = 2^-24 (half an ulp, relative),

where |ref| is the component's own magnitude and |ref - drift| the Euclidean length of the change the term makes to the
component's vector (position or velocity).  The length and not the component: KDK's second force and Hermite's a1, j1 are
evaluated at fp32-rounded coordinates, whose roundings are set by the coordinates and not by d = x_j - x_i, so a component
of the change that is small beside the others has no error bound relative to itself.

K_round: the roundings of the state update, relative to the component.  Every scheme forms a new component in fp64 and
rounds it once to fp32 (batch_kick, batch_drift, hermite_correct): u |v1_c|, u |x1_c|.  The position is formed from the
*rounded* new velocity (kick-drift, Hermite) or half-kicked velocity (KDK), whose rounding u |v_c| enters with the factor h
(h/2 for Hermite): with h |v_c| <= DRIFT_SHARE |x_c| for every body and component (`conditions` asserts it of the
initial state; this is what OFFSET is for) that is DRIFT_SHARE u |x_c|.  KDK's v1 is formed from the rounded v', a second
rounding u |v'_c| <= u |v1_c| + u |change| (the last part is the +1 in KDK's K_term).  Derived: kick-drift 1.3, KDK 2,
Hermite 1.15; taken with a margin of 1.5: K_ROUND = 2, 3, 2.

K_term: the pair term's own error relative to the change it makes, from the kernels' operations (batch_forces and
batch_forces_jerks in n_body_problem_amd/csrc/nbody_batch.hip; all fp32; v_rsq_f32 is documented to 1 ulp = 2 u; every other column adds an
exact zero since its mass word is 0):
  * K_A = 18.5.  d_c = x_j - x_i: 1 u.  r2, an fma chain of three: 2 u from the squares and 3 roundings = 5 u.  inv = rsq(r2):
    2.5 u inherited + 2 u of the instruction = 4.5 u.  s = (m inv)(inv inv): 3 x 4.5 u + 3 products = 16.5 u.
    a_c = fma(d_c, s, 0): 1 + 16.5 + 1 = 18.5 u of |a_c|.
  * K_J = 129.  e_c: 1 u.  rv = d.e, a product and two fma: (1 + 1 + 3) u |d||e| = 5 u.  inv2: 9 u + 1.  c = (3 rv) inv2:
    5 + 10 + 2 = 17 u of at most 3|e|/r.  fma(-c, d_c, e_c): (17 + 1) u 3|e| + 1 u |e| + a rounding of 1 u 4|e| = 59 u |e|;
    times s, 16.5 u of at most 4 |e| s = 66 u |e| s, and the last fma's rounding, 4 u |e| s: 129 u |e| s, and |j| >= |e| s.
  The rest differs from entry to entry by orders of magnitude -- a row beside its source answers the rounding of its
  coordinates a hundred times more strongly than a row across the cube -- so K_term is formed per entry, from the fp64
  reference's own stages (`one_step(detail=True)`) and from nothing a kernel returns:
  * k_cond = 4 sqrt(3) X / r1.  After a drift or a prediction the row's and the source's coordinates are rounded to fp32,
    |delta d_c| <= 2 u X with X the largest coordinate of the two at that stage, so |delta d| <= 2 sqrt(3) u X, and the
    acceleration answers with the tidal tensor, of norm 2 m / r1^3 = (2 / r1)|a1|, r1 the pair's separation at the stage.
    The jerk answers with at most 24 m |e| / r1^4; through the corrector's h^2/12 and relative to h m / r1^2 that is
    h_sigma k_cond with h_sigma = h |e| / r1; the velocities' rounding adds less than 0.02 k_cond.
  * amp = h^2 m / r1^3 x |a0| / (|a0| + |a1|).  The first evaluation's error moves the stage, delta x = h^2/2 delta a0,
    which the tidal tensor at the stage turns into h^2 m / r1^3 K_A u |a0|; through the jerk's gradient the same
    displacement adds 2 h_sigma of that.
  * kappa = (sum of the pieces' lengths) / |ref - drift|.  The pieces of the change can cancel: h/2 |a0|, h/2 |a1|,
    h^2/12 |j0|, h^2/12 |j1| against the length of their signed sum (for the position h^2/3 |a0|, h^2/6 |a1|, h^3/24 |j0|,
    h^3/24 |j1|); the larger of the two ratios is taken.  jerk_share = the jerk's pieces over the velocity's sum.
  * +1: the new velocity's rounding enters the position as h u |v1_c| <= DRIFT_SHARE u |x_c| + h u |change| (K_round covers
    the first part); KDK's second rounding of v' adds another.
  Together (`k_term`):
    kick-drift   K_term = K_A + 1 = 19.5
    KDK          K_term = kappa (K_A (1 + amp) + k_cond) + 2
    Hermite      K_term = kappa (K_A (1 + amp (1 + 2 h_sigma)) + k_cond (1 + h_sigma + 0.02) + jerk_share K_J) + 1
The median over the entries is 31 to 36 at every capacity; the few rows thrown close to their source reach 10^3 (KDK) and
10^5 (Hermite), still far below the 1 / (8 u) at which a dropped term would stop showing.  No margin is put on K_term: it is a
worst case in every factor at once.  Nothing is fitted to a kernel's output; `emulate_fp32` restates the loops' arithmetic in
numpy fp32 (with a rsq moved by up to 1 ulp) so that the CPU test can show that the tolerance holds a correct fp32 kernel.

Secondary quantities (gravity_at, members, energy) are single terms at the exact inputs, so their bounds are relative to
the component: acceleration K_A; potential m inv: 4.5 + 1 = K_P = 5.5; tidal tensor p_a d_b with p_a = ((3 s) inv2) d_a:
16.5 + 1 + 10 + 1 + 1 + 1 + 1 + 1 = K_T = 32.5 of |3 m d_a d_b / r^5|, and on the diagonal K_A - 2 = 16.5 of m / r^3 for the
chain of s plus one rounding of the difference.

Checker.  `check(...)` returns the entries beyond tolerance, worst first, each naming system, source column, row and
component; its first result is the worst |got - ref| / tol."""
import math

import numpy as np

U = 2.0 ** -24
W_WORD = 7.0
EXTENT = 3.5          # edge of the cube the lattice fills
OFFSET = 0.75         # its lower corner on every axis
JITTER = 0.2          # of the spacing, per axis and direction
SIGMA = 0.4           # scale of the velocity field's gradient
#: the velocity gradient: a rotation, a shear and a strain
GRADIENT = np.array([[0.35, -0.90, 0.40], [0.80, -0.30, -0.55], [-0.45, 0.60, 0.50]])
BULK = np.array([0.25, -0.20, 0.15])
DT = 0.25             # the probe step: deliberately long, so that the jerk shows
SOFTENINGS = (0.0, 1e-2)
FILL_POS = (50.0, -60.0, 70.0, 3.0)   # slots beyond a count: heavy enough to show if a loop read them
FILL_VEL = (0.5, 0.25, -0.5, 9.0)

K_A = 18.5
K_J = 129.0
K_P = 5.5
K_T = 32.5
DRIFT_SHARE = 0.3
K_ROUND = {"kick_drift": 2.0, "kdk": 3.0, "hermite": 2.0}
MASS_FACTOR = 4.0     # h^2 m <= MASS_FACTOR r_min^3: the closest rows are thrown about their source, which K_term prices in

CAPACITIES_FULL = (64, 128, 192, 320, 1024)   # every column is the source once
CAPACITY_LARGE = 4096                         # chosen sources
JERK_RESOLVED_SHARE = 0.95

SCHEMES = ("kick_drift", "kdk", "hermite")
COMPONENTS = ("x", "y", "z", "vx", "vy", "vz")


def _hash01(i, salt):
    i = np.asarray(i, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(13))) * np.uint64(3266489917) % np.uint64(1 << 32)
    return h.astype(np.float64) / float(1 << 32)


def lattice_side(n):
    side = max(1, int(round(n ** (1.0 / 3.0))))
    while side ** 3 < n:
        side += 1
    while side > 1 and (side - 1) ** 3 >= n:
        side -= 1
    return side


def spacing(n):
    return EXTENT / lattice_side(n)


def configuration(n, seed=0):
    """(pos, vel): (n, 3) and (n, 4) float32, the fourth velocity word 7."""
    side = lattice_side(n)
    a = EXTENT / side
    i = np.arange(n)
    cell = np.stack([i % side, (i // side) % side, i // (side * side)], axis=1).astype(np.float64)
    jit = np.stack([_hash01(i, 10 * seed + c) for c in range(3)], axis=1)
    x = OFFSET + a * (cell + 0.5 + JITTER * (2.0 * jit - 1.0))
    centre = OFFSET + 0.5 * EXTENT
    noise = np.stack([_hash01(i, 10 * seed + 3 + c) for c in range(3)], axis=1)
    v = SIGMA * (x - centre) @ GRADIENT.T + BULK + 0.02 * (2.0 * noise - 1.0)
    vel = np.full((n, 4), W_WORD, dtype=np.float32)
    vel[:, :3] = v
    return x.astype(np.float32), vel


def separation_bounds(n):
    """(lowest, highest) separation any two bodies of configuration(n) may have."""
    a = spacing(n)
    return (1.0 - 2.0 * JITTER) * a, math.sqrt(3.0) * EXTENT


def separation_range(pos, chunk=512):
    """(min, max) over all pairs of distinct bodies, fp64."""
    x = np.asarray(pos, np.float64)[:, :3]
    lo, hi = np.inf, 0.0
    for b in range(0, len(x), chunk):
        d = x[None, :, :] - x[b:b + chunk, None, :]
        r2 = np.einsum("ijk,ijk->ij", d, d)
        hi = max(hi, float(r2.max()))
        r2[np.arange(r2.shape[0]), np.arange(b, b + r2.shape[0])] = np.inf
        lo = min(lo, float(r2.min()))
    return math.sqrt(lo), math.sqrt(hi)


def probe_mass(n):
    """The source's mass word for capacity n: the largest power of two with h^2 m <= MASS_FACTOR (closest separation)^3,
    heavy enough for the jerk of the far rows to show and light enough for the closest rows to stay conditioned."""
    r = separation_bounds(n)[0]
    return 2.0 ** math.floor(math.log2(MASS_FACTOR * r ** 3 / DT ** 2))


def probe_batch(capacity, counts, sources, mass, coincident=(), seed=0, tracer_from=None):
    """(pos, vel), (B, capacity, 4) float32.  System s is the configuration truncated to counts[s] with the mass word `mass`
    on column sources[s] (none when sources[s] < 0: the null system) and 0.0 on every other; for s in `coincident`, body
    counts[s] - 3 lies exactly on body 7 (position and velocity, so that it stays there).  With `tracer_from` = (B,) massive
    counts, a source at a column c >= tracer_from[s] carries the mass word 1.0 instead.  Slots beyond a count hold FILL_POS /
    FILL_VEL."""
    x, v = configuration(capacity, seed)
    B = len(counts)
    pos = np.empty((B, capacity, 4), dtype=np.float32)
    vel = np.empty((B, capacity, 4), dtype=np.float32)
    pos[:] = np.asarray(FILL_POS, np.float32)
    vel[:] = np.asarray(FILL_VEL, np.float32)
    for s in range(B):
        n = int(counts[s])
        pos[s, :n, :3] = x[:n]
        pos[s, :n, 3] = 0.0
        vel[s, :n] = v[:n]
        if s in coincident:
            pos[s, n - 3, :3] = pos[s, 7, :3]
            vel[s, n - 3, :3] = vel[s, 7, :3]
        c = int(sources[s])
        if c >= 0:
            if c >= n:
                raise ValueError(f"system {s}: source {c} beyond its count {n}")
            pos[s, c, 3] = 1.0 if tracer_from is not None and c >= int(tracer_from[s]) else mass
    return pos, vel


def _eps2(eps):
    return float(np.float32(eps)) ** 2


def acc_jerk(x, v, xs, vs, m, eps2):
    """Acceleration and jerk of test particles at x, v (..., 3) from a source of mass m at xs, vs (broadcast), fp64; a pair
    with r^2 + eps^2 = 0 gives zeros."""
    d = xs - x
    e = vs - v
    r2 = (d * d).sum(-1) + eps2
    ok = r2 > 0.0
    inv2 = np.where(ok, 1.0 / np.where(ok, r2, 1.0), 0.0)
    s = m * inv2 * np.sqrt(inv2)
    rv = (d * e).sum(-1)
    a = s[..., None] * d
    j = s[..., None] * (e - (3.0 * rv * inv2)[..., None] * d)
    return a, j


def one_step(scheme, x, v, sources, mass, dt, eps, variant="full", detail=False):
    """One step of `scheme` of every row of the configuration x, v (n, 3+) about each source column in turn.

    Returns (x1, v1), each (S, n, 3) fp64 with S = len(sources): entry [k, i] is body i's new state in the system whose only
    massive column is sources[k].  The source's own row (the self pair) feels nothing; a negative source is the null system.
    variant: "full", "drift" (the term removed) or "jerkless" (Hermite with j0 = j1 = 0).  mass: a scalar or (S,).
    detail=True also returns a dict of the stages (a0, a1, j0, j1, the stage separation r1)."""
    if scheme not in SCHEMES:
        raise ValueError(scheme)
    if variant not in ("full", "drift", "jerkless") or (variant == "jerkless" and scheme != "hermite"):
        raise ValueError(variant)
    x = np.asarray(x, np.float64)[:, :3]
    v = np.asarray(v, np.float64)[:, :3]
    src = np.asarray(sources, dtype=np.int64).reshape(-1)
    S, n = len(src), len(x)
    h = float(np.float32(dt))
    eps2 = _eps2(eps)
    m = np.broadcast_to(np.asarray(mass, np.float64), (S,)).copy()
    m[src < 0] = 0.0
    if variant == "drift":
        m[:] = 0.0
    c = np.where(src < 0, 0, src)
    X = np.broadcast_to(x[None], (S, n, 3))
    V = np.broadcast_to(v[None], (S, n, 3))
    xs, vs = x[c][:, None, :], v[c][:, None, :]
    mm = np.broadcast_to(m[:, None], (S, n)).copy()
    mm[np.arange(S), c] = 0.0                        # the self pair: nothing, with any softening (d = e = 0)
    jz = 0.0 if variant == "jerkless" else 1.0
    a0, j0 = acc_jerk(X, V, xs, vs, mm, eps2)
    j0 = jz * j0
    if scheme == "kick_drift":
        v1 = V + a0 * h
        x1 = X + v1 * h
        a1, j1, r1, big = a0, j0, None, None
    elif scheme == "kdk":
        vh = V + a0 * (0.5 * h)
        x1 = X + vh * h
        a1, j1 = acc_jerk(x1, vh, xs + vs * h, vs, mm, eps2)
        v1 = vh + a1 * (0.5 * h)
        r1 = np.sqrt(((xs + vs * h - x1) ** 2).sum(-1))
        big = np.maximum(np.abs(x1).max(-1), np.abs(xs + vs * h).max(-1))
    else:
        xp = X + h * (V + h / 2 * (a0 + h / 3 * j0))
        vp = V + h * (a0 + h / 2 * j0)
        a1, j1 = acc_jerk(xp, vp, xs + vs * h, vs, mm, eps2)
        j1 = jz * j1
        v1 = V + h / 2 * ((a0 + a1) + h / 6 * (j0 - j1))
        x1 = X + h / 2 * ((V + v1) + h / 6 * (a0 - a1))
        r1 = np.sqrt(((xs + vs * h - xp) ** 2).sum(-1))
        big = np.maximum(np.abs(xp).max(-1), np.abs(xs + vs * h).max(-1))
    if detail:
        hs = None
        if scheme == "hermite":
            with np.errstate(divide="ignore", invalid="ignore"):
                hs = h * np.sqrt(((vs - vp) ** 2).sum(-1)) / r1
        return x1, v1, {"a0": a0, "a1": a1, "j0": j0, "j1": j1, "r1": r1, "big": big, "hs": hs, "h": h, "mass": mm}
    return x1, v1


def k_term(scheme, detail, x1, v1, xd, vd):
    """K_term of every entry, (S, n), as the module's docstring derives it, from the reference's own stages (`detail` of
    one_step, the new state x1, v1 and the drift xd, vd).  Entries without a term (the self pair, a null system) get 0."""
    mm = detail["mass"]
    if scheme == "kick_drift":
        return np.where(mm > 0.0, K_A + 1.0, 0.0)
    h = detail["h"]
    with np.errstate(divide="ignore", invalid="ignore"):
        n0, n1 = np.linalg.norm(detail["a0"], axis=-1), np.linalg.norm(detail["a1"], axis=-1)
        r1 = detail["r1"]
        kc = 4.0 * math.sqrt(3.0) * detail["big"] / r1
        amp = h * h * mm / r1 ** 3 * n0 / (n0 + n1)
        if scheme == "kdk":
            pv, px = h / 2 * (n0 + n1), h * h / 2 * n0
        else:
            j0, j1 = np.linalg.norm(detail["j0"], axis=-1), np.linalg.norm(detail["j1"], axis=-1)
            jerk = h * h / 12 * (j0 + j1)
            pv = h / 2 * (n0 + n1) + jerk
            px = h * h / 3 * n0 + h * h / 6 * n1 + h / 2 * jerk      # x1 - drift = h^2/3 a0 + h^2/6 a1 + h^3/24 (j0 - j1)
        kappa = np.maximum(pv / np.linalg.norm(v1 - vd, axis=-1), px / np.linalg.norm(x1 - xd, axis=-1))
        if scheme == "kdk":
            kt = kappa * (K_A * (1.0 + amp) + kc) + 2.0
        else:
            hs = detail["hs"]
            kt = kappa * (K_A * (1.0 + amp * (1.0 + 2.0 * hs)) + kc * (1.0 + hs + 0.02) + jerk / pv * K_J) + 1.0
    return np.where(mm > 0.0, kt, 0.0)


def tolerance(ref, drift, kt, kr):
    """tol (..., 6) for states stacked as (..., 6) = x, y, z, vx, vy, vz; kt: a scalar or one K_term per entry (...)."""
    ref = np.asarray(ref, np.float64)
    kt = np.asarray(kt, np.float64)[..., None]
    ch = ref - np.asarray(drift, np.float64)
    lx = np.sqrt((ch[..., :3] ** 2).sum(-1))
    lv = np.sqrt((ch[..., 3:] ** 2).sum(-1))
    length = np.concatenate([np.repeat(lx[..., None], 3, -1), np.repeat(lv[..., None], 3, -1)], axis=-1)
    return kt * U * length + kr * U * np.abs(ref)


def stack(x1, v1):
    return np.concatenate([np.asarray(x1, np.float64)[..., :3], np.asarray(v1, np.float64)[..., :3]], axis=-1)


class Reference:
    """The reference of one (scheme, capacity, eps) for the sources `sources` (distinct columns): `ref` (S, n, 6), `drift`
    (n, 6), which does not depend on the source, `kt` (S, n), every entry's K_term, and `jerkless` (Hermite, on request)."""

    def __init__(self, scheme, capacity, eps, sources=None, jerkless=False, seed=0):
        self.scheme, self.capacity, self.eps = scheme, capacity, eps
        self.sources = np.arange(capacity) if sources is None else np.asarray(sources, np.int64)
        self.index = {int(c): k for k, c in enumerate(self.sources)}
        self.kr = K_ROUND[scheme]
        x, v = configuration(capacity, seed)
        m = probe_mass(capacity)
        x1, v1, detail = one_step(scheme, x, v, self.sources, m, DT, eps, detail=True)
        xd, vd = one_step(scheme, x, v, [-1], m, DT, eps)
        self.kt = k_term(scheme, detail, x1, v1, xd, vd)
        self.ref = stack(x1, v1)
        self.drift = stack(xd, vd)[0]
        self.jerkless = stack(*one_step(scheme, x, v, self.sources, m, DT, eps, variant="jerkless")) if jerkless else None

    def rows(self, sources, count):
        """(ref, tol) of the systems with these sources (-1: the null system) truncated to `count` rows: (len, count, 6)."""
        sources = np.asarray(sources, np.int64)
        k = np.array([self.index[int(c)] if c >= 0 else 0 for c in sources], dtype=np.int64)
        ref = self.ref[k, :count].copy()
        ref[sources < 0] = self.drift[:count]
        kt = self.kt[k, :count].copy()
        kt[sources < 0] = 0.0
        return ref, tolerance(ref, self.drift[None, :count], kt, self.kr)

    def probed(self):
        """(S, n) bool: the entries that carry a term (not the self pair)."""
        p = np.ones(self.ref.shape[:2], dtype=bool)
        p[np.arange(len(self.sources)), self.sources] = False
        return p

    def resolved(self, other, factor=8.0):
        """(S, n) bool: |ref - other| >= factor tol in at least one component."""
        tol = tolerance(self.ref, self.drift[None], self.kt, self.kr)
        return (np.abs(self.ref - other) >= factor * tol).any(-1)


def large_sources(n=CAPACITY_LARGE, count=None):
    """The sources probed at the large capacity for a system of `count` bodies: both ends, the columns about every wave, row
    group and quarter boundary, the last two of the count, and forty hashed ones (the same for every count)."""
    count = n if count is None else count
    fixed = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, count - 2, count - 1]
    hashed = [int(4 + _hash01(k, 77) * (n - 16)) for k in range(40)]
    return sorted(set(c for c in fixed + hashed if 0 <= c < count))


class Layout:
    """The systems of one probe batch of `capacity`: for each of the counts C and C - 5 every probed source, the null system
    and (with `coincident`) the system whose body count - 3 lies on its source, body 7.  `sources[s]` is -1 for a null
    system; `null_of[s]` the null system with the count of system s; `coincident` the set of coincident systems."""

    def __init__(self, capacity, coincident=True):
        self.capacity = capacity
        counts, sources, null_of, self.coincident, self.blocks = [], [], [], set(), []
        for count in (capacity, capacity - 5):
            cols = list(range(count)) if capacity in CAPACITIES_FULL else large_sources(capacity, count)
            first = len(counts)
            block = cols + [-1] + ([7] if coincident else [])
            null = first + len(cols)
            if coincident:
                self.coincident.add(first + len(cols) + 1)
            counts += [count] * len(block)
            sources += block
            null_of += [null] * len(block)
            self.blocks.append((first, len(block), count))
        self.counts = np.array(counts, dtype=np.int64)
        self.sources = np.array(sources, dtype=np.int64)
        self.null_of = np.array(null_of, dtype=np.int64)
        self.num_systems = len(counts)

    def all_sources(self):
        return sorted(set(int(c) for c in self.sources if c >= 0))

    def batch(self, massive=None):
        """(pos, vel) of the batch; `massive`: (B,) massive counts, whose tracer sources get the mass word 1.0."""
        return probe_batch(self.capacity, self.counts, self.sources, probe_mass(self.capacity), self.coincident,
                           tracer_from=massive)


def conditions(capacity, seed=0):
    """What K_round's derivation assumes of the inputs: (x_min, x_max, drift_share) of the configuration, the smallest and
    largest coordinate magnitude and the largest h |v_c| / |x_c|."""
    x, v = configuration(capacity, seed)
    x, v = np.abs(x.astype(np.float64)), np.abs(v[:, :3].astype(np.float64))
    return float(x.min()), float(x.max()), float((DT * v / x).max())


# ---- single terms of the analysis calls: gravity_at (acceleration, potential, tidal tensor), members, energy -------------

def single_terms(capacity, sources, eps, seed=0):
    """For each source and row, fp64: acceleration (S, n, 3), potential (S, n) and tidal tensor (S, n, 6) in the order
    {xx, xy, xz, yy, yz, zz}, with their tolerances (relative to the component; the tensor's diagonal has the two pieces
    of include/nbody_batch_gravity.h).  The self pair gives zeros."""
    x, _ = configuration(capacity, seed)
    x = x.astype(np.float64)
    src = np.asarray(sources, np.int64)
    m = probe_mass(capacity)
    d = x[src][:, None, :] - x[None, :, :]
    r2 = (d * d).sum(-1) + _eps2(eps)
    mm = np.full(r2.shape, m)
    mm[np.arange(len(src)), src] = 0.0
    inv = 1.0 / np.sqrt(np.where(r2 > 0.0, r2, 1.0))
    s = mm * inv ** 3
    acc = s[..., None] * d
    pot = -mm * inv
    ia, ib = np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2])
    t3 = (3.0 * s * inv * inv)[..., None] * d[..., ia] * d[..., ib]
    diag = (ia == ib).astype(np.float64)
    tid = t3 - diag * s[..., None]
    tol_t = U * (K_T * np.abs(t3) + diag * ((K_A - 2.0) * s[..., None] + np.abs(tid)))
    return {"acc": acc, "pot": pot, "tid": tid, "tol_acc": K_A * U * np.abs(acc), "tol_pot": K_P * U * np.abs(pot),
            "tol_tid": tol_t}


def check(got, ref, tol, sources=None, limit=8):
    """Compare got (S, n, 6) with ref under tol.  Returns (worst ratio, failures): failures is a list of dicts (system,
    source, row, component, got, ref, tol, ratio), worst first, at most `limit`."""
    got = np.asarray(got, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(tol > 0.0, np.abs(got - ref) / tol, np.where(got == ref, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    bad = np.argwhere(ratio > 1.0)
    order = np.argsort(-ratio[tuple(bad.T)], kind="stable")[:limit] if len(bad) else []
    out = []
    for s, i, c in bad[order] if len(bad) else []:
        out.append({"system": int(s), "source": int(sources[s]) if sources is not None else None, "row": int(i),
                    "component": COMPONENTS[c], "got": float(got[s, i, c]), "ref": float(ref[s, i, c]),
                    "tol": float(tol[s, i, c]), "ratio": float(ratio[s, i, c])})
    return worst, out


def bitwise_mismatches(got, null, sources, whole=None):
    """The (system, row) whose fp32 words differ from the null system's row: the source's own row of every system with a
    source (the self pair), and every row of the systems marked in `whole` (a tracer's mass word is never read).
    got: (S, n, k), null: (n, k), values that fit fp32."""
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    z = np.ascontiguousarray(null, dtype=np.float32).view(np.uint32)
    sources = np.asarray(sources, np.int64)
    out = []
    for s in np.flatnonzero(sources >= 0):
        c = int(sources[s])
        if not np.array_equal(g[s, c], z[c]):
            out.append((int(s), c))
    if whole is not None:
        for s in np.flatnonzero(np.asarray(whole)):
            out += [(int(s), int(i)) for i in np.flatnonzero((g[s] != z).any(-1))]
    return out


def describe(failures, head=""):
    return "; ".join(f"{head}system {f['system']} source column {f['source']} row {f['row']} {f['component']}: got {f['got']!r} "
                     f"ref {f['ref']!r} tol {f['tol']:.3g} (x{f['ratio']:.3g})" for f in failures)


# ---- an fp32 restatement of the loops' arithmetic, for the CPU test of the derived tolerance ------------------------------

def _f(a):
    return np.asarray(a, np.float32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _rsq(r2, wobble):
    """fp32 1/sqrt, moved by up to one ulp by `wobble` in {-1, 0, 1} (the instruction's documented accuracy)."""
    with np.errstate(divide="ignore"):
        y = (1.0 / np.sqrt(np.asarray(r2, np.float64))).astype(np.float32)
    up = np.nextafter(y, np.float32(np.inf))
    dn = np.nextafter(y, np.float32(0.0))
    out = np.where(wobble > 0, up, np.where(wobble < 0, dn, y))
    return np.where(np.isfinite(y) & (y > 0), out, y).astype(np.float32)


def _term_fp32(x, v, xs, vs, m, eps2, guard, wobble):
    """batch_forces_jerks' pair term (its a is batch_forces' too) in fp32: (a, j), each (..., 3) float32."""
    d = _f(xs) - _f(x)
    e = _f(vs) - _f(v)
    r2 = _fma(d[..., 0], d[..., 0], np.float32(eps2))
    r2 = _fma(d[..., 1], d[..., 1], r2)
    r2 = _fma(d[..., 2], d[..., 2], r2)
    if guard:
        r2 = np.where(r2 >= np.float32(2.0 ** -84), r2, np.float32(np.inf)).astype(np.float32)
    inv = _rsq(r2, wobble)
    inv2 = inv * inv
    s = (_f(m) * inv) * inv2
    rv = _fma(d[..., 2], e[..., 2], _fma(d[..., 1], e[..., 1], d[..., 0] * e[..., 0]))
    c = (np.float32(3.0) * rv) * inv2
    a = np.stack([_fma(d[..., k], s, np.float32(0.0)) for k in range(3)], axis=-1)
    j = np.stack([_fma(_fma(-c, d[..., k], e[..., k]), s, np.float32(0.0)) for k in range(3)], axis=-1)
    return a, j


def _r32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def emulate_fp32(scheme, x, v, sources, mass, dt, eps, seed=1):
    """What a correct fp32 kernel returns: the pair term in fp32 as the loops form it, the state update in fp64 rounded
    once per component as batch_kick / batch_drift / hermite_predict_* / hermite_correct do.  (S, n, 6) float64 holding
    fp32 values."""
    x = _f(np.asarray(x)[:, :3])
    v = _f(np.asarray(v)[:, :3])
    src = np.asarray(sources, np.int64).reshape(-1)
    S, n = len(src), len(x)
    h = float(np.float32(dt))
    eps2 = np.float32(eps) * np.float32(eps)
    guard = float(eps) == 0.0
    rng = np.random.default_rng(seed)
    m = np.broadcast_to(np.asarray(mass, np.float64), (S,)).copy()
    m[src < 0] = 0.0
    c = np.where(src < 0, 0, src)
    mm = np.broadcast_to(m[:, None], (S, n)).copy()
    X = np.broadcast_to(x[None].astype(np.float64), (S, n, 3))
    V = np.broadcast_to(v[None].astype(np.float64), (S, n, 3))
    xs, vs = X[np.arange(S), c][:, None, :], V[np.arange(S), c][:, None, :]

    def term(px, pv, sx, sv):
        a, j = _term_fp32(px, pv, sx, sv, mm, eps2, guard, rng.integers(-1, 2, size=(S, n)))
        return a.astype(np.float64), j.astype(np.float64)

    a0, j0 = term(X, V, xs, vs)
    if scheme == "kick_drift":
        v1 = _r32(a0 * h + V)
        x1 = _r32(v1 * h + X)
    elif scheme == "kdk":
        vh = _r32(a0 * (0.5 * h) + V)
        x1 = _r32(vh * h + X)
        sx1 = _r32(vs * h + xs)
        a1, _ = term(x1, vh, sx1, vs)
        v1 = _r32(a1 * (0.5 * h) + vh)
    else:
        h2, h3, h6 = 0.5 * h, h / 3.0, h / 6.0
        xp = _r32(h * (h2 * (h3 * j0 + a0) + V) + X)
        vp = _r32(h * (h2 * j0 + a0) + V)
        sxp = _r32(h * vs + xs)
        a1, j1 = term(xp, vp, sxp, vs)
        v1 = _r32(h2 * (h6 * (j0 - j1) + (a0 + a1)) + V)
        x1 = _r32(h2 * (h6 * (a0 - a1) + (V + v1)) + X)
    return np.concatenate([x1, v1], axis=-1)
