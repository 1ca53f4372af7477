"""The fp64 numpy reference of nbody_batch_pairs (include/nbody_batch_pairs.h): every body's partner by the smallest two-body
energy and the orbital elements of the pair, from the fp32 state; a float32 emulation of the kernel's search; and the inputs
the GPU suite runs (hard binaries on a jittered lattice plus a few singles), which the CPU suite checks too.

The reference takes the state as float32 and does everything else in float64, as the header's record does; only the rule
"a pair whose fp32 squared distance is 0 is no candidate" looks at a float32 number."""
import numpy as np

EMPTY = dict(partner=-1, mutual=False, energy=0.0, semi_major_axis=0.0, eccentricity=0.0, inclination=0.0, separation=0.0)
FIELDS = ("energy", "semi_major_axis", "eccentricity", "inclination", "separation")


def elements(xi, vi, xj, vj, mu):
    """(energy, a, e, inclination, separation) of pairs: (..., 3) float64 states of the row and its partner, mu (...,)."""
    xi, vi, xj, vj, mu = (np.asarray(u, dtype=np.float64) for u in (xi, vi, xj, vj, mu))
    r, v = xj - xi, vj - vi
    with np.errstate(divide="ignore", invalid="ignore"):
        sep = np.sqrt((r * r).sum(-1))
        energy = 0.5 * (v * v).sum(-1) - mu / sep
        h = np.cross(r, v)
        hn = np.sqrt((h * h).sum(-1))
        inc = np.where(hn > 0, np.arccos(np.clip(np.where(hn > 0, h[..., 2] / hn, 1.0), -1.0, 1.0)), 0.0)
        a = np.where(energy == 0, np.inf, -mu / (2.0 * energy))
        evec = np.cross(v, h) / mu[..., None] - r / sep[..., None]
        e = np.sqrt((evec * evec).sum(-1))
        a = np.where(mu == 0, 0.0, a)
        e = np.where(mu == 0, np.inf, e)
    return energy, a, e, inc, sep


def _row_mass(pos, n, massive):
    """The mass row i adds to mu: its own, or 0 for a test particle."""
    m = n if massive is None else min(int(massive), n)
    mi = pos[:n, 3].astype(np.float64).copy()
    mi[m:] = 0.0
    return m, mi


def pair_energies(pos, vel, n, massive=None, rows=None):
    """(eps, scale, valid): (len(rows), m) float64 energies v^2/2 - mu/r of the rows against the candidate columns, the sum
    v^2/2 + mu/r of the two terms, and which pairs are candidates."""
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    m, mi = _row_mass(pos, n, massive)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    d32 = pos[None, :m, :3] - pos[rows, None, :3]
    r2_32 = (d32[..., 0] * d32[..., 0] + d32[..., 1] * d32[..., 1]) + d32[..., 2] * d32[..., 2]
    d = pos[None, :m, :3].astype(np.float64) - pos[rows, None, :3].astype(np.float64)
    w = vel[None, :m, :3].astype(np.float64) - vel[rows, None, :3].astype(np.float64)
    r = np.sqrt((d * d).sum(-1))
    valid = (np.arange(m)[None, :] != rows[:, None]) & (r2_32 > 0) & (r > 0)
    mu = pos[None, :m, 3].astype(np.float64) + mi[rows, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        kin, pot = 0.5 * (w * w).sum(-1), mu / r
    return np.where(valid, kin - pot, np.inf), kin + pot, valid


def pairs(pos, vel, n, massive=None, chunk=256):
    """The reference of one system: a dict of (capacity,) arrays -- partner, mutual, FIELDS and terms -- and ``binaries``, from the
    (capacity, 4) float32 state, its count n and its massive count (None: off).  Rows are evaluated ``chunk`` at a time."""
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    cap = pos.shape[0]
    out = {k: np.full(cap, v, dtype=np.int32 if k == "partner" else bool if k == "mutual" else np.float64) for k, v in EMPTY.items()}
    m, mi = _row_mass(pos, n, massive)
    for lo in range(0, n, chunk):
        rows = np.arange(lo, min(lo + chunk, n))
        eps, _, valid = pair_energies(pos, vel, n, massive, rows)
        if m:
            j = np.argmin(eps, axis=1)                       # the first of equal minima: ties go to the lower j
            out["partner"][rows] = np.where(valid[np.arange(len(rows)), j], j, -1)
    p = out["partner"]
    has = np.nonzero(p[:n] >= 0)[0]
    out["mutual"][has] = p[p[has]] == has
    if len(has):
        j = p[has]
        mu = pos[j, 3].astype(np.float64) + mi[has]
        for k, val in zip(FIELDS, elements(pos[has, :3], vel[has, :3], pos[j, :3], vel[j, :3], mu)):
            out[k][has] = val
        out["terms"] = np.zeros(cap)                          # v^2/2 + mu/r of the chosen pair: what the energy cancels from
        out["terms"][has] = out["energy"][has] + 2.0 * mu / out["separation"][has]
    out["binaries"] = int((out["mutual"] & (out["energy"] < 0) & (np.arange(cap) < p)).sum())
    return out


def _fma32(a, b, c):
    """fmaf of float32 arrays, up to the double rounding of one in 2^29 results."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def select_f32(pos, vel, n, massive=None, chunk=256):
    """The partner of every row as the kernel's fp32 search chooses it (the header's operation order; the hardware's
    reciprocal square root is emulated by the correctly rounded one): (capacity,) int32."""
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    partner = np.full(pos.shape[0], -1, dtype=np.int32)
    m, mi = _row_mass(pos, n, massive)
    mi = mi.astype(np.float32)
    if m == 0:
        return partner
    for lo in range(0, n, chunk):
        rows = np.arange(lo, min(lo + chunk, n))
        d = pos[None, :m, :3] - pos[rows, None, :3]
        w = vel[None, :m, :3] - vel[rows, None, :3]
        r2 = _fma32(d[..., 2], d[..., 2], _fma32(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        v2 = _fma32(w[..., 2], w[..., 2], _fma32(w[..., 1], w[..., 1], w[..., 0] * w[..., 0]))
        with np.errstate(divide="ignore"):
            inv = (1.0 / np.sqrt(r2.astype(np.float64))).astype(np.float32)
        mu = pos[None, :m, 3] + mi[rows, None]
        with np.errstate(invalid="ignore"):
            eps = _fma32(-mu, inv, np.float32(0.5) * v2)
        eps = np.where((r2 > 0) & ~np.isnan(eps), eps, np.float32(np.inf))
        j = np.argmin(eps, axis=1)
        partner[rows] = np.where(eps[np.arange(len(rows)), j] < np.inf, j, -1)
    return partner


# ---- the inputs -------------------------------------------------------------------------------------------------------------
SPACING = 2.0  # between lattice sites; the binaries' semi-major axes are 0.01 .. 0.05


def _unit(rng, k):
    u = rng.normal(size=(k, 3))
    return u / np.linalg.norm(u, axis=1)[:, None]


def binaries_and_singles(n, seed):
    """(pos, vel): (n, 4) float32.  Hard binaries -- a in [0.01, 0.05], e in [0.1, 0.8], masses in [0.5, 1.5], any phase and
    orientation -- and n % 2 + 2 (n // 20) singles, one object per site of a cubic lattice of spacing 2 with a jitter of
    +-0.3, drifting at up to 0.1 per component (the orbital speeds are 4 .. 20), the bodies in a random order.  So every
    binary member's partner is its companion by a wide margin, and the eccentricities are well away from 0."""
    rng = np.random.default_rng(seed)
    singles = n % 2 + 2 * (n // 20)
    nb = (n - singles) // 2
    objects = nb + singles
    side = max(1, int(np.ceil(objects ** (1.0 / 3.0))))
    sites = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)[:objects]]
    centre = (sites - 0.5 * (side - 1)) * SPACING + rng.uniform(-0.3, 0.3, size=(objects, 3))
    drift = rng.uniform(-0.1, 0.1, size=(objects, 3))
    pos, vel = np.zeros((n, 4)), np.zeros((n, 4))
    m1, m2 = rng.uniform(0.5, 1.5, size=nb), rng.uniform(0.5, 1.5, size=nb)
    a, e, E = rng.uniform(0.01, 0.05, size=nb), rng.uniform(0.1, 0.8, size=nb), rng.uniform(0, 2 * np.pi, size=nb)
    p = _unit(rng, nb)
    q = np.cross(p, _unit(rng, nb))
    q /= np.linalg.norm(q, axis=1)[:, None]
    mu = m1 + m2
    b = a * np.sqrt(1 - e * e)
    rel = (a * (np.cos(E) - e))[:, None] * p + (b * np.sin(E))[:, None] * q
    Edot = np.sqrt(mu / a ** 3) / (1 - e * np.cos(E))
    relv = (-a * np.sin(E) * Edot)[:, None] * p + (b * np.cos(E) * Edot)[:, None] * q
    pos[0:2 * nb:2, :3], pos[1:2 * nb:2, :3] = centre[:nb] - (m2 / mu)[:, None] * rel, centre[:nb] + (m1 / mu)[:, None] * rel
    vel[0:2 * nb:2, :3], vel[1:2 * nb:2, :3] = drift[:nb] - (m2 / mu)[:, None] * relv, drift[:nb] + (m1 / mu)[:, None] * relv
    pos[0:2 * nb:2, 3], pos[1:2 * nb:2, 3] = m1, m2
    pos[2 * nb:, :3], vel[2 * nb:, :3] = centre[nb:], drift[nb:]
    pos[2 * nb:, 3] = rng.uniform(0.5, 1.5, size=singles)
    vel[:, 3] = 3.0 + np.arange(n)  # the fourth words of the velocities: read by nothing
    order = rng.permutation(n)
    return pos[order].astype(np.float32), vel[order].astype(np.float32)


FILL = 0.5  # what the slots beyond a system's count hold: a body's worth of numbers that nothing may read


def ragged(capacity, counts, seed0):
    """(P, V): (len(counts), capacity, 4) float32, system s the binaries_and_singles(counts[s], seed0 + s), the rest FILL."""
    P = np.full((len(counts), capacity, 4), FILL, dtype=np.float32)
    V = np.full((len(counts), capacity, 4), FILL, dtype=np.float32)
    for s, n in enumerate(counts):
        if n:
            P[s, :n], V[s, :n] = binaries_and_singles(n, seed0 + s)
    return P, V


#: capacity -> the counts of the batch the GPU suite runs at it (one, two and four rows per lane, two waves, sixteen waves)
CAPACITIES = {64: [0, 1, 2, 3, 63, 64], 128: [0, 1, 2, 3, 127, 128], 130: [0, 1, 2, 3, 129, 130], 257: [0, 1, 2, 3, 256, 257],
              4096: [4096, 300]}


def gpu_inputs(capacity):
    """(P, V, counts) of the GPU suite's batch at a capacity."""
    counts = CAPACITIES[capacity]
    P, V = ragged(capacity, counts, 9000 + capacity)
    return P, V, counts


#: the analytic case: a binary of a = 1, e = 0.6 (bodies 0 and 2) tilted by 0.4 about the x axis, and a distant single (body 1)
KNOWN = dict(a=1.0, e=0.6, m1=0.75, m2=0.25, inc=0.4)
KNOWN_PHASES = {"pericentre": 0.0, "E=1.3": 1.3, "apocentre": np.pi}


def known_binary(E):
    """(P, V, want): the (1, 3, 4) float32 state at eccentric anomaly E and the binary's (a, e, inclination, energy,
    separation) in closed form."""
    a, e, m1, m2, inc = (KNOWN[k] for k in ("a", "e", "m1", "m2", "inc"))
    mu, b = m1 + m2, a * np.sqrt(1 - e * e)
    ex, ey = np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(inc), np.sin(inc)])
    rel = a * (np.cos(E) - e) * ex + b * np.sin(E) * ey
    Edot = np.sqrt(mu / a ** 3) / (1 - e * np.cos(E))
    relv = -a * np.sin(E) * Edot * ex + b * np.cos(E) * Edot * ey
    P, V = np.zeros((1, 3, 4), np.float32), np.zeros((1, 3, 4), np.float32)
    P[0, 0], P[0, 2], P[0, 1] = [*(-m2 / mu * rel), m1], [*(m1 / mu * rel), m2], [200.0, 50.0, -30.0, 0.5]
    V[0, 0, :3], V[0, 2, :3], V[0, 1, :3] = -m2 / mu * relv, m1 / mu * relv, [0.0, 0.01, 0.0]
    return P, V, (a, e, inc, -mu / (2 * a), a * (1 - e * np.cos(E)))
