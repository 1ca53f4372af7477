"""fp64 numpy restatement of the batch's fourth-order Hermite scheme (NBODY_INTEGRATOR_HERMITE, include/nbody.h):

    xp = x0 + v0 h + a0 h^2/2 + j0 h^3/6            vp = v0 + a0 h + j0 h^2/2
    (a1, j1) = F(xp, vp)
    v1 = v0 + (a0 + a1) h/2 + (j0 - j1) h^2/12
    x1 = x0 + (v0 + v1) h/2 + (a0 - a1) h^2/12

with F the softened acceleration and jerk, a_i = sum_j m_j d / (r^2 + eps^2)^(3/2) and
j_i = sum_j m_j (e - 3 (d.e) d / (r^2 + eps^2)) / (r^2 + eps^2)^(3/2), d = x_j - x_i, e = v_j - v_i; for eps = 0 a pair at
zero distance (the self pair) adds nothing.  Vectorised over a chunk of rows at a time, so 4096 bodies stay cheap.  The
state stays fp64 unless `round_state` rounds it to fp32 after every step, as the batch's buffers do."""
import numpy as np

from conftest import rel_state_error  # noqa: F401  (the metric the Hermite tests apply to this reference)

ROW_CHUNK = 256


def acc_jerk(x, v, m, eps, chunk=ROW_CHUNK):
    """(a, j), each (n, 3) fp64, of bodies at x, v (n, 3) with masses m (n,)."""
    x = np.asarray(x, np.float64)
    v = np.asarray(v, np.float64)
    m = np.asarray(m, np.float64)
    n = x.shape[0]
    a = np.zeros((n, 3))
    j = np.zeros((n, 3))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = x[None, :, :] - x[lo:hi, None, :]          # (rows, n, 3): column minus row
        e = v[None, :, :] - v[lo:hi, None, :]
        r2 = np.einsum("ijk,ijk->ij", d, d) + eps * eps
        with np.errstate(divide="ignore"):
            inv2 = np.where(r2 > 0.0, 1.0 / np.where(r2 > 0.0, r2, 1.0), 0.0)
        s = m[None, :] * inv2 * np.sqrt(inv2)           # m_j / r^3
        rv = np.einsum("ijk,ijk->ij", d, e)
        a[lo:hi] = np.einsum("ij,ijk->ik", s, d)
        j[lo:hi] = np.einsum("ij,ijk->ik", s, e) - np.einsum("ij,ijk->ik", 3.0 * rv * inv2 * s, d)
    return a, j


def step(pos, vel, dt, eps, nsteps=1, round_state=False):
    """`nsteps` Hermite steps of one system: pos = (n, 4) {x, y, z, m}, vel = (n, 3 or 4).  Returns (pos, vel) as fp64
    (n, 4) arrays, the mass and the velocities' 4th column carried over."""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = pos[:, 3]
    x, v = pos[:, :3].copy(), vel[:, :3].copy()
    h = float(dt)
    a, j = acc_jerk(x, v, m, eps)
    for _ in range(nsteps):
        xp = x + h * (v + h / 2 * (a + h / 3 * j))
        vp = v + h * (a + h / 2 * j)
        a1, j1 = acc_jerk(xp, vp, m, eps)
        v1 = v + h / 2 * ((a + a1) + h / 6 * (j - j1))
        x1 = x + h / 2 * ((v + v1) + h / 6 * (a - a1))
        if round_state:
            x1, v1 = x1.astype(np.float32).astype(np.float64), v1.astype(np.float32).astype(np.float64)
            a1, j1 = a1.astype(np.float32).astype(np.float64), j1.astype(np.float32).astype(np.float64)
        x, v, a, j = x1, v1, a1, j1
    out_p = pos.copy()
    out_p[:, :3] = x
    out_v = np.zeros((vel.shape[0], 4))
    out_v[:, :vel.shape[1]] = vel
    out_v[:, :3] = v
    return out_p, out_v


def kepler(e=0.5, a=1.0, masses=(0.5, 0.5)):
    """Two bodies on a bound Kepler orbit of eccentricity e and semi-major axis a (G = 1), both at apocentre, centre of
    mass at rest at the origin: ((2, 4) positions, (2, 4) velocities, period)."""
    m1, m2 = masses
    M = m1 + m2
    ra = a * (1.0 + e)
    va = np.sqrt(M * (1.0 - e) / (a * (1.0 + e)))
    pos = np.array([[m2 / M * ra, 0.0, 0.0, m1], [-m1 / M * ra, 0.0, 0.0, m2]])
    vel = np.array([[0.0, m2 / M * va, 0.0, 0.0], [0.0, -m1 / M * va, 0.0, 0.0]])
    return pos, vel, 2.0 * np.pi * np.sqrt(a ** 3 / M)


#: the Chenciner-Montgomery figure-eight choreography of three unit masses (G = 1) and its period
FIGURE_EIGHT_PERIOD = 6.32591398


def figure_eight():
    x1 = np.array([0.97000436, -0.24308753])
    v3 = np.array([-0.93240737, -0.86473146])
    pos = np.zeros((3, 4))
    vel = np.zeros((3, 4))
    pos[0, :2], pos[1, :2] = x1, -x1
    pos[:, 3] = 1.0
    vel[0, :2] = vel[1, :2] = -v3 / 2
    vel[2, :2] = v3
    return pos, vel


def energy(pos, vel, eps=0.0):
    """Total energy (fp64) of one system."""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = pos[:, 3]
    kin = 0.5 * float((m * (vel[:, :3] ** 2).sum(1)).sum())
    d = pos[None, :, :3] - pos[:, None, :3]
    r2 = (d * d).sum(-1) + eps * eps
    iu = np.triu_indices(len(m), 1)
    pot = -float((m[iu[0]] * m[iu[1]] / np.sqrt(r2[iu])).sum())
    return kin + pot
