"""fp64 numpy restatement of external fields for Hermite batches (nbody_batch_field_set, include/nbody_batch_field.h), built
on hermite_ref.acc_jerk and on the scheme of hermite_adaptive_ref.evolve.  One system; its field is a list of components
(kind, p0, p1, p2), static and centred on the origin, G = 1:

    PLUMMER (M, b, -)          Phi = -M / sqrt(|x|^2 + b^2); at |x| = b = 0 the term is dropped, as a zero-distance pair is
    LOG_HALO (v0, rc, q)       w = (1, 1, 1 / q^2), D = sum w x^2 + rc^2, Phi = v0^2 ln(D) / 2
    MIYAMOTO_NAGAI (M, a, b)   s = sqrt(z^2 + b^2), A = a + s, D = x^2 + y^2 + A^2, Phi = -M / sqrt(D)

with a = -grad Phi and j = da/dt along v, the exact derivatives.  The field's (a, j) are added to the pair sums of every row
-- massive or not -- at the predicted state, before the corrector and before the time-step criterion.  `massive` is the
number of leading bodies that are columns (None: all); a tracer's mass word is carried and read by nothing.  Without
components and without `massive`, evolve is hermite_adaptive_ref.evolve, array for array."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_ref

NONE, PLUMMER, LOG_HALO, MIYAMOTO_NAGAI = 0, 1, 2, 3
KINDS = {"none": NONE, "plummer": PLUMMER, "log_halo": LOG_HALO, "miyamoto_nagai": MIYAMOTO_NAGAI}


def _kind(k):
    return KINDS[k] if isinstance(k, str) else int(k)


def _f32(u):
    return u.astype(np.float32).astype(np.float64)


def potential(x, components):
    """Phi (n,) fp64 at x (n, 3)."""
    x = np.asarray(x, np.float64)
    X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
    phi = np.zeros(x.shape[0])
    for kind, p0, p1, p2 in components:
        kind, p0, p1, p2 = _kind(kind), float(p0), float(p1), float(p2)
        if kind == PLUMMER:
            r2 = X * X + Y * Y + Z * Z + p1 * p1
            phi += np.where(r2 > 0.0, -p0 / np.sqrt(np.where(r2 > 0.0, r2, 1.0)), 0.0)
        elif kind == LOG_HALO:
            phi += 0.5 * (p0 * p0) * np.log(X * X + Y * Y + Z * Z / (p2 * p2) + p1 * p1)
        elif kind == MIYAMOTO_NAGAI:
            A = p1 + np.sqrt(Z * Z + p2 * p2)
            phi += -p0 / np.sqrt(X * X + Y * Y + A * A)
        else:
            assert kind == NONE, kind
    return phi


def field_acc_jerk(x, v, components):
    """(a, j), each (n, 3) fp64, of the field at positions x and velocities v (n, 3)."""
    x = np.asarray(x, np.float64)
    v = np.asarray(v, np.float64)
    a = np.zeros_like(x)
    j = np.zeros_like(x)
    for kind, p0, p1, p2 in components:
        kind, p0, p1, p2 = _kind(kind), float(p0), float(p1), float(p2)
        if kind == PLUMMER:
            r2 = (x * x).sum(1) + p1 * p1
            ok = r2 > 0.0
            u = np.where(ok, np.where(ok, r2, 1.0) ** -1.5, 0.0)          # D^-3/2
            ud = -3.0 * u * (x * v).sum(1) * np.where(ok, 1.0 / np.where(ok, r2, 1.0), 0.0)
            a += -p0 * x * u[:, None]
            j += -p0 * (v * u[:, None] + x * ud[:, None])
        elif kind == LOG_HALO:
            w = np.array([1.0, 1.0, 1.0 / (p2 * p2)])
            D = (w * x * x).sum(1) + p1 * p1
            Dd = 2.0 * (w * x * v).sum(1)
            a += -(p0 * p0) * w * x / D[:, None]
            j += -(p0 * p0) * (w * v / D[:, None] - w * x * (Dd / (D * D))[:, None])
        elif kind == MIYAMOTO_NAGAI:
            X, Y, Z = x[:, 0], x[:, 1], x[:, 2]
            VX, VY, VZ = v[:, 0], v[:, 1], v[:, 2]
            s = np.sqrt(Z * Z + p2 * p2)
            A = p1 + s
            D = X * X + Y * Y + A * A
            f = A / s
            sd = Z * VZ / s
            fd = -p1 * sd / (s * s)
            Dd = 2.0 * (X * VX + Y * VY) + 2.0 * A * sd
            u = D ** -1.5
            ud = -1.5 * D ** -2.5 * Dd
            a += -p0 * np.stack([X * u, Y * u, Z * f * u], axis=1)
            j += -p0 * np.stack([VX * u + X * ud, VY * u + Y * ud, (VZ * f + Z * fd) * u + Z * f * ud], axis=1)
        else:
            assert kind == NONE, kind
    return a, j


def acc_jerk(x, v, m, eps, components=(), massive=None):
    """The pair sums over the first `massive` bodies (None: all) plus the field, (a, j) fp64."""
    m = np.asarray(m, np.float64)
    if massive is not None:
        m = np.where(np.arange(m.shape[0]) < massive, m, 0.0)     # a zero-mass column adds nothing: no column at all
    a, j = hermite_ref.acc_jerk(x, v, m, eps)
    if any(_kind(c[0]) != NONE for c in components):
        fa, fj = field_acc_jerk(x, v, components)
        a, j = a + fa, j + fj
    return a, j


def evolve(pos, vel, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, components=(), massive=None,
           round_state=False, level=None, max_steps=None):
    """hermite_adaptive_ref.evolve with the field and the column bound; the same Result."""
    assert 0 <= levels <= aref.MAX_LEVELS
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = pos[:, 3]
    x, v = pos[:, :3].copy(), vel[:, :3].copy()
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    a, j = acc_jerk(x, v, m, eps, components, massive)
    if round_state:
        a, j = _f32(a), _f32(j)
    clamped = 0
    if level is None:
        level, c = aref.level_for(aref.request_start(a, j, eta_start), dt_max, levels)
        clamped += c
    tick, level_seq, tick_seq, coarsen_ticks = 0, [], [], []
    while tick < target and (max_steps is None or len(level_seq) < max_steps):
        h = dt_max * 2.0 ** -level
        xp = x + h * (v + h / 2 * (a + h / 3 * j))
        vp = v + h * (a + h / 2 * j)
        if round_state:
            xp, vp = _f32(xp), _f32(vp)
        a1, j1 = acc_jerk(xp, vp, m, eps, components, massive)
        if round_state:
            a1, j1 = _f32(a1), _f32(j1)
        v1 = v + h / 2 * ((a + a1) + h / 6 * (j - j1))
        x1 = x + h / 2 * ((v + v1) + h / 6 * (a - a1))
        if round_state:
            x1, v1 = _f32(x1), _f32(v1)
        req = aref.request(a, a1, j, j1, h, eta)
        x, v, a, j = x1, v1, a1, j1
        level_seq.append(level)
        tick_seq.append(tick)
        tick += 1 << (levels - level)
        want, c = aref.level_for(req, dt_max, levels)
        clamped += c
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            coarsen_ticks.append(tick)
            level -= 1
    res = aref.Result()
    res.pos = pos.copy()
    res.pos[:, :3] = x
    res.vel = np.zeros((vel.shape[0], 4))
    res.vel[:, :vel.shape[1]] = vel
    res.vel[:, :3] = v
    res.level_seq, res.tick_seq, res.coarsen_ticks = level_seq, tick_seq, coarsen_ticks
    res.steps, res.clamped, res.ticks, res.level, res.target = len(level_seq), clamped, tick, level, target
    return res


def specific_energy(pos, vel, components):
    """v^2 / 2 + Phi per body, fp64 (a tracer's energy per unit mass in the field alone)."""
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    return 0.5 * (vel[:, :3] ** 2).sum(1) + potential(pos[:, :3], components)


# ---- the orbit of the GPU suite's energy test: one tracer, massive count 0, in a flattened logarithmic halo ------------------
#: v0 = 1, rc = 0.1, q = 0.9: a flat rotation curve of speed 1 outside a core of 0.1, flattened along z
HALO = [("log_halo", 1.0, float(np.float32(0.1)), float(np.float32(0.9)))]      # the fp32 values the batch is given
#: from apocentre at radius ~3 with 0.3 of the circular speed: the orbit plunges to a pericentre about six times closer,
#: inclined.  Its specific energy is ~1.17 (Phi = ln(D) / 2 ~ 1.1 out there), so a relative error means what an absolute one
#: in units of v0^2 means.
ORBIT_POS = np.array([[3.0, 0.0, 0.6, 0.0]], np.float32).astype(np.float64)
ORBIT_VEL = np.array([[0.0, 0.3, 0.05, 0.0]], np.float32).astype(np.float64)
ORBIT_DT_MAX = 1.0 / 8.0
ORBIT_INTERVALS = 320          # to t = 40: several radial periods
ORBIT_LEVELS = 12
ORBIT_ETA = 0.01               # eta = eta_start
