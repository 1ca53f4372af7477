"""fp64 numpy restatement of the batch's adaptive Hermite scheme (nbody_batch_evolve_on, include/nbody_batch_evolve.h),
built on hermite_ref.acc_jerk.  One system, its own step shared by its bodies:

    time     integer ticks of dt_max 2^-levels; a step at level L is 2^(levels - L) ticks, h = dt_max 2^-L (exact in fp64)
    step     hermite_ref.step's predict-evaluate-correct step with that h
    request  per body, from a0, a1, j0, j1 of the step just taken:
                 a2_0 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2        a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3
                 a2_1 = a2_0 + h a3
                 dt^2 = eta (|a1| |a2_1| + |j1|^2) / (|j1| |a3| + |a2_1|^2)          (zero denominator: +inf)
             the system's request is the minimum over its bodies; squares are compared, no root of the request is taken
    level    L* = the smallest level with (dt_max 2^-L*)^2 <= request, at most `levels` (a step that is still too long
             there counts as clamped); L* > L: refine to L* at once; L* < L: coarsen by ONE level, and only on a tick that
             is a multiple of the coarser step
    start    without a level: dt = eta_start |a| / |j| from the evaluation at the current state, minimum over the bodies

Everything is fp64 unless `round_state` rounds to fp32 what the kernel holds in fp32: the predicted state the evaluation
reads, the accelerations and jerks it returns (so the corrector and the request see the rounded ones) and the corrected
state.  `dt_max` is taken as given: pass an fp32-representable value to compare with the batch."""
import numpy as np

import hermite_ref

MAX_LEVELS = 20


def _f32(u):
    return u.astype(np.float32).astype(np.float64)


def request_start(a, j, eta_start):
    """(num, den) per body of the first step: dt^2 = num / den = eta_start^2 |a|^2 / |j|^2."""
    return (eta_start * eta_start) * (a * a).sum(1), (j * j).sum(1)


def request(a0, a1, j0, j1, h, eta):
    """(num, den) per body of Aarseth's dt^2 = num / den from the accelerations and jerks at both ends of a step of length
    h.  As in the kernel nothing is divided: 1 / h^2 and 1 / h^3 are multiplied with, and level_for compares products."""
    d = a0 - a1
    a2_0 = (-6.0 * d - h * (4.0 * j0 + 2.0 * j1)) * (1.0 / (h * h))
    a3 = (12.0 * d + (6.0 * h) * (j0 + j1)) * (1.0 / (h * h * h))
    a2_1 = a2_0 + h * a3
    A1, A2, J1, A3 = (a1 * a1).sum(1), (a2_1 * a2_1).sum(1), (j1 * j1).sum(1), (a3 * a3).sum(1)
    return eta * (np.sqrt(A1 * A2) + J1), np.sqrt(J1 * A3) + A2


def level_for(req, dt_max, levels):
    """(L*, clamped): the smallest level whose squared step h2 is too long for no body -- h2 den > num, never for
    den = 0 -- at most `levels`.  That is the level of the minimum of num / den over the bodies."""
    num, den = req
    L, h2 = 0, float(dt_max) * float(dt_max)
    while L < levels and np.any(h2 * den > num):
        h2 *= 0.25
        L += 1
    return L, bool(np.any(h2 * den > num))


class Result:
    """pos, vel (n, 4) fp64; level_seq[i], tick_seq[i]: level of step i and the tick it started on; coarsen_ticks: the ticks
    on which the level went down; steps, clamped, ticks (the final tick), level (the level the next step would take)."""


def evolve(pos, vel, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, round_state=False, level=None,
           max_steps=None):
    assert 0 <= levels <= MAX_LEVELS
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = pos[:, 3]
    x, v = pos[:, :3].copy(), vel[:, :3].copy()
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    a, j = hermite_ref.acc_jerk(x, v, m, eps)
    if round_state:
        a, j = _f32(a), _f32(j)
    clamped = 0
    if level is None:
        level, c = level_for(request_start(a, j, eta_start), dt_max, levels)
        clamped += c
    tick, level_seq, tick_seq, coarsen_ticks = 0, [], [], []
    while tick < target and (max_steps is None or len(level_seq) < max_steps):
        h = dt_max * 2.0 ** -level
        xp = x + h * (v + h / 2 * (a + h / 3 * j))
        vp = v + h * (a + h / 2 * j)
        if round_state:
            xp, vp = _f32(xp), _f32(vp)
        a1, j1 = hermite_ref.acc_jerk(xp, vp, m, eps)
        if round_state:
            a1, j1 = _f32(a1), _f32(j1)
        v1 = v + h / 2 * ((a + a1) + h / 6 * (j - j1))
        x1 = x + h / 2 * ((v + v1) + h / 6 * (a - a1))
        if round_state:
            x1, v1 = _f32(x1), _f32(v1)
        req = request(a, a1, j, j1, h, eta)
        x, v, a, j = x1, v1, a1, j1
        level_seq.append(level)
        tick_seq.append(tick)
        tick += 1 << (levels - level)
        want, c = level_for(req, dt_max, levels)
        clamped += c
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            coarsen_ticks.append(tick)
            level -= 1
    res = Result()
    res.pos = pos.copy()
    res.pos[:, :3] = x
    res.vel = np.zeros((vel.shape[0], 4))
    res.vel[:, :vel.shape[1]] = vel
    res.vel[:, :3] = v
    res.level_seq, res.tick_seq, res.coarsen_ticks = level_seq, tick_seq, coarsen_ticks
    res.steps, res.clamped, res.ticks, res.level, res.target = len(level_seq), clamped, tick, level, target
    return res
