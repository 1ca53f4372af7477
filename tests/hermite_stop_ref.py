"""fp64 numpy restatement of the stopping conditions of Hermite batches (nbody_batch_stop_set, include/nbody_batch_stop.h)
on top of the adaptive scheme of hermite_adaptive_ref, whose step, request and level rule it takes by import:

    collision  at every acceleration-and-jerk evaluation (each step's, at the predicted positions; the initial one at the
               current positions): some pair i != j has d.d + eps^2 <= R_c^2 + eps^2
    escape     on the corrected positions after every step (and the current ones at the initial evaluation): some body has
               x.x > R_e^2, measured from the coordinate origin
    stopping   the step in which a condition is found is completed (corrector, level, tick); then the system leaves the loop
    report     reason (1 collision | 2 escape), the tick, the pair of smallest d.d + eps^2 (i < j, ties to the smallest i,
               then j) and its separation |d| at the evaluation that found it, the escaper of smallest index

Without conditions (both radii 0) this is hermite_adaptive_ref.evolve, operation for operation.  The deciding quantities
of every evaluation are kept, so that a test can see how far from the radius the decision fell: min_sep_seq[k] is the
smallest separation at evaluation k and max_dist_seq[k] the largest distance from the origin examined with it (k = 0: the
initial evaluation, k >= 1: step k)."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_ref

COLLISION, ESCAPE = 1, 2


def closest_pair(x, eps):
    """(i, j, separation, r2) of the pair i < j of smallest d.d + eps^2 (ties: smallest i, then smallest j)."""
    n = x.shape[0]
    iu, ju = np.triu_indices(n, 1)                      # row-major: ascending i, then ascending j
    d = x[ju] - x[iu]
    d2 = (d * d).sum(1)
    k = int(np.argmin(d2 + eps * eps))                  # the first minimum
    return int(iu[k]), int(ju[k]), float(np.sqrt(d2[k])), float(d2[k] + eps * eps)


def examine(x_eval, x_now, eps, collision_radius, escape_radius):
    """(reason, pair, separation, escaper, smallest separation, largest distance) of one evaluation: collisions among
    x_eval (the positions the evaluation read), escapers among x_now."""
    i, j, sep, r2 = closest_pair(x_eval, eps)
    dist2 = (x_now * x_now).sum(1)
    reason, pair, separation, escaper = 0, (-1, -1), 0.0, -1
    if collision_radius > 0.0 and r2 <= collision_radius * collision_radius + eps * eps:
        reason |= COLLISION
        pair, separation = (i, j), sep
    if escape_radius > 0.0 and np.any(dist2 > escape_radius * escape_radius):
        reason |= ESCAPE
        escaper = int(np.nonzero(dist2 > escape_radius * escape_radius)[0][0])
    return reason, pair, separation, escaper, sep, float(np.sqrt(dist2.max()))


class Result:
    """pos, vel (n, 4) fp64: the state at the stop (or at the target); steps, ticks, level_seq; reason, pair, separation,
    escaper (0, (0, 0), 0.0, 0 when the system did not stop, as the library reports); min_sep_seq, max_dist_seq, dist_seq
    (per evaluation, the distance of every body from the origin); eval_ticks (the tick of every evaluation); prev_min_sep: the smallest separation at the evaluation
    before the one that stopped the system (None at the initial evaluation)."""


def evolve(pos, vel, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, collision_radius=0.0,
           escape_radius=0.0, round_state=False, max_steps=None):
    assert 0 <= levels <= aref.MAX_LEVELS
    f32 = aref._f32
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    m = pos[:, 3]
    x, v = pos[:, :3].copy(), vel[:, :3].copy()
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    a, j = hermite_ref.acc_jerk(x, v, m, eps)
    if round_state:
        a, j = f32(a), f32(j)
    found = examine(x, x, eps, collision_radius, escape_radius)
    min_sep_seq, max_dist_seq, dist_seq = [found[4]], [found[5]], [np.sqrt((x * x).sum(1))]
    level, _ = aref.level_for(aref.request_start(a, j, eta_start), dt_max, levels)
    tick, level_seq, eval_ticks = 0, [], [0]
    while not found[0] and tick < target and (max_steps is None or len(level_seq) < max_steps):
        h = dt_max * 2.0 ** -level
        xp = x + h * (v + h / 2 * (a + h / 3 * j))
        vp = v + h * (a + h / 2 * j)
        if round_state:
            xp, vp = f32(xp), f32(vp)
        a1, j1 = hermite_ref.acc_jerk(xp, vp, m, eps)
        if round_state:
            a1, j1 = f32(a1), f32(j1)
        v1 = v + h / 2 * ((a + a1) + h / 6 * (j - j1))
        x1 = x + h / 2 * ((v + v1) + h / 6 * (a - a1))
        if round_state:
            x1, v1 = f32(x1), f32(v1)
        req = aref.request(a, a1, j, j1, h, eta)
        x, v, a, j = x1, v1, a1, j1
        level_seq.append(level)
        tick += 1 << (levels - level)
        want, _ = aref.level_for(req, dt_max, levels)
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            level -= 1
        found = examine(xp, x, eps, collision_radius, escape_radius)
        eval_ticks.append(tick)
        min_sep_seq.append(found[4])
        max_dist_seq.append(found[5])
        dist_seq.append(np.sqrt((x * x).sum(1)))
    res = Result()
    res.pos = pos.copy()
    res.pos[:, :3] = x
    res.vel = np.zeros((vel.shape[0], 4))
    res.vel[:, :vel.shape[1]] = vel
    res.vel[:, :3] = v
    res.steps, res.ticks, res.target, res.level_seq = len(level_seq), tick, target, level_seq
    res.reason, res.pair, res.separation, res.escaper = found[:4] if found[0] else (0, (0, 0), 0.0, 0)
    res.min_sep_seq, res.max_dist_seq, res.dist_seq = min_sep_seq, max_dist_seq, dist_seq
    res.eval_ticks = eval_ticks
    res.prev_min_sep = min_sep_seq[-2] if len(min_sep_seq) > 1 else None
    return res
