"""fp64 numpy restatement of mergers in Hermite batches (nbody_batch_merge_set, include/nbody_batch_merge.h) on top of the
stopping conditions of hermite_stop_ref and the adaptive scheme of hermite_adaptive_ref, whose step, request, level rule and
examination it takes by import:

    detection  hermite_stop_ref's: at every evaluation some pair has d.d + eps^2 <= R_c^2 + eps^2; the step is completed
    pair       the pair of smallest d.d + eps^2 at that evaluation, i < j, ties to the smallest i, then j
    merger     on the corrected state (the current one at the initial evaluation): m = m_i + m_j, x and v the mass-weighted
               means (the arithmetic mean for m = 0); the survivor keeps slot i and its velocity's w; bodies j and n - 1
               swap slots and the count drops, so the absorbed body's last state lies in the first slot beyond the count
    restart    a and j evaluated afresh at the current state -- not a step; it examines collisions and escapers among the
               current positions -- and the level L = min(levels, max(L*, L_tick)): L* from the first-step rule, L_tick the
               smallest level whose step divides the tick.  Another collision there merges at once; an escaper stops the
               system with reason ESCAPE.  A step that finds both merges first, and the restart judges the escape anew.

With merge=False this is hermite_stop_ref.evolve itself.  `round_state` rounds to fp32 what the kernel holds in fp32, as there,
and the merged mass, position and velocity.  Kept per evaluation: min_sep_seq (the smallest separation), max_dist_seq, eval_ticks and
eval_kind ("start", "step" or "restart"); per step level_seq and tick_seq; per restart restart_seq = (tick, L*, L_tick, L);
per merger an entry of `mergers` (see Merger)."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_ref
import hermite_stop_ref as sref

COLLISION, ESCAPE = sref.COLLISION, sref.ESCAPE


def closest_pair(x, eps):
    """hermite_stop_ref.closest_pair for any n ((-1, -1, inf, inf) below two bodies): the candidates from the Gram matrix,
    |x_i|^2 + |x_j|^2 - 2 x_i.x_j, within its rounding of the minimum; among them the differences themselves decide."""
    n = x.shape[0]
    if n < 2:
        return -1, -1, np.inf, np.inf
    sq = (x * x).sum(1)
    approx = sq[:, None] + sq[None, :] - 2.0 * (x @ x.T)
    approx[np.tril_indices(n)] = np.inf                                             # j > i only
    iu, ju = np.nonzero(approx <= approx.min() + 1e-9 * (1.0 + sq.max()))           # row-major: ascending i, then ascending j
    d = x[ju] - x[iu]
    d2 = (d * d).sum(1)
    k = int(np.argmin(d2 + eps * eps))                                              # the first minimum
    return int(iu[k]), int(ju[k]), float(np.sqrt(d2[k])), float(d2[k] + eps * eps)


def examine(x_eval, x_now, eps, collision_radius, escape_radius):
    """hermite_stop_ref.examine's tuple, with closest_pair above."""
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


def tick_level(tick, levels):
    """The smallest level whose step 2^(levels - L) divides the tick."""
    L = 0
    while L < levels and tick % (1 << (levels - L)) != 0:
        L += 1
    return L


class Merger:
    """tick, survivor, absorbed (before the swap), count_before, separation (at the evaluation that found the pair),
    relative_speed and mass_survivor, mass_absorbed (at the state merged), eval_index (of that evaluation in min_sep_seq),
    mass_before / mass_after and momentum_before / momentum_after (sums over the system's bodies, fp64), momentum_scale
    (sum m |v| over them before the merger)."""


class Result:
    """pos, vel (n0, 4) fp64: all slots, the absorbed bodies' last states beyond `count`; count; steps, ticks, target,
    level_seq, tick_seq; reason (0 or ESCAPE), escaper (0 when the system did not stop, as the library reports);
    mergers; min_sep_seq, max_dist_seq (the largest distance from the origin examined), eval_ticks, eval_kind, restart_seq."""


def evolve(pos, vel, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, collision_radius=0.0,
           escape_radius=0.0, merge=True, round_state=False, max_steps=None):
    if not merge:
        return sref.evolve(pos, vel, n_intervals, dt_max, levels=levels, eta=eta, eta_start=eta_start, eps=eps,
                           collision_radius=collision_radius, escape_radius=escape_radius, round_state=round_state,
                           max_steps=max_steps)
    assert 0 <= levels <= aref.MAX_LEVELS
    f32 = aref._f32 if round_state else (lambda u: u)
    P = np.array(pos, np.float64)
    V = np.zeros((P.shape[0], 4))
    V[:, :np.shape(vel)[1]] = vel
    n = P.shape[0]
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    res = Result()
    res.mergers, res.min_sep_seq, res.max_dist_seq, res.eval_ticks, res.eval_kind, res.restart_seq = [], [], [], [], [], []
    level_seq, tick_seq = [], []
    tick = 0

    def note(found, kind):
        res.min_sep_seq.append(found[4])
        res.max_dist_seq.append(found[5])
        res.eval_ticks.append(tick)
        res.eval_kind.append(kind)

    def restart(kind):
        x, v, m = P[:n, :3], V[:n, :3], P[:n, 3]
        a, j = hermite_ref.acc_jerk(x, v, m, eps)
        a, j = f32(a), f32(j)
        found = examine(x, x, eps, collision_radius, escape_radius)
        note(found, kind)
        want, _ = aref.level_for(aref.request_start(a, j, eta_start), dt_max, levels)
        floor_level = tick_level(tick, levels)
        level = min(levels, max(want, floor_level))
        res.restart_seq.append((tick, want, floor_level, level))
        return a, j, found, level

    a, j, found, level = restart("start")
    while True:
        while found[0] & COLLISION:
            i, k = found[1]
            last = n - 1
            mi, mj = P[i, 3], P[k, 3]
            mg = Merger()
            mg.tick, mg.survivor, mg.absorbed, mg.count_before, mg.separation = tick, i, k, n, found[2]
            mg.relative_speed = float(np.sqrt(((V[k, :3] - V[i, :3]) ** 2).sum()))
            mg.mass_survivor, mg.mass_absorbed = float(mi), float(mj)
            mg.eval_index = len(res.min_sep_seq) - 1
            mg.mass_before = float(P[:n, 3].sum())
            mg.momentum_before = (P[:n, 3:4] * V[:n, :3]).sum(0)
            mg.momentum_scale = float((P[:n, 3] * np.sqrt((V[:n, :3] ** 2).sum(1))).sum())
            M = mi + mj
            if M == 0.0:
                xm, vm = 0.5 * (P[i, :3] + P[k, :3]), 0.5 * (V[i, :3] + V[k, :3])
            else:
                xm, vm = (mj * P[k, :3] + mi * P[i, :3]) / M, (mj * V[k, :3] + mi * V[i, :3]) / M
            absorbed_p, absorbed_v = P[k].copy(), V[k].copy()
            P[i, :3], V[i, :3] = f32(xm), f32(vm)
            P[i, 3] = f32(np.float64(M))
            if k != last:
                P[k], V[k] = P[last], V[last]
            P[last], V[last] = absorbed_p, absorbed_v
            n -= 1
            mg.mass_after = float(P[:n, 3].sum())
            mg.momentum_after = (P[:n, 3:4] * V[:n, :3]).sum(0)
            res.mergers.append(mg)
            a, j, found, level = restart("restart")
        if found[0] or tick >= target or (max_steps is not None and len(level_seq) >= max_steps):
            break
        x, v, m = P[:n, :3], V[:n, :3], P[:n, 3]
        h = dt_max * 2.0 ** -level
        xp = f32(x + h * (v + h / 2 * (a + h / 3 * j)))
        vp = f32(v + h * (a + h / 2 * j))
        a1, j1 = hermite_ref.acc_jerk(xp, vp, m, eps)
        a1, j1 = f32(a1), f32(j1)
        v1 = v + h / 2 * ((a + a1) + h / 6 * (j - j1))
        x1 = x + h / 2 * ((v + v1) + h / 6 * (a - a1))
        x1, v1 = f32(x1), f32(v1)
        req = aref.request(a, a1, j, j1, h, eta)
        P[:n, :3], V[:n, :3], a, j = x1, v1, a1, j1
        level_seq.append(level)
        tick_seq.append(tick)
        tick += 1 << (levels - level)
        want, _ = aref.level_for(req, dt_max, levels)
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            level -= 1
        found = examine(xp, P[:n, :3], eps, collision_radius, escape_radius)
        note(found, "step")
    res.pos, res.vel, res.count = P, V, n
    res.steps, res.ticks, res.target, res.level_seq, res.tick_seq = len(level_seq), tick, target, level_seq, tick_seq
    res.reason, res.escaper = (ESCAPE, found[3]) if found[0] else (0, 0)
    return res
