"""fp64 numpy restatement of per-body collision radii in Hermite batches (nbody_batch_radii_set,
include/nbody_batch_radii.h) on top of hermite_merge_ref, hermite_stop_ref and hermite_adaptive_ref, whose step, request, level
rule, restart and merger it takes by import or restates line for line:

    detection  at every evaluation some pair i != j has d.d + eps^2 <= S^2 + eps^2, S = R_i + R_j; the step is completed
    pair       among the pairs within their own threshold, the one of smallest d.d + eps^2, i < j, ties to the smallest i,
               then j -- not necessarily the closest pair of the system
    stop       (merge=False) the system leaves the loop and reports the pair, as hermite_stop_ref does
    merger     (merge=True) hermite_merge_ref's, and the survivor's radius becomes cbrt(R_i R_i R_i + R_j R_j R_j); the radii of
               slots j and n - 1 swap with their bodies; the restart examines collisions with the new radii

With radii=None this is hermite_merge_ref.evolve itself (collision_radius and all).  `round_state` rounds to fp32 what the
kernel holds in fp32, as there, and S and the merged radius.  Kept per evaluation beside hermite_merge_ref's sequences:
touch_seq, the smallest |d| / S over the pairs (inf where S = 0 < |d|, 0 where both are 0): below 1 a pair touches."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_merge_ref as mref
import hermite_ref

COLLISION, ESCAPE = mref.COLLISION, mref.ESCAPE


def pair_tables(x, R, eps, round_state=False):
    """(r2, thr2, d2, S) of every pair, n x n fp64: d.d + eps^2, S^2 + eps^2, d.d and S = R_i + R_j."""
    d2 = np.zeros((x.shape[0], x.shape[0]))
    for c in range(3):
        d = x[None, :, c] - x[:, None, c]
        d2 += d * d
    S = R[:, None] + R[None, :]
    if round_state:
        S = aref._f32(S)
    return d2 + eps * eps, S * S + eps * eps, d2, S


def colliding_pair(x, R, eps, round_state=False):
    """(i, j, separation, touch): the pair of the rule above ((-1, -1, 0.0, touch) when no pair is within its threshold) and
    the smallest |d| / S over all pairs."""
    n = x.shape[0]
    if n < 2:
        return -1, -1, 0.0, np.inf
    r2, thr2, d2, S = pair_tables(x, np.asarray(R, np.float64), eps, round_state)
    upper = np.triu(np.ones((n, n), bool), 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(S > 0.0, np.sqrt(d2) / S, np.where(d2 > 0.0, np.inf, 0.0))
    touch = float(ratio[upper].min())
    ok = upper & (r2 <= thr2)
    if not ok.any():
        return -1, -1, 0.0, touch
    k = int(np.argmin(np.where(ok, r2, np.inf)))                                    # row-major: the first minimum
    i, j = divmod(k, n)
    return i, j, float(np.sqrt(d2[i, j])), touch


def examine(x_eval, x_now, R, eps, escape_radius, round_state=False):
    """hermite_stop_ref.examine's tuple with the pair rule above; the fifth entry is the smallest |d| / S."""
    i, j, sep, touch = colliding_pair(x_eval, R, eps, round_state)
    dist2 = (x_now * x_now).sum(1)
    reason, pair, separation, escaper = 0, (-1, -1), 0.0, -1
    if i >= 0:
        reason |= COLLISION
        pair, separation = (i, j), sep
    if escape_radius > 0.0 and np.any(dist2 > escape_radius * escape_radius):
        reason |= ESCAPE
        escaper = int(np.nonzero(dist2 > escape_radius * escape_radius)[0][0])
    return reason, pair, separation, escaper, touch, float(np.sqrt(dist2.max()))


def merged_radius(ri, rj):
    return float(np.cbrt(ri * ri * ri + rj * rj * rj))


class Result:
    """hermite_merge_ref.Result's fields, and: radii (n0,) fp64, all slots; pair, separation (of a stop for a collision;
    (0, 0), 0.0 otherwise, as the library reports); touch_seq.  Every merger also has radius_survivor, radius_absorbed
    (before) and radius_after."""


def evolve(pos, vel, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, radii=None, collision_radius=0.0,
           escape_radius=0.0, merge=True, round_state=False, max_steps=None):
    if radii is None:
        return mref.evolve(pos, vel, n_intervals, dt_max, levels=levels, eta=eta, eta_start=eta_start, eps=eps,
                           collision_radius=collision_radius, escape_radius=escape_radius, merge=merge, round_state=round_state,
                           max_steps=max_steps)
    assert collision_radius == 0.0, "radii and collision_radius are both set"
    assert 0 <= levels <= aref.MAX_LEVELS
    f32 = aref._f32 if round_state else (lambda u: u)
    P = np.array(pos, np.float64)
    V = np.zeros((P.shape[0], 4))
    V[:, :np.shape(vel)[1]] = vel
    R = np.array(radii, np.float64).reshape(-1)[:P.shape[0]].copy()
    n = P.shape[0]
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    res = Result()
    res.mergers, res.touch_seq, res.max_dist_seq, res.eval_ticks, res.eval_kind, res.restart_seq = [], [], [], [], [], []
    level_seq, tick_seq = [], []
    tick = 0

    def note(found, kind):
        res.touch_seq.append(found[4])
        res.max_dist_seq.append(found[5])
        res.eval_ticks.append(tick)
        res.eval_kind.append(kind)

    def restart(kind):
        x, v, m = P[:n, :3], V[:n, :3], P[:n, 3]
        a, j = hermite_ref.acc_jerk(x, v, m, eps)
        a, j = f32(a), f32(j)
        found = examine(x, x, R[:n], eps, escape_radius, round_state)
        note(found, kind)
        want, _ = aref.level_for(aref.request_start(a, j, eta_start), dt_max, levels)
        floor_level = mref.tick_level(tick, levels)
        level = min(levels, max(want, floor_level))
        res.restart_seq.append((tick, want, floor_level, level))
        return a, j, found, level

    a, j, found, level = restart("start")
    while True:
        while merge and found[0] & COLLISION:
            i, k = found[1]
            last = n - 1
            mi, mj = P[i, 3], P[k, 3]
            mg = mref.Merger()
            mg.tick, mg.survivor, mg.absorbed, mg.count_before, mg.separation = tick, i, k, n, found[2]
            mg.relative_speed = float(np.sqrt(((V[k, :3] - V[i, :3]) ** 2).sum()))
            mg.mass_survivor, mg.mass_absorbed = float(mi), float(mj)
            mg.radius_survivor, mg.radius_absorbed = float(R[i]), float(R[k])
            mg.eval_index = len(res.touch_seq) - 1
            mg.mass_before = float(P[:n, 3].sum())
            mg.momentum_before = (P[:n, 3:4] * V[:n, :3]).sum(0)
            mg.momentum_scale = float((P[:n, 3] * np.sqrt((V[:n, :3] ** 2).sum(1))).sum())
            M = mi + mj
            if M == 0.0:
                xm, vm = 0.5 * (P[i, :3] + P[k, :3]), 0.5 * (V[i, :3] + V[k, :3])
            else:
                xm, vm = (mj * P[k, :3] + mi * P[i, :3]) / M, (mj * V[k, :3] + mi * V[i, :3]) / M
            absorbed_p, absorbed_v, absorbed_r = P[k].copy(), V[k].copy(), R[k]
            P[i, :3], V[i, :3] = f32(xm), f32(vm)
            P[i, 3] = f32(np.float64(M))
            R[i] = f32(np.float64(merged_radius(R[i], R[k])))
            mg.radius_after = float(R[i])
            if k != last:
                P[k], V[k], R[k] = P[last], V[last], R[last]
            P[last], V[last], R[last] = absorbed_p, absorbed_v, absorbed_r
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
        found = examine(xp, P[:n, :3], R[:n], eps, escape_radius, round_state)
        note(found, "step")
    res.pos, res.vel, res.radii, res.count = P, V, R, n
    res.steps, res.ticks, res.target, res.level_seq, res.tick_seq = len(level_seq), tick, target, level_seq, tick_seq
    res.reason, res.pair, res.separation, res.escaper = found[:4] if found[0] else (0, (0, 0), 0.0, 0)
    return res
