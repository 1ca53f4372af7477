"""fp64 numpy restatement of tracer fates in Hermite batches (nbody_batch_fate_set, include/nbody_batch_fate.h) on top of
hermite_adaptive_ref and hermite_stop_ref, whose request, level rule and reason bits it takes by import:

    columns    the first m bodies are massive and the only columns: acc_jerk sums j < m for every row
    collision  at every evaluation (each step's at the predicted positions, the initial one at the current positions) a pair
               (i, j), j < m, i != j, touches when d.d + eps^2 <= S^2 + eps^2, S = R_i + R_j (or S = R_c); i < m: the system
               stops with the closest touching massive pair; i >= m: tracer i has fate HIT, its target the touching massive
               body of smallest d.d + eps^2 (ties to the smallest index); two tracers are never compared
    escape     on the corrected positions after every step (the current ones at the initial evaluation) x.x > R_e^2: a
               massive body stops the system (the escaper of smallest index), a tracer has fate ESCAPED unless it also HIT
    removal    the step that finds a tracer is completed for it; it does not vote in that step's criterion (or in the
               first-step rule when found at the start) and is frozen from then on
    fates      fate, tick (after the step; 0 at the start), target, separation |d| and relative speed |e| at that evaluation
               (0 for an escape)

Without conditions this is hermite_adaptive_ref.evolve with zero-mass tracers, up to the order of the fp64 sums.  The
deciding quantities of every evaluation are kept: touch_seq[k][i], for a live tracer i the smallest
sqrt((d.d + eps^2) / (S^2 + eps^2)) over the massive bodies (below 1: it touches; inf for massive bodies, dead tracers and
without a collision condition), massive_touch_seq[k] the same over the massive pairs, and dist_seq[k][i] the distance from the
origin examined with it (k = 0: the initial evaluation, k >= 1: step k)."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_stop_ref as sref

COLLISION, ESCAPE = sref.COLLISION, sref.ESCAPE
ALIVE, HIT, ESCAPED = 0, 1, 2
ROW_CHUNK = 256


def acc_jerk(x, v, mass, m, eps, chunk=ROW_CHUNK):
    """hermite_ref.acc_jerk with the columns ending at m: (a, j), each (n, 3) fp64."""
    n = x.shape[0]
    a, j = np.zeros((n, 3)), np.zeros((n, 3))
    if m == 0:
        return a, j
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = x[None, :m, :] - x[lo:hi, None, :]
        e = v[None, :m, :] - v[lo:hi, None, :]
        r2 = np.einsum("ijk,ijk->ij", d, d) + eps * eps
        with np.errstate(divide="ignore"):
            inv2 = np.where(r2 > 0.0, 1.0 / np.where(r2 > 0.0, r2, 1.0), 0.0)
        s = mass[None, :m] * inv2 * np.sqrt(inv2)
        rv = np.einsum("ijk,ijk->ij", d, e)
        a[lo:hi] = np.einsum("ij,ijk->ik", s, d)
        j[lo:hi] = np.einsum("ij,ijk->ik", s, e) - np.einsum("ij,ijk->ik", 3.0 * rv * inv2 * s, d)
    return a, j


class Found:
    """One evaluation: reason, pair, separation, escaper (of the massive bodies, as hermite_stop_ref.examine gives them);
    hit, escaped (boolean per body, tracers only), target, sep, speed (per body); touch, massive_touch, dist."""


def examine(x_eval, v_eval, x_now, alive, m, R, eps, collide, escape_radius, round_state=False):
    n = x_eval.shape[0]
    f = Found()
    f.reason, f.pair, f.separation, f.escaper = 0, (-1, -1), 0.0, -1
    f.hit, f.escaped = np.zeros(n, bool), np.zeros(n, bool)
    f.target, f.sep, f.speed = np.full(n, -1), np.zeros(n), np.zeros(n)
    f.touch, f.massive_touch = np.full(n, np.inf), np.inf
    if collide and m > 0:
        d = x_eval[None, :m, :] - x_eval[:, None, :]
        d2 = (d * d).sum(2)
        S = R[:, None] + R[None, :m]
        if round_state:
            S = aref._f32(S)
        r2, thr2 = d2 + eps * eps, S * S + eps * eps
        formed = np.ones((n, m), bool)
        formed[np.arange(m), np.arange(m)] = False          # the self pair never counts
        formed &= alive[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(formed, np.sqrt(np.where(thr2 > 0.0, r2 / thr2, np.where(r2 > 0.0, np.inf, 0.0))), np.inf)
        ok = formed & (r2 <= thr2)
        upper = np.triu(np.ones((m, m), bool), 1)
        if m > 1:
            f.massive_touch = float(ratio[:m][upper].min())
        if (ok[:m] & upper).any():
            k = int(np.argmin(np.where(ok[:m] & upper, r2[:m], np.inf)))   # row-major: the first minimum
            i, j = divmod(k, m)
            f.reason |= COLLISION
            f.pair, f.separation = (i, j), float(np.sqrt(d2[i, j]))
        f.touch[m:] = ratio[m:].min(1)
        for i in np.nonzero(ok[m:].any(1))[0] + m:
            t = int(np.argmin(np.where(ok[i], r2[i], np.inf)))
            e = v_eval[t] - v_eval[i]
            f.hit[i], f.target[i], f.sep[i], f.speed[i] = True, t, np.sqrt(d2[i, t]), np.sqrt((e * e).sum())
    dist2 = (x_now * x_now).sum(1)
    f.dist = np.sqrt(dist2)
    if escape_radius > 0.0:
        out = alive & (dist2 > escape_radius * escape_radius)
        if out[:m].any():
            f.reason |= ESCAPE
            f.escaper = int(np.nonzero(out[:m])[0][0])
        f.escaped[m:] = out[m:] & ~f.hit[m:]
    return f


class Result:
    """pos, vel (n, 4) fp64; steps, ticks, target, level_seq, tick_seq, level, clamped; reason, pair, separation, escaper (0,
    (0, 0), 0.0, 0 when the system did not stop); per body fate, fate_tick, fate_target (-1 unless HIT), fate_separation,
    fate_speed, fate_step (the evaluation that found it: 0 the initial one, k step k; -1 alive); hit, escaped (totals);
    touch_seq, massive_touch_seq, dist_seq, eval_ticks."""


def evolve(pos, vel, massive, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, radii=None,
           collision_radius=0.0, escape_radius=0.0, round_state=False, max_steps=None):
    assert 0 <= levels <= aref.MAX_LEVELS
    assert radii is None or collision_radius == 0.0, "radii and collision_radius are both set"
    f32 = aref._f32 if round_state else (lambda u: u)
    pos = np.asarray(pos, np.float64)
    vel = np.asarray(vel, np.float64)
    n = pos.shape[0]
    m = min(int(massive), n)
    mass = pos[:, 3]
    x, v = pos[:, :3].copy(), vel[:, :3].copy()
    collide = radii is not None or collision_radius > 0.0
    # a shared R_c is the radius R_c / 2 of every body: the sum is R_c exactly
    R = np.asarray(radii, np.float64).reshape(-1)[:n] if radii is not None else np.full(n, 0.5 * float(collision_radius))
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    alive = np.ones(n, bool)
    res = Result()
    res.fate, res.fate_tick, res.fate_target = np.zeros(n, int), np.zeros(n, np.int64), np.full(n, -1)
    res.fate_separation, res.fate_speed, res.fate_step = np.zeros(n), np.zeros(n), np.full(n, -1)
    res.touch_seq, res.massive_touch_seq, res.dist_seq, res.eval_ticks = [], [], [], []

    def note(found, tick, step):
        res.touch_seq.append(found.touch)
        res.massive_touch_seq.append(found.massive_touch)
        res.dist_seq.append(found.dist)
        res.eval_ticks.append(tick)
        gone = found.hit | found.escaped
        res.fate[found.hit], res.fate[found.escaped] = HIT, ESCAPED
        res.fate_tick[gone], res.fate_step[gone] = tick, step
        res.fate_target[gone], res.fate_separation[gone], res.fate_speed[gone] = found.target[gone], found.sep[gone], found.speed[gone]
        return gone

    a, j = acc_jerk(x, v, mass, m, eps)
    a, j = f32(a), f32(j)
    found = examine(x, v, x, alive, m, R, eps, collide, escape_radius, round_state)
    alive &= ~note(found, 0, 0)
    num, den = aref.request_start(a, j, eta_start)
    level, c = aref.level_for((num[alive], den[alive]), dt_max, levels)
    clamped = int(c)
    tick, level_seq, tick_seq = 0, [], []
    while not found.reason and tick < target and (max_steps is None or len(level_seq) < max_steps):
        h = dt_max * 2.0 ** -level
        xp, vp = x.copy(), v.copy()                           # a dead row keeps its frozen state: it is nobody's column
        xp[alive] = f32(x + h * (v + h / 2 * (a + h / 3 * j)))[alive]
        vp[alive] = f32(v + h * (a + h / 2 * j))[alive]
        a1, j1 = acc_jerk(xp, vp, mass, m, eps)
        a1, j1 = f32(a1), f32(j1)
        v1 = f32(v + h / 2 * ((a + a1) + h / 6 * (j - j1)))
        x1 = f32(x + h / 2 * ((v + v1) + h / 6 * (a - a1)))
        num, den = aref.request(a, a1, j, j1, h, eta)
        x[alive], v[alive] = x1[alive], v1[alive]
        a, j = a1, j1
        level_seq.append(level)
        tick_seq.append(tick)
        tick += 1 << (levels - level)
        found = examine(xp, vp, x, alive, m, R, eps, collide, escape_radius, round_state)
        alive &= ~note(found, tick, len(level_seq))             # found in this step: corrected and written, no vote
        want, c = aref.level_for((num[alive], den[alive]), dt_max, levels)
        clamped += int(c)
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            level -= 1
    res.pos = pos.copy()
    res.pos[:, :3] = x
    res.vel = np.zeros((n, 4))
    res.vel[:, :vel.shape[1]] = vel
    res.vel[:, :3] = v
    res.steps, res.ticks, res.target, res.level_seq, res.tick_seq = len(level_seq), tick, target, level_seq, tick_seq
    res.level, res.clamped = level, clamped
    res.reason, res.pair, res.separation, res.escaper = ((found.reason, found.pair, found.separation, found.escaper)
                                                         if found.reason else (0, (0, 0), 0.0, 0))
    res.hit, res.escaped = int((res.fate == HIT).sum()), int((res.fate == ESCAPED).sum())
    return res
