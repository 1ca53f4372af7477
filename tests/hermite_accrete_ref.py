"""fp64 numpy restatement of accreting tracers in Hermite batches (nbody_batch_accrete_set, include/nbody_batch_accrete.h) on
top of hermite_fate_ref, whose acc_jerk and examine it imports, and hermite_merge_ref's tick_level:

    accretion  after an evaluation -- the initial one, a step's, a restart's -- that gave tracers the fate HIT and did not stop
               the system, those tracers are processed in ascending index, each on the state the one before left: a zero mass
               word gives nothing; otherwise the merger of hermite_merge_ref onto the fate's target t, the tracer absorbed:
               m = m_t + m_i, x and v the mass-weighted means (the arithmetic mean for m = 0), t keeps its slot and its w;
               with radii R_t becomes cbrt(R_t^3 + R_i^3); the tracer stays where the completed step left it and its mass
               word becomes 0; given[i] = m_i
    restart    when a mass moved: a and j afresh at the current state for every row -- not a step -- examined like the
               initial evaluation with the new radii; a tracer found there has the current tick and is accreted at once (a
               chain); a massive collision or escaper there stops the system; the level is min(levels, max(L*, L_tick)), L*
               from the first-step rule over the live rows, and L* > levels counts as clamped
    stopping   a step (or restart) that stops the system accretes nothing

With all tracer mass words zero this is hermite_fate_ref.evolve.  `round_state` rounds to fp32 what the kernel holds in fp32,
as there, and the merged mass, position, velocity and radius.  Kept per evaluation, restarts included: touch_seq,
massive_touch_seq, dist_seq (hermite_fate_ref's), eval_ticks and eval_kind ("start", "step", "restart"); per body fate_eval,
the index of the evaluation that found it (-1 alive); per restart restart_seq = (tick, L*, L_tick, L); per accretion an entry
of `events` = (tick, tracer, target, mass given, evaluation index).  `dead_votes=True` is the wrong scheme the tests compare
with: dead rows vote in the restarts' first-step rule.

The scene builders of tests/test_batch_accrete_gpu.py live here too, so that the CPU test runs the same inputs."""
import numpy as np

import hermite_adaptive_ref as aref
import hermite_fate_ref as fref
from hermite_merge_ref import tick_level
from test_batch_fate_gpu import scene as fate_scene, massive_stop_case as fate_massive_stop_case, start_case as fate_start_case

COLLISION, ESCAPE = fref.COLLISION, fref.ESCAPE
ALIVE, HIT, ESCAPED = fref.ALIVE, fref.HIT, fref.ESCAPED

F32 = lambda x: float(np.float32(x))  # noqa: E731
MARGIN = 1e-3
ETA = F32(0.01)
RE = 6.0                      # the escape radius of the scenes
RP = F32(0.02)                # the radius of a massive body that is hit
H = F32(1.0 / 128.0)          # the fixed step of the scenes
MT = 1e-5                     # the scale of the tracers' mass words


class Result:
    """hermite_fate_ref.Result's fields, and: radii ((n,) fp64, None without), given ((n,) fp64), accretions, events,
    restart_seq, eval_kind, fate_eval."""


def merge_onto(P, V, t, i, f32):
    """hermite_merge_ref's merger with t the survivor and i the absorbed body; i's state stays, its mass word becomes 0."""
    mt, mi = P[t, 3], P[i, 3]
    M = mt + mi
    if M == 0.0:
        xm, vm = 0.5 * (P[t, :3] + P[i, :3]), 0.5 * (V[t, :3] + V[i, :3])
    else:
        xm, vm = (mi * P[i, :3] + mt * P[t, :3]) / M, (mi * V[i, :3] + mt * V[t, :3]) / M
    P[t, :3], V[t, :3] = f32(xm), f32(vm)
    P[t, 3] = f32(np.float64(M))
    P[i, 3] = 0.0


def evolve(pos, vel, massive, n_intervals, dt_max, levels=12, eta=0.01, eta_start=0.01, eps=0.0, radii=None,
           collision_radius=0.0, escape_radius=0.0, round_state=False, max_steps=None, accrete=True, dead_votes=False):
    assert 0 <= levels <= aref.MAX_LEVELS
    assert radii is None or collision_radius == 0.0, "radii and collision_radius are both set"
    f32 = aref._f32 if round_state else (lambda u: u)
    P = np.array(pos, np.float64)
    V = np.zeros((P.shape[0], 4))
    V[:, :np.shape(vel)[1]] = vel
    n = P.shape[0]
    m = min(int(massive), n)
    x, v = P[:, :3], V[:, :3]                                   # views: the state lives in P and V
    collide = radii is not None or collision_radius > 0.0
    R = np.array(radii, np.float64).reshape(-1)[:n].copy() if radii is not None else np.full(n, 0.5 * float(collision_radius))
    dt_max = float(dt_max)
    target = int(n_intervals) << levels
    alive = np.ones(n, bool)
    res = Result()
    res.fate, res.fate_tick, res.fate_target = np.zeros(n, int), np.zeros(n, np.int64), np.full(n, -1)
    res.fate_separation, res.fate_speed, res.fate_step, res.fate_eval = np.zeros(n), np.zeros(n), np.full(n, -1), np.full(n, -1)
    res.touch_seq, res.massive_touch_seq, res.dist_seq, res.eval_ticks, res.eval_kind = [], [], [], [], []
    res.given, res.accretions, res.events, res.restart_seq = np.zeros(n), 0, [], []
    level_seq, tick_seq = [], []
    tick, clamped = 0, 0

    def note(found, kind):
        res.touch_seq.append(found.touch)
        res.massive_touch_seq.append(found.massive_touch)
        res.dist_seq.append(found.dist)
        res.eval_ticks.append(tick)
        res.eval_kind.append(kind)
        gone = found.hit | found.escaped
        res.fate[found.hit], res.fate[found.escaped] = HIT, ESCAPED
        res.fate_tick[gone], res.fate_step[gone], res.fate_eval[gone] = tick, len(level_seq), len(res.touch_seq) - 1
        res.fate_target[gone], res.fate_separation[gone], res.fate_speed[gone] = found.target[gone], found.sep[gone], found.speed[gone]
        return gone

    def evaluate_here(kind):
        """The initial evaluation or a restart: (a, j, found) at the current state; the rows found are dead afterwards."""
        a, j = fref.acc_jerk(x, v, P[:, 3], m, eps)
        a, j = f32(a), f32(j)
        found = fref.examine(x, v, x, alive, m, R, eps, collide, escape_radius, round_state)
        alive[note(found, kind)] = False
        return a, j, found

    def first_level(a, j, floor_level, voters):
        num, den = aref.request_start(a, j, eta_start)
        want, c = aref.level_for((num[voters], den[voters]), dt_max, levels)
        return min(levels, max(want, floor_level)), want, int(c)

    a, j, found = evaluate_here("start")
    level, _, c = first_level(a, j, 0, alive)
    clamped += c
    while True:
        while accrete and collide and found.hit.any() and not found.reason:
            moved = False
            for i in np.nonzero(found.hit)[0]:              # ascending
                mi = P[i, 3]
                if mi == 0.0:
                    continue
                t = int(found.target[i])
                merge_onto(P, V, t, i, f32)
                if radii is not None:
                    R[t] = f32(np.array(np.cbrt(R[t] ** 3 + R[i] ** 3)))
                res.given[i] = mi
                res.accretions += 1
                res.events.append((tick, int(i), t, float(mi), len(res.touch_seq) - 1))
                moved = True
            if not moved:
                break
            a, j, found = evaluate_here("restart")
            floor_level = tick_level(tick, levels)
            level, want, c = first_level(a, j, floor_level, np.ones(n, bool) if dead_votes else alive)
            clamped += c
            res.restart_seq.append((tick, want, floor_level, level))
        if found.reason or tick >= target or (max_steps is not None and len(level_seq) >= max_steps):
            break
        h = dt_max * 2.0 ** -level
        xp, vp = x.copy(), v.copy()                           # a dead row keeps its frozen state: it is nobody's column
        xp[alive] = f32(x + h * (v + h / 2 * (a + h / 3 * j)))[alive]
        vp[alive] = f32(v + h * (a + h / 2 * j))[alive]
        a1, j1 = fref.acc_jerk(xp, vp, P[:, 3], m, eps)
        a1, j1 = f32(a1), f32(j1)
        v1 = f32(v + h / 2 * ((a + a1) + h / 6 * (j - j1)))
        x1 = f32(x + h / 2 * ((v + v1) + h / 6 * (a - a1)))
        num, den = aref.request(a, a1, j, j1, h, eta)
        x[alive], v[alive] = x1[alive], v1[alive]
        a, j = a1, j1
        level_seq.append(level)
        tick_seq.append(tick)
        tick += 1 << (levels - level)
        found = fref.examine(xp, vp, x, alive, m, R, eps, collide, escape_radius, round_state)
        alive[note(found, "step")] = False                     # found in this step: corrected and written, no vote
        want, c = aref.level_for((num[alive], den[alive]), dt_max, levels)
        clamped += int(c)
        if want > level:
            level = want
        elif want < level and tick % (1 << (levels - level + 1)) == 0:
            level -= 1
    res.pos, res.vel = P, V
    res.radii = R if radii is not None else None
    res.steps, res.ticks, res.target, res.level_seq, res.tick_seq = len(level_seq), tick, target, level_seq, tick_seq
    res.level, res.clamped = level, clamped
    res.reason, res.pair, res.separation, res.escaper = ((found.reason, found.pair, found.separation, found.escaper)
                                                         if found.reason else (0, (0, 0), 0.0, 0))
    res.hit, res.escaped = int((res.fate == HIT).sum()), int((res.fate == ESCAPED).sum())
    return res


def reference(p, v, m, n_intervals, dt_max, levels, eps, radii=None, collision_radius=0.0, escape_radius=0.0, **kw):
    """The reference as the GPU tests call it: fp32 state, the tests' eta."""
    return evolve(p, v, m, n_intervals, dt_max, levels=levels, eta=ETA, eta_start=ETA, eps=eps, radii=radii,
                  collision_radius=F32(collision_radius), escape_radius=F32(escape_radius), round_state=True, **kw)


def decisions_are_clear(ref, collide=True, escape_radius=RE):
    """Every decision of the run -- each tracer's touch ratio and distance from the origin at every evaluation up to the one
    that decided its fate, restarts included, and the massive pairs' and bodies' at every evaluation -- lies at least MARGIN
    relative from 1 (from the radius)."""
    n = len(ref.fate)
    for k in range(len(ref.touch_seq)):
        judged = (ref.fate_eval < 0) | (k <= ref.fate_eval)
        if collide:
            t = ref.touch_seq[k][judged]
            if not (np.abs(t[np.isfinite(t)] - 1.0) > MARGIN).all() or not abs(ref.massive_touch_seq[k] - 1.0) > MARGIN:
                return False
        if escape_radius > 0.0:
            d = ref.dist_seq[k][judged]
            d = d[~((ref.fate[judged] == HIT) & (ref.fate_eval[judged] == k))]   # a tracer that hit is not asked its distance
            if not (np.abs(d / escape_radius - 1.0) > MARGIN).all():
                return False
    assert n == len(judged)
    return True


# ---- the scenes of tests/test_batch_accrete_gpu.py ------------------------------------------------------------------------
def tracer_masses(n, m, seed):
    """Mass words around MT for every tracer, with mantissas that are not round."""
    rng = np.random.default_rng(1000 + seed)
    return (MT * rng.uniform(0.5, 1.5, n - m)).astype(np.float32)


def scene(n, m, seed=1, hit_steps=(1, 4, 2), escape_steps=(1, 3), zero=False):
    """test_batch_fate_gpu.scene -- a star, m - 1 planets of mass 1e-3 with radius RP, quiet tracers, hitters aimed at the
    last massive body and escapers, planted in the first tracer rows and the last rows alternately -- with the tracers' mass
    words around MT (all zero with `zero`).  hit_steps (1, 4, 2): the hits come in ascending row order, rows m, m + 1, n - 1.
    (pos, vel, radii, plan)."""
    p, v, R, plan = fate_scene(n, m, seed=seed, hit_steps=hit_steps, escape_steps=escape_steps)
    p[m:, 3] = 0.0 if zero else tracer_masses(n, m, seed)
    return p, v, R, plan


def fixed_step_case(cap, n, m, zero=False):
    p, v, R, plan = scene(n, m, zero=zero)
    return p, v, R, plan, dict(radii=R[None], escape_radius=RE)


def pair_case():
    """Rows 3 and 699 of 700 (waves 0 and 2 of the four) reach planet 2 in the evaluation of step 2; their masses are such that
    (M + a) + b and (M + b) + a differ in fp32."""
    n, m = 700, 3
    p, v, R, plan = scene(n, m, seed=2, hit_steps=(2, 2), escape_steps=())
    rows = sorted(plan)
    assert rows == [3, 699]
    # found by trying random pairs around MT: one in a few hundred depends on the order; the CPU test asserts that this one does
    a, b = np.float32(float.fromhex("0x1.f5ce8p-17")), np.float32(float.fromhex("0x1.b1bedp-17"))
    p[3, 3], p[699, 3] = a, b
    return p, v, R, n, m, rows


def adaptive_case():
    """A star, two planets and 45 tracers, levels = 8: three hitters aimed at planet 2 (steps 2, 5, 9 of the fixed-step
    plan), one escaper, and row 10, massless, which lies 0.008 from the star -- inside its radius -- with speed 2: it is
    removed by the initial evaluation, gives nothing, and from then on would ask every restart for the finest level."""
    n, m = 48, 3
    p, v, R, plan = scene(n, m, seed=5, hit_steps=(2, 5, 9), escape_steps=(18,))
    p[10] = [0.0, 0.008, 0.0, 0.0]
    v[10, :3] = [2.0, 0.0, 0.0]
    return p, v, R, n, m


def chain_case(shared=False):
    """m = 3, radii: tracer A (row 3, radius 0.015) reaches planet 2 in the evaluation of step 1 and is accreted; planet 2
    grows from RP to cbrt(RP^3 + RA^3) = 0.02249.  Tracer B (row 49, radius 0.005), which rides with the planet at 0.0262, lay
    outside RP + RB = 0.025 and lies inside 0.02749: the restart finds it, at the same tick, and the planet grows again.
    shared: the same with one collision radius 0.02 for all, crossed by A in step 1: nothing grows, B lives."""
    n, m = 50, 3
    p, v, R, _ = scene(n, m, seed=4, hit_steps=(), escape_steps=())
    t, A, B = 2, 3, 49
    RA, RB = 0.015, 0.005
    h = float(H)
    u = np.array([0.6, 0.0, 0.8])
    w = np.array([0.0, 1.0, 0.0])
    reach = float(RP) if shared else float(RP) + RA
    p[A, :3] = p[t, :3] + u * (reach + 1.28 * h * 0.5)
    v[A, :3] = v[t, :3] - 1.28 * u
    p[B, :3] = p[t, :3] + w * 0.0262
    v[B, :3] = v[t, :3]
    R[A], R[B] = RA, RB
    return p, v, R, n, m, (t, A, B)


def start_case():
    """test_batch_fate_gpu.start_case -- tracer 20 at 0.004 from planet 1, inside its radius: so close that its |a| / |j| alone
    would refine the first step; tracer 21 outside RE; tracer 22 outside RE and within planet 2's radius -- with mass words."""
    p, v, R, n, m = fate_start_case()
    p[m:, 3] = tracer_masses(n, m, 9)
    return p, v, R, n, m


def massive_stop_case():
    """test_batch_fate_gpu.massive_stop_case -- planets 1 and 2 touch in step 3, tracer 12 hits planet 1 in that same step --
    with mass words; tracer 13, which hits in step 1, carries none, so that the massive bodies' run is the one they make
    alone."""
    p, v, R, n, m = fate_massive_stop_case()
    p[m:, 3] = tracer_masses(n, m, 3)
    p[13, 3] = 0.0
    return p, v, R, n, m
