"""GPU: per-body collision radii for Hermite batches (BatchedSystem.set_radii / radii, include/nbody_batch_radii.h) against
the uniform rule on the kernels that were there before, and against the fp64 reference (hermite_radii_ref): radii R_c / 2
everywhere are the uniform rule bit for bit, per-pair thresholds at the initial evaluation across waves and row groups, a
merged body that grows and swallows a neighbour at the same tick, a Kepler pair and a triple that follow the reference, quiet
radii that change no bit, the batch's invariances with the radii among the results, and the life cycle of the setting.

The builders of the inputs are used by test_batch_radii_cpu.py as well, which asserts on the CPU that they tell the per-pair
rule from the uniform one.  Every comparison with the reference first asserts that each deciding |d| / S of the reference is
more than 1e-3 relative away from 1, so that fp32 rounding cannot move a decision."""
import numpy as np
import pytest

import hermite_radii_ref as rref
import hermite_ref
from hermite_ref import rel_state_error
from test_batch_hermite_gpu import MIXED_COUNTS, mixed_batch

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
MARGIN = 1e-3
ETA = dict(eta=F32(0.01), eta_start=F32(0.01))


class Run:
    """What a fresh Hermite batch gave: p, v, res (EvolveResult), st (StopResult), mg (MergeResult), counts, radii, err."""


def evolve(P, V, counts, n_intervals, dt_max, eps, radii=None, collision_radius=0.0, escape_radius=0.0, action="merge",
           log_capacity=8, max_bodies=None, launch_steps=None, split=None, **kw):
    """hermite batch run; radii: (B, n) or None (then collision_radius is the uniform rule's, on the kernels before)."""
    import n_body_problem_amd as nb
    B = P.shape[0]
    max_bodies = max_bodies or P.shape[1]
    Pf = np.zeros((B, max_bodies, 4), np.float32)
    Vf = np.zeros((B, max_bodies, 4), np.float32)
    m = min(max_bodies, P.shape[1])
    Pf[:, :m], Vf[:, :m] = P[:, :m], V[:, :m]
    r = Run()
    with nb.BatchedSystem(B, max_bodies, counts=counts, integrator="hermite") as b:
        b.set_state(Pf, Vf)
        b.set_stop_conditions(collision_radius, escape_radius)
        b.set_collision_action(action, log_capacity)
        if radii is not None:
            b.set_radii(np.asarray(radii, np.float32)[:, :max_bodies])
        if launch_steps:
            b.set_evolve_launch_steps(launch_steps)
        r.err = None
        try:
            if split:
                first = b.evolve(split, dt_max, softening=eps, **kw)
                r.res = b.evolve(n_intervals - split, dt_max, softening=eps, **kw)
                r.res.steps = r.res.steps + first.steps
            else:
                r.res = b.evolve(n_intervals, dt_max, softening=eps, **kw)
        except nb.NBodyError as e:
            r.err, r.res = e, b.evolve_stats()
        r.p, r.v = b.download()
        r.st, r.mg, r.counts = b.stops(), b.mergers(), b.counts
        r.radii = b.radii() if radii is not None else None
    return r


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_same_run(a, b):
    """States, counts, stops, mergers and ticks bit for bit."""
    assert a.err is None and b.err is None
    assert same_bits(a.p, b.p) and same_bits(a.v, b.v) and a.counts.tolist() == b.counts.tolist()
    for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
        assert np.array_equal(getattr(a.res, name), getattr(b.res, name)), name
    assert np.array_equal(a.st.reason, b.st.reason) and np.array_equal(a.st.ticks, b.st.ticks) and np.array_equal(a.st.pair, b.st.pair)
    assert same_bits(a.st.separation, b.st.separation) and np.array_equal(a.st.escaper, b.st.escaper)
    assert np.array_equal(a.mg.count, b.mg.count) and a.mg.events.tobytes() == b.mg.events.tobytes()


def decided_clearly(ref):
    return all(abs(t - 1.0) > MARGIN for t in ref.touch_seq)


def check_event(ev, mg):
    assert (int(ev["tick"]), int(ev["survivor"]), int(ev["absorbed"]), int(ev["count_before"])) == \
        (mg.tick, mg.survivor, mg.absorbed, mg.count_before)
    for name in ("separation", "relative_speed", "mass_survivor", "mass_absorbed"):
        want = getattr(mg, name)
        assert abs(float(ev[name]) - want) <= 1e-5 * abs(want), (name, ev[name], want)


def ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---- 1. radii R_c / 2 everywhere are the uniform rule -----------------------------------------------------------------------

def planted_uniform_case():
    """Plummer spheres of 65 (x2), 257 and 1000 bodies.  R_c is a third of the smallest separation in any of them; then body
    n - 3 of systems 0, 2 and 3 is re-placed R_c / 2 from body 5 (inside), and body 64 of system 1 at 1.5 R_c from body 5
    (outside: nothing collides there)."""
    import n_body_problem_amd as nb
    import hermite_merge_ref as mref
    counts = [65, 65, 257, 1000]
    P = np.zeros((4, 1024, 4), np.float32)
    V = np.zeros((4, 1024, 4), np.float32)
    dmin = np.inf
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=810 + s)
        V[s, :n, 3] = np.arange(n)
        dmin = min(dmin, mref.closest_pair(P[s, :n, :3].astype(np.float64), 0.0)[2])
    rc = F32(dmin / 3.0)
    off = np.array([0.3, 0.4, 0.0], np.float32) * np.float32(rc)                    # |.| = rc / 2
    for s in (0, 2, 3):
        P[s, counts[s] - 3, :3] = P[s, 5, :3] + off
    P[1, 64, :3] = P[1, 5, :3] + 3.0 * off
    return P, V, counts, rc


@pytest.mark.parametrize("eps", [1e-2, 0.0])
@pytest.mark.parametrize("action", ["stop", "merge"])
def test_radii_of_half_the_collision_radius_are_the_uniform_rule_on_planted_pairs_bit_for_bit(action, eps):
    P, V, counts, rc = planted_uniform_case()
    half = np.float32(rc) * np.float32(0.5)
    assert float(half + half) == rc                                                 # S == R_c exactly
    uniform = evolve(P, V, counts, 2, F32(1e-3), eps, collision_radius=rc, action=action, levels=4, **ETA)
    radii = evolve(P, V, counts, 2, F32(1e-3), eps, radii=np.full((4, 1024), half, np.float32), action=action, levels=4, **ETA)
    print(action, eps, "stops", uniform.st, "mergers", uniform.mg.count, "counts", uniform.counts)
    assert_same_run(radii, uniform)
    if action == "stop":
        assert uniform.st.reason.tolist() == [1, 0, 1, 1] and uniform.st.pair.tolist() == [[5, 62], [0, 0], [5, 254], [5, 997]]
        assert np.array_equal(radii.radii, np.full((4, 1024), half, np.float32))
    else:
        assert uniform.mg.count.tolist() == [1, 0, 1, 1] and uniform.counts.tolist() == [64, 65, 256, 999]
        grown = np.cbrt(2.0 * float(half) ** 3)
        for s, n in enumerate(counts):
            want = np.full(1024, half, np.float32)
            if s != 1:
                assert ulps(radii.radii[s, 5], grown) <= 1, (radii.radii[s, 5], grown)
                want[5] = radii.radii[s, 5]
            assert np.array_equal(radii.radii[s], want)                             # the absorbed body's R_c / 2 at slot n - 1


@pytest.mark.parametrize("eps", [1e-2, 0.0])
@pytest.mark.parametrize("action", ["stop", "merge"])
def test_radii_of_half_the_collision_radius_are_the_uniform_rule_on_kepler_pairs_over_a_period(action, eps):
    pos, vel, period = hermite_ref.kepler(e=0.9)
    rcs = [0.3, 0.15, 0.05]                                                         # the pericentre is at 0.1: the last never collides
    P, V = pos[None].astype(np.float32), vel[None].astype(np.float32)
    dt_max = F32(period / 64)
    got = []
    for rc in rcs:                                                                  # one batch per radius: the uniform rule has one
        half = np.float32(rc) * np.float32(0.5)
        assert float(half + half) == F32(rc)
        uniform = evolve(P, V, [2], 64, dt_max, eps, collision_radius=rc, action=action, **ETA)
        radii = evolve(P, V, [2], 64, dt_max, eps, radii=np.full((1, 2), half, np.float32), action=action, **ETA)
        assert_same_run(radii, uniform)
        got.append((int(uniform.st.reason[0]), int(uniform.mg.count[0]), int(uniform.res.ticks[0])))
        if action == "merge" and uniform.mg.count[0]:
            assert ulps(radii.radii[0, 0], np.cbrt(2.0 * float(half) ** 3)) <= 1 and radii.radii[0, 1] == half
    print(action, eps, got)
    assert [g[0] + g[1] for g in got] == [1, 1, 0] and got[2][2] == 64 << 12
    assert action == "merge" or got[0][2] < got[1][2] < 64 << 12                    # the wider radius stops earlier


# ---- 2. per-pair thresholds at the initial evaluation ----------------------------------------------------------------------

#: (bodies, capacity, wide pair, close pair): capacity 128 has 64 threads and two rows per lane, 512 and 1024 have 128 and 256
#: threads and four rows per lane in two groups.  The wide pairs sit in different waves ((63, 64): lanes 63 and 0), different
#: row groups of one lane ((0, 256) at 128 threads: rows 0 and 2) and both ((257, 770) = (T + 1, 3 T + 2) at T = 256)
PER_PAIR = [(65, 128, (63, 64), (5, 40)), (257, 512, (0, 256), (63, 64)), (1000, 1024, (257, 770), (0, 999))]
WIDE_D, WIDE_R, CLOSE_D, CLOSE_R = 0.3, 0.2, 0.1, 0.01


def per_pair_case(n, wide, close):
    """n bodies on a jittered unit lattice (nothing within 0.7 of anything), every radius 0.01; then the wide pair 0.3 apart
    with radii 0.2 (S = 0.4 > d) and the close pair 0.1 apart with radii 0.01 (S = 0.02 < d)."""
    rng = np.random.default_rng(n)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    P = np.zeros((n, 4), np.float32)
    V = np.zeros((n, 4), np.float32)
    P[:, :3] = grid - grid.mean(0) + rng.uniform(-0.1, 0.1, (n, 3))
    P[:, 3] = 1.0 / n
    V[:, :3] = rng.normal(0.0, 0.01, (n, 3))
    V[:, 3] = np.arange(n)
    R = np.full(n, CLOSE_R, np.float32)
    P[wide[1], :3] = P[wide[0], :3] + np.float32([0.0, 0.6, 0.8]) * np.float32(WIDE_D)
    P[close[1], :3] = P[close[0], :3] + np.float32([0.8, 0.0, 0.6]) * np.float32(CLOSE_D)
    R[list(wide)] = WIDE_R
    return P, V, R


@pytest.mark.parametrize("n,cap,wide,close", PER_PAIR)
def test_a_wide_pair_of_large_bodies_collides_and_a_closer_pair_of_small_ones_does_not(n, cap, wide, close):
    P, V, R = per_pair_case(n, wide, close)
    eps, dt_max = 1e-2, F32(1e-3)
    stopped = rref.evolve(P, V, 1, dt_max, levels=4, eps=eps, radii=R, merge=False, **ETA)
    merged = rref.evolve(P, V, 1, dt_max, levels=4, eps=eps, radii=R, **ETA)
    assert stopped.pair == wide and stopped.ticks == 0 and decided_clearly(stopped)
    assert [(m.tick, m.survivor, m.absorbed) for m in merged.mergers] == [(0,) + wide] and decided_clearly(merged)
    assert merged.ticks == 1 << 4 and merged.count == n - 1
    s = evolve(P[None], V[None], [n], 1, dt_max, eps, radii=R[None], action="stop", max_bodies=cap, levels=4, **ETA)
    m = evolve(P[None], V[None], [n], 1, dt_max, eps, radii=R[None], action="merge", max_bodies=cap, levels=4, **ETA)
    print(n, cap, "stop", s.st, "merger", m.mg.events[0, 0])
    assert s.err is None and s.st.reason[0] == 1 and tuple(s.st.pair[0]) == wide and s.st.ticks[0] == 0 and s.res.steps[0] == 0
    assert abs(float(s.st.separation[0]) - stopped.separation) <= 1e-5 * stopped.separation
    assert same_bits(s.p[0, :n], P) and same_bits(s.v[0, :n], V) and np.array_equal(s.radii[0, :n], R) and s.counts.tolist() == [n]
    assert m.err is None and m.mg.count.tolist() == [1] and m.counts.tolist() == [n - 1] and not m.st.stopped.any()
    check_event(m.mg.events[0, 0], merged.mergers[0])
    assert m.res.ticks[0] == merged.ticks
    assert np.abs(m.radii[0, :n] - merged.radii).max() <= 1e-6 * WIDE_R and m.radii[0, n - 1] == np.float32(WIDE_R)
    assert rel_state_error(m.p[0, :n], merged.pos) <= 1e-5 and rel_state_error(m.v[0, :n], merged.vel) <= 1e-5
    assert np.array_equal(m.v[0, :n, 3], merged.vel[:, 3].astype(np.float32))       # every body where the reference has it
    assert not m.p[0, n:].any() and not m.v[0, n:].any() and not m.radii[0, n:].any()   # slots beyond the first count


def one_sided_case(inside):
    """Three bodies far apart but for bodies 0 and 2, 0.3 apart: R_0 just above (inside) or below 0.3, R_2 = 0, R_1 = 0.05."""
    P = np.float32([[0.0, 0.0, 0.0, 0.5], [4.0, 1.0, 0.0, 0.25], [0.18, 0.24, 0.0, 0.25]])
    V = np.zeros((3, 4), np.float32)
    R = np.float32([0.3 * (1.0 + (2e-3 if inside else -2e-3)), 0.05, 0.0])
    return P, V, R


@pytest.mark.parametrize("eps", [1e-2, 0.0])
def test_a_large_body_and_a_point_collide_exactly_when_the_point_is_within_its_radius_and_a_coincident_pair_always(eps):
    P = np.zeros((3, 3, 4), np.float32)
    V = np.zeros((3, 3, 4), np.float32)
    R = np.zeros((3, 3), np.float32)
    P[0], V[0], R[0] = one_sided_case(True)
    P[1], V[1], R[1] = one_sided_case(False)
    P[2] = np.float32([[1.0, 2.0, 3.0, 0.5], [1.0, 2.0, 3.0, 0.25], [-2.0, 0.0, 0.0, 0.25]])   # coincident, every radius 0
    for s in range(3):
        ref = rref.evolve(P[s], V[s], 1, F32(1e-3), levels=4, eps=eps, radii=R[s], merge=False, **ETA)
        assert decided_clearly(ref) and (ref.reason, ref.pair) == [(1, (0, 2)), (0, (0, 0)), (1, (0, 1))][s]
    r = evolve(P, V, [3, 3, 3], 1, F32(1e-3), eps, radii=R, action="stop", levels=4, **ETA)
    print(eps, r.st)
    assert r.err is None and r.st.reason.tolist() == [1, 0, 1] and r.st.pair.tolist() == [[0, 2], [0, 0], [0, 1]]
    assert r.st.ticks.tolist() == [0, 0, 0] and r.res.ticks.tolist() == [0, 1 << 4, 0] and r.st.separation[2] == 0.0
    assert abs(float(r.st.separation[0]) - 0.3) <= 1e-6
    m = evolve(P, V, [3, 3, 3], 1, F32(1e-3), eps, radii=R, action="merge", levels=4, **ETA)
    assert m.err is None and m.mg.count.tolist() == [1, 0, 1] and m.counts.tolist() == [2, 3, 2] and not m.st.stopped.any()
    assert m.radii[2].tolist() == [0.0, 0.0, 0.0] and m.p[2, 0, 3] == 0.75


# ---- 3. growth ------------------------------------------------------------------------------------------------------------------

def growth_case():
    """A and B touch (0.52 apart, radii 0.3).  C (radius 0.25) is 0.663 from each, beyond their reach of 0.55, and 0.61 from
    their centre of mass: within the merged body's reach of cbrt(2 x 0.027) + 0.25 = 0.628."""
    P = np.float32([[0.0, 0.0, 0.0, 0.5], [0.52, 0.0, 0.0, 0.5], [0.26, 0.61, 0.0, 0.25]])
    V = np.zeros((3, 4), np.float32)
    V[:, :3] = [[0.0, 0.05, 0.0], [0.0, -0.05, 0.0], [0.02, 0.0, 0.0]]
    V[:, 3] = [20.0, 21.0, 22.0]
    R = np.float32([0.3, 0.3, 0.25])
    return P, V, R


@pytest.mark.parametrize("eps", [1e-2, 0.0])
def test_a_merged_body_grows_and_swallows_a_neighbour_at_the_same_tick(eps):
    P, V, R = growth_case()
    ref = rref.evolve(P, V, 2, F32(1e-2), levels=6, eps=eps, radii=R, round_state=True, **ETA)
    assert [(m.tick, m.survivor, m.absorbed, m.count_before) for m in ref.mergers] == [(0, 0, 1, 3), (0, 0, 1, 2)]
    assert ref.count == 1 and ref.ticks == 2 << 6 and decided_clearly(ref) and ref.eval_kind[:3] == ["start", "restart", "restart"]
    r = evolve(P[None], V[None], [3], 2, F32(1e-2), eps, radii=R[None], levels=6, **ETA)
    print(eps, r.mg, r.radii, ref.radii)
    assert r.err is None and r.mg.count.tolist() == [2] and r.counts.tolist() == [1] and not r.st.stopped.any()
    assert r.res.ticks[0] == ref.ticks and r.res.steps[0] == ref.steps
    check_event(r.mg.events[0, 0], ref.mergers[0])
    check_event(r.mg.events[0, 1], ref.mergers[1])
    assert ulps(r.radii[0, 0], ref.radii[0]) <= 1 and r.radii[0, 1:].tolist() == [0.25, 0.30000001192092896]
    assert r.v[0, :, 3].tolist() == ref.vel[:, 3].tolist() == [20.0, 22.0, 21.0] and r.p[0, 0, 3] == 1.25
    assert rel_state_error(r.p[0], ref.pos) <= 1e-5 and rel_state_error(r.v[0], ref.vel) <= 1e-5


# ---- 4. dynamics ------------------------------------------------------------------------------------------------------------

def kepler_radii_case():
    """A Kepler pair (e = 0.9, masses 0.75 and 0.25) with radii 0.2 and 0.1: it merges where the separation falls to 0.3."""
    pos, vel, period = hermite_ref.kepler(e=0.9, masses=(0.75, 0.25))
    P, V = pos.astype(np.float32), vel.astype(np.float32)
    V[:, 3] = [3.0, 4.0]
    return P, V, np.float32([0.2, 0.1]), F32(period / 64)


@pytest.mark.parametrize("eps", [1e-2, 0.0])
def test_a_kepler_pair_of_unequal_masses_and_radii_merges_at_the_reference_tick(eps):
    P, V, R, dt_max = kepler_radii_case()
    ref = rref.evolve(P, V, 64, dt_max, levels=12, eps=eps, radii=R, round_state=True, **ETA)
    assert len(ref.mergers) == 1 and ref.count == 1 and ref.ticks == 64 << 12 and 0 < ref.mergers[0].tick < 64 << 12
    assert decided_clearly(ref)
    r = evolve(P[None], V[None], [2], 64, dt_max, eps, radii=R[None], **ETA)
    print(eps, "steps", r.res.steps[0], ref.steps, "merger", r.mg.events[0, 0], "reference tick", ref.mergers[0].tick, r.radii)
    assert r.err is None and r.mg.count.tolist() == [1] and r.counts.tolist() == [1] and r.st.reason[0] == 0
    assert r.res.steps[0] == ref.steps and r.res.ticks[0] == 64 << 12
    check_event(r.mg.events[0, 0], ref.mergers[0])
    assert ulps(r.radii[0, 0], ref.radii[0]) <= 1 and r.radii[0, 1] == np.float32(0.1)
    assert rel_state_error(r.p[0], ref.pos) <= 1e-5 and rel_state_error(r.v[0], ref.vel) <= 1e-5
    assert r.p[0, :, 3].tolist() == [1.0, 0.25] and r.v[0, :, 3].tolist() == [3.0, 4.0]


def triple_radii_case():
    """test_batch_merge_gpu's triple -- a Kepler pair (e = 0.9) and a bound third body on a wide circular orbit -- with radii
    0.2, 0.1 and 0.05."""
    pos, vel, period = hermite_ref.kepler(e=0.9)
    P = np.zeros((3, 4), np.float32)
    V = np.zeros((3, 4), np.float32)
    P[:2], V[:2] = pos, vel
    P[2] = [0.0, 5.0, 0.0, 0.25]
    V[2, 0] = -np.sqrt(1.25 / 5.0)
    V[:, 3] = [7.0, 8.0, 9.0]
    return P, V, np.float32([0.2, 0.1, 0.05]), F32(period / 64)


@pytest.mark.parametrize("eps", [1e-2, 0.0])
def test_three_bodies_with_radii_merge_inside_an_interval_and_follow_the_reference_to_the_end_time(eps):
    P, V, R, dt_max = triple_radii_case()
    ref = rref.evolve(P, V, 64, dt_max, levels=12, eps=eps, radii=R, round_state=True, **ETA)
    assert len(ref.mergers) == 1 and ref.count == 2 and ref.reason == 0 and ref.ticks == 64 << 12 and decided_clearly(ref)
    assert ref.mergers[0].tick % (1 << 12) != 0
    r = evolve(P[None], V[None], [3], 64, dt_max, eps, radii=R[None], **ETA)
    print(eps, "steps", r.res.steps[0], ref.steps, "merger", r.mg.events[0, 0], r.radii)
    assert r.err is None and r.counts.tolist() == [2] and r.mg.count.tolist() == [1] and r.st.reason[0] == 0
    check_event(r.mg.events[0, 0], ref.mergers[0])
    assert r.res.steps[0] == ref.steps and r.res.ticks[0] == ref.ticks
    assert rel_state_error(r.p[0], ref.pos) <= 1e-5 and rel_state_error(r.v[0], ref.vel) <= 1e-5
    assert r.v[0, :, 3].tolist() == [7.0, 9.0, 8.0]                                 # the third body moved into slot 1
    assert ulps(r.radii[0, 0], ref.radii[0]) <= 1 and r.radii[0, 1:].tolist() == [np.float32(0.05), np.float32(0.1)]


# ---- 5. quiet radii ----------------------------------------------------------------------------------------------------------

def test_radii_that_never_trigger_change_no_bit():
    P, V = mixed_batch(MIXED_COUNTS, 4096, seed0=300)
    quiet_radii = np.full((len(MIXED_COUNTS), 4096), 1e-6, np.float32)
    for eps in (1e-2, 0.0):
        plain = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, action="stop", levels=6)
        for action in ("stop", "merge"):
            quiet = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, radii=quiet_radii, action=action, levels=6)
            assert plain.err is None and quiet.err is None
            assert same_bits(quiet.p, plain.p) and same_bits(quiet.v, plain.v)
            for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
                assert np.array_equal(getattr(quiet.res, name), getattr(plain.res, name)), name
            assert quiet.counts.tolist() == MIXED_COUNTS and not quiet.mg.count.any() and not quiet.st.stopped.any()
            assert np.array_equal(quiet.radii, quiet_radii)


# ---- 6. independence -----------------------------------------------------------------------------------------------------------

def head_on_radii(n=65):
    """test_batch_merge_gpu's head_on -- a Plummer sphere whose bodies 5 and 61 approach head-on at unit speed from 0.05
    apart -- with radii 0.012 and 0.008 for the two and 0.001 for the rest."""
    import n_body_problem_amd as nb
    pos, vel = nb.plummer(n, seed=41)
    pos[61, :3] = pos[5, :3] + np.float32([0.05, 0.0, 0.0])
    vel[61, :3] = vel[5, :3] + np.float32([-1.0, 0.0, 0.0])
    vel[:, 3] = np.arange(n)
    R = np.full(n, 0.001, np.float32)
    R[5], R[61] = 0.012, 0.008
    return pos, vel, R


def test_states_counts_radii_and_logs_do_not_depend_on_slot_batch_capacity_neighbours_launch_budget_or_a_split_of_the_call():
    n, eps, dt_max = 65, 1e-3, F32(1e-3)
    pos, vel, R = head_on_radii(n)
    ref = rref.evolve(pos, vel, 100, dt_max, levels=6, eps=eps, radii=R, round_state=True, **ETA)
    assert len(ref.mergers) == 1 and (ref.mergers[0].survivor, ref.mergers[0].absorbed) == (5, 61) and ref.steps > 10
    assert 0 < ref.mergers[0].tick < 60 << 6 and decided_clearly(ref)
    got = []
    for B, cap, slot, budget, other, split in ((1, 128, 0, 128, None, None), (5, 4096, 4, 1, 200, None), (5, 128, 0, 128, 2, None),
                                                (1, 4096, 0, 1, None, 60), (5, 128, 4, 1, 100, 60)):
        counts = [other or n] * B
        counts[slot] = n
        P, V = mixed_batch(counts, cap, seed0=50 + B)
        radii = np.full((B, cap), 0.001, np.float32)
        if other == 2:
            for s in range(B):
                if s != slot:
                    P[s, :2], V[s, :2] = hermite_ref.kepler(e=0.99)[:2]
                    radii[s, :2] = 0.02                                              # these neighbours merge too
        P[slot, :n], V[slot, :n], radii[slot, :n] = pos, vel, R
        r = evolve(P, V, counts, 100, dt_max, eps, radii=radii, max_bodies=cap, launch_steps=budget, split=split, levels=6, **ETA)
        assert r.err is None
        got.append((r.p[slot, :n].copy(), r.v[slot, :n].copy(), r.radii[slot, :n].copy(), int(r.res.steps[slot]),
                    int(r.res.ticks[slot]) if not split else 100 << 6, int(r.counts[slot]), int(r.mg.count[slot]),
                    r.mg.events[slot].tobytes(), int(r.st.reason[slot])))
    ev = np.frombuffer(got[0][7], dtype=r.mg.events.dtype)
    print("steps", got[0][3], "reference", ref.steps, "merger", ev[0], "radius", got[0][2][5])
    assert got[0][3] == ref.steps and got[0][4] == ref.ticks and got[0][5] == n - 1 and got[0][6] == 1 and got[0][8] == 0
    check_event(ev[0], ref.mergers[0])
    assert rel_state_error(got[0][0], ref.pos) <= 1e-5 and rel_state_error(got[0][1], ref.vel) <= 1e-5
    assert ulps(got[0][2][5], ref.radii[5]) <= 1 and got[0][2][n - 1] == np.float32(0.008) and got[0][2][61] == np.float32(0.001)
    for g in got[1:]:
        assert g[3:] == got[0][3:]
        assert same_bits(g[0], got[0][0]) and same_bits(g[1], got[0][1]) and same_bits(g[2], got[0][2])


# ---- 7. life cycle -------------------------------------------------------------------------------------------------------------

def test_the_life_cycle_of_the_radii():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, R, dt_max = kepler_radii_case()
    eps, rc = 1e-2, 0.3
    Pf = np.full((2, 4, 4), 7.0, np.float32)                                        # slots beyond the counts hold 7
    Vf = np.full((2, 4, 4), 7.0, np.float32)
    Pf[:, :2], Vf[:, :2] = P, V
    Rf = np.full((2, 4), 0.5, np.float32)
    Rf[:, :2] = R
    uniform = evolve(Pf, Vf, [2, 2], 64, dt_max, eps, collision_radius=rc, action="stop", **ETA)
    assert uniform.st.reason.tolist() == [1, 1]
    with nb.BatchedSystem(2, 4, counts=[2, 2], integrator="hermite") as b:
        with pytest.raises(nb.NBodyError) as err:
            b.radii()
        assert err.value.status == _lib.NBODY_ERR_STATE and "no radii" in str(err.value)
        for bad in (-1.0, np.nan, np.inf):
            wrong = Rf.copy()
            wrong[1, 1] = bad
            with pytest.raises(nb.NBodyError) as err:
                b.set_radii(wrong)
            assert err.value.status == _lib.NBODY_ERR_INVALID and "system 1, slot 1" in str(err.value)
            wrong[1, 1], wrong[1, 2] = R[1], bad                                    # beyond the count: copied, never examined
            b.set_radii(wrong)
            assert np.array_equal(b.radii(), wrong, equal_nan=True)
        with pytest.raises(ValueError):
            b.set_radii(np.zeros((3, 4), np.float32))
        with pytest.raises(ValueError):
            b.set_radii(np.zeros((2, 5), np.float32))
        # radii and a collision radius together are refused by evolve; so are radii with another integrator
        b.set_state(Pf, Vf)
        b.set_radii(Rf)
        b.set_stop_conditions(collision_radius=rc)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(64, dt_max, softening=eps, **ETA)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "radii and collision_radius are both set" in str(err.value)
        b.set_stop_conditions()
        b.set_integrator("kdk")
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(64, dt_max, softening=eps, **ETA)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "HERMITE" in str(err.value)
        # step_n ignores the radii
        b.set_integrator("hermite")
        b.set_radii(np.full((2, 4), 10.0, np.float32))                              # everything touches
        b.step_n(3, 1e-3, eps)
        with_radii = b.download()
        b.set_radii(None)
        b.set_state(Pf, Vf)
        b.step_n(3, 1e-3, eps)
        without = b.download()
        assert same_bits(with_radii[0], without[0]) and same_bits(with_radii[1], without[1])
        # a stop under radii, which a new set_radii forgets; the slots beyond the counts are never written
        b.set_state(Pf, Vf)
        b.set_radii(Rf[:, :2])                                                      # (B, n < max_bodies): the rest is 0
        assert np.array_equal(b.radii(), np.concatenate([Rf[:, :2], np.zeros((2, 2), np.float32)], 1))
        b.set_radii(Rf)
        res = b.evolve(64, dt_max, softening=eps, **ETA)
        st = b.stops()
        assert st.reason.tolist() == [1, 1] and st.pair.tolist() == [[0, 1], [0, 1]] and (res.ticks < 64 << 12).all()
        assert np.array_equal(st.ticks, uniform.st.ticks)                           # S = 0.3 = R_c: the same step finds it
        p, v = b.download()
        assert (p[:, 2:] == 7.0).all() and (v[:, 2:] == 7.0).all() and np.array_equal(b.radii(), Rf)
        b.set_radii(Rf)
        assert not b.stops().stopped.any()
        # set_radii(None) brings the uniform behaviour back bit for bit
        b.set_radii(None)
        b.set_state(Pf, Vf)
        b.set_stop_conditions(collision_radius=rc)
        res = b.evolve(64, dt_max, softening=eps, **ETA)
        p, v = b.download()
        st = b.stops()
        assert same_bits(p, uniform.p) and same_bits(v, uniform.v) and np.array_equal(res.ticks, uniform.res.ticks)
        assert np.array_equal(st.pair, uniform.st.pair) and same_bits(st.separation, uniform.st.separation)
        # under MERGE an absorbed body is what gets written beyond the count
        b.set_stop_conditions()
        b.set_state(Pf, Vf)
        b.set_counts([2, 2])
        b.set_radii(Rf)
        b.set_collision_action("merge")
        b.evolve(64, dt_max, softening=eps, **ETA)
        p, v = b.download()
        rr = b.radii()
        assert b.counts.tolist() == [1, 1] and (p[:, 2:] == 7.0).all() and (v[:, 2:] == 7.0).all()
        assert rr[:, 1].tolist() == [np.float32(0.1)] * 2 and (rr[:, 2:] == 0.5).all() and p[0, 1, 3] == 0.25
