"""GPU: stopping conditions for Hermite batches (BatchedSystem.set_stop_conditions / stops, include/nbody_batch_stop.h):
collisions and escapers against the fp64 reference step for step, a pair found at the initial evaluation across waves and
row groups, conditions that never trigger change no bit, a stopped state is the plain evolve's after as many steps, the
batch's invariances for reports and stopped states, and what freezes, keeps and forgets a stop.

Every comparison with the reference first asserts, on the CPU, that the reference's deciding quantity (a separation, or a
distance from the origin) is more than 1e-3 relative away from the radius at the stopping evaluation and at the one
before, so that fp32 rounding cannot move the stop by a step."""
import numpy as np
import pytest

import hermite_ref
import hermite_stop_ref as sref
from hermite_ref import rel_state_error
from test_batch_hermite_gpu import MIXED_COUNTS, mixed_batch

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
MARGIN = 1e-3
NEVER = dict(collision_radius=1e-6, escape_radius=1e6)   # radii no system here can meet


def evolve(P, V, counts, n_intervals, dt_max, eps, collision_radius=0.0, escape_radius=0.0, max_bodies=None, launch_steps=None,
           conditions=True, **kw):
    """(positions, velocities, EvolveResult, StopResult, error or None) of a fresh Hermite batch."""
    import n_body_problem_amd as nb
    B = P.shape[0]
    max_bodies = max_bodies or P.shape[1]
    Pf = np.zeros((B, max_bodies, 4), np.float32)
    Vf = np.zeros((B, max_bodies, 4), np.float32)
    m = min(max_bodies, P.shape[1])
    Pf[:, :m], Vf[:, :m] = P[:, :m], V[:, :m]
    with nb.BatchedSystem(B, max_bodies, counts=counts, integrator="hermite") as b:
        b.set_state(Pf, Vf)
        if conditions:
            b.set_stop_conditions(collision_radius, escape_radius)
        if launch_steps:
            b.set_evolve_launch_steps(launch_steps)
        err = None
        try:
            res = b.evolve(n_intervals, dt_max, softening=eps, **kw)
        except nb.NBodyError as e:
            err, res = e, b.evolve_stats()
        p, v = b.download()
        return p, v, res, b.stops(), err


def decided_clearly(now, before, radius):
    return abs(now / radius - 1.0) > MARGIN and abs(before / radius - 1.0) > MARGIN


@pytest.mark.parametrize("e,rc", [(0.9, 0.3), (0.5, 0.8)])
@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_a_kepler_pair_stops_at_the_reference_step_with_its_separation_and_state(e, rc, eps):
    pos, vel, period = hermite_ref.kepler(e=e)
    P, V = pos[None].astype(np.float32), vel[None].astype(np.float32)
    dt_max = F32(period / 64)
    ref = sref.evolve(P[0], V[0], 64, dt_max, levels=12, eta=F32(0.01), eta_start=F32(0.01), eps=eps, collision_radius=F32(rc),
                      round_state=True)
    assert ref.reason == sref.COLLISION and ref.steps > 3
    assert decided_clearly(ref.separation, ref.prev_min_sep, rc), (ref.separation, ref.prev_min_sep)
    p, v, res, st, err = evolve(P, V, [2], 64, dt_max, eps, collision_radius=rc)
    sep_err = abs(float(st.separation[0]) / ref.separation - 1.0)
    ep, ev = rel_state_error(p[0], ref.pos), rel_state_error(v[0], ref.vel)
    print(f"e {e} eps {eps}: steps {res.steps[0]} (reference {ref.steps}) tick {st.ticks[0]} separation {st.separation[0]} "
          f"(reference {ref.separation}, rel {sep_err:.3g}) state {ep:.3g} {ev:.3g}")
    assert err is None
    assert st.reason[0] == 1 and st.stopped[0] and tuple(st.pair[0]) == (0, 1) and st.escaper[0] == -1
    assert res.steps[0] == ref.steps and res.ticks[0] == st.ticks[0] == ref.ticks < 64 << 12
    assert sep_err <= 1e-5
    assert ep <= 1e-5 and ev <= 1e-5


def escape_case():
    """A Kepler pair about the origin and a light third body shot outwards at twice its escape speed."""
    pos, vel, period = hermite_ref.kepler(e=0.3)
    P = np.zeros((1, 3, 4), np.float32)
    V = np.zeros((1, 3, 4), np.float32)
    P[0, :2], V[0, :2] = pos, vel
    P[0, 2] = [0.0, 3.0, 0.0, 1e-3]
    V[0, 2, :3] = [0.0, 2.0 * np.sqrt(2.0 / 3.0), 0.0]
    return P, V, F32(period / 64)


def test_an_escaper_stops_its_system_and_both_conditions_in_one_step_give_reason_3():
    P, V, dt_max = escape_case()
    re_ = 5.0
    kw = dict(levels=12, eta=F32(0.01), eta_start=F32(0.01), eps=0.0, round_state=True)
    ref = sref.evolve(P[0], V[0], 64, dt_max, escape_radius=re_, **kw)
    assert ref.reason == sref.ESCAPE and ref.escaper == 2 and ref.steps > 3
    assert decided_clearly(ref.dist_seq[-1][2], ref.dist_seq[-2][2], re_)
    assert max(d[:2].max() for d in ref.dist_seq) < re_ * (1.0 - MARGIN)
    p, v, res, st, err = evolve(P, V, [3], 64, dt_max, 0.0, escape_radius=re_)
    print("escape: steps", res.steps[0], "reference", ref.steps, "tick", st.ticks[0], st)
    assert err is None and st.reason[0] == 2 and st.escaper[0] == 2 and tuple(st.pair[0]) == (-1, -1) and st.separation[0] == 0.0
    assert res.steps[0] == ref.steps and res.ticks[0] == st.ticks[0] == ref.ticks
    assert rel_state_error(p[0], ref.pos) <= 1e-5 and rel_state_error(v[0], ref.vel) <= 1e-5
    # the pair closes in from apocentre all the while: a collision radius between its separations at the escaping step's
    # evaluation and at the one before makes both conditions trigger in that step
    seps = ref.min_sep_seq
    assert all(a > b for a, b in zip(seps, seps[1:]))
    rc = 0.5 * (seps[-1] + seps[-2])
    assert decided_clearly(seps[-1], seps[-2], rc), seps[-2:]
    both = sref.evolve(P[0], V[0], 64, dt_max, escape_radius=re_, collision_radius=F32(rc), **kw)
    assert both.reason == 3 and both.steps == ref.steps and both.pair == (0, 1)
    p, v, res, st, err = evolve(P, V, [3], 64, dt_max, 0.0, escape_radius=re_, collision_radius=rc)
    assert err is None and st.reason[0] == 3 and tuple(st.pair[0]) == (0, 1) and st.escaper[0] == 2
    assert res.steps[0] == ref.steps and st.ticks[0] == ref.ticks
    assert abs(float(st.separation[0]) / both.separation - 1.0) <= 1e-5


PLANTED = [65, 257, 1000, 4096]


@pytest.fixture(scope="module")
def planted():
    """Plummer spheres of PLANTED bodies twice over: systems 0 .. 3 with bodies 5 and n - 3 re-placed at separation R_c / 2
    (different waves and, at 4096, different row groups of a lane), systems 4 .. 7 as they are.  R_c is a third of the
    smallest separation in any of the spheres, so every other pair is farther than 2 R_c."""
    import n_body_problem_amd as nb
    counts = PLANTED + PLANTED
    P = np.zeros((8, 4096, 4), np.float32)
    V = np.zeros((8, 4096, 4), np.float32)
    dmin = np.inf
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=700 + s % 4)
        x = P[s, :n, :3].astype(np.float64)
        for lo in range(0, n, 512):
            d = np.sqrt(((x[None] - x[lo:lo + 512, None]) ** 2).sum(-1))
            d[np.arange(d.shape[0]), lo + np.arange(d.shape[0])] = np.inf
            dmin = min(dmin, float(d.min()))
    rc = F32(dmin / 3.0)
    want = []
    for s, n in enumerate(PLANTED):
        P[s, n - 3, :3] = P[s, 5, :3] + np.array([0.3, 0.4, 0.0], np.float32) * np.float32(rc)    # |.| = rc / 2
        x = P[s, :n, :3].astype(np.float64)
        sep = float(np.sqrt(((x[n - 3] - x[5]) ** 2).sum()))
        assert 0.4 * rc < sep < 0.6 * rc
        for lo in range(0, n, 512):                       # every other pair is farther than 2 R_c
            d = np.sqrt(((x[None] - x[lo:lo + 512, None]) ** 2).sum(-1))
            rows = lo + np.arange(d.shape[0])
            d[np.arange(d.shape[0]), rows] = np.inf
            for i, j in ((5, n - 3), (n - 3, 5)):
                if lo <= i < lo + d.shape[0]:
                    d[i - lo, j] = np.inf
            assert d.min() > 2.0 * rc, (n, d.min(), rc)
        want.append(sep)
    return P, V, counts, rc, want


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_a_pair_within_the_radius_at_the_start_stops_its_system_before_any_step(planted, eps):
    P, V, counts, rc, want = planted
    p, v, res, st, err = evolve(P, V, counts, 2, F32(1e-3), eps, collision_radius=rc, levels=2)
    print("R_c", rc, st, res)
    assert err is None
    for s, n in enumerate(PLANTED):
        assert st.reason[s] == 1 and tuple(st.pair[s]) == (5, n - 3) and st.ticks[s] == 0 and st.escaper[s] == -1
        assert res.steps[s] == 0 and res.ticks[s] == 0
        assert abs(float(st.separation[s]) / want[s] - 1.0) <= 1e-5, (n, st.separation[s], want[s])
        assert np.array_equal(p[s], P[s]) and np.array_equal(v[s], V[s])          # not a bit of the state moved
    for s in range(4, 8):
        assert st.reason[s] == 0 and not st.stopped[s] and res.ticks[s] == 2 << 2 and res.steps[s] >= 2
        assert st.ticks[s] == 0 and tuple(st.pair[s]) == (0, 0) and st.separation[s] == 0.0 and st.escaper[s] == 0


def test_conditions_that_never_trigger_change_no_bit():
    P, V = mixed_batch(MIXED_COUNTS, 4096, seed0=300)
    for eps in (1e-2, 0.0):
        plain = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, conditions=False, levels=6)
        quiet = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, levels=6, **NEVER)
        assert np.array_equal(quiet[0].view(np.uint32), plain[0].view(np.uint32))
        assert np.array_equal(quiet[1].view(np.uint32), plain[1].view(np.uint32))
        for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
            assert np.array_equal(getattr(quiet[2], name), getattr(plain[2], name)), name
        assert not quiet[3].stopped.any() and not quiet[3].ticks.any() and not quiet[3].pair.any()


def kepler_pair_batch(eccentricities):
    P = np.zeros((len(eccentricities), 2, 4), np.float32)
    V = np.zeros_like(P)
    for s, e in enumerate(eccentricities):
        pos, vel, period = hermite_ref.kepler(e=e)
        P[s], V[s] = pos, vel
    return P, V, F32(period / 64)


def test_a_stopped_state_is_the_plain_evolve_after_as_many_steps_bit_for_bit():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, dt_max = kepler_pair_batch([0.9, 0.5])              # R_c = 0.3: the second pair never comes closer than 0.5
    p, v, res, st, err = evolve(P, V, [2, 2], 64, dt_max, 0.0, collision_radius=0.3)
    assert err is None and st.reason.tolist() == [1, 0] and 3 < res.steps[0] and res.ticks[1] == 64 << 12
    whole = evolve(P, V, [2, 2], 64, dt_max, 0.0, conditions=False)
    assert np.array_equal(p[1], whole[0][1]) and np.array_equal(v[1], whole[1][1]) and res.steps[1] == whole[2].steps[1]
    alone = evolve(P[:1], V[:1], [2], 64, dt_max, 0.0, conditions=False, max_steps=int(res.steps[0]))
    assert isinstance(alone[4], nb.NBodyError) and alone[4].status == _lib.NBODY_ERR_STATE
    assert alone[2].steps[0] == res.steps[0] and alone[2].ticks[0] == res.ticks[0]
    assert np.array_equal(p[0].view(np.uint32), alone[0][0].view(np.uint32))
    assert np.array_equal(v[0].view(np.uint32), alone[1][0].view(np.uint32))


def test_reports_and_stopped_states_do_not_depend_on_slot_batch_capacity_neighbours_or_launch_budget():
    import n_body_problem_amd as nb
    n, rc, eps, dt_max = 64, 0.02, 1e-3, F32(1e-3)
    pos, vel = nb.plummer(n, seed=41)
    pos[61, :3] = pos[5, :3] + np.float32([0.05, 0.0, 0.0])   # bodies 5 and 61 approach head-on at unit speed
    vel[61, :3] = vel[5, :3] + np.float32([-1.0, 0.0, 0.0])
    ref = sref.evolve(pos, vel, 100, dt_max, levels=6, eta=F32(0.01), eta_start=F32(0.01), eps=eps, collision_radius=F32(rc),
                      round_state=True)
    assert ref.reason == 1 and ref.pair == (5, 61) and ref.steps > 10
    assert decided_clearly(ref.separation, ref.prev_min_sep, rc)
    got = []
    for B, cap, slot, budget, other in ((1, 64, 0, None, None), (3, 1024, 2, 1, 300), (2, 64, 1, 128, 2), (4, 1024, 0, 7, 1000)):
        counts = [other or n] * B
        counts[slot] = n
        P, V = mixed_batch(counts, cap, seed0=50 + B)
        if other == 2:
            P[1 - slot, :2], V[1 - slot, :2] = hermite_ref.kepler(e=0.99)[:2]
        P[slot, :n], V[slot, :n] = pos, vel
        p, v, res, st, err = evolve(P, V, counts, 100, dt_max, eps, collision_radius=rc, max_bodies=cap, launch_steps=budget, levels=6)
        assert err is None
        got.append((p[slot, :n].copy(), v[slot, :n].copy(), int(res.steps[slot]), int(res.ticks[slot]), int(st.reason[slot]),
                    int(st.ticks[slot]), tuple(st.pair[slot]), st.separation[slot:slot + 1].view(np.uint32)[0], int(st.escaper[slot])))
    print("steps", got[0][2], "reference", ref.steps, "report", got[0][4:])
    assert got[0][4] == 1 and got[0][6] == (5, 61) and got[0][2] == ref.steps and got[0][5] == ref.ticks
    assert abs(float(np.uint32(got[0][7]).view(np.float32)) / ref.separation - 1.0) <= 1e-5
    for g in got[1:]:
        assert g[2:] == got[0][2:]
        assert np.array_equal(g[0].view(np.uint32), got[0][0].view(np.uint32))
        assert np.array_equal(g[1].view(np.uint32), got[0][1].view(np.uint32))


def report(st):
    return (st.reason.tolist(), st.ticks.tolist(), st.pair.tolist(), st.separation.view(np.uint32).tolist(), st.escaper.tolist())


def test_a_stop_freezes_its_system_and_what_forgets_the_caches_forgets_it():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, dt_max = kepler_pair_batch([0.9, 0.5])
    with nb.BatchedSystem(2, 2, integrator="hermite") as b:
        def stop_again():
            b.set_state(P, V)
            b.set_stop_conditions(collision_radius=0.3)
            res = b.evolve(64, dt_max, softening=0.0)
            assert b.stops().reason.tolist() == [1, 0]
            return res
        first = stop_again()
        st, (p, v) = b.stops(), b.download()
        res = b.evolve(8, dt_max, softening=0.0)                                  # frozen; the other system advances
        p2, v2 = b.download()
        assert report(b.stops()) == report(st)
        assert np.array_equal(p2[0].view(np.uint32), p[0].view(np.uint32)) and np.array_equal(v2[0].view(np.uint32), v[0].view(np.uint32))
        assert res.steps[0] == 0 and res.ticks[0] == 0 and res.steps[1] >= 8 and res.ticks[1] == 8 << 12
        assert not np.array_equal(p2[1], p[1])
        zero = ([0, 0], [0, 0], [[0, 0], [0, 0]], [0, 0], [0, 0])
        for forget in ("set_state", "invalidate_forces", "step_n", "set_stop_conditions"):
            stop_again()
            if forget == "set_state":
                b.set_state(P, V)
            elif forget == "invalidate_forces":
                b.invalidate_forces()
            elif forget == "step_n":
                b.step_n(1, 1e-4, 0.0)
            else:
                b.set_stop_conditions(collision_radius=0.3)
            assert report(b.stops()) == zero, forget
        again = stop_again()                                                      # and a forgotten stop is found anew
        assert again.steps[0] == first.steps[0]
        b.set_state(P, V)
        b.set_stop_conditions()                                                   # off: the run goes through
        res = b.evolve(64, dt_max, softening=0.0)
        assert report(b.stops()) == zero and res.ticks.tolist() == [64 << 12] * 2
        for bad in (dict(collision_radius=-1.0), dict(escape_radius=float("nan")), dict(collision_radius=float("inf")),
                    dict(escape_radius=-0.5)):
            with pytest.raises(nb.NBodyError) as err:
                b.set_stop_conditions(**bad)
            assert err.value.status == _lib.NBODY_ERR_INVALID and "radius" in str(err.value), bad
    with nb.BatchedSystem(2, 2, integrator="kdk") as b:
        b.set_state(P, V)
        b.set_stop_conditions(collision_radius=0.3)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(1, dt_max, softening=0.0)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "NBODY_INTEGRATOR_HERMITE" in str(err.value)


def test_running_out_of_steps_counts_unfinished_systems_only_never_stopped_ones():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, dt_max = kepler_pair_batch([0.9, 0.5])               # the first stops after 100 steps, the second needs 184
    with nb.BatchedSystem(2, 2, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_stop_conditions(collision_radius=0.3)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(64, dt_max, softening=0.0, max_steps=120)
        assert err.value.status == _lib.NBODY_ERR_STATE
        assert "system 1 " in str(err.value) and "1 of 2 systems are unfinished" in str(err.value), str(err.value)
        st = b.stops()
        assert st.reason.tolist() == [1, 0] and b.evolve_stats().steps.tolist()[1] == 120
        res = b.evolve(64, dt_max, softening=0.0)                                 # completes the second, the first stays frozen
        assert res.ticks[1] == 64 << 12 and res.steps[0] == 0 and report(b.stops()) == report(st)
