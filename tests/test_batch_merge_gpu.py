"""GPU: mergers for Hermite batches (BatchedSystem.set_collision_action("merge") / mergers / counts,
include/nbody_batch_merge.h) against the fp64 reference (hermite_merge_ref): a Kepler pair merged at the reference's tick, a
third body carried on after a merger inside an interval, pairs and a clump found at the initial evaluation across waves and
row groups, a radius that never triggers changes no bit, the batch's invariances for states, counts and logs, an escape after
a merger, the log's capacity, and what the merged system is to the later calls.

Every comparison with the reference first asserts, on the CPU, that each deciding separation of the reference is more than
1e-3 relative away from the radius, at the evaluations that decide and at the ones before, so that fp32 rounding cannot move a
merger by a step."""
import numpy as np
import pytest

import hermite_merge_ref as mref
import hermite_ref
import hermite_stop_ref as sref
from hermite_ref import rel_state_error
from test_batch_hermite_gpu import MIXED_COUNTS, mixed_batch

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
MARGIN = 1e-3
ETA = dict(eta=F32(0.01), eta_start=F32(0.01))


class Run:
    """What a fresh Hermite batch gave: p, v, res (EvolveResult), st (StopResult), mg (MergeResult), counts, err."""


def evolve(P, V, counts, n_intervals, dt_max, eps, collision_radius=0.0, escape_radius=0.0, action="merge", log_capacity=8,
           max_bodies=None, launch_steps=None, split=None, **kw):
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
        if action is not None:
            b.set_collision_action(action, log_capacity)
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
    return r


def decided_clearly(ref, rc):
    """Every evaluation of the reference that decides a merger, the one before it and the one after it (the restart) lie
    clear of the radius; so does the closest approach of the whole run."""
    seps = ref.min_sep_seq
    for mg in ref.mergers:
        for k in (mg.eval_index - 1, mg.eval_index, mg.eval_index + 1):
            if 0 <= k < len(seps) and not abs(seps[k] / rc - 1.0) > MARGIN:
                return False
    return all(abs(s / rc - 1.0) > MARGIN for s in seps)


def check_event(ev, mg):
    assert (int(ev["tick"]), int(ev["survivor"]), int(ev["absorbed"]), int(ev["count_before"])) == \
        (mg.tick, mg.survivor, mg.absorbed, mg.count_before)
    for name in ("separation", "relative_speed", "mass_survivor", "mass_absorbed"):
        assert abs(float(ev[name]) / getattr(mg, name) - 1.0) <= 1e-5, (name, ev[name], getattr(mg, name))


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_a_kepler_pair_merges_at_the_reference_tick_and_the_merged_body_coasts_to_the_end(eps):
    pos, vel, period = hermite_ref.kepler(e=0.9)
    P, V = pos[None].astype(np.float32), vel[None].astype(np.float32)
    V[0, :, 3] = [3.0, 4.0]
    dt_max, rc = F32(period / 64), 0.3
    ref = mref.evolve(P[0], V[0], 64, dt_max, levels=12, eps=eps, collision_radius=F32(rc), round_state=True, **ETA)
    assert len(ref.mergers) == 1 and ref.count == 1 and ref.ticks == 64 << 12 and ref.reason == 0
    assert decided_clearly(ref, rc), ref.min_sep_seq
    r = evolve(P, V, [2], 64, dt_max, eps, collision_radius=rc)
    ev = r.mg.events[0, 0]
    ep, evv = rel_state_error(r.p[0], ref.pos), rel_state_error(r.v[0], ref.vel)
    print(f"eps {eps}: steps {r.res.steps[0]} (reference {ref.steps}) merger {ev} (reference tick {ref.mergers[0].tick}, separation "
          f"{ref.mergers[0].separation}, speed {ref.mergers[0].relative_speed}) state {ep:.3g} {evv:.3g}")
    assert r.err is None and r.mg.count.tolist() == [1] and r.counts.tolist() == [1]
    assert r.res.ticks[0] == 64 << 12 and r.st.reason[0] == 0 and not r.st.stopped[0]
    assert r.res.steps[0] == ref.steps
    check_event(ev, ref.mergers[0])
    assert not r.mg.events[0, 1:]["count_before"].any()
    assert ep <= 1e-5 and evv <= 1e-5                                               # slot 0 the merged body, slot 1 the absorbed one
    assert rel_state_error(r.p[0, 1:2], ref.pos[1:2]) <= 1e-5 and rel_state_error(r.v[0, 1:2], ref.vel[1:2]) <= 1e-5
    assert r.p[0, :, 3].tolist() == [1.0, 0.5] and r.v[0, :, 3].tolist() == [3.0, 4.0]


def triple(third_mass=0.25, distance=5.0):
    """A Kepler pair (e = 0.9) about the origin and a bound third body on a wide circular orbit."""
    pos, vel, period = hermite_ref.kepler(e=0.9)
    P = np.zeros((1, 3, 4), np.float32)
    V = np.zeros((1, 3, 4), np.float32)
    P[0, :2], V[0, :2] = pos, vel
    P[0, 2] = [0.0, distance, 0.0, third_mass]
    V[0, 2, 0] = -np.sqrt((1.0 + third_mass) / distance)
    V[0, :, 3] = [7.0, 8.0, 9.0]
    return P, V, F32(period / 64)


def triple_case():
    P, V, dt_max = triple()
    return {eps: mref.evolve(P[0], V[0], 64, dt_max, levels=12, eps=eps, collision_radius=F32(0.3), round_state=True, **ETA)
            for eps in (0.0, 1e-2)}


@pytest.fixture(scope="module")
def triple_refs():
    return triple_case()


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_three_bodies_merge_inside_an_interval_and_follow_the_reference_to_the_end_time(triple_refs, eps):
    P, V, dt_max = triple()
    rc, levels = 0.3, 12
    ref = triple_refs[eps]
    assert len(ref.mergers) == 1 and ref.count == 2 and ref.reason == 0 and ref.ticks == 64 << levels
    assert ref.mergers[0].tick % (1 << levels) != 0 and ref.mergers[0].tick < ref.tick_seq[-1]
    assert any(floor > want for r_ in triple_refs.values() for _, want, floor, _ in r_.restart_seq)   # L_tick, not L*, sets a level
    assert decided_clearly(ref, rc)
    r = evolve(P, V, [3], 64, dt_max, eps, collision_radius=rc)
    ep, ev = rel_state_error(r.p[0], ref.pos), rel_state_error(r.v[0], ref.vel)
    print(f"eps {eps}: steps {r.res.steps[0]} (reference {ref.steps}) restart {ref.restart_seq} merger {r.mg.events[0, 0]} "
          f"state {ep:.3g} {ev:.3g}")
    assert r.err is None and r.counts.tolist() == [2] and r.mg.count.tolist() == [1] and r.st.reason[0] == 0
    check_event(r.mg.events[0, 0], ref.mergers[0])
    assert r.res.steps[0] == ref.steps and r.res.ticks[0] == ref.ticks
    assert ep <= 1e-5 and ev <= 1e-5
    assert r.v[0, :, 3].tolist() == ref.vel[:, 3].tolist() == [7.0, 9.0, 8.0]       # the third body moved into slot 1


PLANTED = [65, 257, 1000, 4096]
PLANTED_COUNTS = PLANTED + [65, 65]


def planted_case():
    """Plummer spheres: systems 0 .. 3 of PLANTED bodies with bodies 5 and n - 3 re-placed at separation R_c / 2 (different
    waves and, at 4096, different row groups of a lane); system 4 with the partner in the last slot (nothing moves); system
    5 with bodies 5, 20 and n - 3 mutually within R_c (two mergers at one tick).  R_c is a third of the smallest separation
    in any of the spheres, so every other pair is farther than 2 R_c.  The reference runs once, for eps = 1e-2."""
    import n_body_problem_amd as nb
    P = np.zeros((6, 4096, 4), np.float32)
    V = np.zeros((6, 4096, 4), np.float32)
    dmin = np.inf
    for s, n in enumerate(PLANTED_COUNTS):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=700 + s % 4)
        V[s, :n, 3] = np.arange(n)
        dmin = min(dmin, mref.closest_pair(P[s, :n, :3].astype(np.float64), 0.0)[2])
    rc = F32(dmin / 3.0)
    off = np.array([0.3, 0.4, 0.0], np.float32) * np.float32(rc)                    # |.| = rc / 2
    for s, n in enumerate(PLANTED):
        P[s, n - 3, :3] = P[s, 5, :3] + off
    P[4, 64, :3] = P[4, 5, :3] + off
    P[5, 62, :3] = P[5, 5, :3] + off
    P[5, 20, :3] = P[5, 5, :3] + np.array([-0.2, 0.1, 0.3], np.float32) * np.float32(rc)
    dt_max, eps = F32(1e-3), 1e-2
    # fp32 rounding of the reference's state up to 257 bodies, where the step counts are compared; above, its fp64 sums
    # rounded to fp32 make it take 96 steps of noise where the plain fp64 reference takes 6 (DESIGN.md 3.6 on the GPU's)
    refs = [mref.evolve(P[s, :n], V[s, :n], 3, dt_max, levels=6, eps=eps, collision_radius=rc, round_state=n <= 257, **ETA)
            for s, n in enumerate(PLANTED_COUNTS)]
    return P, V, rc, dt_max, eps, refs


@pytest.fixture(scope="module")
def planted():
    return planted_case()


def test_planted_pairs_and_a_clump_merge_at_the_initial_evaluation_across_waves_and_row_groups(planted):
    P, V, rc, dt_max, eps, refs = planted
    want = [[(5, n - 3, n)] for n in PLANTED] + [[(5, 64, 65)], [(5, 20, 65), (5, 62, 64)]]
    for s, ref in enumerate(refs):
        assert [(mg.survivor, mg.absorbed, mg.count_before) for mg in ref.mergers] == want[s] and ref.ticks == 3 << 6
        assert all(mg.tick == 0 for mg in ref.mergers) and ref.eval_kind[:len(want[s]) + 1] == ["start"] + ["restart"] * len(want[s])
        assert decided_clearly(ref, rc) and min(ref.min_sep_seq[len(want[s]):]) > 1.5 * rc
    r = evolve(P, V, PLANTED_COUNTS, 3, dt_max, eps, collision_radius=rc, levels=6, **ETA)
    print("R_c", rc, "counts", r.counts, "steps", r.res.steps, [ref.steps for ref in refs], r.mg.count)
    assert r.err is None and not r.st.stopped.any()
    for s, (n, ref) in enumerate(zip(PLANTED_COUNTS, refs)):
        k = len(want[s])
        assert r.counts[s] == ref.count == n - k and r.mg.count[s] == k and r.res.ticks[s] == 3 << 6
        for e, mg in enumerate(ref.mergers):
            check_event(r.mg.events[s, e], mg)
        assert not r.mg.events[s, k:]["count_before"].any()
        # the absorbed bodies' states are the planted ones, bit for bit, in the slots beyond the count, the most recent first
        for q, mg in enumerate(reversed(ref.mergers)):
            slot = n - k + q
            src = int(ref.vel[slot, 3])                                             # w holds the body's first index
            assert src == mg.absorbed and r.v[s, slot, 3] == src
            assert np.array_equal(r.p[s, slot], P[s, src]) and np.array_equal(r.v[s, slot], V[s, src])
        assert np.array_equal(r.v[s, :n, 3], ref.vel[:, 3].astype(np.float32))      # every body where the reference has it
        assert abs(float(r.p[s, 5, 3]) / ref.pos[5, 3] - 1.0) <= 1e-6
        ep, ev = rel_state_error(r.p[s, :n], ref.pos), rel_state_error(r.v[s, :n], ref.vel)
        assert ep <= 1e-5 and ev <= 1e-5, (n, ep, ev)
        if n <= 257:                                                                # above, fp32 sums cost steps
            assert r.res.steps[s] == ref.steps, (n, r.res.steps[s], ref.steps)
        assert np.array_equal(r.p[s, n:], P[s, n:]) and np.array_equal(r.v[s, n:], V[s, n:])   # slots beyond the first count


def test_a_radius_that_never_triggers_changes_no_bit_under_merge():
    P, V = mixed_batch(MIXED_COUNTS, 4096, seed0=300)
    for eps in (1e-2, 0.0):
        plain = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, action=None, levels=6)
        quiet = evolve(P, V, MIXED_COUNTS, 2, F32(1e-3), eps, collision_radius=1e-6, escape_radius=1e6, levels=6)
        assert plain.err is None and quiet.err is None
        assert np.array_equal(quiet.p.view(np.uint32), plain.p.view(np.uint32))
        assert np.array_equal(quiet.v.view(np.uint32), plain.v.view(np.uint32))
        for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
            assert np.array_equal(getattr(quiet.res, name), getattr(plain.res, name)), name
        assert quiet.counts.tolist() == MIXED_COUNTS and not quiet.mg.count.any() and not quiet.st.stopped.any()


def head_on(n=65):
    """A Plummer sphere whose bodies 5 and 61 approach head-on at unit speed from 0.05 apart."""
    import n_body_problem_amd as nb
    pos, vel = nb.plummer(n, seed=41)
    pos[61, :3] = pos[5, :3] + np.float32([0.05, 0.0, 0.0])
    vel[61, :3] = vel[5, :3] + np.float32([-1.0, 0.0, 0.0])
    vel[:, 3] = np.arange(n)
    return pos, vel


def test_states_counts_and_logs_do_not_depend_on_slot_batch_capacity_neighbours_launch_budget_or_a_split_of_the_call():
    n, rc, eps, dt_max = 65, 0.02, 1e-3, F32(1e-3)
    pos, vel = head_on(n)
    ref = mref.evolve(pos, vel, 100, dt_max, levels=6, eps=eps, collision_radius=F32(rc), round_state=True, **ETA)
    assert len(ref.mergers) == 1 and (ref.mergers[0].survivor, ref.mergers[0].absorbed) == (5, 61) and ref.steps > 10
    assert 0 < ref.mergers[0].tick < 60 << 6 and decided_clearly(ref, rc)
    got = []
    # capacities 128, 256 and 4096: two and four rows per lane, one wave and sixteen
    for B, cap, slot, budget, other, split in ((1, 128, 0, None, None, None), (3, 256, 2, 1, 200, None), (2, 4096, 1, 128, 2, None),
                                                (4, 256, 0, 7, 250, 60), (1, 128, 0, 1, None, 60)):
        counts = [other or n] * B
        counts[slot] = n
        P, V = mixed_batch(counts, cap, seed0=50 + B)
        if other == 2:
            P[1 - slot, :2], V[1 - slot, :2] = hermite_ref.kepler(e=0.99)[:2]
        P[slot, :n], V[slot, :n] = pos, vel
        r = evolve(P, V, counts, 100, dt_max, eps, collision_radius=rc, max_bodies=cap, launch_steps=budget, split=split, levels=6, **ETA)
        assert r.err is None
        got.append((r.p[slot, :n].copy(), r.v[slot, :n].copy(), int(r.res.steps[slot]), int(r.res.ticks[slot]) if not split else 100 << 6,
                    int(r.counts[slot]), int(r.mg.count[slot]), r.mg.events[slot].tobytes(), int(r.st.reason[slot])))
    ev = np.frombuffer(got[0][6], dtype=r.mg.events.dtype)
    print("steps", got[0][2], "reference", ref.steps, "merger", ev[0])
    assert got[0][2] == ref.steps and got[0][3] == ref.ticks and got[0][4] == n - 1 and got[0][5] == 1 and got[0][7] == 0
    check_event(ev[0], ref.mergers[0])
    assert rel_state_error(got[0][0], ref.pos) <= 1e-5 and rel_state_error(got[0][1], ref.vel) <= 1e-5
    for g in got[1:]:
        assert g[2:] == got[0][2:]
        assert np.array_equal(g[0].view(np.uint32), got[0][0].view(np.uint32))
        assert np.array_equal(g[1].view(np.uint32), got[0][1].view(np.uint32))


def escape_case():
    """The stop tests' case: a Kepler pair about the origin and a light third body shot outwards at twice its escape speed."""
    pos, vel, period = hermite_ref.kepler(e=0.3)
    P = np.zeros((1, 3, 4), np.float32)
    V = np.zeros((1, 3, 4), np.float32)
    P[0, :2], V[0, :2] = pos, vel
    P[0, 2] = [0.0, 3.0, 0.0, 1e-3]
    V[0, 2, :3] = [0.0, 2.0 * np.sqrt(2.0 / 3.0), 0.0]
    return P, V, F32(period / 64)


def test_a_pair_merges_the_run_goes_on_and_an_escaper_stops_it_with_its_index_after_the_merger():
    P, V, dt_max = escape_case()
    rc, re_ = 1.25, 5.0
    ref = mref.evolve(P[0], V[0], 64, dt_max, levels=12, eps=0.0, collision_radius=F32(rc), escape_radius=re_, round_state=True, **ETA)
    assert len(ref.mergers) == 1 and ref.reason == mref.ESCAPE and ref.escaper == 1 and ref.count == 2
    assert ref.steps - ref.tick_seq.index(next(t for t in ref.tick_seq if t >= ref.mergers[0].tick)) > 3   # it ran on after the merger
    assert decided_clearly(ref, rc)
    assert abs(ref.max_dist_seq[-1] / re_ - 1.0) > MARGIN and abs(ref.max_dist_seq[-2] / re_ - 1.0) > MARGIN
    assert ref.max_dist_seq[-1] > re_ > ref.max_dist_seq[-2]
    r = evolve(P, V, [3], 64, dt_max, 0.0, collision_radius=rc, escape_radius=re_)
    print("steps", r.res.steps[0], "reference", ref.steps, "ticks", r.st.ticks[0], ref.ticks, r.st, r.mg)
    assert r.err is None and r.st.reason[0] == 2 and r.st.escaper[0] == 1 and tuple(r.st.pair[0]) == (-1, -1) and r.st.separation[0] == 0.0
    assert r.counts.tolist() == [2] and r.mg.count.tolist() == [1]
    check_event(r.mg.events[0, 0], ref.mergers[0])
    assert r.res.steps[0] == ref.steps and r.res.ticks[0] == r.st.ticks[0] == ref.ticks < 64 << 12
    assert rel_state_error(r.p[0], ref.pos) <= 1e-5 and rel_state_error(r.v[0], ref.vel) <= 1e-5


def clump():
    """Three bodies within 0.1 of each other at the start and a fourth far away."""
    P = np.array([[[0.0, 0.0, 0.0, 0.5], [2.0, 0.0, 0.0, 0.125], [0.06, 0.0, 0.0, 0.25], [0.0, 0.09, 0.0, 0.125]]], np.float32)
    V = np.zeros((1, 4, 4), np.float32)
    V[0, :, :3] = [[0.0, 0.1, 0.0], [0.0, -0.3, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.1]]
    V[0, :, 3] = [10.0, 11.0, 12.0, 13.0]
    return P, V


def test_the_log_keeps_its_capacity_of_events_and_counts_every_merger():
    P, V = clump()
    ref = mref.evolve(P[0], V[0], 4, F32(1e-2), levels=8, eps=0.0, collision_radius=F32(0.1), round_state=True, **ETA)
    assert len(ref.mergers) == 2 and decided_clearly(ref, 0.1)
    full = evolve(P, V, [4], 4, F32(1e-2), 0.0, collision_radius=0.1, levels=8, **ETA)
    one = evolve(P, V, [4], 4, F32(1e-2), 0.0, collision_radius=0.1, log_capacity=1, levels=8, **ETA)
    none = evolve(P, V, [4], 4, F32(1e-2), 0.0, collision_radius=0.1, log_capacity=0, levels=8, **ETA)
    for r in (full, one, none):
        assert r.err is None and r.mg.count.tolist() == [2] and r.counts.tolist() == [2] and r.res.ticks[0] == 4 << 8
        assert np.array_equal(r.p.view(np.uint32), full.p.view(np.uint32)) and np.array_equal(r.v.view(np.uint32), full.v.view(np.uint32))
    assert full.mg.events.shape == (1, 8) and one.mg.events.shape == (1, 1) and none.mg.events.shape == (1, 0)
    check_event(full.mg.events[0, 0], ref.mergers[0])
    check_event(full.mg.events[0, 1], ref.mergers[1])
    assert one.mg.events[0, 0].tobytes() == full.mg.events[0, 0].tobytes()
    assert full.v[0, :, 3].tolist() == [10.0, 11.0, 13.0, 12.0] and full.res.steps[0] == ref.steps
    assert rel_state_error(full.p[0], ref.pos) <= 1e-5 and rel_state_error(full.v[0], ref.vel) <= 1e-5


def test_later_calls_see_the_merged_system_and_the_action_stop_brings_the_stop_back(triple_refs):
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, dt_max = triple()
    rc, eps = 0.3, 1e-2
    ref = triple_refs[eps]
    live = slice(0, ref.count)
    with nb.BatchedSystem(1, 3, integrator="hermite") as b:
        b.set_state(P, V)
        before = b.momentum()[0]
        b.set_stop_conditions(collision_radius=rc)
        b.set_collision_action("merge")
        b.evolve(64, dt_max, softening=eps, **ETA)
        assert b.counts.tolist() == [2]
        mom, en = b.momentum()[0], b.energy(eps)[0]
        mg = ref.mergers[0]                                                         # its sums over the bodies: before, after, sum m |v|
        print("momentum", before, mom, "reference", mg.momentum_before, mg.momentum_after, mg.momentum_scale, "energy", en)
        assert mom[3] == 1.25                                                       # the two live bodies, not the absorbed slot
        assert np.abs(before[:3] - mg.momentum_before).max() <= 1e-5 * mg.momentum_scale
        assert np.abs(mom[:3] - mg.momentum_after).max() <= 1e-5 * mg.momentum_scale
        # states within 1e-5 of the largest coordinate (5) are speeds within 1e-4 of theirs (0.5), kinetic energies within
        # 2e-4, and the kinetic energy is 1.6 times the total
        assert abs(en[2] / hermite_ref.energy(ref.pos[live], ref.vel[live], eps) - 1.0) <= 1e-3
        b.step_n(2, 1e-3, eps)                                                      # fixed steps run on the merged system
        p, v = b.download()
        pr, vr = hermite_ref.step(ref.pos[live], ref.vel[live], 1e-3, eps, nsteps=2)
        assert rel_state_error(p[0, live], pr) <= 1e-5 and rel_state_error(v[0, live], vr) <= 1e-5
        assert rel_state_error(p[0, 2:], ref.pos[2:]) <= 1e-5 and p[0, 2, 3] == 0.5    # the absorbed slot is left alone
        assert not b.mergers().count.any()                                          # step_n forgets the log, as it forgets stops
        b.set_counts([3])
        b.set_state(P, V)
        b.set_collision_action("stop")
        stopped = sref.evolve(P[0], V[0], 64, dt_max, levels=12, eps=eps, collision_radius=F32(rc), round_state=True, **ETA)
        res = b.evolve(64, dt_max, softening=eps, **ETA)
        st = b.stops()
        assert st.reason.tolist() == [1] and tuple(st.pair[0]) == (0, 1) and st.ticks[0] == stopped.ticks == res.ticks[0]
        assert res.steps[0] == stopped.steps and b.counts.tolist() == [3] and not b.mergers().count.any()
        assert abs(float(st.separation[0]) / stopped.separation - 1.0) <= 1e-5
        with pytest.raises(nb.NBodyError) as err:
            b.set_collision_action("merge", log_capacity=4096)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "log_capacity" in str(err.value)
        with pytest.raises(ValueError):
            b.set_collision_action("bounce")
