"""GPU: accreting tracers for Hermite batches (BatchedSystem.set_hit_action / accretions, include/nbody_batch_accrete.h): a
tracer that hits a massive body gives it its mass word.  With zero mass words ACCRETE is REMOVE bit for bit; planted hitters
give exactly their masses, in ascending order, and the target moves; two tracers of different waves at one evaluation; an
adaptive run with restarts at ticks no coarse step divides; radii that grow and a chain at one tick; an accretion at the initial
evaluation; a step that stops the system accretes nothing; chunked calls, what forgets, the batch's invariances, the total
mass, and what is refused.

The inputs are built in hermite_accrete_ref and are first run through the reference alone, on the CPU, by
test_batch_accrete_cpu.py, which asserts that every decision -- at the restart evaluations too -- lies at least MARGIN
relative from its radius.

Shapes: capacity 64 (one row per lane), 128 (two), 1024 and -- once -- 4096 (four, in groups of two), counts that are no
multiples of 64, m 1 or 3.  Planets have mass 1e-3, tracers around 1e-5.  A few steps to a few dozen per run."""
import ctypes

import numpy as np
import pytest

import hermite_accrete_ref as aref
import hermite_fate_ref as fref
from hermite_ref import rel_state_error

pytestmark = pytest.mark.gpu

H, RE, RP, ETA = aref.H, aref.RE, aref.RP, aref.ETA
TOL = 1e-5                    # the project's parity tolerance for states against the fp64 reference (rel_state_error)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


class Run:
    pass


def run(P, V, counts, massive, chunks, dt_max, levels, eps, radii=None, collision_radius=0.0, escape_radius=0.0, hit="accrete",
        tracers="remove", launch_steps=None, max_steps=0, cap=None, merge=False):
    """A fresh Hermite batch taken through evolve(c) for c in chunks: state, figures, stops, fates, accretions, radii and
    total mass after every chunk."""
    import n_body_problem_amd as nb
    B = P.shape[0]
    cap = cap or P.shape[1]
    Pf, Vf = np.zeros((B, cap, 4), np.float32), np.zeros((B, cap, 4), np.float32)
    Pf[:, :P.shape[1]], Vf[:, :P.shape[1]] = P, V
    out = []
    with nb.BatchedSystem(B, cap, counts=counts, integrator="hermite") as b:
        b.set_state(Pf, Vf)
        if massive is not None:
            b.set_massive_counts(massive)
        if tracers:
            b.set_tracer_action(tracers)
        if hit:
            b.set_hit_action(hit)
        if radii is not None:
            Rf = np.zeros((B, cap), np.float32)
            Rf[:, :radii.shape[1]] = radii
            b.set_radii(Rf)
        if collision_radius or escape_radius:
            b.set_stop_conditions(collision_radius, escape_radius)
        if launch_steps:
            b.set_evolve_launch_steps(launch_steps)
        mass0 = b.momentum()[:, 3].copy()
        for c in chunks:
            r = Run()
            r.err, r.mass0 = None, mass0
            try:
                r.res = b.evolve(c, dt_max, levels=levels, eta=ETA, eta_start=ETA, softening=eps, max_steps=max_steps)
            except nb.NBodyError as e:
                r.err, r.res = e, b.evolve_stats()
            r.p, r.v = b.download()
            r.stops = b.stops()
            r.fates = b.fates() if tracers == "remove" else None
            r.acc = b.accretions() if hit == "accrete" else None
            r.radii = b.radii() if radii is not None else None
            r.mass = b.momentum()[:, 3].copy()
            out.append(r)
    return out


def figures(res):
    return [x.tolist() for x in (res.steps, res.min_level, res.max_level, res.clamped, res.ticks)]


def fate_tuple(f, s=None):
    pick = (lambda a: a) if s is None else (lambda a: a[s])
    return (pick(f.fate).tolist(), pick(f.ticks).tolist(), pick(f.target).tolist(), bits(pick(f.separation)).tolist(),
            bits(pick(f.relative_speed)).tolist(), pick(f.hit).tolist(), pick(f.escaped).tolist())


def stop_tuple(st):
    return (st.reason.tolist(), st.ticks.tolist(), st.pair.tolist(), bits(st.separation).tolist(), st.escaper.tolist())


def check_against(ref, g, s, n, tick_scale=1):
    """Fates, given and the count are the reference's; states within TOL; mass words bit for bit."""
    f = g.fates
    assert f.fate[s, :n].tolist() == ref.fate.tolist()
    assert f.target[s, :n].tolist() == ref.fate_target.tolist()
    assert f.ticks[s, :n].tolist() == (ref.fate_tick * tick_scale).tolist()
    assert (f.hit[s], f.escaped[s]) == (ref.hit, ref.escaped)
    for i in np.nonzero(ref.fate == fref.HIT)[0]:
        assert abs(float(f.separation[s, i]) / ref.fate_separation[i] - 1.0) <= TOL, (i, f.separation[s, i], ref.fate_separation[i])
        assert abs(float(f.relative_speed[s, i]) / ref.fate_speed[i] - 1.0) <= TOL, (i, f.relative_speed[s, i], ref.fate_speed[i])
    assert same_bits(g.acc.given[s, :n], ref.given.astype(np.float32)) and not g.acc.given[s, n:].any()
    assert g.acc.count[s] == ref.accretions
    assert same_bits(g.p[s, :n, 3], ref.pos[:, 3].astype(np.float32))
    if ref.radii is not None:
        assert same_bits(g.radii[s, :n], ref.radii.astype(np.float32))
    ep, ev = rel_state_error(g.p[s, :n], ref.pos), rel_state_error(g.v[s, :n], ref.vel)
    print("state error against the reference: positions", ep, "velocities", ev)
    assert ep <= TOL and ev <= TOL


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,n,m", [(64, 50, 3), (128, 100, 1), (1024, 700, 3), (4096, 3000, 3)])
def test_with_zero_mass_words_accrete_is_remove_bit_for_bit(cap, n, m):
    p, v, R, plan, kw = aref.fixed_step_case(cap, n, m, zero=True)
    for eps in (0.0, 1e-2):
        want = run(p[None], v[None], [n], [m], (3, 2), H, 0, eps, cap=cap, hit=None, **kw)
        got = run(p[None], v[None], [n], [m], (3, 2), H, 0, eps, cap=cap, **kw)    # without the feature: no set_hit_action
        for g, w in zip(got, want):
            assert g.err is None and same_bits(g.p, w.p) and same_bits(g.v, w.v) and figures(g.res) == figures(w.res)
            assert fate_tuple(g.fates) == fate_tuple(w.fates) and stop_tuple(g.stops) == stop_tuple(w.stops)
            assert same_bits(g.radii, w.radii)
            assert not g.acc.given.any() and not g.acc.count.any()
        assert got[1].fates.hit[0] == 3 and got[1].fates.escaped[0] == 2 and got[1].res.steps[0] == 2


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,n,m", [(64, 50, 3), (128, 100, 3), (1024, 700, 3)])
def test_fixed_step_hitters_give_their_masses_in_ascending_order_and_the_target_moves(cap, n, m):
    p, v, R, plan, kw = aref.fixed_step_case(cap, n, m)
    steps, t = 5, m - 1
    ref = aref.reference(p, v, m, steps, H, 0, 0.0, radii=R, escape_radius=RE)
    got = run(p[None], v[None], [n], [m], (steps,), H, 0, 0.0, cap=cap, **kw)[0]
    removed = run(p[None], v[None], [n], [m], (steps,), H, 0, 0.0, cap=cap, hit="remove", **kw)[0]
    assert got.err is None and got.res.steps[0] == steps and not got.stops.reason.any()
    check_against(ref, got, 0, n)
    hitters = sorted(r for r, (kind, _) in plan.items() if kind == "hit")
    assert np.nonzero(got.acc.given[0])[0].tolist() == hitters and got.acc.count[0] == 3
    assert same_bits(got.acc.given[0, hitters], p[hitters, 3])                    # the planted masses
    total = np.float32(p[t, 3])
    for r in hitters:                                                               # ascending: the order they hit in, too
        total = np.float32(total + p[r, 3])
    assert same_bits(got.p[0, t, 3], total)
    assert (bits(got.p[0, hitters, 3]) == 0).all()                                 # +0
    others = [i for i in range(n) if i != t and i not in hitters]
    assert same_bits(got.p[0, others, 3], p[others, 3]) and same_bits(got.v[0, :n, 3], v[:, 3])
    assert same_bits(got.radii, removed.radii)                                     # the tracers have no radius: nothing grows
    assert fate_tuple(got.fates)[0] == fate_tuple(removed.fates)[0]
    moved = rel_state_error(got.v[0, t:t + 1], removed.v[0, t:t + 1])
    print("the target's velocity against the run that removes:", moved)
    assert moved > 100 * TOL                                                        # a missing accretion would show


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_two_tracers_of_different_waves_onto_one_target_at_one_evaluation_are_summed_ascending():
    p, v, R, n, m, rows = aref.pair_case()
    M, a, b = p[2, 3], p[rows[0], 3], p[rows[1], 3]
    ascending, descending = np.float32(np.float32(M + a) + b), np.float32(np.float32(M + b) + a)
    assert not same_bits(ascending, descending)
    ref = aref.reference(p, v, m, 4, H, 0, 0.0, radii=R, escape_radius=RE)
    got = run(p[None], v[None], [n], [m], (4,), H, 0, 0.0, cap=1024, radii=R[None], escape_radius=RE)[0]
    assert got.err is None and got.acc.count[0] == 2 and got.fates.ticks[0, rows].tolist() == [2, 2]
    assert same_bits(got.p[0, 2, 3], ascending)
    check_against(ref, got, 0, n)


# ---- 4 ----------------------------------------------------------------------------------------------------------------
def test_an_adaptive_run_follows_the_reference_through_restarts_and_a_dead_tracer_does_not_vote_in_them():
    p, v, R, n, m = aref.adaptive_case()
    ref = aref.reference(p, v, m, 24, H, 8, 0.0, radii=R, escape_radius=RE)
    with_vote = aref.reference(p, v, m, 24, H, 8, 0.0, radii=R, escape_radius=RE, dead_votes=True)
    got = run(p[None], v[None], [n], [m], (24,), H, 8, 0.0, radii=R[None], escape_radius=RE)[0]
    print("steps", got.res.steps[0], "reference", ref.steps, "with the dead tracer's vote", with_vote.steps, "levels",
          got.res.min_level[0], got.res.max_level[0], "restarts", ref.restart_seq)
    assert got.err is None and not got.stops.reason.any()
    assert ref.accretions == 3 and any(tick % (1 << 8) for tick, _, _, _ in ref.restart_seq)
    assert all(level >= floor_level for _, _, floor_level, level in ref.restart_seq)   # not coarser than the tick allows
    assert with_vote.steps >= ref.steps + 9                          # row 10, dead from the start, would refine every restart
    assert got.res.steps[0] == ref.steps and got.res.ticks[0] == ref.ticks == 24 << 8
    assert got.res.min_level[0] == min(ref.level_seq) and got.res.max_level[0] == max(ref.level_seq)
    assert got.res.clamped[0] == ref.clamped
    check_against(ref, got, 0, n)


# ---- 5 ----------------------------------------------------------------------------------------------------------------
def test_radii_grow_by_the_cube_rule_and_the_grown_planet_swallows_a_neighbour_at_the_same_tick():
    p, v, R, n, m, (t, A, B) = aref.chain_case()
    ref = aref.reference(p, v, m, 3, H, 0, 0.0, radii=R, escape_radius=RE)
    got = run(p[None], v[None], [n], [m], (3,), H, 0, 0.0, cap=64, radii=R[None], escape_radius=RE)[0]
    assert got.err is None and got.res.steps[0] == 3
    assert got.fates.fate[0, [A, B]].tolist() == [fref.HIT, fref.HIT] and got.fates.ticks[0, [A, B]].tolist() == [1, 1]
    assert got.fates.target[0, [A, B]].tolist() == [t, t] and got.acc.count[0] == 2
    once = np.float32(np.cbrt(float(R[t]) ** 3 + float(R[A]) ** 3))                # fp64, rounded once, twice over
    twice = np.float32(np.cbrt(float(once) ** 3 + float(R[B]) ** 3))
    assert same_bits(got.radii[0, t], twice) and twice > once > R[t]
    others = [i for i in range(n) if i != t]
    assert same_bits(got.radii[0, others], R[others]) and not got.radii[0, n:].any()
    check_against(ref, got, 0, n)
    # B lay outside RP + RB and lies inside the grown radius plus its own: found by the restart evaluation alone
    removed = run(p[None], v[None], [n], [m], (3,), H, 0, 0.0, cap=64, radii=R[None], escape_radius=RE, hit="remove")[0]
    assert removed.fates.fate[0, [A, B]].tolist() == [fref.HIT, 0]
    p, v, R, n, m, (t, A, B) = aref.chain_case(shared=True)                         # a shared collision radius: nothing grows
    ref = aref.reference(p, v, m, 3, H, 0, 0.0, collision_radius=0.02, escape_radius=RE)
    got = run(p[None], v[None], [n], [m], (3,), H, 0, 0.0, cap=64, collision_radius=0.02, escape_radius=RE)[0]
    assert got.err is None and got.fates.fate[0, [A, B]].tolist() == [fref.HIT, 0] and got.acc.count[0] == 1
    check_against(ref, got, 0, n)


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_an_accretion_found_at_the_initial_evaluation_has_tick_zero_and_the_restart_chooses_the_first_level():
    p, v, R, n, m = aref.start_case()
    ref = aref.reference(p, v, m, 2, H, 8, 0.0, radii=R, escape_radius=RE)
    got = run(p[None], v[None], [n], [m], (2,), H, 8, 0.0, cap=64, radii=R[None], escape_radius=RE)[0]
    assert got.err is None and not got.stops.reason.any()
    assert [(e[0], e[1], e[2]) for e in ref.events] == [(0, 20, 1), (0, 22, 2)]
    check_against(ref, got, 0, n)
    for i in (20, 22):                                                 # untouched except the mass word
        assert same_bits(got.p[0, i, :3], p[i, :3]) and same_bits(got.v[0, i], v[i]) and bits(got.p[0, i, 3]) == 0
        assert got.fates.ticks[0, i] == 0 and same_bits(got.acc.given[0, i], p[i, 3])
    assert same_bits(got.p[0, 21], p[21]) and got.fates.fate[0, 21] == fref.ESCAPED and got.acc.given[0, 21] == 0
    assert got.res.steps[0] == ref.steps and got.res.max_level[0] == max(ref.level_seq) and got.res.min_level[0] == min(ref.level_seq)
    voting = aref.reference(p, v, m, 2, H, 8, 0.0, radii=R, escape_radius=RE, dead_votes=True)
    assert voting.level_seq[0] > ref.level_seq[0] and got.res.max_level[0] < voting.level_seq[0]


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_a_step_in_which_two_massive_bodies_touch_accretes_nothing():
    p, v, R, n, m = aref.massive_stop_case()
    ref = aref.reference(p, v, m, 8, H, 0, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == fref.COLLISION and ref.steps == 3 and ref.fate_step[12] == 3 and ref.accretions == 0
    got = run(p[None], v[None], [n], [m], (8, 4), H, 0, 0.0, cap=64, radii=R[None], escape_radius=RE)
    alone = run(p[None, :m], v[None, :m], [m], None, (8,), H, 0, 0.0, radii=R[None, :m], escape_radius=RE, tracers=None, hit=None, cap=64)[0]
    g = got[0]
    assert g.err is None and g.res.steps[0] == 3
    assert stop_tuple(g.stops) == stop_tuple(alone.stops) and g.stops.reason[0] == 1 and tuple(g.stops.pair[0]) == (1, 2)
    assert same_bits(g.p[0, :m], alone.p[0, :m]) and same_bits(g.v[0, :m], alone.v[0, :m])
    assert g.fates.fate[0, 12] == fref.HIT and g.fates.ticks[0, 12] == g.stops.ticks[0]
    assert not g.acc.given.any() and g.acc.count[0] == 0 and same_bits(g.p[0, :n, 3], p[:, 3]) and p[12, 3] > 0
    check_against(ref, g, 0, n)
    again = got[1]                                                     # frozen in the next evolve
    assert again.res.steps[0] == 0 and same_bits(again.p, g.p) and same_bits(again.v, g.v)
    assert stop_tuple(again.stops) == stop_tuple(g.stops) and fate_tuple(again.fates) == fate_tuple(g.fates)
    assert not again.acc.given.any() and again.acc.count[0] == 0


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_chunked_calls_are_one_call_and_what_forgets_the_fates_zeroes_given_and_the_count():
    import n_body_problem_amd as nb
    cap, n, m = 128, 100, 3
    p, v, R, plan, kw = aref.fixed_step_case(cap, n, m)
    whole = run(p[None], v[None], [n], [m], (7,), H, 0, 0.0, cap=cap, **kw)[0]
    parts = run(p[None], v[None], [n], [m], (3, 2, 2), H, 0, 0.0, cap=cap, **kw)
    last = parts[2]
    assert same_bits(last.p, whole.p) and same_bits(last.v, whole.v) and same_bits(last.radii, whole.radii)
    assert same_bits(last.acc.given, whole.acc.given) and last.acc.count.tolist() == whole.acc.count.tolist() == [3]
    assert last.fates.fate.tolist() == whole.fates.fate.tolist() and fate_tuple(last.fates)[2:] == fate_tuple(whole.fates)[2:]
    assert parts[0].acc.count[0] == 2 and parts[1].acc.count[0] == 3    # hits in steps 1, 2 and 4
    P = np.zeros((1, cap, 4), np.float32)
    V = np.zeros_like(P)
    P[0, :n], V[0, :n] = p, v
    Rf = np.zeros((1, cap), np.float32)
    Rf[0, :n] = R
    with nb.BatchedSystem(1, cap, counts=[n], integrator="hermite") as b:
        b.set_massive_counts([m])
        b.set_tracer_action("remove")
        b.set_hit_action("accrete")
        b.set_radii(Rf)
        b.set_stop_conditions(escape_radius=RE)
        forgetters = {"set_state": lambda: b.set_state(P, V), "invalidate_forces": b.invalidate_forces,
                      "step_n": lambda: b.step_n(1, 1e-6, 0.0), "set_stop_conditions": lambda: b.set_stop_conditions(escape_radius=RE),
                      "set_radii": lambda: b.set_radii(Rf), "set_massive_counts": lambda: b.set_massive_counts([m]),
                      "set_tracer_action": lambda: b.set_tracer_action("remove"), "set_hit_action": lambda: b.set_hit_action("accrete")}
        for name, forget in forgetters.items():
            b.set_state(P, V)
            b.set_radii(Rf)
            b.evolve(3, H, levels=0, eta=ETA, eta_start=ETA, softening=0.0)
            a = b.accretions()
            assert a.count[0] == 2 and np.count_nonzero(a.given) == 2, name
            forget()
            a = b.accretions()
            assert not a.given.any() and not a.count.any() and not b.fates().fate.any(), name
        b.set_state(P, V)
        b.set_radii(Rf)
        b.evolve(3, H, levels=0, eta=ETA, eta_start=ETA, softening=0.0)  # and forgotten accretions are found anew
        a = b.accretions()
        assert same_bits(a.given, parts[0].acc.given) and a.count.tolist() == parts[0].acc.count.tolist()


# ---- 9 ----------------------------------------------------------------------------------------------------------------
def test_states_fates_and_given_do_not_depend_on_slot_batch_capacity_neighbours_or_launch_budget():
    import n_body_problem_amd as nb
    p, v, R, n, m = aref.adaptive_case()
    got = []
    for B, cap, slot, budget, other in ((1, 64, 0, None, 0), (3, 1024, 2, 1, 300), (2, 128, 1, None, 2), (4, 1024, 0, 7, 1000)):
        counts = [other] * B
        massive = [min(other, 5)] * B
        counts[slot], massive[slot] = n, m
        P, V, Rs = np.zeros((B, cap, 4), np.float32), np.zeros((B, cap, 4), np.float32), np.zeros((B, cap), np.float32)
        for s in range(B):
            if counts[s] and s != slot:
                P[s, :counts[s]], V[s, :counts[s]] = nb.uniform_cube(counts[s], seed=70 * B + s, random_masses=True, speed=0.1)
                Rs[s, :counts[s]] = 1e-3
        P[slot, :n], V[slot, :n], Rs[slot, :n] = p, v, R
        g = run(P, V, counts, massive, (24,), H, 8, 0.0, radii=Rs, escape_radius=RE, launch_steps=budget)[0]
        assert g.err is None
        got.append((g.p[slot, :n].copy(), g.v[slot, :n].copy(), g.radii[slot, :n].copy(), g.acc.given[slot, :n].copy(),
                    int(g.res.steps[slot]), int(g.acc.count[slot]), [x[:n] for x in fate_tuple(g.fates, slot)[:5]]))
        assert not g.acc.given[slot, n:].any()
    assert got[0][5] == 3
    for g in got[1:]:
        assert all(same_bits(x, y) for x, y in zip(g[:4], got[0][:4])) and g[4:] == got[0][4:]


# ---- 10 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fixed", "adaptive", "chain"])
def test_the_total_mass_is_preserved_up_to_the_rounding_of_each_sum(case):
    if case == "fixed":
        p, v, R, plan, kw = aref.fixed_step_case(128, 100, 3)
        g = run(p[None], v[None], [100], [3], (5,), H, 0, 0.0, cap=128, **kw)[0]
    elif case == "adaptive":
        p, v, R, n, m = aref.adaptive_case()
        g = run(p[None], v[None], [n], [m], (24,), H, 8, 0.0, radii=R[None], escape_radius=RE)[0]
    else:
        p, v, R, n, m, _ = aref.chain_case()
        g = run(p[None], v[None], [n], [m], (3,), H, 0, 0.0, radii=R[None], escape_radius=RE)[0]
    k = int(g.acc.count[0])
    drift = abs(g.mass[0] - g.mass0[0]) / g.mass0[0]
    print("accretions", k, "relative change of the total mass", drift)
    assert k >= 2 and drift <= k * 2.0 ** -23
    assert abs(g.acc.given[0].astype(np.float64).sum() - (g.p[0, :3, 3].astype(np.float64).sum() - p[:3, 3].astype(np.float64).sum())) \
        <= k * 2.0 ** -23 * g.mass0[0]


# ---- 11 ---------------------------------------------------------------------------------------------------------------
def test_refusals_defaults_and_running_out_of_steps():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    cap, n, m = 64, 50, 3
    p, v, R, plan, kw = aref.fixed_step_case(cap, n, m)
    P, V, Rf = np.zeros((2, cap, 4), np.float32), np.zeros((2, cap, 4), np.float32), np.zeros((2, cap), np.float32)
    P[:, :n], V[:, :n], Rf[:, :n] = p, v, R
    planted = [r for r in plan]
    P[1, planted, :3], V[1, planted] = P[1, m + 10, :3], V[1, m + 10]   # system 1: nobody planted
    with nb.BatchedSystem(2, cap, counts=[n, n], integrator="hermite") as b:
        b.set_state(P, V)
        b.set_massive_counts([m, m])
        b.set_tracer_action("remove")
        with pytest.raises(nb.NBodyError) as err:                        # the default is remove: nothing is kept
            b.accretions()
        assert err.value.status == _lib.NBODY_ERR_STATE and "REMOVE" in str(err.value)
        with pytest.raises(ValueError):
            b.set_hit_action("merge")
        cfg = _lib.BatchAccreteConfig(2)
        assert b._lib.nbody_batch_accrete_set(b._h, ctypes.byref(cfg)) == _lib.NBODY_ERR_INVALID
        assert b"unknown hit action" in b._lib.nbody_batch_last_error(b._h)
        with pytest.raises(nb.NBodyError):
            b.accretions()                                                 # the refused call changed nothing
        b.set_hit_action("accrete")
        assert not b.accretions().given.any()
        cfg = _lib.BatchFateConfig(2)                                      # the tracer actions stay two
        assert b._lib.nbody_batch_fate_set(b._h, ctypes.byref(cfg)) == _lib.NBODY_ERR_INVALID
        assert b"unknown tracer action" in b._lib.nbody_batch_last_error(b._h)
        b.set_radii(Rf)
        b.set_collision_action("merge")
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(1, H, levels=0, softening=0.0)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "MERGE together with massive counts" in str(err.value)
        b.set_collision_action("stop")
        b.set_stop_conditions(collision_radius=0.01, escape_radius=RE)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(1, H, levels=0, softening=0.0)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "radii and collision_radius are both set" in str(err.value)
        b.set_tracer_action("refuse")
        b.set_stop_conditions(escape_radius=RE)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(1, H, levels=0, softening=0.0)
        assert err.value.status == _lib.NBODY_ERR_INVALID and "massive counts are set together with a stopping condition" in str(err.value)
        dp, dv = b.download()
        assert same_bits(dp, P) and same_bits(dv, V)                    # the refused calls changed nothing
        # out of steps: the same call again continues, accretions kept, and gives the whole run's result
        b.set_tracer_action("remove")
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(5, H, levels=0, softening=0.0, max_steps=3)
        assert err.value.status == _lib.NBODY_ERR_STATE and "2 of 2 systems are unfinished" in str(err.value)
        part = b.accretions()
        assert part.count.tolist() == [2, 0]
        res = b.evolve(5, H, levels=0, softening=0.0, max_steps=3)
        assert res.ticks.tolist() == [5, 5]
        done, fates, (dp, dv), radii = b.accretions(), b.fates(), b.download(), b.radii()
    whole = run(P, V, [n, n], [m, m], (5,), H, 0, 0.0, radii=Rf, escape_radius=RE)[0]
    assert same_bits(done.given, whole.acc.given) and done.count.tolist() == whole.acc.count.tolist() == [3, 0]
    assert fate_tuple(fates) == fate_tuple(whole.fates) and same_bits(dp, whole.p) and same_bits(dv, whole.v) and same_bits(radii, whole.radii)
    # ACCRETE with an escape radius only, or without massive counts: today's run bit for bit
    a = run(P, V, [n, n], [m, m], (5,), H, 0, 0.0, escape_radius=RE)[0]
    c = run(P, V, [n, n], [m, m], (5,), H, 0, 0.0, escape_radius=RE, hit=None)[0]
    assert same_bits(a.p, c.p) and same_bits(a.v, c.v) and figures(a.res) == figures(c.res) and fate_tuple(a.fates) == fate_tuple(c.fates)
    assert a.fates.escaped[0] == 2 and not a.acc.given.any() and not a.acc.count.any()
    q, w, _, _ = aref.scene(50, 50, hit_steps=(), escape_steps=())
    never = dict(collision_radius=1e-7, escape_radius=1e6)
    a = run(q[None], w[None], [50], None, (2,), H, 6, 1e-2, **never)[0]
    c = run(q[None], w[None], [50], None, (2,), H, 6, 1e-2, hit=None, tracers=None, **never)[0]
    assert same_bits(a.p, c.p) and same_bits(a.v, c.v) and figures(a.res) == figures(c.res) and not a.acc.given.any()
