"""GPU: external fields for Hermite batches (BatchedSystem.set_external_field, include/nbody_batch_field.h).  A Plummer term
is a body fixed at the origin bit for bit; systems whose components are all NONE run as with the field off; fixed and
adaptive steps agree with the fp64 reference (hermite_field_ref) at every workgroup shape, with and without massive counts;
the batch's bit-for-bit invariances hold; the setter forgets and restores what its header says; the refusals leave the state
alone; a tracer in a logarithmic halo keeps its energy; and the potential is the fp64 formula.

Capacities 64, 128 and above are the three workgroup shapes (one, two and four rows per lane); the body counts 5, 60, 64, 100,
128, 257 and 1000 sit below, at and above the wave and the row-group boundaries.  eps = 0 runs the guard, eps = 1e-2 does not."""
import numpy as np
import pytest

import hermite_field_ref as fref
from hermite_ref import rel_state_error

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
EPSILONS = [0.0, 1e-2]
#: all three kinds together: a bulge, a disc and a flattened halo of comparable pull at the clusters' scale (~1)
BULGE, DISC, HALO = ("plummer", 0.3, 0.05, 0.0), ("miyamoto_nagai", 1.0, 0.5, 0.1), ("log_halo", 0.7, 1.0, 0.9)
GALAXY = [BULGE, DISC, HALO]
#: capacity -> the counts run at it
SHAPES = {64: [5, 60, 64], 128: [100, 128], 1000: [257, 1000]}


def as_array(components, B):
    """(B, C, 4) float64 from a list of named components."""
    rows = [[fref.KINDS[c[0]], c[1], c[2], c[3]] for c in components]
    return np.broadcast_to(np.asarray(rows, np.float64)[None], (B, len(rows), 4)).copy()


def varied(B):
    """(B, 4, 4): the three kinds in an order that turns with the system, a NONE among them at a place that moves too."""
    out = np.zeros((B, 4, 4))
    for s in range(B):
        comps = [GALAXY[(s + k) % 3] for k in range(3)]
        comps.insert(s % 4, ("none", 5.0, 6.0, 7.0))
        out[s] = as_array(comps, 1)[0]
    return out


def named(row):
    """A reference component list from one system's (C, 4) array."""
    return [(int(k), F32(a), F32(b), F32(c)) for k, a, b, c in row]


def clusters(counts, cap, seed0=700, fill=0.0):
    """System s: a Plummer sphere of counts[s] bodies drifting through the field, the rest set to `fill`."""
    import n_body_problem_amd as nb
    P = np.full((len(counts), cap, 4), fill, dtype=np.float32)
    V = np.full((len(counts), cap, 4), fill, dtype=np.float32)
    for s, n in enumerate(counts):
        if n:
            P[s, :n], V[s, :n] = nb.plummer(n, seed=seed0 + s)
            V[s, :n, 3] = 3.0 + s                                            # the fourth words: preserved
    return P, V


def evolve(P, V, counts, n_intervals, dt_max, eps, field=None, massive=None, chunks=None, launch_steps=None, **kw):
    """(positions, velocities, result of the last call) of a fresh Hermite batch of P's capacity."""
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        if massive is not None:
            b.set_massive_counts(massive)
        if field is not None:
            b.set_external_field(field)
        if launch_steps:
            b.set_evolve_launch_steps(launch_steps)
        for c in chunks or [n_intervals]:
            res = b.evolve(c, dt_max, softening=eps, **kw)
        p, v = b.download()
        return p, v, res


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- 1. Plummer is a fixed body ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_scale", [0.0, 0.05])
@pytest.mark.parametrize("n_t", [60, 127, 300])
def test_a_plummer_term_is_a_body_fixed_at_the_origin_bit_for_bit(n_t, b_scale):
    rng = np.random.default_rng(n_t)
    M = 1.0
    r = rng.uniform(0.3, 2.0, n_t)
    u = rng.normal(size=(n_t, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n_t, 3)))
    w /= np.linalg.norm(w, axis=1)[:, None]
    TP = np.zeros((n_t, 4), np.float32)
    TV = np.zeros((n_t, 4), np.float32)
    TP[:, :3] = (r[:, None] * u)
    TV[:, :3] = (rng.uniform(0.4, 1.1, n_t) * np.sqrt(M / r))[:, None] * w + 0.2 * u       # eccentric, bound
    TP[:, 3], TV[:, 3] = 0.37, 9.0                                                       # mass words nobody reads
    dt_max, kw = F32(1.0 / 16.0), dict(levels=12, eta=0.01, eta_start=0.01)
    A = evolve(TP[None], TV[None], [n_t], 3, dt_max, b_scale, field=[("plummer", M, b_scale, 0.0)], massive=[0], **kw)
    BP = np.zeros((1, n_t + 1, 4), np.float32)
    BV = np.zeros_like(BP)
    BP[0, 0, 3] = M
    BP[0, 1:], BV[0, 1:] = TP, TV
    B = evolve(BP, BV, [n_t + 1], 3, dt_max, b_scale, massive=[1], **kw)
    assert same_bits(A[0][0], B[0][0, 1:]) and same_bits(A[1][0], B[1][0, 1:])
    assert same_bits(B[0][0, 0], BP[0, 0]) and same_bits(B[1][0, 0], BV[0, 0])           # the body never left the origin
    for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
        assert np.array_equal(getattr(A[2], name), getattr(B[2], name)), name
    assert A[2].steps[0] > 3                                                             # the field drove the step
    assert not same_bits(A[0][0], TP)


# ---- 2. NONE changes nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("massive", [None, [100, 8, 8, 0]], ids=["all massive", "massive counts"])
def test_systems_whose_components_are_all_none_run_as_with_the_field_off(massive, eps):
    counts = [100, 100, 60, 100]
    P, V = clusters(counts, 128)
    field = varied(4)
    field[0, :, 0] = field[2, :, 0] = 0                                                  # systems 0 and 2: NONE four times
    dt_max = F32(1.0 / 64.0)
    off = evolve(P, V, counts, 2, dt_max, eps, massive=massive, levels=6)
    on = evolve(P, V, counts, 2, dt_max, eps, field=field, massive=massive, levels=6)
    for s in (0, 2):
        assert same_bits(on[0][s], off[0][s]) and same_bits(on[1][s], off[1][s]), s
        assert on[2].steps[s] == off[2].steps[s] and on[2].max_level[s] == off[2].max_level[s]
    for s in (1, 3):
        assert not same_bits(on[0][s, :counts[s]], off[0][s, :counts[s]]), s


# ---- 3. fixed steps against the fp64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("cap", sorted(SHAPES))
def test_three_fixed_steps_match_the_fp64_reference_with_every_massive_count(cap, eps):
    base = SHAPES[cap]
    counts = [n for n in base for _ in range(4)]
    massive = [m for n in base for m in (0, 1, 8, n)]
    P, V = clusters(counts, cap)
    field = varied(len(counts))
    dt = F32(1e-3)
    p, v, res = evolve(P, V, counts, 3, dt, eps, field=field, massive=massive, levels=0)
    assert np.array_equal(res.steps, [3] * len(counts)) and np.array_equal(res.ticks, [3] * len(counts))
    worst = []
    for s, (n, m) in enumerate(zip(counts, massive)):
        assert same_bits(p[s, :n, 3], P[s, :n, 3]) and same_bits(v[s, :n, 3], V[s, :n, 3])
        r = fref.evolve(P[s, :n], V[s, :n], 3, dt, levels=0, eps=eps, components=named(field[s]), massive=m)
        ep, ev = rel_state_error(p[s, :n], r.pos), rel_state_error(v[s, :n], r.vel)
        worst.append((n, m, ep, ev))
        assert ep < 1e-5 and ev < 1e-5, (n, m, eps, ep, ev)
    print("n, massive, pos, vel:", worst)
    # the field is there: without it the tracers of a system with no massive body do not turn
    plain = fref.evolve(P[0, :counts[0]], V[0, :counts[0]], 3, dt, levels=0, eps=eps, massive=0)
    assert rel_state_error(p[0, :counts[0]], plain.pos) > 1e-9 or rel_state_error(v[0, :counts[0]], plain.vel) > 1e-6


# ---- 4. adaptive steps against the fp64 reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("cap", sorted(SHAPES))
def test_a_few_adaptive_intervals_match_the_fp64_reference_per_system(cap):
    base = SHAPES[cap] if cap < 1000 else [257]
    cap = min(cap, 257)
    counts = [n for n in base for _ in range(3)]
    dt_max, eps, n_intervals, levels = F32(1e-3), 1e-2, 3, 6
    P, V = clusters(counts, cap)
    field = varied(len(counts))
    worst = []
    for massive in (None, [m for n in base for m in (0, 8, n)]):
        p, v, res = evolve(P, V, counts, n_intervals, dt_max, eps, field=field, massive=massive, levels=levels)
        for s, n in enumerate(counts):
            assert same_bits(p[s, :n, 3], P[s, :n, 3]) and same_bits(v[s, :n, 3], V[s, :n, 3])
            kw = dict(levels=levels, eta=F32(0.01), eta_start=F32(0.01), eps=eps, components=named(field[s]),
                      massive=None if massive is None else massive[s])
            r = fref.evolve(P[s, :n], V[s, :n], n_intervals, dt_max, **kw)
            rr = fref.evolve(P[s, :n], V[s, :n], n_intervals, dt_max, round_state=True, **kw)
            rounding = max(rel_state_error(rr.pos, r.pos), rel_state_error(rr.vel, r.vel))
            ep, ev = rel_state_error(p[s, :n], r.pos), rel_state_error(v[s, :n], r.vel)
            worst.append((n, kw["massive"], int(res.steps[s]), r.steps, ep, ev, rounding))
            assert rounding < 1e-6, (n, rounding)
            assert ep < 1e-5 and ev < 1e-5, (n, ep, ev)
            assert res.ticks[s] == n_intervals << levels
    print("n, massive, steps, reference steps, pos, vel, reference rounded against unrounded:", worst)


# ---- 5. invariances ---------------------------------------------------------------------------------------------------------
def test_a_system_is_independent_of_slot_batch_size_capacity_and_neighbours_bit_for_bit():
    n, m = 60, 8
    P1, V1 = clusters([n], n, seed0=41)
    row = varied(2)[1]
    dt_max = F32(1.0 / 32.0)
    results = []
    for B, cap, slot in ((1, 60, 0), (3, 64, 0), (4, 300, 3), (2, 1000, 1)):
        counts = [min(cap, 33 + 61 * s) for s in range(B)]
        P, V = clusters(counts, cap, seed0=90 + B)
        counts[slot] = n
        P[slot], V[slot] = 0.0, 0.0
        P[slot, :n], V[slot, :n] = P1[0], V1[0]
        field = varied(B)[::-1].copy()
        field[slot] = row
        massive = [3 * s for s in range(B)]
        massive[slot] = m
        p, v, res = evolve(P, V, counts, 2, dt_max, 1e-2, field=field, massive=massive, levels=8)
        results.append((p[slot, :n].copy(), v[slot, :n].copy(), int(res.steps[slot]), int(res.max_level[slot])))
    for p, v, steps, level in results[1:]:
        assert (steps, level) == results[0][2:]
        assert same_bits(p, results[0][0]) and same_bits(v, results[0][1])


def test_the_launch_budget_the_split_into_calls_and_running_out_of_steps_change_no_bit():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    counts = [5, 60, 100, 128]
    massive = [0, 1, 100, 8]
    P, V = clusters(counts, 128, seed0=55)
    field = varied(4)
    dt_max, kw = F32(1.0 / 32.0), dict(levels=8)
    whole = evolve(P, V, counts, 8, dt_max, 0.0, field=field, massive=massive, **kw)
    assert whole[2].steps.min() >= 8 and whole[2].steps.max() > whole[2].steps.min() + 1
    for launch_steps in (1, 7, 1000):
        got = evolve(P, V, counts, 8, dt_max, 0.0, field=field, massive=massive, launch_steps=launch_steps, **kw)
        assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]) and np.array_equal(got[2].steps, whole[2].steps)
    split = evolve(P, V, counts, 8, dt_max, 0.0, field=field, massive=massive, chunks=[2, 5, 1], **kw)
    assert same_bits(split[0], whole[0]) and same_bits(split[1], whole[1])
    budget = int(whole[2].steps.min()) + 1
    with nb.BatchedSystem(4, 128, counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_massive_counts(massive)
        b.set_external_field(field)
        with pytest.raises(nb.NBodyError) as err:
            b.evolve(8, dt_max, softening=0.0, max_steps=budget, **kw)
        assert err.value.status == _lib.NBODY_ERR_STATE and "unfinished after max_steps" in str(err.value)
        st = b.evolve_stats()
        assert (st.steps == budget).any() and (st.ticks < 8 << 8).any()
        res = b.evolve(8, dt_max, softening=0.0, **kw)
        assert np.array_equal(res.ticks, [8 << 8] * 4) and np.array_equal(res.steps + st.steps, whole[2].steps)
        p, v = b.download()
    assert same_bits(p, whole[0]) and same_bits(v, whole[1])


# ---- 6. the setter ----------------------------------------------------------------------------------------------------------
def test_the_setter_forgets_the_caches_none_restores_the_run_without_a_field_and_idle_slots_are_untouched():
    import n_body_problem_amd as nb
    counts = [0, 60, 5, 64]
    P, V = clusters(counts, 64, seed0=66, fill=np.nan)
    P[0, :4], V[0, :4] = 3.0, 1.0                                  # a system with count 0: contents that a step would move
    field = varied(4)
    dt_max = F32(1.0 / 64.0)
    fresh_on = evolve(P, V, counts, 3, dt_max, 1e-2, field=field, levels=6)
    fresh_off = evolve(P, V, counts, 3, dt_max, 1e-2, levels=6)
    for s, n in enumerate(counts):
        assert same_bits(fresh_on[0][s, n:], P[s, n:]) and same_bits(fresh_on[1][s, n:], V[s, n:]), s
        assert np.isfinite(fresh_on[0][s, :n]).all() and np.isfinite(fresh_on[1][s, :n]).all()
    assert fresh_on[2].steps[0] == 0
    assert not same_bits(fresh_on[0][1, :60], fresh_off[0][1, :60])
    with nb.BatchedSystem(4, 64, counts=counts, integrator="hermite") as b:
        assert b.external_field() is None and not b.field_potential().any()
        b.set_state(P, V)
        b.evolve(5, dt_max, softening=1e-2, levels=6)              # without a field: leaves caches and a level behind
        b.positions.copy_(b.positions.new_tensor(P))
        b.velocities.copy_(b.velocities.new_tensor(V))
        b.set_external_field(field)                                # ... which the setter forgets, as a new state would
        got = b.external_field()
        assert got.shape == (4, 4, 4) and np.array_equal(got, field.astype(np.float32))
        res = b.evolve(3, dt_max, softening=1e-2, levels=6)
        p, v = b.download()
        assert same_bits(p, fresh_on[0]) and same_bits(v, fresh_on[1]) and np.array_equal(res.steps, fresh_on[2].steps)
        b.positions.copy_(b.positions.new_tensor(P))
        b.velocities.copy_(b.velocities.new_tensor(V))
        b.set_external_field(None)                                 # NULL forgets too, and the run is the one without a field
        assert b.external_field() is None
        res = b.evolve(3, dt_max, softening=1e-2, levels=6)
        p, v = b.download()
        assert same_bits(p, fresh_off[0]) and same_bits(v, fresh_off[1]) and np.array_equal(res.steps, fresh_off[2].steps)
        b.set_external_field(GALAXY)                               # named components go to every system; set_state keeps them
        b.set_state(P, V)
        assert np.array_equal(b.external_field(), as_array(GALAXY, 4).astype(np.float32))
        b.set_counts(counts)
        assert np.array_equal(b.external_field(), as_array(GALAXY, 4).astype(np.float32))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_fixed_steps_conditions_and_invalid_components_are_refused_and_change_nothing():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    counts = [60, 33]
    P, V = clusters(counts, 64, seed0=77)
    dt_max = F32(1.0 / 64.0)

    def refused(call, *words):
        with pytest.raises(nb.NBodyError) as err:
            call()
        assert err.value.status == _lib.NBODY_ERR_INVALID, str(err.value)
        for word in words:
            assert word in str(err.value), (word, str(err.value))
        p, v = b.download()
        assert same_bits(p, P) and same_bits(v, V)                 # nothing ran

    for integrator in ("kick_drift", "kdk", "hermite"):
        with nb.BatchedSystem(2, 64, counts=counts, integrator=integrator) as b:
            b.set_state(P, V)
            b.set_external_field(GALAXY)
            refused(lambda: b.step_n(2, dt_max, 1e-2), "nbody_batch_step_n", "external field", "levels = 0")
            if integrator != "hermite":
                refused(lambda: b.evolve(1, dt_max, softening=1e-2), "NBODY_INTEGRATOR_HERMITE")
            b.set_external_field(None)
            b.step_n(1, dt_max, 1e-2)                              # off again: fixed steps run
            assert not same_bits(b.download()[0], P)
    with nb.BatchedSystem(2, 64, counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_external_field(GALAXY)
        go = lambda: b.evolve(1, dt_max, softening=1e-2, levels=4)  # noqa: E731
        message = ("external field is set together with",)
        b.set_stop_conditions(collision_radius=1e-3)
        refused(go, *message)
        b.set_stop_conditions(escape_radius=50.0)
        refused(go, *message)
        b.set_stop_conditions()
        b.set_radii(np.full((2, 64), 1e-4, np.float32))
        refused(go, *message)
        b.set_collision_action("merge")
        refused(go, *message)                                      # merge, acting through the radii
        b.set_radii(None)
        b.set_stop_conditions(collision_radius=1e-3)
        refused(go, *message)                                      # merge, acting through the collision radius
        b.set_collision_action("stop")
        b.set_massive_counts([8, 8])
        b.set_tracer_action("remove")
        refused(go, *message)                                      # tracer remove, where it would act
        b.set_tracer_action("refuse")
        refused(go, "massive counts are set together with")        # the older refusal comes first
        b.set_stop_conditions()
        b.set_tracer_action("remove")                              # remove without a condition acts nowhere: the field runs
        res = b.evolve(1, dt_max, softening=1e-2, levels=4)
        assert res.steps.min() >= 1 and not same_bits(b.download()[0], P)
    with nb.BatchedSystem(2, 64, counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_external_field(GALAXY)
        good = b.external_field()
        bad = as_array(GALAXY, 2)
        for system, comp, column, value, words in ((1, 0, 1, -1.0, ("PLUMMER", "mass")), (0, 0, 2, 1e-10, ("NBODY_MIN_SOFTENING",)),
                                                   (1, 2, 2, 0.0, ("LOG_HALO", "rc")), (0, 2, 3, float("nan"), ("LOG_HALO", "q")),
                                                   (1, 1, 3, 0.0, ("MIYAMOTO_NAGAI", "scale height")),
                                                   (0, 1, 1, float("inf"), ("MIYAMOTO_NAGAI", "mass")),
                                                   (1, 2, 0, 7.0, ("unknown kind",))):
            field = bad.copy()
            field[system, comp, column] = value
            refused(lambda: b.set_external_field(field), "nbody_batch_field_set", f"system {system}", f"component {comp}", *words)
            assert np.array_equal(b.external_field(), good)
        refused(lambda: b.set_external_field(np.zeros((2, 5, 4))), "n_components (5)")
        with pytest.raises(ValueError):
            b.set_external_field(np.zeros((3, 2, 4)))
        with pytest.raises(ValueError):
            b.set_external_field([("hernquist", 1.0, 1.0, 0.0)])
        assert np.array_equal(b.external_field(), good)
        want = evolve(P, V, counts, 1, dt_max, 1e-2, field=GALAXY, levels=4)
        b.evolve(1, dt_max, softening=1e-2, levels=4)              # after all the refusals: the run of a fresh handle
        p, v = b.download()
        assert same_bits(p, want[0]) and same_bits(v, want[1])


# ---- 8. an eccentric orbit in the halo --------------------------------------------------------------------------------------
def test_a_tracer_on_an_eccentric_orbit_in_the_halo_keeps_its_energy_and_the_reference_step_count():
    """hermite_field_ref's orbit (test_batch_field_cpu.py holds the scheme to 1e-5 on it): massive count 0, eta = 0.01."""
    import n_body_problem_amd as nb
    P, V = fref.ORBIT_POS[None].astype(np.float32), fref.ORBIT_VEL[None].astype(np.float32)
    ref = fref.evolve(P[0], V[0], fref.ORBIT_INTERVALS, fref.ORBIT_DT_MAX, levels=fref.ORBIT_LEVELS, eta=F32(fref.ORBIT_ETA),
                      eta_start=F32(fref.ORBIT_ETA), components=fref.HALO, massive=0, round_state=True)

    def specific_energy(b):
        v = b.download()[1][0, 0, :3].astype(np.float64)
        return 0.5 * float(v @ v) + float(b.field_potential()[0, 0])

    with nb.BatchedSystem(1, 1, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_massive_counts([0])
        b.set_external_field(fref.HALO)
        e0 = specific_energy(b)
        res = b.evolve(fref.ORBIT_INTERVALS, fref.ORBIT_DT_MAX, levels=fref.ORBIT_LEVELS, eta=fref.ORBIT_ETA,
                       eta_start=fref.ORBIT_ETA, softening=0.0)
        e1 = specific_energy(b)
    steps, de = int(res.steps[0]), abs(e1 / e0 - 1.0)
    print(f"steps {steps} (reference {ref.steps}) levels {res.min_level[0]}..{res.max_level[0]} E {e0:.6f} dE/E {de:.3g}")
    assert abs(e0 - fref.specific_energy(P[0], V[0], fref.HALO)[0]) < 1e-12
    assert res.ticks[0] == fref.ORBIT_INTERVALS << fref.ORBIT_LEVELS and res.clamped[0] == 0
    assert abs(steps - ref.steps) <= 0.05 * ref.steps, (steps, ref.steps)
    assert de <= 1e-4, de


# ---- 9. the potential -------------------------------------------------------------------------------------------------------
def test_the_potential_is_the_fp64_formula_and_zero_beyond_the_counts():
    import n_body_problem_amd as nb
    counts = [0, 5, 257, 300]
    P, V = clusters(counts, 300, seed0=99, fill=np.nan)
    P[2, 0, :3] = 0.0                                              # a body at the centre: the bulge with b = 0 counts 0 there
    # one logarithm alone; the two negative terms; all three with a halo too weak to cancel them anywhere (a sum that crosses
    # zero has no relative error to speak of)
    field = np.zeros((4, 3, 4))
    field[0] = field[1] = as_array([HALO, ("none", 0, 0, 0), ("none", 0, 0, 0)], 1)[0]
    field[2] = as_array([("plummer", 0.3, 0.0, 0.0), ("none", 1, 1, 1), DISC], 1)[0]
    field[3] = as_array([BULGE, DISC, ("log_halo", 0.1, 1.0, 0.9)], 1)[0]
    with nb.BatchedSystem(4, 300, counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_external_field(field)
        phi = b.field_potential()
        energy = b.field_energy()
    assert phi.shape == (4, 300) and phi.dtype == np.float64 and energy.shape == (4,)
    for s, n in enumerate(counts):
        assert not phi[s, n:].any()
        want = fref.potential(P[s, :n, :3].astype(np.float64), named(field[s]))
        assert np.all(np.abs(phi[s, :n] - want) <= 1e-12 * np.abs(want)), (s, np.abs(phi[s, :n] / want - 1.0).max())
        assert abs(energy[s] - float((P[s, :n, 3].astype(np.float64) * want).sum())) <= 1e-12 * max(1.0, abs(energy[s]))
    assert np.isfinite(phi).all() and phi[3, :300].min() < 0.0
