"""GPU: test particles for batched ensembles (BatchedSystem.set_massive_counts, include/nbody_batch_massive.h).  With
massive counts set the first m bodies of a system are massive and the rest feel them and exert nothing.  Checked bit for bit
against code that exists without the feature: the same state with the tracers' mass words zero (a zero-mass column adds
fma(d, +0, a), which leaves a as it is) and the massive bodies alone; against the fp64 Hermite reference; at the edges
(m = 0, m = n, m > n, off again, a change between calls); through evolve with everything nbody_batch_evolve.h promises; for
the batch's invariances; and for what is refused.

Shapes: every workgroup shape (capacity 64: one row per lane, 128: two, 1024 and 4096: four in groups of two) and the
(n, m) pairs of PAIRS where they fit.  Two steps per run."""
import numpy as np
import pytest

import hermite_ref
from hermite_ref import rel_state_error

pytestmark = pytest.mark.gpu

F32 = lambda x: float(np.float32(x))  # noqa: E731
DT, STEPS = 1e-3, 2
INTEGRATORS = ("kick_drift", "kdk", "hermite")
#: (n, m, where the massive bodies come from); unsoftened runs are compared for the Plummer systems only
PAIRS = [(1, 0, "plummer"), (1, 1, "plummer"), (2, 1, "plummer"), (3, 2, "cube"), (64, 1, "plummer"), (65, 64, "plummer"),
         (65, 65, "cube"), (130, 63, "plummer"), (257, 2, "cube"), (257, 129, "plummer"), (1000, 8, "cube"),
         (1000, 1000, "plummer"), (4096, 3, "plummer")]
CAPACITIES = (64, 128, 1024, 4096)
MIN_SEPARATION = 1e-3


def pairs_of(cap):
    return [q for q in PAIRS if q[0] == 4096] if cap == 4096 else [q for q in PAIRS if q[0] <= cap]


def min_separation(x):
    """The smallest distance between two of the points x (k, 3), fp64 from the fp32 values."""
    x = np.asarray(x, np.float64)
    best = np.inf
    for lo in range(0, len(x) - 1, 256):
        d = x[None, lo + 1:, :] - x[lo:lo + 256, None, :]
        r2 = np.einsum("ijk,ijk->ij", d, d)
        r2[np.tril_indices(r2.shape[0], -1, r2.shape[1])] = np.inf      # column lo + 1 + j against row lo + i: j >= i only
        best = min(best, float(r2.min()))
    return np.sqrt(best)


def tracers(k, seed, mass_word=1.0):
    """k tracers at seeded positions in [-2, 2]^3 with speeds up to 0.1, mass word 1.0 and a fourth velocity word to keep."""
    rng = np.random.default_rng(seed)
    p = np.zeros((k, 4), np.float32)
    v = np.zeros((k, 4), np.float32)
    p[:, :3] = rng.uniform(-2.0, 2.0, (k, 3))
    v[:, :3] = rng.uniform(-0.1, 0.1, (k, 3))
    p[:, 3] = mass_word
    v[:, 3] = 7.0
    if k > 1:
        assert min_separation(p[:, :3]) >= MIN_SEPARATION
    return p, v


def system(n, m, kind, seed):
    """(n, 4) positions and velocities: m massive bodies, then n - m tracers with mass word 1.0."""
    import n_body_problem_amd as nb
    p = np.zeros((n, 4), np.float32)
    v = np.zeros((n, 4), np.float32)
    if m:
        p[:m], v[:m] = nb.plummer(m, seed=seed) if kind == "plummer" else nb.uniform_cube(m, seed=seed, random_masses=True, speed=0.1)
        v[:m, 3] = 5.0
    p[m:], v[m:] = tracers(n - m, seed + 1)
    return p, v


_CASES = {}


def case(cap):
    """The batch of a capacity: positions, velocities, counts, massive counts, kinds."""
    if cap not in _CASES:
        pairs = pairs_of(cap)
        P = np.zeros((len(pairs), cap, 4), np.float32)
        V = np.zeros_like(P)
        for s, (n, m, kind) in enumerate(pairs):
            P[s, :n], V[s, :n] = system(n, m, kind, 500 + 10 * s)
        _CASES[cap] = (P, V, [q[0] for q in pairs], [q[1] for q in pairs], [q[2] for q in pairs])
    return _CASES[cap]


def zero_tracer_masses(P, massive):
    Z = P.copy()
    for s, m in enumerate(massive):
        Z[s, m:, 3] = 0.0
    return Z


def step(P, V, counts, integrator, eps, massive=None, k=STEPS, dt=DT):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator=integrator) as b:
        b.set_state(P, V)
        if massive is not None:
            b.set_massive_counts(massive)
        b.step_n(k, dt, eps)
        return b.download()


_RUNS = {}


def runs(cap, integrator, eps):
    """Computed once per (capacity, integrator, softening): the run under test (massive counts set, mass words 1.0), the
    feature-off run with the tracers' mass words zero, and the feature-off run of the massive bodies alone."""
    key = (cap, integrator, eps)
    if key not in _RUNS:
        P, V, counts, massive, _ = case(cap)
        on = step(P, V, counts, integrator, eps, massive)
        off = step(zero_tracer_masses(P, massive), V, counts, integrator, eps)
        alone = step(P, V, massive, integrator, eps)
        _RUNS[key] = (on, off, alone)
    return _RUNS[key]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("cap", CAPACITIES)
def test_massive_counts_equal_zero_mass_words_bit_for_bit_and_keep_the_fourth_words(cap, integrator):
    P, V, counts, massive, kinds = case(cap)
    for eps in (1e-2, 0.0):
        (p, v), (p0, v0), _ = runs(cap, integrator, eps)
        for s, (n, m, kind) in enumerate(zip(counts, massive, kinds)):
            assert same_bits(p[s, :n, 3], P[s, :n, 3]) and same_bits(v[s, :n, 3], V[s, :n, 3]), (n, m, eps)
            assert same_bits(p[s, n:], P[s, n:]) and same_bits(v[s, n:], V[s, n:]), (n, m, eps)
            if eps == 0.0 and kind != "plummer":
                continue
            assert np.isfinite(p0[s, :n]).all() and np.isfinite(v0[s, :n]).all(), (n, m, eps)
            assert same_bits(p[s, :n, :3], p0[s, :n, :3]) and same_bits(v[s, :n, :3], v0[s, :n, :3]), (n, m, eps)
            if m < n:  # the bodies have moved: the comparison is not one of untouched states
                assert not same_bits(p[s, m:n, :3], P[s, m:n, :3])


@pytest.mark.parametrize("integrator", INTEGRATORS)
@pytest.mark.parametrize("cap", CAPACITIES)
def test_tracers_change_no_bit_of_the_massive_bodies(cap, integrator):
    _, _, counts, massive, _ = case(cap)
    for eps in (1e-2, 0.0):
        (p, v), _, (pa, va) = runs(cap, integrator, eps)
        for s, m in enumerate(massive):
            assert same_bits(p[s, :m], pa[s, :m]) and same_bits(v[s, :m], va[s, :m]), (counts[s], m, eps)


@pytest.mark.parametrize("cap", CAPACITIES)
def test_two_hermite_steps_match_the_fp64_reference_with_massless_tracers(cap):
    P, V, counts, massive, kinds = case(cap)
    Z = zero_tracer_masses(P, massive)
    worst = []
    # 4096 bodies cost the reference seconds per run: unsoftened only there, the guarded kernel of the same shape as 1024's
    for eps in ((1e-2, 0.0) if cap < 4096 else (0.0,)):
        (p, v), _, _ = runs(cap, "hermite", eps)
        for s, (n, m, kind) in enumerate(zip(counts, massive, kinds)):
            if eps == 0.0 and kind != "plummer":
                continue
            pr, vr = hermite_ref.step(Z[s, :n], V[s, :n], DT, eps, nsteps=STEPS)
            ep, ev = rel_state_error(p[s, :n], pr), rel_state_error(v[s, :n], vr)
            worst.append((n, m, eps, ep, ev))
            assert ep < 1e-5 and ev < 1e-5, (n, m, eps, ep, ev)
    print("n, m, eps, pos, vel:", worst)


def straight_line(P, V, k, dt):
    """x <- (float)((double)x + (double)v (double)dt) per step: what every integrator's update gives for a = j = 0 (the
    product of two fp32 values is exact in fp64, so the fp64 sum is the fused one)."""
    x = P[..., :3].copy()
    h = np.float64(np.float32(dt))
    for _ in range(k):
        x = (x.astype(np.float64) + V[..., :3].astype(np.float64) * h).astype(np.float32)
    return x


def test_without_massive_bodies_every_body_moves_on_its_rounded_straight_line():
    counts = [1, 65, 300, 40]
    massive = [0, 0, 0, 40]
    P = np.zeros((4, 512, 4), np.float32)
    V = np.zeros_like(P)
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = tracers(n, 40 + s)
    P[3, :40], V[3, :40] = system(40, 40, "plummer", 44)
    for integrator in INTEGRATORS:
        for eps in (1e-2, 0.0):
            p, v = step(P, V, counts, integrator, eps, massive, k=3)
            want = straight_line(P, V, 3, DT)
            for s, n in enumerate(counts[:3]):
                assert same_bits(p[s, :n, :3], want[s, :n]) and same_bits(v[s, :n], V[s, :n]), (integrator, eps, n)
                assert same_bits(p[s, :n, 3], P[s, :n, 3])
            assert not same_bits(v[3, :40, :3], V[3, :40, :3])
    import n_body_problem_amd as nb
    with nb.BatchedSystem(4, 512, counts=counts, integrator="hermite") as b:   # evolve: both criteria are 0 / 0, level 0
        b.set_state(P, V)
        b.set_massive_counts(massive)
        res = b.evolve(3, F32(DT), levels=6, softening=0.0)
        p, v = b.download()
    assert res.steps[:3].tolist() == [3, 3, 3] and res.max_level[:3].tolist() == [0, 0, 0] and res.ticks.tolist() == [3 << 6] * 4
    for s, n in enumerate(counts[:3]):
        assert same_bits(p[s, :n, :3], want[s, :n]) and same_bits(v[s, :n], V[s, :n])


@pytest.mark.parametrize("integrator", INTEGRATORS)
def test_all_bodies_massive_more_than_all_and_off_again_are_the_run_without_the_feature(integrator):
    import n_body_problem_amd as nb
    P, V, counts, _, _ = case(128)
    B = len(counts)
    eps = 1e-2
    want = step(P, V, counts, integrator, eps)
    for massive in (counts, [128] * B, [min(n + 1, 128) for n in counts]):
        got = step(P, V, counts, integrator, eps, massive)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), massive
    with nb.BatchedSystem(B, 128, counts=counts, integrator=integrator) as b:
        assert b.massive_counts is None
        b.set_massive_counts([1] * B)
        assert b.massive_counts.tolist() == [1] * B
        b.set_state(P, V)                                  # the values belong to the handle: a new state keeps them
        b.set_counts(counts)
        assert b.massive_counts.tolist() == [1] * B
        b.step_n(STEPS, DT, eps)
        ones = b.download()
        b.set_massive_counts(None)
        assert b.massive_counts is None
        b.set_state(P, V)
        b.step_n(STEPS, DT, eps)
        off = b.download()
    assert same_bits(off[0], want[0]) and same_bits(off[1], want[1])
    assert not same_bits(ones[0], want[0])
    kept = step(P, V, counts, integrator, eps, [1] * B)
    assert same_bits(ones[0], kept[0]) and same_bits(ones[1], kept[1])


@pytest.mark.parametrize("integrator", ("kdk", "hermite"))
def test_new_massive_counts_between_two_calls_drop_the_caches(integrator):
    import n_body_problem_amd as nb
    P, V, counts, massive, _ = case(128)
    B = len(counts)
    eps = 1e-2
    for second in ([min(1, n) for n in counts], None):
        with nb.BatchedSystem(B, 128, counts=counts, integrator=integrator) as b:
            b.set_state(P, V)
            b.set_massive_counts(massive)
            b.step_n(STEPS, DT, eps)
            mid = b.download()
            b.set_massive_counts(second)                   # the cached accelerations (and jerks) are those of the old columns
            b.step_n(STEPS, DT, eps)
            got = b.download()
        want = step(mid[0], mid[1], counts, integrator, eps, second)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), second
        stale = step(mid[0], mid[1], counts, integrator, eps, massive)
        assert not same_bits(got[1], stale[1])


def evolve_case():
    """System 0: a star, a planet on an e = 0.9 orbit and 60 tracers; system 1: an e = 0.5 pair of unequal masses and 255
    tracers."""
    P = np.zeros((2, 512, 4), np.float32)
    V = np.zeros_like(P)
    pos, vel, period = hermite_ref.kepler(e=0.9, masses=(0.999, 0.001))
    P[0, :2], V[0, :2] = pos, vel
    P[0, 2:62], V[0, 2:62] = tracers(60, 71)
    pos, vel, _ = hermite_ref.kepler(e=0.5, masses=(0.75, 0.25))
    P[1, :2], V[1, :2] = pos, vel
    P[1, 2:257], V[1, 2:257] = tracers(255, 72)
    return P, V, [62, 257], [2, 2], F32(period / 64)


def evolve(P, V, counts, massive, dt_max, eps, chunks=(4,), launch_steps=None, max_steps=0):
    """(positions, velocities, the last call's figures, calls that ran out of steps) of a fresh Hermite batch."""
    import n_body_problem_amd as nb
    interrupted = 0
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        if massive is not None:
            b.set_massive_counts(massive)
        if launch_steps:
            b.set_evolve_launch_steps(launch_steps)
        for c in chunks:
            for attempt in range(3):
                try:
                    res = b.evolve(c, dt_max, levels=12, softening=eps, max_steps=max_steps)
                    break
                except nb.NBodyError as e:
                    assert e.status == -5 and max_steps > 0, e
                    interrupted += 1
            else:
                raise AssertionError("three calls did not finish the interval")
        p, v = b.download()
    return p, v, res, interrupted


def figures(res):
    return [x.tolist() for x in (res.steps, res.min_level, res.max_level, res.clamped, res.ticks)]


@pytest.mark.parametrize("eps", [0.0, 1e-2])
def test_evolve_equals_the_zero_mass_run_and_keeps_its_promises(eps):
    P, V, counts, massive, dt_max = evolve_case()
    p0, v0, res0, _ = evolve(zero_tracer_masses(P, massive), V, counts, None, dt_max, eps)
    assert np.isfinite(p0).all() and np.isfinite(v0).all()
    p, v, res, _ = evolve(P, V, counts, massive, dt_max, eps)
    print("steps", res.steps, "levels", res.min_level, res.max_level)
    assert figures(res) == figures(res0) and res.ticks.tolist() == [4 << 12] * 2 and res.steps.min() > 4
    for s, n in enumerate(counts):
        assert same_bits(p[s, :n, :3], p0[s, :n, :3]) and same_bits(v[s, :n, :3], v0[s, :n, :3])
        assert same_bits(p[s, :n, 3], P[s, :n, 3]) and same_bits(v[s, :n, 3], V[s, :n, 3])
    # the launch budget
    q, w, r, _ = evolve(P, V, counts, massive, dt_max, eps, launch_steps=1)
    assert same_bits(q, p) and same_bits(w, v) and figures(r) == figures(res)
    # evolve(2) twice is evolve(4)
    q, w, r, _ = evolve(P, V, counts, massive, dt_max, eps, chunks=(2, 2))
    assert same_bits(q, p) and same_bits(w, v) and r.ticks.tolist() == [2 << 12] * 2
    # out of steps, and the same call again
    half = int(res.steps.max()) // 2 + 1
    q, w, r, interrupted = evolve(P, V, counts, massive, dt_max, eps, max_steps=half)
    assert interrupted == 1
    assert same_bits(q, p) and same_bits(w, v) and r.ticks.tolist() == [4 << 12] * 2


def test_a_system_is_independent_of_slot_batch_size_capacity_and_neighbours_bit_for_bit():
    import n_body_problem_amd as nb
    n, m = 257, 129
    p0, v0 = system(n, m, "plummer", 900)
    results = []
    for B, cap, slot, other in ((1, n, 0, (0, 0)), (3, 1024, 0, (500, 7)), (5, 4096, 3, (4096, 4096)), (2, 2048, 1, (7, 0))):
        counts = [other[0] if s != slot else n for s in range(B)]
        massive = [other[1] if s != slot else m for s in range(B)]
        P = np.zeros((B, cap, 4), np.float32)
        V = np.zeros_like(P)
        for s in range(B):
            if counts[s]:
                P[s, :counts[s]], V[s, :counts[s]] = nb.uniform_cube(counts[s], seed=1000 * B + s, random_masses=True, speed=0.1)
        P[slot, :n], V[slot, :n] = p0, v0
        p, v = step(P, V, counts, "hermite", 1e-3, massive, k=3)
        with nb.BatchedSystem(B, cap, counts=counts, integrator="hermite") as b:
            b.set_state(P, V)
            b.set_massive_counts(massive)
            res = b.evolve(2, F32(1e-3), levels=6, softening=1e-3)
            pe, ve = b.download()
        results.append((p[slot, :n].copy(), v[slot, :n].copy(), pe[slot, :n].copy(), ve[slot, :n].copy(), int(res.steps[slot])))
    for got in results[1:]:
        assert got[4] == results[0][4]
        for x, y in zip(got[:4], results[0][:4]):
            assert same_bits(x, y)


def test_evolve_refuses_massive_counts_with_stops_or_radii_and_bad_values_are_refused():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    P, V, counts, massive, dt_max = evolve_case()
    with nb.BatchedSystem(2, 512, counts=counts, integrator="hermite") as b:
        b.set_state(P, V)
        b.set_massive_counts(massive)
        settings = ((lambda: b.set_stop_conditions(collision_radius=1e-4), lambda: b.set_stop_conditions()),
                    (lambda: b.set_stop_conditions(escape_radius=100.0), lambda: b.set_stop_conditions()),
                    (lambda: b.set_radii(np.full((2, 512), 1e-5, np.float32)), lambda: b.set_radii(None)))
        for switch_on, switch_off in settings:
            switch_on()
            with pytest.raises(nb.NBodyError) as err:
                b.evolve(1, dt_max, softening=0.0)
            assert err.value.status == _lib.NBODY_ERR_INVALID and "massive counts" in str(err.value)
            p, v = b.download()
            assert same_bits(p, P) and same_bits(v, V)
            b.set_massive_counts(None)
            b.evolve(1, dt_max, softening=0.0)             # the same call goes through without massive counts
            b.set_state(P, V)
            switch_off()
            b.set_massive_counts(massive)
        b.evolve(1, dt_max, softening=0.0)                 # and with them once the conditions are off
        for bad in ([-1, 2], [2, 513]):
            with pytest.raises(nb.NBodyError) as err:
                b.set_massive_counts(bad)
            bad_system = 0 if bad[0] < 0 else 1
            assert err.value.status == _lib.NBODY_ERR_INVALID
            assert f"nbody_batch_massive_set: massive count of system {bad_system} ({bad[bad_system]})" in str(err.value)
            assert b.massive_counts.tolist() == massive    # a refused call changes nothing
        for wrong in ([2], [2, 2, 2]):
            with pytest.raises(ValueError):
                b.set_massive_counts(wrong)
