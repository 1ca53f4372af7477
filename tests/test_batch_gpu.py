"""GPU: batched ensembles (n_body_problem_amd.BatchedSystem, nbody_batch_*) against the CPU oracle, system by system, and
the invariances that make a system's result a function of that system alone."""
import ctypes

import numpy as np
import pytest

from conftest import rel_state_error

pytestmark = pytest.mark.gpu

MIXED_COUNTS = [1, 2, 63, 64, 65, 257, 1000, 4096]


def make_system(n, seed, kind):
    import n_body_problem_amd as nb
    if kind == "plummer":
        return nb.plummer(n, seed=seed)
    return nb.uniform_cube(n, seed=seed, random_masses=True, speed=0.1)


def mixed_batch(counts, max_bodies, seed0=100, fill=0.0):
    """(B, max_bodies, 4) arrays: system s = a Plummer sphere (even s) or a random-mass cube (odd s) of counts[s] bodies,
    slots beyond the count set to `fill`; and the list of the per-system (pos, vel)."""
    B = len(counts)
    P = np.full((B, max_bodies, 4), fill, dtype=np.float32)
    V = np.full((B, max_bodies, 4), fill, dtype=np.float32)
    systems = []
    for s, n in enumerate(counts):
        p, v = make_system(n, seed0 + s, "plummer" if s % 2 == 0 else "cube") if n else (np.zeros((0, 4), np.float32),) * 2
        P[s, :n], V[s, :n] = p, v
        systems.append((p, v))
    return P, V, systems


def run_batch(P, V, counts, k, dt, eps, integrator="kick_drift", max_bodies=None):
    import n_body_problem_amd as nb
    B = P.shape[0]
    max_bodies = max_bodies or P.shape[1]
    Pf = np.zeros((B, max_bodies, 4), np.float32)
    Vf = np.zeros((B, max_bodies, 4), np.float32)
    m = min(max_bodies, P.shape[1])
    Pf[:, :m], Vf[:, :m] = P[:, :m], V[:, :m]
    with nb.BatchedSystem(B, max_bodies, counts=counts, integrator=integrator) as b:
        b.set_state(Pf, Vf)
        b.step_n(k, dt, eps)
        return b.download()


@pytest.mark.parametrize("eps", [1e-3, 0.0])
def test_accelerations_match_the_fp64_oracle_per_system(oracle_mod, eps):
    P, V, systems = mixed_batch(MIXED_COUNTS, 4096)
    p, v = run_batch(P, np.zeros_like(V), MIXED_COUNTS, 1, 1.0, eps)   # v = 0, dt = 1: the velocities now hold a
    for s, n in enumerate(MIXED_COUNTS):
        acc = v[s, :n, :3].astype(np.float64)
        if n == 1:
            assert np.all(acc == 0.0)
            continue
        a64 = oracle_mod.accel_f64(systems[s][0], eps=eps)
        err = np.linalg.norm(acc - a64) / np.linalg.norm(a64)
        assert err < 1e-5, (n, eps, err)


@pytest.mark.parametrize("integrator", ["kick_drift", "kdk"])
def test_state_after_two_steps_matches_the_fp32_oracle(oracle_mod, integrator):
    dt, eps = 1e-3, 1e-3
    P, V, systems = mixed_batch(MIXED_COUNTS, 4096, seed0=300)
    p, v = run_batch(P, V, MIXED_COUNTS, 2, dt, eps, integrator)
    step = oracle_mod.step_f32 if integrator == "kick_drift" else oracle_mod.step_kdk_f32
    for s, n in enumerate(MIXED_COUNTS):
        pr, vr = step(*systems[s], dt, eps, nsteps=2)
        assert np.array_equal(p[s, :n, 3], pr[:, 3]) and np.array_equal(v[s, :n, 3], vr[:, 3])
        if n == 1:   # a lone body drifts exactly
            assert np.array_equal(p[s, :n], pr) and np.array_equal(v[s, :n], vr)
            continue
        assert rel_state_error(p[s, :n], pr) < 1e-6 and rel_state_error(v[s, :n], vr) < 1e-6, (integrator, n)


@pytest.mark.parametrize("integrator", ["kick_drift", "kdk"])
def test_a_system_is_independent_of_slot_batch_size_capacity_and_neighbours_bit_for_bit(integrator):
    dt, eps, k = 1e-3, 1e-3, 3
    probes = [(60, "plummer"), (257, "cube"), (1000, "plummer")]
    for n, kind in probes:
        p0, v0 = make_system(n, 77, kind)
        results = []
        # (B, max_bodies, slot, seed of the neighbours, counts of the neighbours)
        for B, cap, slot, seed, other in ((1, n, 0, 0, 0), (3, 1024, 0, 1, 500), (5, 4096, 3, 2, 4096), (2, 2048, 1, 3, 7)):
            counts = [other if s != slot else n for s in range(B)]
            P, V, _ = mixed_batch(counts, cap, seed0=1000 * seed)
            P[slot, :n], V[slot, :n] = p0, v0
            p, v = run_batch(P, V, counts, k, dt, eps, integrator)
            results.append((p[slot, :n].copy(), v[slot, :n].copy()))
        for p, v in results[1:]:
            assert np.array_equal(p, results[0][0]) and np.array_equal(v, results[0][1]), (integrator, n)


def test_slots_beyond_the_count_are_never_touched_and_poison_nothing(oracle_mod):
    dt, eps = 1e-3, 1e-3
    counts = [0, 5, 64, 100, 700]
    P, V, systems = mixed_batch(counts, 1024, seed0=900, fill=np.nan)
    P[0, :10] = 3.0        # a system with count 0: contents that a step would move
    V[0, :10] = 1.0
    for integrator in ("kick_drift", "kdk"):
        p, v = run_batch(P, V, counts, 3, dt, eps, integrator)
        for s, n in enumerate(counts):
            assert np.array_equal(p[s, n:].view(np.uint32), P[s, n:].view(np.uint32))
            assert np.array_equal(v[s, n:].view(np.uint32), V[s, n:].view(np.uint32))
            if n:
                step = oracle_mod.step_f32 if integrator == "kick_drift" else oracle_mod.step_kdk_f32
                pr, vr = step(*systems[s], dt, eps, nsteps=3)
                assert np.isfinite(p[s, :n]).all() and rel_state_error(p[s, :n], pr) < 1e-6
                assert rel_state_error(v[s, :n], vr) < 1e-6


@pytest.mark.parametrize("integrator", ["kick_drift", "kdk"])
def test_k_fused_steps_equal_k_single_steps_and_set_state_invalidates(integrator):
    import n_body_problem_amd as nb
    dt, eps, k = 1e-3, 1e-2, 5
    counts = [64, 300, 1024, 17]
    P, V, _ = mixed_batch(counts, 1024, seed0=40)
    P2, V2, _ = mixed_batch(counts, 1024, seed0=41)
    with nb.BatchedSystem(len(counts), 1024, counts=counts, integrator=integrator) as b:
        b.set_state(P, V)
        b.step_n(k, dt, eps)
        fused = b.download()
        b.set_state(P, V)
        for _ in range(k):
            b.step_n(1, dt, eps)
        single = b.download()
        b.set_state(P2, V2)            # new contents: the cached accelerations of P's last step must not be used
        b.step_n(2, dt, eps)
        after = b.download()
    with nb.BatchedSystem(len(counts), 1024, counts=counts, integrator=integrator) as fresh:
        fresh.set_state(P2, V2)
        fresh.step_n(2, dt, eps)
        want = fresh.download()
    for x, y in zip(fused, single):
        assert np.array_equal(x, y)
    for x, y in zip(after, want):
        assert np.array_equal(x, y)


def test_long_calls_cut_into_launches_keep_the_bits():
    """k = 300 runs as launches of 128 + 128 + 44 steps; 300 single steps must give the same state (KDK: through the cache)."""
    import n_body_problem_amd as nb
    counts = [32, 64]
    P, V, _ = mixed_batch(counts, 64, seed0=5)
    for integrator in ("kick_drift", "kdk"):
        out = []
        for chunks in ([300], [1] * 300):
            with nb.BatchedSystem(2, 64, counts=counts, integrator=integrator) as b:
                b.set_state(P, V)
                for c in chunks:
                    b.step_n(c, 1e-3, 1e-2)
                out.append(b.download())
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), integrator


def test_per_system_energy_and_momentum_match_the_oracle(oracle_mod):
    import n_body_problem_amd as nb
    counts = [1, 63, 256, 1000, 4096, 0]
    P, V, systems = mixed_batch(counts, 4096, seed0=60)
    for eps in (1e-2, 0.0):
        with nb.BatchedSystem(len(counts), 4096, counts=counts) as b:
            b.set_state(P, V)
            e, mom = b.energy(eps), b.momentum()
        assert e.shape == (len(counts), 3) and mom.shape == (len(counts), 4)
        for s, n in enumerate(counts):
            if n == 0:
                assert np.all(e[s] == 0) and np.all(mom[s] == 0)
                continue
            er = oracle_mod.energy(*systems[s], eps)
            mr = oracle_mod.momentum(*systems[s])
            assert np.isclose(e[s, 0], er[0], rtol=1e-9, atol=1e-15)
            assert np.isclose(e[s, 1], er[1], rtol=1e-5, atol=1e-15), (n, eps, e[s], er)
            assert np.isclose(e[s, 2], e[s, 0] + e[s, 1], rtol=1e-12)
            scale = float(np.abs(systems[s][1][:, :3]).max() * systems[s][0][:, 3].sum())
            assert np.allclose(mom[s, :3], mr[:3], rtol=1e-9, atol=1e-9 * scale) and np.isclose(mom[s, 3], mr[3], rtol=1e-12)


def test_energy_conservation_per_system_tracks_the_oracle(oracle_mod):
    import n_body_problem_amd as nb
    B, n, steps, dt, eps = 16, 1024, 300, 1e-3, 1e-2
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    for s in range(B):
        P[s], V[s] = nb.plummer(n, seed=2000 + s)
    with nb.BatchedSystem(B, n) as b:
        b.set_state(P, V)
        e0 = b.energy(eps)[:, 2]
        b.step_n(steps, dt, eps)
        e1 = b.energy(eps)[:, 2]
    for s in range(B):
        pr, vr = oracle_mod.step_f32(P[s], V[s], dt, eps, nsteps=steps)
        r0, r1 = oracle_mod.energy(P[s], V[s], eps)[2], oracle_mod.energy(pr, vr, eps)[2]
        drift, ref = abs((e1[s] - e0[s]) / e0[s]), abs((r1 - r0) / r0)
        assert drift <= 3.0 * ref + 2e-6, (s, drift, ref)


def test_many_tiny_systems_at_scale(oracle_mod):
    import n_body_problem_amd as nb
    B, n, dt, eps = 16384, 64, 1e-3, 1e-3
    rng = np.random.default_rng(7)
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    P[:, :, :3] = rng.uniform(-1, 1, (B, n, 3))
    P[:, :, 3] = rng.uniform(0.5, 1.5, (B, n)) / n
    V[:, :, :3] = rng.uniform(-0.1, 0.1, (B, n, 3))
    with nb.BatchedSystem(B, n) as b:
        b.set_state(P, V)
        b.step_n(2, dt, eps)
        p, v = b.download()
    for s in (0, 1, 4095, 8192, 12345, B - 1):
        pr, vr = oracle_mod.step_f32(P[s], V[s], dt, eps, nsteps=2)
        assert rel_state_error(p[s], pr) < 1e-6 and rel_state_error(v[s], vr) < 1e-6, s


def test_handle_level_argument_errors_leave_the_state_alone():
    import torch
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    lib = _lib.load()
    with nb.BatchedSystem(3, 128) as b:
        P, V, _ = mixed_batch([128, 128, 128], 128)
        b.set_state(P, V)
        before = [t.clone() for t in (b.positions, b.velocities)]
        h, pp, vp = b._h, ctypes.c_void_p(b.positions.data_ptr()), ctypes.c_void_p(b.velocities.data_ptr())
        for args in ((pp, vp, -1, 1e-3, 1e-3), (pp, vp, 1, 1e-3, 1e-12), (pp, vp, 1, 1e-3, -1.0),
                     (pp, vp, 1, float("nan"), 1e-3), (pp, vp, 1, 1e-3, float("inf")), (None, vp, 1, 1e-3, 1e-3),
                     (pp, None, 1, 1e-3, 1e-3)):
            assert lib.nbody_batch_step_n_on(h, *args) == _lib.NBODY_ERR_INVALID, args
            assert lib.nbody_batch_last_error(h)
        for bad in ([129, 1, 1], [-1, 1, 1]):
            with pytest.raises(nb.NBodyError) as e:
                b.set_counts(bad)
            assert e.value.status == _lib.NBODY_ERR_INVALID
        assert list(b.counts) == [128, 128, 128]
        assert lib.nbody_batch_set_integrator(h, 7) == _lib.NBODY_ERR_INVALID
        out = (ctypes.c_double * 9)()
        assert lib.nbody_batch_energy(h, pp, vp, 1e-12, out) == _lib.NBODY_ERR_INVALID
        b.step_n(0, 1e-3, 1e-3)
        b.sync()
        assert all(torch.equal(x, y) for x, y in zip(before, (b.positions, b.velocities)))
