"""GPU: the radial profiles of batched ensembles (BatchedSystem.radial_profile, include/nbody_batch_radial.h).

1. Against the reference (hermite_radial_ref, Python floats in the pinned order) at capacities 64 (one wave, one row per
   lane), 128 (two rows per lane), 320 (four rows per lane, two waves) and 4096 (sixteen waves, the raised LDS limit), counts
   0, 1, 2, 65 and the capacity, 1, 8, 9 and 32 shells, shared and per-system edges, both weights, spherical shells and each
   projection axis, masks of none, sparse and all-false.  Exact: count, selected, below, above, unmeasured, shells, projected
   and every sum made of +, - and x alone (weight, total_weight, U, L, M, V), and every body's shell.  The inputs make s, rv
   and v2 exact and keep every squared edge away from every attainable s (test_batch_radial_cpu.py asserts both premises).
   The four sums that pass through the device's fp64 square root and division -- radius, vr1, vr2, vt2 -- are held to
       |got - ref| <= (members + 16) * 2^-52 * sum of w_i A_i,     A_i = r, |u|, v2, v2 of the reference,
   which allows one ulp each for the square root and the division, carried through the square, and the worst-case rounding
   of `members` running sums whose inputs differ by that much.  The worst observed ratio to the bound is printed per
   capacity, with whether the device was bit-equal.
   Observed on an MI355X: worst error / bound 0 at every capacity and case -- the device was bit-equal to the reference, these
   four sums and the body records included.  The bound stays.
2. Placement: a system's records are the same bytes across slot, batch size and capacity; lean calls leave the rest identical.
3. Identities with correlation() and structure(), and invariance under a common velocity.
4. evolve after radial_profile is the evolve without it, plain and with a recorded stop; 32 shells after 8 agree with a fresh
   handle.
5. Every error is raised with the function named, and leaves the state and a later call untouched."""
import ctypes

import numpy as np
import pytest

import hermite_radial_ref as rref

pytestmark = pytest.mark.gpu

SYSTEM_EXACT = ("selected", "below", "above", "unmeasured", "shells", "projected", "total_weight", "centre", "velocity")
ULP = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", rref.CAPACITIES)
def test_every_word_against_the_reference(capacity):
    import n_body_problem_amd as nb
    worst, equal = 0.0, True
    pos, vel, counts = rref.lattice_batch(capacity)
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(pos), np.array(vel))                  # copies: the shared inputs are read-only
        for case in rref.CASES:
            name = case[0]
            p, v, c, kw, (systems, shells, bodies, scale) = rref.reference(capacity, name)
            assert np.array_equal(bits(p.astype(np.float64)), bits(pos.astype(np.float64))) and list(c) == list(counts)
            res = batch.radial_profile(kw["edges"], centre=kw["centre"], velocity=kw["velocity"], weight=kw["weight"],
                                       subset=kw["subset"], projected=kw["projected"], bodies=True)
            assert res.shells == case[1] and res.count.shape == (B, case[1]) and res.count.dtype == np.int64
            assert res.M.shape == (B, case[1], 6) and res.L.shape == (B, case[1], 3) and res.body_shell.shape == (B, capacity)
            for word in SYSTEM_EXACT:
                assert res.systems[word].tobytes() == systems[word].tobytes(), (name, word, res.systems[word], systems[word])
            for word in rref.EXACT_WORDS:
                assert res.shell_records[word].tobytes() == shells[word].tobytes(), (name, word)
            assert np.array_equal(res.below + res.count.sum(axis=1) + res.above + res.unmeasured, res.selected)
            for k, word in enumerate(rref.ROOTED_WORDS):
                error = np.abs(res.shell_records[word] - shells[word])
                bound = (shells["count"] + 16) * ULP * scale[:, :, k]
                ratio = float(np.max(np.where(bound > 0, error / np.where(bound > 0, bound, 1.0), 0.0)))
                worst = max(worst, ratio)
                equal = equal and res.shell_records[word].tobytes() == shells[word].tobytes()
                print(f"capacity {capacity} {name} {word}: largest error / bound {ratio:.3g}")
                assert np.all(error <= bound), (name, word, error.max())
            # the body records: the shell exact; radius one square root, radial_velocity one division of it
            assert np.array_equal(res.body_shell, bodies["shell"]) and not res.body_records["reserved"].any()
            assert np.all(np.abs(res.body_radius - bodies["radius"]) <= ULP * bodies["radius"])
            assert np.all(np.abs(res.body_radial_velocity - bodies["radial_velocity"]) <= 3 * ULP * np.abs(bodies["radial_velocity"]))
            equal = equal and res.body_records.tobytes() == bodies.tobytes()
            # lean calls: the remaining records are the same bits
            lean = batch.radial_profile(kw["edges"], centre=kw["centre"], velocity=kw["velocity"], weight=kw["weight"],
                                        subset=kw["subset"], projected=kw["projected"], shells=False)
            assert lean.count is None and lean.body_shell is None and lean.systems.tobytes() == res.systems.tobytes(), name
            only = batch.radial_profile(kw["edges"], centre=kw["centre"], velocity=kw["velocity"], weight=kw["weight"],
                                        subset=kw["subset"], projected=kw["projected"])
            assert only.body_records is None and only.systems.tobytes() == res.systems.tobytes()
            assert only.shell_records.tobytes() == res.shell_records.tobytes(), name
        # a torch mask and a (3,) frame are the numpy ones
        import torch
        p, v, c, kw, (systems, shells, bodies, scale) = rref.reference(capacity, "1-number-sparse")
        res = batch.radial_profile(torch.as_tensor(kw["edges"]), centre=rref.CENTRE, velocity=rref.VELOCITY, weight="number",
                                   subset=torch.as_tensor(np.array(kw["subset"])).bool())
        assert res.systems.tobytes() == systems.tobytes() and res.shell_records["M"].tobytes() == shells["M"].tobytes()
    print(f"capacity {capacity}: worst error / bound {worst:.3g}; the device was {'bit-equal' if equal else 'not bit-equal'} to the reference")


# ---- 2. placement -----------------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bytes_in_another_slot_batch_size_and_capacity():
    import n_body_problem_amd as nb
    n = 60
    body, speed = nb.plummer(n, seed=4100)
    rng = np.random.default_rng(4101)
    mask = rng.random(n) < 0.8
    mine = np.geomspace(0.05, 3.0, 10)
    centre, velocity = np.array([0.03, -0.02, 0.01]), np.array([0.01, 0.0, -0.02])
    for projected in (None, 1):
        first = None
        for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (320, 4, 1), (4096, 2, 1)):
            P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
            counts = [min(capacity, 11 + 3 * s) for s in range(B)]
            for s in range(B):
                P[s, :counts[s]], V[s, :counts[s]] = nb.plummer(counts[s], seed=4200 + s)
            P[slot, :n], V[slot, :n], counts[slot] = body, speed, n
            S = rng.random((B, capacity)) < 0.5
            S[slot, :n] = mask
            edges = np.geomspace(0.1, 2.0, 10)[None, :] * (1.0 + np.arange(B))[:, None]
            edges[slot] = mine
            C, U = rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 3)) * 0.1
            C[slot], U[slot] = centre, velocity
            with nb.BatchedSystem(B, capacity, counts=counts) as batch:
                batch.set_state(P, V)
                res = batch.radial_profile(edges, centre=C, velocity=U, subset=S, projected=projected, bodies=True)
                lean = batch.radial_profile(edges, centre=C, velocity=U, subset=S, projected=projected, shells=False)
                plain = batch.radial_profile(edges, centre=C, velocity=U, subset=S, projected=projected)
            assert lean.systems.tobytes() == res.systems.tobytes() and plain.systems.tobytes() == res.systems.tobytes()
            assert plain.shell_records.tobytes() == res.shell_records.tobytes()
            assert (res.body_shell[slot, n:] == rref.NOT_TAKING).all() and not res.body_radius[slot, n:].any()
            got = res.systems[slot].tobytes() + res.shell_records[slot].tobytes() + res.body_records[slot, :n].tobytes()
            assert res.count[slot].sum() > n // 2 and res.selected[slot] == mask.sum()
            if first is None:
                first = got
            assert got == first, (projected, capacity, B, slot)


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def test_the_counts_add_up_and_are_correlations_counts_around_a_body_at_the_centre():
    import n_body_problem_amd as nb
    capacity = 320
    pos, vel, counts = rref.lattice_batch(capacity)
    pos, vel = np.array(pos), np.array(vel)
    pos[~np.isfinite(pos)] = 9.0
    vel[~np.isfinite(vel)] = 1.0
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(pos, vel)
        # edges that bracket everything, about a centre no lattice point is at
        res = batch.radial_profile([0.0, 1000.0], centre=(0.5, 0.5, 0.5), weight="number")
        assert np.array_equal(res.count[:, 0], res.selected) and np.array_equal(res.selected, counts)
        assert not res.below.any() and not res.above.any() and np.array_equal(res.weight_sum[:, 0], counts.astype(np.float64))
        # about body 0 of every system: correlation() with that body as the only row and edges whose squares fp32 holds
        edges = np.arange(0.0, 9.0)
        rows = np.zeros((B, capacity), bool)
        rows[:, 0] = True
        corr = batch.correlation(edges.astype(np.float32), rows=rows)
        res = batch.radial_profile(edges, centre=pos[:, 0, :3].astype(np.float64), weight="number")
        has = np.asarray(counts) > 0
        assert np.array_equal(res.count[has], corr.counts[has]) and res.count.sum() > 0
        assert np.array_equal(res.below[has], corr.below[has] + 1) and np.array_equal(res.above[has], corr.above[has])
        # a velocity added to every body and passed as the frame's changes no byte of the sums
        shift = np.array([5.0, -3.0, 2.0], dtype=np.float32)
        e = rref.half_edges(9)
        base = batch.radial_profile(e, centre=rref.CENTRE, velocity=rref.VELOCITY, bodies=True)
        moved = np.array(vel)
        moved[:, :, :3] += shift
        batch.set_state(pos, moved)
        same = batch.radial_profile(e, centre=rref.CENTRE, velocity=np.array(rref.VELOCITY) + shift.astype(np.float64), bodies=True)
        assert same.shell_records.tobytes() == base.shell_records.tobytes() and same.body_records.tobytes() == base.body_records.tobytes()
        for word in SYSTEM_EXACT[:-1]:
            assert same.systems[word].tobytes() == base.systems[word].tobytes(), word
        assert base.count.sum() > 0 and np.abs(base.vr1).sum() > 0


def test_edges_at_the_lagrangian_radii_of_a_plummer_sphere_enclose_their_fractions():
    """centre=structure().centre and edges at its Lagrangian radii pushed up by one part in 10^9: the weight within edge q is
    at least fractions[q] of the total (to the round-off of two sums in different orders), and no longer without its
    outermost member."""
    import n_body_problem_amd as nb
    n, capacity, B = 300, 320, 3
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    for s in range(B):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=4300 + s)
    fractions = (0.1, 0.5, 0.9)
    with nb.BatchedSystem(B, capacity, counts=[n] * B) as batch:
        batch.set_state(P, V)
        st = batch.structure(fractions=fractions)
        edges = np.concatenate([np.zeros((B, 1)), st.lagrangian * (1.0 + 1.0e-9)], axis=1)
        res = batch.radial_profile(edges, centre=st, bodies=True)
        named = batch.radial_profile(edges, centre="density")
        given = batch.radial_profile(edges, centre=st.centre)
    assert named.shell_records.tobytes() == res.shell_records.tobytes() == given.shell_records.tobytes()
    assert np.array_equal(bits(res.centre), bits(st.centre)) and not res.below.any() and not res.unmeasured.any()
    assert np.allclose(res.total_weight, st.total_weight, rtol=1e-13, atol=0.0)
    inside = res.cumulative_weight() / res.total_weight[:, None]
    print(f"weight fractions within the pushed Lagrangian radii: {inside.tolist()}")
    for s in range(B):
        for q, f in enumerate(fractions):
            assert inside[s, q] >= f - 1e-13, (s, q, inside[s, q])
            members = (res.body_shell[s] >= 0) & (res.body_shell[s] <= q)
            last = np.argmax(np.where(members, res.body_radius[s], -1.0))
            assert res.body_radius[s, last] == pytest.approx(st.lagrangian[s, q], rel=1e-12)
            assert (res.cumulative_weight()[s, q] - float(P[s, last, 3])) / res.total_weight[s] < f


# ---- 4. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between, stop=None):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        if stop:
            b.set_stop_conditions(**stop)
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.radial_profile(np.geomspace(0.05, 8.0, 33), centre="density", bodies=True)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.radial_profile([0.1, 1.0], weight="number", subset=mask, projected=2, shells=False)
        r = b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, r, b.stops() if stop else None


@pytest.mark.parametrize("stop", [None, dict(escape_radius=2.5)], ids=["plain", "with a stop recorded"])
def test_evolve_radial_profile_evolve_is_the_two_evolves_alone_bit_for_bit(stop):
    import n_body_problem_amd as nb
    counts = [40, 17, 64]
    P, V = np.zeros((3, 64, 4), np.float32), np.zeros((3, 64, 4), np.float32)
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=4400 + s)
    pa, va, ra, sa = two_evolves(P, V, counts, False, stop)
    pb, vb, rb, sb = two_evolves(P, V, counts, True, stop)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(ra.steps, rb.steps) and np.array_equal(ra.ticks, rb.ticks)
    if stop:
        assert sa.stopped.any()                                    # a Plummer sphere has bodies beyond 2.5
        assert np.array_equal(sa.reason, sb.reason) and np.array_equal(sa.ticks, sb.ticks) and np.array_equal(sa.escaper, sb.escaper)


def test_a_call_with_32_shells_after_one_with_8_agrees_with_a_fresh_handle():
    """The shell and edge buffers are sized by the first call and grown by a later, larger one."""
    import n_body_problem_amd as nb
    capacity = 128
    p, v, counts, kw8, (systems8, shells8, _, _) = rref.reference(capacity, "8-mass")
    _, _, _, kw32, _ = rref.reference(capacity, "32-own-number-y-sparse")

    def call(batch, kw):
        return batch.radial_profile(kw["edges"], centre=kw["centre"], velocity=kw["velocity"], weight=kw["weight"],
                                    subset=kw["subset"], projected=kw["projected"], bodies=True)
    with nb.BatchedSystem(len(counts), capacity, counts=counts) as batch:
        batch.set_state(np.array(p), np.array(v))
        small = call(batch, kw8)
        grown = call(batch, kw32)
        again = call(batch, kw8)
    with nb.BatchedSystem(len(counts), capacity, counts=counts) as fresh:
        fresh.set_state(np.array(p), np.array(v))
        alone = call(fresh, kw32)
    assert grown.systems.tobytes() == alone.systems.tobytes() and grown.shell_records.tobytes() == alone.shell_records.tobytes()
    assert grown.body_records.tobytes() == alone.body_records.tobytes() and grown.count.sum() > 0
    assert again.shell_records.tobytes() == small.shell_records.tobytes() and again.systems.tobytes() == small.systems.tobytes()
    for word in rref.EXACT_WORDS:
        assert small.shell_records[word].tobytes() == shells8[word].tobytes(), word


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_the_state_and_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    capacity = 64
    P, V, counts, kw, _ = rref.reference(capacity, "8-mass")
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        before = batch.radial_profile(kw["edges"], bodies=True)
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchRadialSystem * B)()
        out[2].selected = -7                                       # a refused call writes nothing
        doubles = lambda values: (ctypes.c_double * len(values))(*values)   # noqa: E731
        good = doubles([0.0, 1.0, 2.0])
        nan, inf = float("nan"), float("inf")
        tied = np.tile(np.array([0.0, 1.0, 2.0]), (B, 1))
        tied[3, 2] = 1.0
        zeros = [0.0] * (3 * B)
        bad_centre, bad_velocity = list(zeros), list(zeros)
        bad_centre[3 * 2 + 1], bad_velocity[3 * 4] = nan, -inf
        #        pos, vel, shells, edges, per_system, centre, velocity, weight, projected, subset, systems, shells_out, bodies
        cases = [((None, vel, 2, good, 0, None, None, 0, -1, None, out, None, None), b"NULL argument"),
                 ((pos, None, 2, good, 0, None, None, 0, -1, None, out, None, None), b"NULL argument"),
                 ((pos, vel, 2, None, 0, None, None, 0, -1, None, out, None, None), b"NULL argument"),
                 ((pos, vel, 2, good, 0, None, None, 0, -1, None, None, None, None), b"NULL argument"),
                 ((pos, vel, 0, good, 0, None, None, 0, -1, None, out, None, None), b"shells must be 1 ... 32"),
                 ((pos, vel, 33, good, 0, None, None, 0, -1, None, out, None, None), b"shells must be 1 ... 32"),
                 ((pos, vel, 2, doubles([-0.5, 1.0, 2.0]), 0, None, None, 0, -1, None, out, None, None),
                  b"edge 0 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, doubles([0.0, nan, 2.0]), 0, None, None, 0, -1, None, out, None, None),
                  b"edge 1 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, doubles([0.0, 1.0, inf]), 0, None, None, 0, -1, None, out, None, None),
                  b"edge 2 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, doubles([0.0, 1.0, 1.0]), 0, None, None, 0, -1, None, out, None, None),
                  b"edge 2 of all systems is not above edge 1: the edges must be strictly ascending"),
                 ((pos, vel, 2, doubles(tied.ravel().tolist()), 1, None, None, 0, -1, None, out, None, None),
                  b"edge 2 of system 3 is not above edge 1"),
                 ((pos, vel, 2, good, 0, None, None, 2, -1, None, out, None, None), b"weight must be"),
                 ((pos, vel, 2, good, 0, None, None, -1, -1, None, out, None, None), b"weight must be"),
                 ((pos, vel, 2, good, 0, None, None, 0, 3, None, out, None, None), b"projected must be -1 ... 2"),
                 ((pos, vel, 2, good, 0, None, None, 0, -2, None, out, None, None), b"projected must be -1 ... 2"),
                 ((pos, vel, 2, good, 0, doubles(bad_centre), None, 0, -1, None, out, None, None), b"the centre of system 2 must be finite"),
                 ((pos, vel, 2, good, 0, None, doubles(bad_velocity), 0, -1, None, out, None, None),
                  b"the velocity of system 4 must be finite")]
        for args, message in cases:
            assert lib.nbody_batch_radial_profile(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_radial_profile: ") and message in error, (args, error)
            assert out[2].selected == -7
        assert lib.nbody_batch_radial_profile(None, pos, vel, 2, good, 0, None, None, 0, -1, None, out, None, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_radial_profile: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="shells must be"):
            batch.radial_profile(np.arange(34.0))
        with pytest.raises(ValueError, match="shells must be"):
            batch.radial_profile([1.0])
        with pytest.raises(ValueError, match="edges must have shape"):
            batch.radial_profile(np.zeros((B + 1, 3)))
        with pytest.raises(ValueError, match="weight must be"):
            batch.radial_profile([0.0, 1.0], weight="charge")
        with pytest.raises(ValueError, match="projected must be"):
            batch.radial_profile([0.0, 1.0], projected=3)
        with pytest.raises(ValueError, match="centre must"):
            batch.radial_profile([0.0, 1.0], centre="mass")
        with pytest.raises(ValueError, match="centre must have shape"):
            batch.radial_profile([0.0, 1.0], centre=np.zeros((B, 2)))
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.radial_profile([0.0, 1.0], subset=np.ones((B, capacity), np.int32))
        with pytest.raises(ValueError, match="subset must have shape"):
            batch.radial_profile([0.0, 1.0], subset=np.ones((B, capacity - 1), bool))
        with pytest.raises(nb.NBodyError, match="nbody_batch_radial_profile: edge 1 of all systems is not above edge 0"):
            batch.radial_profile([1.0, 0.5])
        with pytest.raises(nb.NBodyError, match="nbody_batch_radial_profile: the centre of system 0 must be finite"):
            batch.radial_profile([0.0, 1.0], centre=(0.0, np.inf, 0.0))
        assert lib.nbody_batch_radial_profile(h, pos, vel, 2, good, 0, None, None, 0, -1, None, out, None, None) == _lib.NBODY_OK
        assert out[2].selected == counts[2] and out[2].shells == 2 and out[2].projected == -1
        after = batch.radial_profile(kw["edges"], bodies=True)
        p, v = batch.download()
    assert after.systems.tobytes() == before.systems.tobytes() and after.shell_records.tobytes() == before.shell_records.tobytes()
    assert after.body_records.tobytes() == before.body_records.tobytes()
    assert np.array_equal(np.asarray(p).view(np.uint32), P.view(np.uint32)) and np.array_equal(np.asarray(v).view(np.uint32), V.view(np.uint32))
