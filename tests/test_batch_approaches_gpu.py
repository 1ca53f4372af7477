"""GPU: the approach lists of batched ensembles (BatchedSystem.approaches, include/nbody_batch_approaches.h).  Every word of
every record and every list entry equal the reference (hermite_approaches_ref: the phases decided on exact integers) exactly,
at every workgroup shape, with ragged counts, in both modes, with and without a subset and at list capacities that count only,
that cut a system in the middle of a row and that hold everything; a system's result is the same bytes wherever it runs; with
a horizon of 0, or with no relative motion, the list is contacts()' list, and a velocity added to every body changes no byte;
bodies in free flight are within reach at a step only if the list said so, and the pairs of the `end` phase are the ones
within reach at the horizon that neither were before nor pass closer on the way; the call disturbs no evolve; the buffers
grow; and every error is reported.

Capacities: 64 (one wave, one row per lane), 128 (two rows per lane), 320 (four rows per lane, two waves: the placement
across waves and across q), 4096 (sixteen waves, 128 KiB of dynamic LDS: the raised limit).  Counts 0, 1, 2, 65 and the
capacity.  The inputs are small integers, so every word of every chain and of the predicate is exact
(test_batch_approaches_cpu.py checks the premise and that the inputs contain what they are there for): the exact agreement
asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_approaches_ref as aref

pytestmark = pytest.mark.gpu


def check_against_reference(res, refs, capacity, tag, bodies=True):
    """Every word of every record and every entry; the order of the list; first as the exclusive sum; the pads."""
    for s, ref in enumerate(refs):
        want = aref.system_record(ref, capacity)
        assert res.systems[s].tobytes() == want.tobytes(), (tag, s, res.systems[s], want)
        aref.check_phases(res.systems[s])
        if bodies:
            assert res.body_records[s].tobytes() == ref["bodies"].tobytes(), (tag, s)
            assert np.array_equal(res.first[s], np.concatenate([[0], np.cumsum(res.upper[s])[:-1]]))
            aref.check_identity(res.body_records[s], int(res.pairs[s]))
        if res.entries is not None:
            assert res.entries.shape == (len(refs), capacity)
            assert res.entries[s].tobytes() == aref.listed(ref, capacity).tobytes(), (tag, s)
            m = int(res.stored[s])
            key = res.i[s, :m].astype(np.int64) * 4096 + res.j[s, :m]
            assert (res.i[s, :m] < res.j[s, :m]).all() and (np.diff(key) > 0).all(), (tag, s)      # strictly ascending in (i, j)
            assert res.entries[s, m:].tobytes() == aref.pad(capacity - m).tobytes()


def loaded(nb, capacity, **kw):
    P, V, counts, _ = aref.gpu_inputs(capacity)
    batch = nb.BatchedSystem(len(counts), capacity, counts=counts, **kw)
    batch.set_state(np.array(P), np.array(V))                      # copies: the shared inputs are read-only
    return batch


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", aref.CAPACITIES)
def test_the_records_and_the_list_equal_the_reference_exactly(capacity):
    import n_body_problem_amd as nb
    B = aref.B
    with loaded(nb, capacity) as batch:
        for mode in aref.MODES:
            for with_subset in (False, True):
                H, kw = aref.gpu_arguments(capacity, mode, with_subset)
                refs = aref.gpu_reference(capacity, mode, with_subset)
                most = max(r["system"]["pairs"] for r in refs)
                cut = aref.truncating_capacity(refs)
                tag = (capacity, mode, with_subset)
                counted = batch.approaches(H, capacity=0, **kw)
                print(f"{tag}: pairs {counted.pairs.tolist()} (reference {[r['system']['pairs'] for r in refs]}), now "
                      f"{counted.now_pairs.tolist()}, passing {counted.passing.tolist()}, ending {counted.ending.tolist()}, "
                      f"max_degree {counted.max_degree.tolist()}; capacities 0, {cut}, {most}")
                assert counted.entries.shape == (B, 0) and not counted.stored.any()
                check_against_reference(counted, refs, 0, tag + (0,))
                truncated = batch.approaches(H, capacity=cut, **kw)
                check_against_reference(truncated, refs, cut, tag + (cut,))
                assert truncated.truncated.any() and truncated.stored.max() == cut
                full = batch.approaches(H, capacity=most, **kw)
                check_against_reference(full, refs, most, tag + (most,))
                assert not full.truncated.any() and np.array_equal(full.stored, full.pairs)
                for s in range(B):
                    assert full.pairs_of(s).tolist() == np.stack([refs[s]["list"]["i"], refs[s]["list"]["j"]], axis=1).tolist()
                # capacity=None: the full list; bodies=False: the same system records; lists=False: the counting call
                auto = batch.approaches(H, **kw)
                assert auto.systems.tobytes() == full.systems.tobytes() and auto.entries.tobytes() == full.entries.tobytes()
                lean = batch.approaches(H, capacity=most, bodies=False, **kw)
                assert lean.degree is None and lean.systems.tobytes() == full.systems.tobytes() and lean.entries.tobytes() == full.entries.tobytes()
                listless = batch.approaches(H, lists=False, **kw)
                assert listless.entries is None and listless.time is None and listless.systems.tobytes() == counted.systems.tobytes()
                for name in full.systems.dtype.names:
                    assert name == "stored" or listless.systems[name].tobytes() == full.systems[name].tobytes(), name
                assert listless.body_records.tobytes() == full.body_records.tobytes()
                bare = batch.approaches(H, lists=False, bodies=False, **kw)
                assert bare.systems.tobytes() == counted.systems.tobytes() and bare.degree is None
                # the derived words: a passage lies inside its horizon and within its threshold, an end at it
                for s in range(B):
                    m = int(full.stored[s])
                    phase, time = full.phase[s, :m], full.time[s, :m]
                    assert (time[phase == aref.NOW] == 0).all() and (time[phase == aref.END] == aref.HORIZON[s]).all()
                    assert ((time[phase == aref.PASSAGE] > 0) & (time[phase == aref.PASSAGE] < aref.HORIZON[s])).all()
                    if mode == "radius":                           # fp64 from fp32 words: a few ulps of rounding
                        assert (full.miss_distance[s, :m] <= aref.RADIUS[s] * (1 + 1e-12)).all()
        # uint8 and torch subsets, torch radii and a torch horizon, a scalar radius and a scalar horizon are the numpy ones
        import torch
        subset = aref.gpu_subset(capacity)
        R = aref.gpu_inputs(capacity)[3]
        refs = aref.gpu_reference(capacity, "radii", True)
        H = np.array(aref.HORIZON, np.float32)
        res = batch.approaches(torch.as_tensor(H), radii=torch.as_tensor(np.array(R)), subset=torch.as_tensor(np.array(subset)))
        check_against_reference(res, refs, max(r["system"]["pairs"] for r in refs), (capacity, "torch"))
        res = batch.approaches(H, radii=R, subset=subset.astype(np.uint8), lists=False)
        check_against_reference(res, refs, 0, (capacity, "uint8"))
        scalar = batch.approaches(6.0, 3.0, lists=False)
        each = batch.approaches(np.full(B, 6.0, np.float32), torch.full((B,), 3.0), lists=False)
        assert scalar.systems.tobytes() == each.systems.tobytes() and scalar.pairs[4] == aref.gpu_reference(capacity, "radius", False)[4]["system"]["pairs"]


# ---- 2. placement -----------------------------------------------------------------------------------------------------------------
def placement_systems():
    """name -> (positions, velocities, subset, radii): three systems with approaches in both modes, of every phase but for the
    wide cube under radii, where none is decided at the horizon."""
    rng = np.random.default_rng(173)
    line = np.ones((50, 4), np.float32)
    line[:, :3] = [(2 * i, 0, 0) for i in range(50)]
    out = {}
    for name, body in {"narrow": aref.cube(64, 171, 4), "wide": aref.cube(37, 172, 6), "line": line}.items():
        vel = np.zeros_like(body)
        vel[:, :3] = rng.integers(-aref.SPEED, aref.SPEED + 1, (len(body), 3))
        out[name] = (body, vel, rng.random(len(body)) < 0.8, rng.integers(0, 3, len(body)).astype(np.float32))
    return out


def test_a_systems_result_is_the_same_bytes_in_another_slot_batch_size_and_capacity():
    import n_body_problem_amd as nb
    rng = np.random.default_rng(174)
    for name, (body, vel, take, mine) in placement_systems().items():
        n = len(body)
        for mode in aref.MODES:
            ref = aref.reference(body, vel, n, n, 2, radius=3.0 if mode == "radius" else None, radii=mine if mode == "radii" else None,
                                 subset=take)
            room = ref["system"]["pairs"] + 2
            first = None
            for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (320, 4, 1), (4096, 2, 1)):
                P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
                counts = [min(capacity, 11 + 3 * s) for s in range(B)]
                for s in range(B):
                    P[s, :counts[s]] = aref.cube(counts[s], 40 + s, 3)
                    V[s, :counts[s], :3] = rng.integers(-2, 3, (counts[s], 3))
                P[slot, :n], V[slot, :n], counts[slot] = body, vel, n
                S, R = rng.random((B, capacity)) < 0.5, rng.integers(0, 3, (B, capacity)).astype(np.float32)
                S[slot, :n], R[slot, :n] = take, mine
                radius, horizon = (1.0 + np.arange(B)).astype(np.float32), (3.0 + np.arange(B)).astype(np.float32)
                radius[slot], horizon[slot] = 3.0, 2.0
                with nb.BatchedSystem(B, capacity, counts=counts) as batch:
                    batch.set_state(P, V)
                    res = batch.approaches(horizon, radius if mode == "radius" else None, radii=R if mode == "radii" else None, subset=S,
                                           capacity=room)
                assert res.body_records[slot, :n].tobytes() == ref["bodies"].tobytes(), (name, mode, capacity, B)
                rest = res.body_records[slot, n:]
                assert not rest["degree"].any() and not rest["upper"].any() and (rest["first"] == ref["system"]["pairs"]).all() and not rest["now"].any()
                got = res.systems[slot].tobytes() + res.body_records[slot, :n].tobytes() + res.entries[slot].tobytes()
                assert res.systems[slot].tobytes() == aref.system_record(ref, room).tobytes() and res.entries[slot].tobytes() == aref.listed(ref, room).tobytes()
                if first is None:
                    first = got
                assert got == first, (name, mode, capacity, B)
            assert ref["system"]["now"] > 0 and ref["system"]["passing"] > 0, (name, mode, ref["system"])
            assert ref["system"]["ending"] > 0 or (name, mode) == ("wide", "radii"), (name, mode, ref["system"])


# ---- 3. identities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [64, 320])
def test_without_a_horizon_or_without_relative_motion_the_approaches_are_the_contacts_and_a_common_velocity_changes_nothing(capacity):
    import n_body_problem_amd as nb
    P, V, counts, R = aref.gpu_inputs(capacity)
    B = len(counts)
    subset = aref.gpu_subset(capacity)
    P = np.array(P)
    P[3, 9, 0] = 7.0                                               # finite everywhere: contacts() measures what approaches() does
    still = np.array(V)
    still[3, 5, 1] = 0.0
    drift = np.zeros_like(still)
    drift[..., :3] = (2.0, -1.0, 1.0)                              # the same velocity for every body: no relative motion
    H = np.array(aref.HORIZON, np.float32)
    for mode in aref.MODES:
        kw = {"radius": np.array(aref.RADIUS, np.float32)} if mode == "radius" else {"radii": R}
        with nb.BatchedSystem(B, capacity, counts=counts) as batch:
            batch.set_state(P, still)
            touching = batch.contacts(subset=subset, **kw)
            moving = batch.approaches(H, subset=subset, **kw)
            frozen = batch.approaches(0.0, subset=subset, **kw)
            batch.set_state(P, still + drift)                      # one integer velocity added to all: every w is the same bits
            shifted = batch.approaches(H, subset=subset, **kw)
            batch.set_state(P, drift)
            resting = batch.approaches(H, subset=subset, **kw)
        assert moving.pairs[4] > touching.pairs[4] > 0
        for res, tag in ((frozen, "H = 0"), (resting, "no relative motion")):
            for name in ("i", "j", "r2"):
                assert getattr(res, name).tobytes() == getattr(touching, name).tobytes(), (mode, tag, name)
            assert np.array_equal(res.pairs, touching.pairs) and np.array_equal(res.now_pairs, touching.pairs), (mode, tag)
            assert not res.passing.any() and not res.ending.any() and not res.phase[res.i >= 0].any()
            assert np.array_equal(res.now, touching.degree) and np.array_equal(res.degree, touching.degree)
            assert np.array_equal(res.upper, touching.upper) and np.array_equal(res.first, touching.first)
            assert np.array_equal(res.approaching, touching.touching) and np.array_equal(res.max_degree, touching.max_degree)
        assert np.array_equal(moving.now, touching.degree) and np.array_equal(moving.now_pairs, touching.pairs), mode
        for a, b in ((shifted.systems, moving.systems), (shifted.body_records, moving.body_records), (shifted.entries, moving.entries)):
            assert a.tobytes() == b.tobytes(), mode


# ---- 4. free flight -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [64, 320])
def test_in_free_flight_every_pair_within_reach_at_a_step_is_listed_and_the_end_phase_is_what_is_within_reach_at_the_horizon(capacity):
    """Zero mass words and softening 1: no body feels another, so a kick-drift step of dt = 1 moves every body by its velocity
    and the positions stay exact integers.  At every t = 1 .. H the contacts() pairs are in the approach list; the pairs of
    phase 2 are exactly the contacts() pairs at t = H that are neither `now` nor `passage` entries."""
    import n_body_problem_amd as nb
    P, V, counts, R = aref.gpu_inputs(capacity)
    P, V = np.array(P), np.array(V)
    P[..., 3] = 0.0                                                # massless
    P[3, 9, 0], V[3, 5, 1] = 7.0, 0.0                              # finite everywhere
    B, H = len(counts), 6
    for mode in aref.MODES:
        kw = {"radius": np.array(aref.RADIUS, np.float32)} if mode == "radius" else {"radii": R}
        with nb.BatchedSystem(B, capacity, counts=counts) as batch:
            batch.set_state(P, V)
            res = batch.approaches(float(H), **kw)
            listed = [{(int(i), int(j)): int(p) for i, j, p in zip(res.i[s], res.j[s], res.phase[s]) if i >= 0} for s in range(B)]
            assert not res.truncated.any()
            seen = [set() for _ in range(B)]
            for t in range(1, H + 1):
                batch.step_n(1, 1.0, 1.0)
                p, v = batch.download()
                assert np.array_equal(p[..., :3], P[..., :3] + t * V[..., :3]) and np.array_equal(v[..., :3], V[..., :3])   # straight lines
                at = batch.contacts(**kw)
                for s in range(B):
                    pairs = {(int(i), int(j)) for i, j in at.pairs_of(s)}
                    assert pairs <= set(listed[s]), (mode, s, t, sorted(pairs - set(listed[s]))[:5])
                    seen[s] |= pairs
            for s in range(B):                                     # `at` is the state at t = H
                end = {pair for pair, phase in listed[s].items() if phase == aref.END}
                at_end = {(int(i), int(j)) for i, j in at.pairs_of(s)}
                assert end == {pair for pair in at_end if listed[s][pair] not in (aref.NOW, aref.PASSAGE)}, (mode, s)
            print(f"{capacity} {mode}: listed {[len(x) for x in listed]}, within reach at a step {[len(x) for x in seen]}, "
                  f"ending {res.ending.tolist()}")
            assert res.ending[4] > 0 and res.passing[4] > 0 and len(seen[4]) > 0


# ---- 5. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.approaches(0.5, 0.3)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.approaches(2.0, radii=np.full((P.shape[0], P.shape[1]), 0.1, np.float32), subset=mask, capacity=5)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_approaches_evolve_is_the_two_evolves_alone_bit_for_bit():
    import n_body_problem_amd as nb
    counts = [40, 17, 64]
    P, V = np.zeros((3, 64, 4), np.float32), np.zeros((3, 64, 4), np.float32)
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=80 + s)
    pa, va, ra = two_evolves(P, V, counts, False)
    pb, vb, rb = two_evolves(P, V, counts, True)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert ra.steps.sum() > 0


# ---- 6. the buffers ---------------------------------------------------------------------------------------------------------------
def test_a_call_with_more_capacity_and_one_in_the_other_mode_after_a_small_call_agree_with_a_fresh_handle():
    """The list buffer is sized by the first call and grown by a later, larger one; each mode has its own threshold buffer."""
    import n_body_problem_amd as nb
    R = aref.gpu_inputs(128)[3]
    subset = aref.gpu_subset(128)
    H, radius = np.array(aref.HORIZON, np.float32), np.array(aref.RADIUS, np.float32)
    refs = aref.gpu_reference(128, "radius", False)
    most = max(r["system"]["pairs"] for r in refs)
    other = aref.gpu_reference(128, "radii", True)
    room = max(r["system"]["pairs"] for r in other) + 7
    with loaded(nb, 128) as batch:
        small = batch.approaches(H, radius, capacity=1, bodies=False)
        check_against_reference(small, refs, 1, "capacity 1 first", bodies=False)
        grown = batch.approaches(H, radius, capacity=most)
        changed = batch.approaches(H, radii=R, subset=subset, capacity=room)
        again = batch.approaches(H, radius, capacity=2)
    with loaded(nb, 128) as fresh:
        alone = fresh.approaches(H, radii=R, subset=subset, capacity=room)
    check_against_reference(grown, refs, most, "all after 1")
    check_against_reference(changed, other, room, "radii after radius")
    check_against_reference(again, refs, 2, "2 after all")
    for a, b in ((changed.systems, alone.systems), (changed.body_records, alone.body_records), (changed.entries, alone.entries)):
        assert a.tobytes() == b.tobytes()


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    R = aref.gpu_inputs(64)[3]
    B = aref.B
    with loaded(nb, 64) as batch:
        before = batch.approaches(np.array(aref.HORIZON, np.float32), np.array(aref.RADIUS, np.float32))
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchApproachSystem * B)()
        bodies = (_lib.BatchApproachBody * (B * 64))()
        entries = (_lib.BatchApproach * (B * 4))()
        out[2].bodies, bodies[70].degree, entries[9].i = -7, -7, -7   # a refused call writes nothing
        floats = lambda values: (ctypes.c_float * len(values))(*values)   # noqa: E731
        good, hor, radii = floats(list(aref.RADIUS)), floats(list(aref.HORIZON)), floats(R.ravel().tolist())

        def with_one(values, s, value):
            r = list(values)
            r[s] = value
            return floats(r)

        def with_radii(s, slot, value):
            r = np.array(R)
            r[s, slot] = value
            return floats(r.ravel().tolist())
        cases = [((None, vel, hor, good, None, None, 4, out, bodies, entries), b"NULL argument"),
                 ((pos, None, hor, good, None, None, 4, out, bodies, entries), b"NULL argument"),
                 ((pos, vel, None, good, None, None, 4, out, bodies, entries), b"NULL argument"),
                 ((pos, vel, hor, good, None, None, 4, None, bodies, entries), b"NULL argument"),
                 ((pos, vel, with_one(aref.HORIZON, 3, -0.5), good, None, None, 4, out, bodies, entries), b"the horizon of system 3 must be finite and >= 0"),
                 ((pos, vel, with_one(aref.HORIZON, 0, float("nan")), good, None, None, 4, out, bodies, entries), b"the horizon of system 0 must be finite and >= 0"),
                 ((pos, vel, with_one(aref.HORIZON, 4, float("inf")), good, None, None, 4, out, bodies, entries), b"the horizon of system 4 must be finite and >= 0"),
                 ((pos, vel, hor, good, radii, None, 4, out, bodies, entries), b"exactly one of radius and radii must be given"),
                 ((pos, vel, hor, None, None, None, 4, out, bodies, entries), b"exactly one of radius and radii must be given"),
                 ((pos, vel, hor, with_one(aref.RADIUS, 3, -0.5), None, None, 4, out, bodies, entries), b"the radius of system 3 must be finite and >= 0"),
                 ((pos, vel, hor, with_one(aref.RADIUS, 0, float("nan")), None, None, 4, out, bodies, entries), b"the radius of system 0 must be finite and >= 0"),
                 ((pos, vel, hor, with_one(aref.RADIUS, 4, float("inf")), None, None, 4, out, bodies, entries), b"the radius of system 4 must be finite and >= 0"),
                 ((pos, vel, hor, None, with_radii(4, 63, -1.0), None, 4, out, bodies, entries), b"radius of system 4, slot 63"),
                 ((pos, vel, hor, None, with_radii(3, 0, float("nan")), None, 4, out, bodies, entries), b"radius of system 3, slot 0"),
                 ((pos, vel, hor, None, with_radii(2, 1, float("inf")), None, 4, out, bodies, entries), b"radius of system 2, slot 1"),
                 ((pos, vel, hor, good, None, None, -1, out, bodies, None), b"capacity must be >= 0"),
                 ((pos, vel, hor, good, None, None, 4, out, bodies, None), b"list_out must be given iff capacity > 0"),
                 ((pos, vel, hor, good, None, None, 0, out, bodies, entries), b"list_out must be given iff capacity > 0"),
                 ((pos, vel, hor, good, None, None, 2 ** 27 // B + 1, out, bodies, entries), b"n_systems x capacity must not exceed 2^27")]
        for args, message in cases:
            assert lib.nbody_batch_approaches(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_approaches: ") and message in error, (args, error)
            assert out[2].bodies == -7 and bodies[70].degree == -7 and entries[9].i == -7
        assert lib.nbody_batch_approaches(None, pos, vel, hor, good, None, None, 4, out, bodies, entries) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_approaches: batch is NULL" in lib.nbody_batch_last_error(None)
        # a radius beyond the count is never examined
        assert lib.nbody_batch_approaches(h, pos, vel, hor, None, with_radii(2, 2, float("nan")), None, 0, out, None, None) == _lib.NBODY_OK
        with pytest.raises(ValueError, match="exactly one of radius and radii"):
            batch.approaches(1.0)
        with pytest.raises(ValueError, match="exactly one of radius and radii"):
            batch.approaches(1.0, 1.0, radii=R)
        with pytest.raises(ValueError, match="horizon must be a scalar or have shape"):
            batch.approaches(np.ones(B + 1), 1.0)
        with pytest.raises(ValueError, match="radius must be a scalar or have shape"):
            batch.approaches(1.0, np.ones(B + 1))
        with pytest.raises(ValueError, match="radii must have shape"):
            batch.approaches(1.0, radii=np.ones((B, 63), np.float32))
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.approaches(1.0, 1.0, subset=np.ones((B, 64), np.int32))
        with pytest.raises(ValueError, match="subset must have shape"):
            batch.approaches(1.0, 1.0, subset=np.ones((B, 63), bool))
        with pytest.raises(ValueError, match="capacity must be an integer >= 0"):
            batch.approaches(1.0, 1.0, capacity=-1)
        with pytest.raises(ValueError, match="exceed 2\\^27"):
            batch.approaches(1.0, 1.0, capacity=2 ** 27)
        with pytest.raises(nb.NBodyError, match="nbody_batch_approaches: the horizon of system 0 must be finite and >= 0"):
            batch.approaches(-1.0, 1.0)
        with pytest.raises(nb.NBodyError, match="nbody_batch_approaches: the radius of system 0 must be finite and >= 0"):
            batch.approaches(1.0, -1.0)
        assert lib.nbody_batch_approaches(h, pos, vel, hor, good, None, None, 4, out, bodies, entries) == _lib.NBODY_OK
        want = aref.gpu_reference(64, "radius", False)
        assert out[2].bodies == 2 and out[4].pairs == want[4]["system"]["pairs"] and out[4].stored == 4
        assert bodies[4 * 64 + 5].degree == want[4]["bodies"]["degree"][5] and entries[4 * 4 + 1].j == want[4]["list"]["j"][1]
        assert entries[4 * 4 + 1].phase == want[4]["list"]["phase"][1]
        after = batch.approaches(np.array(aref.HORIZON, np.float32), np.array(aref.RADIUS, np.float32))
    assert after.systems.tobytes() == before.systems.tobytes() and after.entries.tobytes() == before.entries.tobytes()
