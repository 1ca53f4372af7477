"""GPU: the mutual gravity of labelled sets of batched ensembles (BatchedSystem.mutual_gravity,
include/nbody_batch_mutual_gravity.h).

1. Every word against the reference (hermite_mutual_gravity_ref: IEEE doubles in the pinned order).  Capacities 64, 128, 256,
   1024 and 4096; counts 0, 1, 2, 3, 63, 64, 65, 129, 257 and the capacity as far as the capacity holds them in one batch, and
   at 4096 one system of 4096 bodies in 2 sets and one of 1025 in 8, only; K = 1, 2, 3, 5 and 8; labels interleaved, contiguous,
   sets of 0, 1, 63, 64 and 65 bodies by rank scattered over the system, everything unlabelled; an unmeasured body and a
   coincident pair in every system of 63 bodies or more; the softening 0 and above; a centre and a velocity or none.  The
   integers and the system record are byte-equal; every floating word, which passes through the device's square root and
   division, is held to hermite_mutual_gravity_ref.BOUND = 6.4e-15 of its absolute companion: four times the spread 1.6e-15
   that the reference itself shows when every root and quotient is moved by up to one ulp at random
   (test_batch_mutual_gravity_cpu.py measures it again).  Whether the device was in fact bit-equal is printed, not asserted.
   No case is left out: the one decision, s2 == 0, is exact.
2. Against shipped code, with every body in a set: the potential against energy()'s and against members()' per-body one.
3. Identities exact by construction: renamed sets, garbage in a body of no set, what centre and velocity change, the closed
   form, matrix=False.
4. Placement: one system's records are the same bytes in another slot, batch size and capacity.
5. Non-interference: evolve, mutual_gravity, evolve is the two evolves alone; 8 sets after 1 set agree with a fresh handle.
6. Errors: each refused with the function named, leaving the state and a later call untouched."""
import ctypes

import numpy as np
import pytest

import hermite_mutual_gravity_ref as mref

pytestmark = pytest.mark.gpu


def check_against_reference(res, refs, tag):
    """Returns (worst error, whether the floating words were bit-equal)."""
    worst, equal = 0.0, True
    for s, ref in enumerate(refs):
        assert res.systems[s].tobytes() == ref["system"].tobytes(), (tag, s, res.systems[s], ref["system"])
        got = res.entries[s]
        assert np.array_equal(got["pairs"], ref["entries"]["pairs"]), (tag, s)
        error = mref.error_of(got, ref)
        assert error <= mref.BOUND, (tag, s, error)
        worst = max(worst, error)
        equal = equal and got.tobytes() == ref["entries"].tobytes()
        members = res.members[s].astype(np.int64)
        assert np.array_equal(got["pairs"], members[:, None] * members[None, :] - np.diag(members)), (tag, s)
        assert int(res.total_pairs[s]) == int(got["pairs"].sum())
        empty = (members[:, None] == 0) | (members[None, :] == 0)
        assert got[empty].tobytes() == np.zeros(int(empty.sum()), mref.ENTRY_DTYPE).tobytes(), (tag, s)   # an empty set reads 0
    return worst, equal


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", mref.CAPACITIES)
def test_every_word_against_the_reference(capacity):
    """Observed on an MI355X: see profiles/batch_rate_mutual_gravity.txt and DESIGN.md."""
    import n_body_problem_amd as nb
    P, V, counts = mref.gpu_inputs(capacity)
    B = len(counts)
    worst, equal, compared = 0.0, True, 0
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))                  # copies: the shared inputs are read-only
        for name, sets, kind, eps, frame in mref.cases_of(capacity):
            L = mref.gpu_labels(capacity, name)
            centre, velocity = mref.gpu_frames(capacity, frame)
            res = batch.mutual_gravity(L, sets=sets, softening=eps, centre=centre, velocity=velocity)
            refs = mref.gpu_reference(capacity, name)
            assert res.entries.shape == (B, sets, sets) and res.sets == sets and res.pairs.dtype == np.int64 and res.force.shape == (B, sets, sets, 3)
            assert np.array_equal(res.selected + res.left_out + res.unmeasured, np.minimum(counts, capacity))
            error, same = check_against_reference(res, refs, (capacity, name))
            print(f"capacity {capacity} {name}: pairs {res.total_pairs.tolist()}, coincident {res.coincident.tolist()}, unmeasured "
                  f"{res.unmeasured.tolist()}, largest error {error:.3g} (bound {mref.BOUND:.3g}); {'bit-equal' if same else 'not bit-equal'}")
            worst, equal, compared = max(worst, error), equal and same, compared + 1
            lean = batch.mutual_gravity(L, sets=sets, softening=eps, centre=centre, velocity=velocity, matrix=False)
            assert lean.entries is None and lean.potential is None and lean.systems.tobytes() == res.systems.tobytes(), name
        if capacity != 4096:                                       # torch labels, uint8 wire labels and masks are the integer ones
            import torch
            L = mref.gpu_labels(capacity, "interleaved-3-soft")
            for labels in (torch.as_tensor(np.array(L)), mref.wire_labels(L).astype(np.int16) - 256 * (mref.wire_labels(L) == 255),
                           tuple(L == a for a in range(3))):
                res = batch.mutual_gravity(labels, sets=3, softening=0.0625)
                check_against_reference(res, mref.gpu_reference(capacity, "interleaved-3-soft"), (capacity, "torch, int16 and masks"))
    assert compared == len(mref.cases_of(capacity))
    print(f"capacity {capacity}: worst error {worst:.3g} of the bound {mref.BOUND:.3g}; the device was "
          f"{'bit-equal' if equal else 'not bit-equal'} to the reference")
    if capacity != 4096:
        last = mref.gpu_reference(capacity, "interleaved-2-frame")[-1]["system"]
        assert last["coincident"] == 2 and last["unmeasured"] == 2 and last["pairs"] > 0                     # the inputs work


# ---- 2. against shipped code ----------------------------------------------------------------------------------------------------
#: The fp32 pair term of energy() and members(): m_j * rsq(fma(dz, dz, fma(dy, dy, fma(dx, dx, eps2)))) on fp32 differences.
#: Relative to the exact m_j / r, with u = 2^-24:
#:   the three differences, one rounding each: r2 is a sum of squares, so at most 2 u on r2;
#:   the three fused steps of the r2 chain, one rounding each of a partial sum no larger than r2 (eps2's own rounding is one
#:     of them at most): at most 3 u on r2; together 5 u on r2, which is 2.5 u on 1 / r;
#:   the reciprocal square root, accurate to one ulp: at most 2 u;  the product with m_j: u.
#: 5.5 u per term (the issue's count was six), so 5.5 u of the companion sum |m_i m_j / r|; 1.001 covers the second order.  The
#: fp64 sums of either side and this call's own BOUND add at most 4096 x 2^-53 + 6.4e-15.
SHIPPED_BOUND = 5.5 * 2.0 ** -24 * 1.001 + 4096 * 2.0 ** -53 + mref.BOUND


@pytest.mark.parametrize("eps", (0.0, 0.03125))
def test_the_potential_against_energy_and_members_with_every_body_in_a_set(eps):
    """sum_ab potential / 2 against energy(eps)'s potential, and sum_b potential[a, b] against sum_{i in a} m_i times
    members(eps, max_iterations=1).potential, both within SHIPPED_BOUND of the companion (derived above from the roundings of
    nbody_batch_analysis.hip's fp32 pair term, not fitted)."""
    import n_body_problem_amd as nb
    n, capacity, B, sets = 300, 320, 3, 3
    counts = [n, n, n - 9]
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    for s in range(B):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=290 + s)
    labels = np.random.default_rng(291).integers(0, sets, size=(B, capacity))
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(P, V)
        res = batch.mutual_gravity(labels, sets=sets, softening=eps)
        energy = batch.energy(eps)[:, 1]
        phi = batch.members(eps, max_iterations=1).potential
    assert np.array_equal(res.selected, counts) and not res.left_out.any() and not res.unmeasured.any() and not res.coincident.any()
    for s in range(B):
        ref = mref.reference(P[s], V[s], counts[s], labels[s], sets, eps)
        companion = ref["absolute"][:, :, 0]
        total = res.total_potential_energy()[s]
        error = abs(total - energy[s]) / (companion.sum() / 2.0)
        print(f"eps {eps} system {s}: potential {total!r} against energy() {energy[s]!r}: {error:.3g} of the companion (bound {SHIPPED_BOUND:.3g})")
        assert error <= SHIPPED_BOUND
        m = P[s, :counts[s], 3].astype(np.float64)
        for a in range(sets):
            mine = res.potential[s, a, :].sum()
            theirs = (m * phi[s, :counts[s]])[labels[s, :counts[s]] == a].sum()
            error = abs(mine - theirs) / companion[a].sum()
            print(f"eps {eps} system {s} set {a}: {mine!r} against members() {theirs!r}: {error:.3g} of the companion")
            assert error <= SHIPPED_BOUND


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def test_renaming_the_sets_permutes_the_entries_byte_for_byte():
    import n_body_problem_amd as nb
    P, V, counts = mref.gpu_inputs(256)
    B = len(counts)
    L = np.array(mref.gpu_labels(256, "ranks-8-frame"))
    centre, velocity = mref.gpu_frames(256, True)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])                      # set a becomes set perm[a]
    renamed = np.where(L >= 0, perm[np.maximum(L, 0)], -1)
    with nb.BatchedSystem(B, 256, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        one = batch.mutual_gravity(L, sets=8, centre=centre, velocity=velocity)
        two = batch.mutual_gravity(renamed, sets=8, centre=centre, velocity=velocity)
    assert one.total_pairs.sum() > 0
    assert two.entries[:, perm[:, None], perm[None, :]].tobytes() == one.entries.tobytes()
    assert two.members[:, perm].tobytes() == one.members.tobytes() and two.mass[:, perm].tobytes() == one.mass.tobytes()
    for word in ("selected", "left_out", "unmeasured", "total_pairs", "coincident"):
        assert np.array_equal(getattr(one, word), getattr(two, word)), word


def test_a_body_of_no_set_may_hold_anything_and_the_frame_changes_only_its_words():
    import n_body_problem_amd as nb
    P, V, counts = mref.gpu_inputs(128)
    B = len(counts)
    L = np.array(mref.gpu_labels(128, "interleaved-3-soft"))
    L[:, 20:40:3] = -1
    centre, velocity = mref.gpu_frames(128, True)
    with nb.BatchedSystem(B, 128, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        plain = batch.mutual_gravity(L, sets=3, softening=0.0625)
        moved = batch.mutual_gravity(L, sets=3, softening=0.0625, centre=centre)
        boosted = batch.mutual_gravity(L, sets=3, softening=0.0625, velocity=velocity)
        garbage_p, garbage_v = np.array(P), np.array(V)
        garbage_p[:, 20:40:3, :] = np.nan
        garbage_v[:, 23, :] = -np.inf
        batch.set_state(garbage_p, garbage_v)
        garbage = batch.mutual_gravity(L, sets=3, softening=0.0625)
    assert garbage.systems.tobytes() == plain.systems.tobytes() and garbage.entries.tobytes() == plain.entries.tobytes()
    assert plain.left_out.max() > 0 and plain.total_pairs.sum() > 0
    for word in ("pairs", "potential", "force", "power"):           # the centre: torque and virial alone
        assert moved.entries[word].tobytes() == plain.entries[word].tobytes(), word
    assert moved.entries["torque"].tobytes() != plain.entries["torque"].tobytes()
    assert moved.entries["virial"].tobytes() != plain.entries["virial"].tobytes()
    for word in ("pairs", "potential", "force", "torque", "virial"):  # the velocity: power alone
        assert boosted.entries[word].tobytes() == plain.entries[word].tobytes(), word
    assert boosted.entries["power"].tobytes() != plain.entries["power"].tobytes()
    assert moved.systems.tobytes() == plain.systems.tobytes() == boosted.systems.tobytes()


def test_the_closed_form_holds_on_the_device_bit_for_bit():
    import n_body_problem_amd as nb
    pos, vel, labels, centre, velocity = mref.closed_form_state()
    n = len(pos)
    P, V = np.zeros((2, 64, 4), np.float32), np.zeros((2, 64, 4), np.float32)
    P[1, :n], V[1, :n] = pos, vel
    L = np.full((2, 64), -1)
    L[1, :n] = labels
    with nb.BatchedSystem(2, 64, counts=[0, n]) as batch:
        batch.set_state(P, V)
        res = batch.mutual_gravity(L, sets=2, centre=np.stack([centre, centre]), velocity=velocity)
    for (a, b), words in mref.closed_form().items():
        assert mref.floats_of(res.entries)[1, a, b].tobytes() == words.tobytes(), (a, b, mref.floats_of(res.entries)[1, a, b], words)
    assert res.members[1].tolist() == [1, 36] and res.mass[1, 0] == 4.0 and res.total_pairs[1] == 36 + 36 + 36 * 35
    assert res.systems[0].tobytes() == mref.reference(P[0], V[0], 0, L[0], 2)["system"].tobytes() and not res.entries[0].tobytes().strip(b"\0")


# ---- 4. placement -----------------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bytes_in_any_slot_batch_and_capacity():
    import n_body_problem_amd as nb
    n = 150
    body_p, body_v = mref.state(n, 4242)
    labels = mref.labelling("ranks", n, n, 8, 4243)
    centre, velocity = mref.CENTRE, mref.VELOCITY
    ref = mref.reference(body_p, body_v, n, labels, 8, 0.02, centre, velocity)
    first = None
    for capacity, B, slot in ((256, 1, 0), (256, 5, 3), (1024, 2, 1), (4096, 1, 0), (192, 3, 2)):
        P, V = np.full((B, capacity, 4), 7.0, np.float32), np.full((B, capacity, 4), -3.0, np.float32)
        L = np.zeros((B, capacity), np.int64)
        counts = [min(40 + 9 * s, capacity) for s in range(B)]
        P[slot, :n], V[slot, :n], L[slot, :n], counts[slot] = body_p, body_v, labels, n
        C, W = np.tile(centre + 1.0, (B, 1)), np.tile(velocity - 1.0, (B, 1))
        C[slot], W[slot] = centre, velocity
        with nb.BatchedSystem(B, capacity, counts=counts) as batch:
            batch.set_state(P, V)
            res = batch.mutual_gravity(L, sets=8, softening=0.02, centre=C, velocity=W)
        got = res.systems[slot].tobytes() + res.entries[slot].tobytes()
        if first is None:
            first = got
            assert res.systems[slot].tobytes() == ref["system"].tobytes() and mref.error_of(res.entries[slot], ref) <= mref.BOUND
            assert res.total_pairs[slot] > 0
        assert got == first, (capacity, B, slot)


# ---- 5. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            labels = np.arange(P.shape[1])[None, :] % 3 - 1 + np.zeros((P.shape[0], 1), np.int64)
            b.mutual_gravity(labels, softening=0.01, centre="density")
            b.mutual_gravity(labels % 2, sets=8, matrix=False)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_mutual_gravity_evolve_is_the_two_evolves_alone_bit_for_bit():
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


def test_a_call_with_8_sets_after_one_with_1_set_agrees_with_a_fresh_handle():
    import n_body_problem_amd as nb
    P, V, counts = mref.gpu_inputs(128)
    B = len(counts)
    L1, L8 = mref.gpu_labels(128, "interleaved-1"), mref.gpu_labels(128, "contiguous-8-soft-frame")
    centre, velocity = mref.gpu_frames(128, True)
    with nb.BatchedSystem(B, 128, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        small = batch.mutual_gravity(L1, sets=1)
        check_against_reference(small, mref.gpu_reference(128, "interleaved-1"), "1 set first")
        grown = batch.mutual_gravity(L8, sets=8, softening=0.05, centre=centre, velocity=velocity)
        again = batch.mutual_gravity(L1)                            # sets from the labels
    with nb.BatchedSystem(B, 128, counts=counts) as fresh:
        fresh.set_state(np.array(P), np.array(V))
        alone = fresh.mutual_gravity(L8, sets=8, softening=0.05, centre=centre, velocity=velocity)
    check_against_reference(grown, mref.gpu_reference(128, "contiguous-8-soft-frame"), "8 sets after 1")
    assert grown.systems.tobytes() == alone.systems.tobytes() and grown.entries.tobytes() == alone.entries.tobytes()
    assert again.systems.tobytes() == small.systems.tobytes() and again.entries.tobytes() == small.entries.tobytes()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, V, counts = mref.gpu_inputs(64)
    B = len(counts)
    L = mref.gpu_labels(64, "interleaved-3-soft")
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        before = batch.mutual_gravity(L, sets=3, softening=0.0625)
        state = [a.copy() for a in batch.download()]
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchMutualGravitySystem * B)()
        out[2].selected = -7                                       # a refused call writes nothing
        wire = np.ascontiguousarray(mref.wire_labels(L))
        good = wire.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
        bad = wire.copy()
        bad[4, 17] = 3                                             # not below 3 sets, not 255
        bad = bad.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
        doubles = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))   # noqa: E731
        frame = np.zeros((B, 3))
        nan_frame, inf_frame = frame.copy(), frame.copy()
        nan_frame[5, 1], inf_frame[2, 0] = np.nan, np.inf
        cases = [((None, vel, 3, good, 0.0, None, None, out, None), b"NULL argument"),
                 ((pos, None, 3, good, 0.0, None, None, out, None), b"NULL argument"),
                 ((pos, vel, 3, None, 0.0, None, None, out, None), b"NULL argument"),
                 ((pos, vel, 3, good, 0.0, None, None, None, None), b"NULL argument"),
                 ((pos, vel, 0, good, 0.0, None, None, out, None), b"sets must be 1 ... 8"),
                 ((pos, vel, 9, good, 0.0, None, None, out, None), b"sets must be 1 ... 8"),
                 ((pos, vel, 2, good, 0.0, None, None, out, None), b"the label 2 of body 2 of system 0 must be below sets (2) or 255"),
                 ((pos, vel, 3, bad, 0.0, None, None, out, None), b"the label 3 of body 17 of system 4 must be below sets (3) or 255"),
                 ((pos, vel, 3, good, -1.0, None, None, out, None), b"softening must be finite, 0 or >= NBODY_MIN_SOFTENING"),
                 ((pos, vel, 3, good, 1e-12, None, None, out, None), b"softening must be finite, 0 or >= NBODY_MIN_SOFTENING"),
                 ((pos, vel, 3, good, float("nan"), None, None, out, None), b"softening must be finite"),
                 ((pos, vel, 3, good, 0.0, doubles(nan_frame), None, out, None), b"the centre of system 5 must be finite"),
                 ((pos, vel, 3, good, 0.0, None, doubles(inf_frame), out, None), b"the velocity of system 2 must be finite")]
        for args, message in cases:
            assert lib.nbody_batch_mutual_gravity(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_mutual_gravity: ") and message in error, (args, error)
            assert out[2].selected == -7
        assert lib.nbody_batch_mutual_gravity(None, pos, vel, 3, good, 0.0, None, None, out, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_mutual_gravity: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="sets must be"):
            batch.mutual_gravity(L, sets=9)
        with pytest.raises(ValueError, match="sets must be"):
            batch.mutual_gravity(np.full((B, 64), 8))
        with pytest.raises(ValueError, match="of body 2 of system 0 must be below sets"):
            batch.mutual_gravity(L, sets=2)
        with pytest.raises(ValueError, match="labels must have shape"):
            batch.mutual_gravity(L[:, :63])
        with pytest.raises(ValueError, match="labels must be integers"):
            batch.mutual_gravity(L.astype(np.float32))
        with pytest.raises(ValueError, match="overlap"):
            batch.mutual_gravity((L >= 0, L == 1))
        with pytest.raises(ValueError, match="centre must have shape"):
            batch.mutual_gravity(L, centre=np.zeros((B + 1, 3)))
        with pytest.raises(nb.NBodyError, match="nbody_batch_mutual_gravity: softening must be finite"):
            batch.mutual_gravity(L, softening=-0.5)
        assert lib.nbody_batch_mutual_gravity(h, pos, vel, 3, good, 0.0625, None, None, out, None) == _lib.NBODY_OK
        assert out[2].selected == counts[2] and out[2].sets == 3
        after = batch.mutual_gravity(L, sets=3, softening=0.0625)
        for a, b in zip(state, batch.download()):
            assert a.tobytes() == b.tobytes()
    assert after.systems.tobytes() == before.systems.tobytes() and after.entries.tobytes() == before.entries.tobytes()
