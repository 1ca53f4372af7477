"""GPU: the pair velocity statistics of batched ensembles (BatchedSystem.pair_velocities,
include/nbody_batch_pair_velocities.h).

1. Every word against the reference (hermite_pair_velocities_ref: IEEE doubles in the pinned order, the bin decision from
   hermite_correlation_ref).  Capacities 64, 128, 256, 1024 and 4096; counts 0, 1, 2, 3, 63, 64, 65, 129, 257 and the capacity
   as far as the capacity holds them in one batch, and at 4096 one system of 4096 and one of 1025 bodies at 8 bins only; bins 1,
   G - 1, G, G + 1 and 32 for the G = 8 built; both weights, the masks, per-system edges.  The integers are equal; weight,
   r2, rv and v2 (+, -, x alone) are bit-equal; r1, vr1, vr2, vt2 and v1, which pass through the device's square root and
   division, are held to hermite_pair_velocities_ref.BOUND = 2.72e-14 of the sum of their absolute addends: four times the
   spread 6.8e-15 that the reference itself shows when every root and quotient is moved by up to one ulp at random
   (test_batch_pair_velocities_cpu.py measures it again).  Whether the device was in fact bit-equal is printed, not asserted.
   No case is left out: the bin decision is an exact fp32 chain on these inputs and needs no margin.
2. Against shipped code: on finite velocities every integer of the system record and every count is correlation()'s.
3. Identities exact by construction: rigid rotation, Hubble flow, rows and sources swapped, bins=False.
4. Placement: one system's records are the same bytes in another slot, batch size and capacity.
5. Non-interference: evolve, pair_velocities, evolve is the two evolves alone; 32 bins after 1 bin agree with a fresh handle.
6. Errors: each refused with the function named, leaving the state and a later call untouched."""
import ctypes

import numpy as np
import pytest

import hermite_pair_velocities_ref as pref

pytestmark = pytest.mark.gpu

WEIGHT_NAMES = {pref.WEIGHT_MASS: "mass", pref.WEIGHT_NUMBER: "number"}
SYSTEM_INTEGERS = ("rows", "sources", "both", "pairs", "below", "above", "unmeasured")


def check_against_reference(res, refs, tag):
    """Returns (worst error, whether the rooted words were bit-equal)."""
    worst, equal = 0.0, True
    for s, ref in enumerate(refs):
        assert res.systems[s].tobytes() == ref["system"].tobytes(), (tag, s, res.systems[s], ref["system"])
        got = res.bin_records[s]
        for word in pref.INTEGERS:
            assert np.array_equal(got[word], ref["bins"][word]), (tag, s, word, got[word], ref["bins"][word])
        for word in pref.EXACT_WORDS:
            assert got[word].tobytes() == ref["bins"][word].tobytes(), (tag, s, word, got[word], ref["bins"][word])
        error = pref.error_of(got, ref)
        assert error <= pref.BOUND, (tag, s, error)
        worst = max(worst, error)
        equal = equal and all(got[w].tobytes() == ref["bins"][w].tobytes() for w in pref.ROOTED_WORDS)
        assert res.below[s] + got["count"].sum() + res.above[s] + res.unmeasured[s] == res.pairs[s]
        assert res.pairs[s] == int(res.rows[s]) * int(res.sources[s]) - int(res.both[s])
        assert (got["approaching"] + got["receding"] <= got["count"]).all()
        empty = got["count"] == 0
        assert got[empty].tobytes() == np.zeros(int(empty.sum()), pref.BIN_DTYPE).tobytes(), (tag, s)   # an empty bin reads 0
    return worst, equal


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", pref.CAPACITIES)
def test_every_word_against_the_reference(capacity):
    """Observed on an MI355X: see the module's docstring and profiles/batch_rate_pair_velocities.txt."""
    import n_body_problem_amd as nb
    P, V, counts, _ = pref.gpu_inputs(capacity)
    B = len(counts)
    worst, equal, compared = 0.0, True, 0
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))                  # copies: the shared inputs are read-only
        for name, bins, weight, kind, per_system in pref.cases_of(capacity):
            rows, sources = pref.gpu_masks(capacity, kind)
            edges = pref.gpu_edges(capacity, bins, per_system)
            res = batch.pair_velocities(edges, rows=rows, sources=sources, weight=WEIGHT_NAMES[weight])
            refs = pref.gpu_reference(capacity, name)
            assert res.bin_records.shape == (B, bins) and res.bins == bins and res.count.dtype == np.int64 and res.v2.dtype == np.float64
            error, same = check_against_reference(res, refs, (capacity, name))
            print(f"capacity {capacity} {name}: pairs {res.pairs.tolist()}, unmeasured {res.unmeasured.tolist()}, largest error of "
                  f"r1, vr1, vr2, vt2, v1 {error:.3g} (bound {pref.BOUND:.3g}); {'bit-equal' if same else 'not bit-equal'}")
            worst, equal, compared = max(worst, error), equal and same, compared + 1
            lean = batch.pair_velocities(edges, rows=rows, sources=sources, weight=WEIGHT_NAMES[weight], bins=False)
            assert lean.bin_records is None and lean.count is None and lean.systems.tobytes() == res.systems.tobytes(), name
        if capacity != 4096:                                       # uint8 masks and torch masks and edges are the bool ones
            import torch
            rows, sources = pref.gpu_masks(capacity, "sparse")
            res = batch.pair_velocities(torch.as_tensor(pref.shared_edges(pref.G_BUILT + 1)), rows=rows.astype(np.uint8),
                                        sources=torch.as_tensor(np.array(sources)), weight="mass")
            check_against_reference(res, pref.gpu_reference(capacity, "mass-sparse"), (capacity, "uint8 and torch"))
    assert compared == len(pref.cases_of(capacity))
    print(f"capacity {capacity}: worst error {worst:.3g} of the bound {pref.BOUND:.3g}; the device was "
          f"{'bit-equal' if equal else 'not bit-equal'} to the reference")
    last = pref.gpu_reference(capacity, pref.cases_of(capacity)[-1][0])[-1 if capacity != 4096 else 0]
    assert last["system"]["below"] > 0 and last["system"]["unmeasured"] > 0 and (last["bins"]["count"] > 0).any()   # the inputs work


# ---- 2. against shipped code ----------------------------------------------------------------------------------------------------
def test_on_finite_velocities_every_integer_is_correlations():
    import n_body_problem_amd as nb
    n, capacity, B = 300, 320, 3
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    for s in range(B):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=190 + s)
    P[1, 7, 2] = np.nan                                             # a coordinate: unmeasured in both
    rng = np.random.default_rng(191)
    rows, sources = rng.random((B, capacity)) < 0.5, rng.random((B, capacity)) < 0.3
    with nb.BatchedSystem(B, capacity, counts=[n, n, n - 9]) as batch:
        batch.set_state(P, V)
        for edges in (np.array([0.0, 0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2], np.float32), np.linspace(0.01, 4.0, 33).astype(np.float32),
                      np.array([0.3, 0.9], np.float32)):
            for r, s in ((None, None), (rows, sources), (rows, rows), (None, sources)):
                ours = batch.pair_velocities(edges, rows=r, sources=s, weight="mass")
                theirs = batch.correlation(edges, rows=r, sources=s)
                for word in SYSTEM_INTEGERS:
                    assert np.array_equal(getattr(ours, word), getattr(theirs, word)), word
                assert np.array_equal(ours.count, theirs.counts) and ours.count.sum() > 0 and np.array_equal(ours.auto, theirs.auto)
        assert ours.unmeasured[1] > 0


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def identity_state(n, capacity, seed, velocity):
    """Positions on 1 / 8 within +-4 (no subnormals, every product exact); velocity(x) gives the velocity words."""
    rng = np.random.default_rng(seed)
    P, V = np.zeros((1, capacity, 4), np.float32), np.zeros((1, capacity, 4), np.float32)
    P[0, :n, :3] = rng.integers(-32, 33, size=(n, 3)) / 8.0
    P[0, :n, 3] = rng.integers(1, 5, size=n) / 2.0
    V[0, :n, :3] = velocity(P[0, :n, :3])
    return P, V


@pytest.mark.parametrize("capacity,n", ((128, 100), (1024, 700)))
def test_rigid_rotation_has_no_radial_velocity_and_a_hubble_flow_has_no_other(capacity, n):
    import n_body_problem_amd as nb
    edges = np.array([0.0, 1.0, 2.0, 3.5, 5.0, 9.0], np.float32)
    P, V = identity_state(n, capacity, 300 + capacity, lambda x: np.stack([-x[:, 1], x[:, 0], np.zeros(len(x))], axis=1))
    with nb.BatchedSystem(1, capacity, counts=[n]) as batch:
        batch.set_state(P, V)
        for weight in ("number", "mass"):
            res = batch.pair_velocities(edges, weight=weight)
            assert res.count.sum() > 0 and not res.rv.any() and not res.vr1.any() and not res.vr2.any()
            assert not res.approaching.any() and not res.receding.any()
            assert res.vt2.tobytes() == res.v2.tobytes()
    P, V = identity_state(n, capacity, 400 + capacity, lambda x: 0.5 * x)
    with nb.BatchedSystem(1, capacity, counts=[n]) as batch:
        batch.set_state(P, V)
        rng = np.random.default_rng(5)
        rows, sources = rng.random((1, capacity)) < 0.5, rng.random((1, capacity)) < 0.5
        for weight in ("number", "mass"):
            res = batch.pair_velocities(edges, weight=weight)
            assert res.rv.tobytes() == (0.5 * res.r2).tobytes() and res.v2.tobytes() == (0.25 * res.r2).tobytes()
            assert np.array_equal(res.receding, res.count) and not res.approaching.any() and res.count.sum() > 0
            # vr1 against 0.5 r1: the sum of the absolute addends of vr1 is vr1 itself here (every vr > 0)
            assert (np.abs(res.vr1 - 0.5 * res.r1) <= pref.BOUND * np.abs(res.vr1)).all(), (res.vr1, 0.5 * res.r1)
            print(f"capacity {capacity} {weight}: |vr1 - r1 / 2| / vr1 at most "
                  f"{np.max(np.abs(res.vr1 - 0.5 * res.r1)[res.count > 0] / res.vr1[res.count > 0]):.3g}")
            # rows and sources swapped: the same integers
            there, back = batch.pair_velocities(edges, rows=rows, sources=sources, weight=weight), \
                batch.pair_velocities(edges, rows=sources, sources=rows, weight=weight)
            for word in pref.INTEGERS:
                assert np.array_equal(getattr(there, word), getattr(back, word)), word
            for word in ("pairs", "below", "above", "unmeasured", "both"):
                assert np.array_equal(getattr(there, word), getattr(back, word)), word
            assert np.array_equal(there.rows, back.sources) and np.array_equal(there.sources, back.rows)
            lean = batch.pair_velocities(edges, rows=rows, sources=sources, weight=weight, bins=False)
            assert lean.systems.tobytes() == there.systems.tobytes()


# ---- 4. placement -----------------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bytes_in_another_slot_batch_size_and_capacity():
    import n_body_problem_amd as nb
    rng = np.random.default_rng(173)
    for name, n, state in (("gaussian", 63, pref.gaussian_state), ("lattice", 37, pref.lattice_state)):
        body_p, body_v = state(n, 500 + n)
        rows, sources = rng.random(n) < 0.6, rng.random(n) < 0.6
        mine = (0.25 + 0.75 * np.arange(18)).astype(np.float32)
        first = None
        for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (256, 4, 1), (1024, 2, 1), (4096, 2, 1)):
            P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
            counts = [min(capacity, 11 + 3 * s) for s in range(B)]
            for s in range(B):
                P[s, :counts[s]], V[s, :counts[s]] = pref.gaussian_state(counts[s], 40 + s)
            P[slot, :n], V[slot, :n], counts[slot] = body_p, body_v, n
            R, S = rng.random((B, capacity)) < 0.5, rng.random((B, capacity)) < 0.5
            R[slot, :n], S[slot, :n] = rows, sources
            edges = (1.0 + np.arange(B)[:, None] + 2.0 * np.arange(18)[None, :]).astype(np.float32)
            edges[slot] = mine
            with nb.BatchedSystem(B, capacity, counts=counts) as batch:
                batch.set_state(P, V)
                res = batch.pair_velocities(edges, rows=R, sources=S, weight="mass")
            got = res.systems[slot].tobytes() + res.bin_records[slot].tobytes()
            if first is None:
                first = got
                ref = pref.reference(body_p, body_v, n, pref.GAUSSIAN_Q, mine, rows, sources, pref.WEIGHT_MASS)
                assert res.systems[slot].tobytes() == ref["system"].tobytes() and pref.exact_equal(res.bin_records[slot], ref["bins"])
                assert pref.error_of(res.bin_records[slot], ref) <= pref.BOUND and res.count[slot].sum() > 0
            assert got == first, (name, capacity, B)


# ---- 5. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.pair_velocities(np.linspace(0.0, 3.0, 33), weight="mass")
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.pair_velocities([0.1, 1.0], rows=mask, sources=~mask, bins=False)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_pair_velocities_evolve_is_the_two_evolves_alone_bit_for_bit():
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


def test_a_call_with_32_bins_after_one_with_1_bin_agrees_with_a_fresh_handle():
    import n_body_problem_amd as nb
    P, V, counts, _ = pref.gpu_inputs(128)
    B = len(counts)
    rows, sources = pref.gpu_masks(128, "disjoint")
    edges = pref.gpu_edges(128, 32, True)
    with nb.BatchedSystem(B, 128, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        small = batch.pair_velocities(pref.shared_edges(1))
        check_against_reference(small, pref.gpu_reference(128, "bins1"), "1 bin first")
        grown = batch.pair_velocities(edges, rows=rows, sources=sources, weight="mass")
        again = batch.pair_velocities(pref.shared_edges(1))
    with nb.BatchedSystem(B, 128, counts=counts) as fresh:
        fresh.set_state(np.array(P), np.array(V))
        alone = fresh.pair_velocities(edges, rows=rows, sources=sources, weight="mass")
    check_against_reference(grown, pref.gpu_reference(128, "mass-disjoint-own-edges"), "32 bins after 1")
    assert grown.systems.tobytes() == alone.systems.tobytes() and grown.bin_records.tobytes() == alone.bin_records.tobytes()
    assert again.systems.tobytes() == small.systems.tobytes() and again.bin_records.tobytes() == small.bin_records.tobytes()


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, V, counts, _ = pref.gpu_inputs(64)
    B = len(counts)
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        before = batch.pair_velocities(pref.shared_edges(8), weight="mass")
        state = [a.copy() for a in batch.download()]
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchPairVelocitiesSystem * B)()
        out[2].rows = -7                                           # a refused call writes nothing
        floats = lambda values: (ctypes.c_float * len(values))(*values)   # noqa: E731
        good = floats([0.0, 1.0, 2.0])
        tied = np.tile(np.array([0.0, 1.0, 2.0], np.float32), (B, 1))
        tied[3, 2] = 1.0
        cases = [((None, vel, 2, good, 0, None, None, 1, out, None), b"NULL argument"),
                 ((pos, None, 2, good, 0, None, None, 1, out, None), b"NULL argument"),
                 ((pos, vel, 2, None, 0, None, None, 1, out, None), b"NULL argument"),
                 ((pos, vel, 2, good, 0, None, None, 1, None, None), b"NULL argument"),
                 ((pos, vel, 0, good, 0, None, None, 1, out, None), b"bins must be 1 ... 32"),
                 ((pos, vel, 33, good, 0, None, None, 1, out, None), b"bins must be 1 ... 32"),
                 ((pos, vel, 2, good, 0, None, None, 2, out, None), b"weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER"),
                 ((pos, vel, 2, good, 0, None, None, -1, out, None), b"weight must be"),
                 ((pos, vel, 2, floats([-0.5, 1.0, 2.0]), 0, None, None, 1, out, None), b"edge 0 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, floats([0.0, float("nan"), 2.0]), 0, None, None, 0, out, None), b"edge 1 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, floats([0.0, 1.0, float("inf")]), 0, None, None, 0, out, None), b"edge 2 of all systems must be finite and >= 0"),
                 ((pos, vel, 2, floats([0.0, 1.0, 1.0]), 0, None, None, 1, out, None), b"edge 2 of all systems is not above edge 1"),
                 ((pos, vel, 2, floats(tied.ravel().tolist()), 1, None, None, 1, out, None),
                  b"edge 2 of system 3 is not above edge 1: the edges must be strictly ascending")]
        for args, message in cases:
            assert lib.nbody_batch_pair_velocities(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_pair_velocities: ") and message in error, (args, error)
            assert out[2].rows == -7
        assert lib.nbody_batch_pair_velocities(None, pos, vel, 2, good, 0, None, None, 1, out, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_pair_velocities: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="bins must be"):
            batch.pair_velocities(np.arange(34.0))
        with pytest.raises(ValueError, match="bins must be"):
            batch.pair_velocities([1.0])
        with pytest.raises(ValueError, match="edges must have shape"):
            batch.pair_velocities(np.zeros((B + 1, 3)))
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.pair_velocities([0.0, 1.0], rows=np.ones((B, 64), np.int32))
        with pytest.raises(ValueError, match="shape"):
            batch.pair_velocities([0.0, 1.0], sources=np.ones((B, 63), bool))
        with pytest.raises(ValueError, match="weight must be one of"):
            batch.pair_velocities([0.0, 1.0], weight="charge")
        with pytest.raises(nb.NBodyError, match="nbody_batch_pair_velocities: edge 1 of all systems is not above edge 0"):
            batch.pair_velocities([1.0, 0.5])
        assert lib.nbody_batch_pair_velocities(h, pos, vel, 2, good, 0, None, None, 1, out, None) == _lib.NBODY_OK
        assert out[2].rows == counts[2] and out[2].bins == 2 and out[2].weight == 1 and out[2].reserved == 0
        after = batch.pair_velocities(pref.shared_edges(8), weight="mass")
        for a, b in zip(state, batch.download()):
            assert a.tobytes() == b.tobytes()
    assert after.systems.tobytes() == before.systems.tobytes() and after.bin_records.tobytes() == before.bin_records.tobytes()
