"""GPU: the contact lists of batched ensembles (BatchedSystem.contacts, include/nbody_batch_contacts.h).  Every word of every
record and every list entry equal the reference (hermite_contacts_ref: the full matrix of the exact integer r2) exactly, at
every workgroup shape, with ragged counts, in both modes, with and without a subset and at list capacities that count only,
that cut a system in the middle of a row and that hold everything; a system's result is the same bytes wherever it runs; on
Plummer spheres the degrees, the number of pairs, the connected components and the short tree edges are what neighbours(),
correlation(), groups() and spanning_tree() say; under per-body radii the closest contact is the pair evolve() stops for; the
call disturbs no evolve; the buffers grow; and every error is reported.

Capacities: 64 (one wave, one row per lane), 128 (two rows per lane), 320 (four rows per lane, two waves: the placement
across waves and across q), 4096 (sixteen waves, 64 KiB of dynamic LDS: the raised limit).  Counts 0, 1, 2, 65 and the
capacity.  The inputs are integers, so every r2 and every threshold is exact (test_batch_contacts_cpu.py checks the premise
and that the inputs contain what they are there for): the exact agreement asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_contacts_ref as kref

pytestmark = pytest.mark.gpu


def check_against_reference(res, refs, capacity, tag, bodies=True):
    """Every word of every record and every entry; the order of the list; first as the exclusive sum; the pads."""
    for s, ref in enumerate(refs):
        want = kref.system_record(ref, capacity)
        assert res.systems[s].tobytes() == want.tobytes(), (tag, s, res.systems[s], want)
        if bodies:
            assert res.body_records[s].tobytes() == ref["bodies"].tobytes(), (tag, s)
            assert np.array_equal(res.first[s], np.concatenate([[0], np.cumsum(res.upper[s])[:-1]]))
            kref.check_identity(res.body_records[s], int(res.pairs[s]))
        if res.entries is not None:
            assert res.entries.shape == (len(refs), capacity)
            assert res.entries[s].tobytes() == kref.listed(ref, capacity).tobytes(), (tag, s)
            m = int(res.stored[s])
            key = res.i[s, :m].astype(np.int64) * 4096 + res.j[s, :m]
            assert (res.i[s, :m] < res.j[s, :m]).all() and (np.diff(key) > 0).all(), (tag, s)      # strictly ascending in (i, j)
            assert (res.i[s, m:] == -1).all() and (res.j[s, m:] == -1).all() and np.isposinf(res.r2[s, m:]).all()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", kref.CAPACITIES)
def test_the_records_and_the_list_equal_the_reference_exactly(capacity):
    import n_body_problem_amd as nb
    P, counts, _ = kref.gpu_inputs(capacity)
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))             # copies: the shared inputs are read-only
        for mode in kref.MODES:
            for with_subset in (False, True):
                kw = kref.gpu_arguments(capacity, mode, with_subset)
                refs = kref.gpu_reference(capacity, mode, with_subset)
                most = max(r["system"]["pairs"] for r in refs)
                cut = kref.truncating_capacity(refs)
                tag = (capacity, mode, with_subset)
                counted = batch.contacts(capacity=0, **kw)
                print(f"{tag}: pairs {counted.pairs.tolist()} (reference {[r['system']['pairs'] for r in refs]}), touching "
                      f"{counted.touching.tolist()}, max_degree {counted.max_degree.tolist()}, closest {counted.closest.tolist()}; "
                      f"capacities 0, {cut}, {most}")
                assert counted.entries.shape == (B, 0) and not counted.stored.any()
                check_against_reference(counted, refs, 0, tag + (0,))
                truncated = batch.contacts(capacity=cut, **kw)
                check_against_reference(truncated, refs, cut, tag + (cut,))
                assert truncated.truncated.any() and truncated.stored.max() == cut
                full = batch.contacts(capacity=most, **kw)
                check_against_reference(full, refs, most, tag + (most,))
                assert not full.truncated.any() and np.array_equal(full.stored, full.pairs)
                for s in range(B):
                    assert full.pairs_of(s).tolist() == np.stack([refs[s]["list"]["i"], refs[s]["list"]["j"]], axis=1).tolist()
                # capacity=None: the full list; bodies=False: the same system records; lists=False: the counting call
                auto = batch.contacts(**kw)
                assert auto.systems.tobytes() == full.systems.tobytes() and auto.entries.tobytes() == full.entries.tobytes()
                lean = batch.contacts(capacity=most, bodies=False, **kw)
                assert lean.degree is None and lean.systems.tobytes() == full.systems.tobytes() and lean.entries.tobytes() == full.entries.tobytes()
                # lists=False is the counting call, so `stored` is 0 as at capacity 0: the same bytes as that call's records, and
                # the same as the listing call's in every other word
                listless = batch.contacts(lists=False, **kw)
                assert listless.entries is None and listless.systems.tobytes() == counted.systems.tobytes()
                for name in full.systems.dtype.names:
                    assert name == "stored" or listless.systems[name].tobytes() == full.systems[name].tobytes(), name
                assert listless.body_records.tobytes() == full.body_records.tobytes()
                bare = batch.contacts(lists=False, bodies=False, **kw)
                assert bare.systems.tobytes() == counted.systems.tobytes() and bare.degree is None
        # uint8 and torch subsets, a torch radius and a scalar one are the numpy ones
        import torch
        subset = kref.gpu_subset(capacity)
        refs = kref.gpu_reference(capacity, "radii", True)
        res = batch.contacts(radii=torch.as_tensor(np.array(kref.gpu_inputs(capacity)[2])), subset=torch.as_tensor(np.array(subset)))
        check_against_reference(res, refs, max(r["system"]["pairs"] for r in refs), (capacity, "torch"))
        res = batch.contacts(radii=kref.gpu_inputs(capacity)[2], subset=subset.astype(np.uint8), lists=False)
        check_against_reference(res, refs, 0, (capacity, "uint8"))
        scalar = batch.contacts(3.0, lists=False)
        each = batch.contacts(np.full(B, 3.0, np.float32), lists=False)
        assert scalar.systems.tobytes() == each.systems.tobytes() and scalar.pairs[4] == kref.gpu_reference(capacity, "radius", False)[4]["system"]["pairs"]


# ---- 2. placement -----------------------------------------------------------------------------------------------------------------
def placement_systems():
    """name -> (bodies, subset, radii): three systems with contacts in both modes."""
    line = np.ones((50, 4), np.float32)
    line[:, :3] = [(2 * i, 0, 0) for i in range(50)]
    rng = np.random.default_rng(73)
    out = {}
    for name, body in {"narrow": kref.cube(64, 71, 4), "wide": kref.cube(37, 72, 6), "line": line}.items():
        out[name] = (body, rng.random(len(body)) < 0.8, rng.integers(0, 3, len(body)).astype(np.float32))
    return out


def placement_reference(body, take, mine, mode):
    n = len(body)
    return kref.reference(body, n, n, radius=3.0 if mode == "radius" else None, radii=mine if mode == "radii" else None, subset=take)


def test_a_systems_result_is_the_same_bytes_in_another_slot_batch_size_and_capacity():
    import n_body_problem_amd as nb
    rng = np.random.default_rng(74)
    for name, (body, take, mine) in placement_systems().items():
        n = len(body)
        for mode in kref.MODES:
            ref = placement_reference(body, take, mine, mode)
            room = ref["system"]["pairs"] + 2
            first = None
            for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (320, 4, 1), (4096, 2, 1)):
                P = np.zeros((B, capacity, 4), np.float32)
                counts = [min(capacity, 11 + 3 * s) for s in range(B)]
                for s in range(B):
                    P[s, :counts[s]] = kref.cube(counts[s], 40 + s, 3)
                P[slot, :n], counts[slot] = body, n
                S, R = rng.random((B, capacity)) < 0.5, rng.integers(0, 3, (B, capacity)).astype(np.float32)
                S[slot, :n], R[slot, :n] = take, mine
                radius = (1.0 + np.arange(B)).astype(np.float32)
                radius[slot] = 3.0
                with nb.BatchedSystem(B, capacity, counts=counts) as batch:
                    batch.set_state(P, np.zeros_like(P))
                    res = batch.contacts(radius if mode == "radius" else None, radii=R if mode == "radii" else None, subset=S, capacity=room)
                assert res.body_records[slot, :n].tobytes() == ref["bodies"].tobytes(), (name, mode, capacity, B)
                rest = res.body_records[slot, n:]
                assert not rest["degree"].any() and not rest["upper"].any() and (rest["first"] == ref["system"]["pairs"]).all() and (rest["nearest"] == -1).all()
                got = res.systems[slot].tobytes() + res.body_records[slot, :n].tobytes() + res.entries[slot].tobytes()
                assert res.systems[slot].tobytes() == kref.system_record(ref, room).tobytes() and res.entries[slot].tobytes() == kref.listed(ref, room).tobytes()
                if first is None:
                    first = got
                assert got == first, (name, mode, capacity, B)
            assert ref["system"]["pairs"] > 0


# ---- 3. against code that ships -------------------------------------------------------------------------------------------------
def components(n, pairs):
    """The label of every body under a union-find over the listed edges: the lowest index of its component."""
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)                          # the lower root stays a root: it is the lowest member
    return np.array([find(a) for a in range(n)])


def test_on_plummer_spheres_the_list_is_what_neighbours_correlation_groups_and_the_spanning_tree_say():
    """Coordinates that are no integers: no reference, but the siblings evaluate the same predicate on the same r2 and the
    same fp32 product b * b, so every comparison is exact."""
    import n_body_problem_amd as nb
    n, capacity, B = 300, 320, 3
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    for s in range(B):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=90 + s)
    with nb.BatchedSystem(B, capacity, counts=[n] * B) as batch:
        batch.set_state(P, V)
        tree = batch.spanning_tree()
        for b in (0.08, 0.25, 0.6):
            res = batch.contacts(b)
            print(f"b = {b}: pairs {res.pairs.tolist()}, touching {res.touching.tolist()}, max_degree {res.max_degree.tolist()}, "
                  f"closest {res.closest.tolist()} at {res.closest_distance.tolist()}")
            assert res.pairs.min() > 0 and not res.truncated.any()
            assert np.array_equal(res.degree, batch.neighbours(k=1, radius=b, lists=False).within)
            assert np.array_equal(2 * res.pairs, batch.correlation([b, 2 * b]).below)
            groups = batch.groups(b)
            b2 = np.float32(b) * np.float32(b)
            for s in range(B):
                labels = components(n, res.pairs_of(s))
                assert np.array_equal(labels, groups.group[s, :n]) and (groups.group[s, n:] == -1).all(), (b, s)
                listed = {(int(i), int(j)): r2 for i, j, r2 in zip(res.i[s], res.j[s], res.r2[s].view(np.uint32)) if i >= 0}
                ends, _ = tree.edges_of(s)
                short = [(int(i), int(j), bits) for (i, j), r2, bits in zip(ends, tree.r2[s], tree.r2[s].view(np.uint32)) if r2 <= b2]
                assert short and all(listed.get((i, j)) == bits for i, j, bits in short), (b, s)
                assert res.partners_of(s, int(res.closest[s, 0])).tolist().count(int(res.closest[s, 1])) == 1
                assert float(res.r2[s, :int(res.stored[s])].min()) == float(res.closest_r2[s])


# ---- 4. against evolve ------------------------------------------------------------------------------------------------------------
def evolve_inputs():
    """(capacity, counts, P, R): distinct integer positions and integer radii.  Systems 1 and 2 are stretched by 10, beyond
    every sum of two radii; system 3 has two bodies put beside each other with radii 1."""
    capacity, counts = 128, [128, 40, 2, 17, 100]
    rng = np.random.default_rng(404)
    P, R = np.zeros((len(counts), capacity, 4), np.float32), np.zeros((len(counts), capacity), np.float32)
    for s, n in enumerate(counts):
        spacing = 10 if s in (1, 2) else 1
        cells = rng.choice(13 ** 3, size=n, replace=False)        # distinct cells: no coincident bodies
        P[s, :n, 0], P[s, :n, 1], P[s, :n, 2] = spacing * (cells % 13), spacing * (cells // 13 % 13), spacing * (cells // 169)
        P[s, :n, 3] = 1.0 / n
        R[s, :n] = rng.integers(0, 3, n)
    P[3, 1, :3] = P[3, 0, :3] + [0, 0, 20]
    P[3, 2, :3] = P[3, 0, :3] + [0, 1, 20]
    R[3, 1] = R[3, 2] = 1
    return capacity, counts, P, R


def test_under_radii_the_closest_contact_is_the_pair_evolve_stops_for():
    """Distinct integer positions, zero velocities, no softening: evolve's first evaluation examines every pair against
    fmaf(S, S, 0) and stops for the touching pair of smallest r2, ties to the smallest i, then j -- `closest`.  A pair that does
    not touch is at least 1 in r2 beyond its threshold (integers), so the one short interval moves nothing across it."""
    import n_body_problem_amd as nb
    capacity, counts, P, R = evolve_inputs()
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts, integrator="hermite") as batch:
        batch.set_state(P, np.zeros_like(P))
        batch.set_radii(R)
        res = batch.contacts(radii=batch.radii())
        same = batch.contacts(radii=R)
        assert res.systems.tobytes() == same.systems.tobytes() and res.entries.tobytes() == same.entries.tobytes()
        for s, n in enumerate(counts):                             # the reference, and the margin of the non-contacts
            ref = kref.reference(P[s], n, capacity, radii=R[s])
            assert res.body_records[s].tobytes() == ref["bodies"].tobytes() and res.systems[s].tobytes() == kref.system_record(ref, res.capacity).tobytes()
            codes, t2 = kref.r2_codes(P[s], n), kref.thresholds(n, radii=R[s])
            off = ~np.eye(n, dtype=bool)
            assert (codes[off] > 0).all() and (codes[off & (codes > t2)] >= t2[off & (codes > t2)] + 1).all()
        batch.evolve(1, 2.0 ** -20, softening=0.0)
        stops = batch.stops()
        print(f"pairs {res.pairs.tolist()}, closest {res.closest.tolist()}, stopped {stops.stopped.tolist()}, pair {stops.pair.tolist()}")
        touching = res.pairs > 0
        assert touching.tolist() == [True, False, False, True, True]
        assert np.array_equal(stops.stopped, touching)
        assert np.array_equal(stops.pair[touching], res.closest[touching])


# ---- 5. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.contacts(0.3)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.contacts(radii=np.full((P.shape[0], P.shape[1]), 0.1, np.float32), subset=mask, capacity=5)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_contacts_evolve_is_the_two_evolves_alone_bit_for_bit():
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
    P, counts, R = kref.gpu_inputs(128)
    subset = kref.gpu_subset(128)
    refs = kref.gpu_reference(128, "radius", False)
    most = max(r["system"]["pairs"] for r in refs)
    other = kref.gpu_reference(128, "radii", True)
    room = max(r["system"]["pairs"] for r in other) + 7
    with nb.BatchedSystem(5, 128, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        small = batch.contacts(np.array(kref.RADIUS, np.float32), capacity=1, bodies=False)
        check_against_reference(small, refs, 1, "capacity 1 first", bodies=False)
        grown = batch.contacts(np.array(kref.RADIUS, np.float32), capacity=most)
        changed = batch.contacts(radii=R, subset=subset, capacity=room)
        again = batch.contacts(np.array(kref.RADIUS, np.float32), capacity=2)
    with nb.BatchedSystem(5, 128, counts=counts) as fresh:
        fresh.set_state(np.array(P), np.zeros_like(P))
        alone = fresh.contacts(radii=R, subset=subset, capacity=room)
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
    P, counts, R = kref.gpu_inputs(64)
    B = len(counts)
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        before = batch.contacts(np.array(kref.RADIUS, np.float32))
        lib, h, pos = batch._lib, batch._h, _ptr(batch.positions)
        out = (_lib.BatchContactSystem * B)()
        bodies = (_lib.BatchContactBody * (B * 64))()
        entries = (_lib.BatchContact * (B * 4))()
        out[2].bodies, bodies[70].degree, entries[9].i = -7, -7, -7   # a refused call writes nothing
        floats = lambda values: (ctypes.c_float * len(values))(*values)   # noqa: E731
        good, radii = floats(list(kref.RADIUS)), floats(R.ravel().tolist())

        def with_radius(s, value):
            r = list(kref.RADIUS)
            r[s] = value
            return floats(r)

        def with_radii(s, slot, value):
            r = np.array(R)
            r[s, slot] = value
            return floats(r.ravel().tolist())
        cases = [((None, good, None, None, 4, out, bodies, entries), b"NULL argument"),
                 ((pos, good, None, None, 4, None, bodies, entries), b"NULL argument"),
                 ((pos, good, radii, None, 4, out, bodies, entries), b"exactly one of radius and radii must be given"),
                 ((pos, None, None, None, 4, out, bodies, entries), b"exactly one of radius and radii must be given"),
                 ((pos, with_radius(3, -0.5), None, None, 4, out, bodies, entries), b"the radius of system 3 must be finite and >= 0"),
                 ((pos, with_radius(0, float("nan")), None, None, 4, out, bodies, entries), b"the radius of system 0 must be finite and >= 0"),
                 ((pos, with_radius(4, float("inf")), None, None, 4, out, bodies, entries), b"the radius of system 4 must be finite and >= 0"),
                 ((pos, None, with_radii(4, 63, -1.0), None, 4, out, bodies, entries), b"radius of system 4, slot 63"),
                 ((pos, None, with_radii(3, 0, float("nan")), None, 4, out, bodies, entries), b"radius of system 3, slot 0"),
                 ((pos, None, with_radii(2, 1, float("inf")), None, 4, out, bodies, entries), b"radius of system 2, slot 1"),
                 ((pos, good, None, None, -1, out, bodies, None), b"capacity must be >= 0"),
                 ((pos, good, None, None, 4, out, bodies, None), b"list_out must be given iff capacity > 0"),
                 ((pos, good, None, None, 0, out, bodies, entries), b"list_out must be given iff capacity > 0"),
                 ((pos, good, None, None, 2 ** 28 // B + 1, out, bodies, entries), b"n_systems x capacity must not exceed 2^28")]
        for args, message in cases:
            assert lib.nbody_batch_contacts(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_contacts: ") and message in error, (args, error)
            assert out[2].bodies == -7 and bodies[70].degree == -7 and entries[9].i == -7
        assert lib.nbody_batch_contacts(None, pos, good, None, None, 4, out, bodies, entries) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_contacts: batch is NULL" in lib.nbody_batch_last_error(None)
        # a radius beyond the count is never examined
        assert lib.nbody_batch_contacts(h, pos, None, with_radii(2, 2, float("nan")), None, 0, out, None, None) == _lib.NBODY_OK
        with pytest.raises(ValueError, match="exactly one of radius and radii"):
            batch.contacts()
        with pytest.raises(ValueError, match="exactly one of radius and radii"):
            batch.contacts(1.0, radii=R)
        with pytest.raises(ValueError, match="radius must be a scalar or have shape"):
            batch.contacts(np.ones(B + 1))
        with pytest.raises(ValueError, match="radii must have shape"):
            batch.contacts(radii=np.ones((B, 63), np.float32))
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.contacts(1.0, subset=np.ones((B, 64), np.int32))
        with pytest.raises(ValueError, match="subset must have shape"):
            batch.contacts(1.0, subset=np.ones((B, 63), bool))
        with pytest.raises(ValueError, match="capacity must be an integer >= 0"):
            batch.contacts(1.0, capacity=-1)
        with pytest.raises(ValueError, match="exceed 2\\^28"):
            batch.contacts(1.0, capacity=2 ** 28)
        with pytest.raises(nb.NBodyError, match="nbody_batch_contacts: the radius of system 0 must be finite and >= 0"):
            batch.contacts(-1.0)
        assert lib.nbody_batch_contacts(h, pos, good, None, None, 4, out, bodies, entries) == _lib.NBODY_OK
        want = kref.gpu_reference(64, "radius", False)
        assert out[2].bodies == 2 and out[4].pairs == want[4]["system"]["pairs"] and out[4].stored == 4
        assert bodies[4 * 64 + 5].degree == want[4]["bodies"]["degree"][5] and entries[4 * 4 + 1].j == want[4]["list"]["j"][1]
        after = batch.contacts(np.array(kref.RADIUS, np.float32))
    assert after.systems.tobytes() == before.systems.tobytes() and after.entries.tobytes() == before.entries.tobytes()
