"""GPU: the groups of batched ensembles (BatchedSystem.groups, include/nbody_batch_groups.h).  The labels, sizes and every
system word equal the reference (hermite_groups_ref: a union-find over fp64 distances for the labels, a mirror of the header's
schedule for the sweeps) exactly, and the group records equal its sequential fp64 sums bit for bit, at every workgroup shape and
with ragged counts; a bounded run ends where the mirror ends; per-system linking lengths, min_members, the weights and massive
counts do what the header says; a system's records are the same bits wherever it runs; the call disturbs no evolve and follows
the counts after a merger; every error is reported; and the result composes with members().

Capacities: 64 (one wave, one row per lane), 128 (two rows per lane), 320 (four rows per lane, two waves: the hook and the
exits across waves), 4096 (sixteen waves, 80 KiB of dynamic LDS: the raised limit).  The inputs are permuted chains, two
Plummer clumps joined by a bridge with and without its middle body, and uniform cubes; test_batch_groups_cpu.py shows that no
pair of them comes within 1e-4 of its linking length, so that the exact agreement asked here is the kernel's to meet."""
import numpy as np
import pytest

import hermite_groups_ref as gref

pytestmark = pytest.mark.gpu

SYSTEM_WORDS = ("groups", "grouped", "singles", "largest", "largest_count", "sweeps")


def run_groups(P, V, counts, b, massive=None, **kw):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))                  # copies: the shared inputs are read-only
        if massive is not None:
            batch.set_massive_counts(massive)
        return batch.groups(b, **kw)


def system_bits(res, s):
    return np.array([getattr(res, name)[s] for name in SYSTEM_WORDS] + [int(res.converged[s])], dtype=np.int64)


def slot_bits(res, s):
    """Every per-body and per-slot word of system s, the slots beyond the count included."""
    doubles = np.concatenate([res.weight[s][:, None], res.centre[s], res.velocity[s]], axis=1)
    return (res.group[s], res.size[s], res.count[s], res.sources[s], np.ascontiguousarray(doubles).view(np.uint64))


def same_slots(a, sa, c, sc, n=None):
    for x, y in zip(slot_bits(a, sa), slot_bits(c, sc)):
        assert np.array_equal(x[:n], y[:n])


def check_against_reference(res, refs, counts, tag="", truth=True):
    for s, (n, ref) in enumerate(zip(counts, refs)):
        print(f"{tag} system {s} (n = {n}): {res.groups[s]} groups, largest {res.largest[s]} with {res.largest_count[s]}, "
              f"{res.singles[s]} singles, {res.sweeps[s]} sweeps (reference {ref['groups']}, {ref['largest']}, {ref['largest_count']}, "
              f"{ref['singles']}, {ref['sweeps']})")
        for name in SYSTEM_WORDS:
            assert getattr(res, name)[s] == ref[name], (s, name, getattr(res, name)[s], ref[name])
        assert int(res.converged[s]) == ref["converged"], s
        assert np.array_equal(res.group[s, :n], ref["group"]), (s, np.flatnonzero(res.group[s, :n] != ref["group"])[:8])
        assert np.array_equal(res.size[s, :n], ref["size"]), s
        if truth:                                              # the union-find, which knows nothing of sweeps
            assert np.array_equal(res.group[s, :n], ref["true_group"]) and np.array_equal(res.size[s, :n], ref["true_size"]), s
        assert np.array_equal(res.count[s, :n], ref["count"]) and np.array_equal(res.sources[s, :n], ref["sources"]), s
        for name in ("weight", "centre", "velocity"):           # sums and quotients, bit for bit
            got, want = getattr(res, name)[s, :n], ref[name]
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (s, name, np.abs(got - want).max())
        # beyond the count: the empty records
        assert (res.group[s, n:] == -1).all() and not res.size[s, n:].any(), s
        for name in ("weight", "centre", "velocity", "count", "sources"):
            assert not getattr(res, name)[s, n:].any(), (s, name)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("capacity", gref.CAPACITIES)
def test_the_groups_equal_the_union_find_and_the_records_its_sums_bit_for_bit(capacity, which):
    P, V, counts, b = gref.gpu_inputs(capacity, which)
    res = run_groups(P, V, counts, b)
    B = len(counts)
    assert res.group.shape == (B, capacity) and res.group.dtype == np.int32 and res.size.dtype == np.int32
    assert res.centre.shape == (B, capacity, 3) and res.velocity.shape == (B, capacity, 3) and res.weight.dtype == np.float64
    assert res.groups.shape == (B,) and res.groups.dtype == np.int32 and res.converged.dtype == np.bool_
    check_against_reference(res, gref.reference(capacity, which), counts, f"capacity {capacity} {which}")
    assert res.converged.all() and res.sweeps.max() <= 16
    for s, n in enumerate(counts):
        if n == 0:                                             # a system without bodies: all zero, no root, no sweep, converged
            assert system_bits(res, s).tolist() == [0, 0, 0, -1, 0, 0, 1]
    # without the per-slot and per-body records the system records are the same bits
    for kw in (dict(records=False), dict(bodies=False), dict(records=False, bodies=False)):
        lean = run_groups(P, V, counts, b, **kw)
        assert (lean.weight is None) == ("records" in kw) and (lean.group is None) == ("bodies" in kw)
        assert (lean.centre is None and lean.count is None) == ("records" in kw) and (lean.size is None) == ("bodies" in kw)
        for s in range(B):
            assert np.array_equal(system_bits(lean, s), system_bits(res, s)), (kw, s)
        if "records" not in kw:
            assert np.array_equal(lean.weight.view(np.uint64), res.weight.view(np.uint64)) and np.array_equal(lean.count, res.count)
        if "bodies" not in kw:
            assert np.array_equal(lean.group, res.group) and np.array_equal(lean.size, res.size)


# ---- 2. a bounded run ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", gref.CAPACITIES)
def test_one_sweep_on_the_permuted_chain_is_not_converged_and_ends_where_the_mirror_ends(capacity):
    P, V, counts, b = gref.gpu_inputs(capacity, "a")
    res = run_groups(P, V, counts, b, max_sweeps=1)
    refs = [gref.groups(P[s], V[s], n, b[s], max_sweeps=1) for s, n in enumerate(counts)]
    check_against_reference(res, refs, counts, f"capacity {capacity}, one sweep", truth=False)
    assert res.sweeps[0] == 1 and not res.converged[0] and res.groups[0] > 1           # the chain is in pieces
    assert res.converged.tolist() == [False, True, False, True, False, False]          # empty and lone converge at once
    few = run_groups(P, V, counts, b, max_sweeps=3)
    refs = [gref.groups(P[s], V[s], n, b[s], max_sweeps=3) for s, n in enumerate(counts)]
    check_against_reference(few, refs, counts, f"capacity {capacity}, three sweeps", truth=False)
    assert not few.converged[0]


# ---- 3. per-system linking lengths ---------------------------------------------------------------------------------------------
def test_the_same_state_in_every_slot_with_growing_linking_lengths():
    pos, vel, b = gref.ladder_inputs()
    n, B = gref.LADDER_BODIES, gref.LADDER_SLOTS
    P, V = np.broadcast_to(pos, (B, n, 4)), np.broadcast_to(vel, (B, n, 4))
    res = run_groups(P, V, [n] * B, b, min_members=1)
    refs = [gref.groups(pos, vel, n, b[s], min_members=1) for s in range(B)]
    check_against_reference(res, refs, [n] * B, "ladder")
    # with min_members = 1 groups counts every connected set: a longer linking length can only join them
    assert np.all(np.diff(res.groups) <= 0) and res.groups[0] > res.groups[-1] and np.all(np.diff(res.largest_count) >= 0)
    # a scalar is that length in every slot
    one = run_groups(P, V, [n] * B, float(b[2]), min_members=1)
    for s in range(B):
        assert np.array_equal(system_bits(one, s), system_bits(res, 2))
        same_slots(one, s, res, 2)


# ---- 4. min_members, weights, massive counts -----------------------------------------------------------------------------------
def test_min_members_changes_groups_and_grouped_alone():
    P, V, counts, b = gref.gpu_inputs(128, "b")
    base = run_groups(P, V, counts, b)
    for k in (1, 3, 5, 129):
        res = run_groups(P, V, counts, b, min_members=k)
        for s, n in enumerate(counts):
            ref = gref.groups(P[s], V[s], n, b[s], min_members=k)
            assert (res.groups[s], res.grouped[s]) == (ref["groups"], ref["grouped"]), (k, s)
            assert np.array_equal(system_bits(res, s)[2:], system_bits(base, s)[2:]), (k, s)
            same_slots(res, s, base, s)
        assert [len(g) for g in res.groups_of(1)] == sorted((int(c) for c in res.count[1] if c >= k), reverse=True)
    assert base.groups[1] > 0 and run_groups(P, V, counts, b, min_members=129).groups.tolist() == [0] * 5


def test_massive_counts_leave_the_links_alone_and_the_tracers_mass_words_unread():
    P, V, counts, massive, b = gref.massive_inputs()
    plain = run_groups(P, V, counts, b)
    res = run_groups(P, V, counts, b, massive=massive)
    refs = [gref.groups(P[s], V[s], n, b[s], m=massive[s]) for s, n in enumerate(counts)]
    check_against_reference(res, refs, counts, "massive")
    # all bodies still link: the labels, sizes and every system word are those without massive counts
    for s in range(len(counts)):
        assert np.array_equal(system_bits(res, s), system_bits(plain, s)), s
    assert np.array_equal(res.group, plain.group) and np.array_equal(res.size, plain.size) and np.array_equal(res.count, plain.count)
    # sources counts the massive members: per system they add up to min(massive, count)
    assert res.sources.sum(axis=1).tolist() == [min(m, n) for m, n in zip(massive, counts)]
    assert plain.sources.sum(axis=1).tolist() == counts
    assert not res.weight[3].any() and not res.centre[3].any() and res.count[3].sum() == counts[3]      # no source: weightless groups
    # the tracers' mass words are not read: NaN there changes no bit
    poisoned = np.array(P)
    for s, (m, n) in enumerate(zip(massive, counts)):
        poisoned[s, min(m, n):, 3] = np.nan
    again = run_groups(poisoned, V, counts, b, massive=massive)
    for s in range(len(counts)):
        assert np.array_equal(system_bits(again, s), system_bits(res, s)), s
        same_slots(again, s, res, s)
    assert not np.isnan(again.weight).any() and not np.isnan(again.centre).any()


def test_weight_number_gives_test_particles_of_zero_mass_a_centre():
    P, V, counts, massive, b = gref.massive_inputs()
    P = np.array(P)
    for s, (m, n) in enumerate(zip(massive, counts)):
        P[s, min(m, n):, 3] = 0.0                              # tracers as users hold them: zero mass words
    by_mass = run_groups(P, V, counts, b, massive=massive)
    by_number = run_groups(P, V, counts, b, massive=massive, weight="number")
    refs = [gref.groups(P[s], V[s], n, b[s], m=massive[s], weight="number") for s, n in enumerate(counts)]
    check_against_reference(by_number, refs, counts, "number")
    assert np.array_equal(by_number.group, by_mass.group) and np.array_equal(by_number.sources, by_mass.sources)
    roots = by_number.roots(3)
    assert len(roots) and np.array_equal(by_number.weight[3, roots], by_number.count[3, roots].astype(np.float64))
    assert not by_mass.weight[3].any() and not by_mass.centre[3].any() and np.abs(by_number.centre[3, roots]).min() > 0
    lone = [r for r in roots if by_number.count[3, r] == 1][0]              # a group of one test particle sits where it is
    assert np.array_equal(by_number.centre[3, lone], P[3, lone, :3].astype(np.float64))
    assert np.array_equal(by_number.velocity[3, lone], V[3, lone, :3].astype(np.float64))


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------------
def test_a_system_gives_the_same_bits_in_another_slot_batch_and_capacity():
    n = gref.INVARIANCE_BODIES
    (pos, vel, b), (other_pos, other_vel, other_b) = gref.invariance_inputs()
    runs = []
    for cap, B, slot in ((64, 1, 0), (64, 5, 3), (320, 2, 1), (4096, 3, 2)):
        P, V = np.full((B, cap, 4), gref.FILL, dtype=np.float32), np.full((B, cap, 4), gref.FILL, dtype=np.float32)
        P[:, :n], V[:, :n] = other_pos, other_vel
        P[slot, :n], V[slot, :n] = pos, vel
        lengths = np.full(B, other_b, dtype=np.float32)
        lengths[slot] = b
        runs.append((run_groups(P, V, [n] * B, lengths), slot))
    first, slot0 = runs[0]
    assert first.groups[slot0] >= 3 and first.sweeps[slot0] >= 2                          # there is something to compare
    for res, slot in runs[1:]:
        assert np.array_equal(system_bits(res, slot), system_bits(first, slot0))
        same_slots(res, slot, first, slot0, n)
        assert (res.group[slot, n:] == -1).all() and not res.weight[slot, n:].any()


# ---- 6. changes nothing ----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.groups(0.3)
            b.groups([0.1, 0.5, 2.0], min_members=1, weight="number", max_sweeps=1, records=False, bodies=False)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_groups_evolve_is_the_two_evolves_alone_bit_for_bit():
    import n_body_problem_amd as nb
    counts = [40, 17, 64]
    P, V = np.full((3, 64, 4), gref.FILL, np.float32), np.full((3, 64, 4), gref.FILL, np.float32)
    for s, n in enumerate(counts):
        P[s, :n], V[s, :n] = nb.plummer(n, seed=80 + s)
    pa, va, ra = two_evolves(P, V, counts, False)
    pb, vb, rb = two_evolves(P, V, counts, True)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert ra.steps.sum() > 0


def test_after_a_merger_the_records_follow_the_lowered_counts():
    import hermite_pairs_ref as pref
    import n_body_problem_amd as nb
    counts = [30, 12]
    P, V = pref.ragged(64, counts, 6200)
    with nb.BatchedSystem(2, 64, counts=counts, integrator="hermite") as b:
        b.set_stop_conditions(collision_radius=0.02)
        b.set_collision_action("merge")
        b.set_state(P, V)
        b.evolve(4, 1.0 / 256.0, levels=8, softening=0.0)
        merged = b.mergers().count
        live = b.counts
        assert merged.sum() > 0 and np.array_equal(live, np.asarray(counts) - merged)
        res = b.groups(0.5, min_members=1)
        p, v = b.download()
    for s, n in enumerate(live):
        assert (res.group[s, n:] == -1).all() and not res.size[s, n:].any() and not res.count[s, n:].any(), s
        assert res.count[s].sum() == n and res.grouped[s] == n and (res.group[s, :n] >= 0).all()
        assert res.weight[s].sum() == pytest.approx(p[s, :n, 3].astype(np.float64).sum(), rel=1e-12)
    # and the records are those of a fresh batch that holds the merged state with the lowered counts
    fresh = run_groups(p, v, live.tolist(), 0.5, min_members=1)
    for s in range(2):
        assert np.array_equal(system_bits(fresh, s), system_bits(res, s)), s
        same_slots(fresh, s, res, s)


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import ctypes
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, V, counts, b = gref.gpu_inputs(64, "a")
    B = len(counts)
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        before = batch.groups(b)
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchGroupSystem * B)()
        out[2].sweeps = -7                                         # a refused call writes nothing
        good = (ctypes.c_float * B)(*[float(x) for x in b])

        def lengths(value, at=4):
            a = (ctypes.c_float * B)(*[float(x) for x in b])
            a[at] = value
            return a
        cases = [((None, vel, good, 2, 0, 64, out, None, None), b"NULL argument"),
                 ((pos, None, good, 2, 0, 64, out, None, None), b"NULL argument"),
                 ((pos, vel, None, 2, 0, 64, out, None, None), b"NULL argument"),
                 ((pos, vel, good, 2, 0, 64, None, None, None), b"NULL argument"),
                 ((pos, vel, lengths(-0.5), 2, 0, 64, out, None, None), b"the linking length of system 4 must be finite and >= 0"),
                 ((pos, vel, lengths(float("nan"), 0), 2, 0, 64, out, None, None), b"the linking length of system 0 must be finite and >= 0"),
                 ((pos, vel, lengths(float("inf"), 5), 2, 0, 64, out, None, None), b"the linking length of system 5 must be finite and >= 0"),
                 ((pos, vel, good, 0, 0, 64, out, None, None), b"min_members must be >= 1"),
                 ((pos, vel, good, -3, 0, 64, out, None, None), b"min_members must be >= 1"),
                 ((pos, vel, good, 2, 2, 64, out, None, None), b"weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER"),
                 ((pos, vel, good, 2, -1, 64, out, None, None), b"weight must be NBODY_BATCH_WEIGHT_MASS or NBODY_BATCH_WEIGHT_NUMBER"),
                 ((pos, vel, good, 2, 0, 0, out, None, None), b"max_sweeps must be 1 ... 64"),
                 ((pos, vel, good, 2, 0, 65, out, None, None), b"max_sweeps must be 1 ... 64"),
                 ((pos, vel, good, 2, 0, -1, out, None, None), b"max_sweeps must be 1 ... 64")]
        for args, message in cases:
            assert lib.nbody_batch_groups(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_groups: ") and message in error, (args, error)
            assert out[2].sweeps == -7
        assert lib.nbody_batch_groups(None, pos, vel, good, 2, 0, 64, out, None, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_groups: batch is NULL" in lib.nbody_batch_last_error(None)
        for bad in (dict(min_members=0), dict(max_sweeps=0), dict(max_sweeps=65)):
            with pytest.raises(nb.NBodyError):
                batch.groups(b, **bad)
        with pytest.raises(nb.NBodyError, match="linking length of system 0"):
            batch.groups(-1.0)
        with pytest.raises(ValueError):
            batch.groups(b, weight="charge")
        with pytest.raises(ValueError):
            batch.groups([0.5, 0.5])
        assert lib.nbody_batch_groups(h, pos, vel, good, 1, 1, 1, out, None, None) == _lib.NBODY_OK     # the ends of the ranges
        assert lib.nbody_batch_groups(h, pos, vel, lengths(0.0), 2, 0, 64, out, None, None) == _lib.NBODY_OK
        assert out[2].sweeps == before.sweeps[2] and out[2].largest_count == before.largest_count[2] and out[4].groups == 0
        after = batch.groups(b)
    for s in range(B):
        assert np.array_equal(system_bits(after, s), system_bits(before, s))
        same_slots(after, s, before, s)


# ---- 8. the result's helpers, and members() from the largest group ------------------------------------------------------------------
def test_groups_of_largest_mask_and_roots_agree_with_the_arrays():
    P, V, counts, b = gref.gpu_inputs(320, "b")
    res = run_groups(P, V, counts, b, min_members=3)
    for s, n in enumerate(counts):
        roots = res.roots(s)
        assert np.array_equal(roots, np.flatnonzero(res.count[s] > 0)) and np.array_equal(roots, np.unique(res.group[s, :n]))
        listed = res.groups_of(s)
        assert len(listed) == res.groups[s] and sum(len(g) for g in listed) == res.grouped[s]
        sizes = [len(g) for g in listed]
        assert sizes == sorted(sizes, reverse=True) and all(k >= 3 for k in sizes)
        for g in listed:
            assert (res.group[s, g] == g[0]).all() and res.size[s, g[0]] == len(g) and np.array_equal(g, np.sort(g))
        for g, h in zip(listed, listed[1:]):
            assert len(g) > len(h) or g[0] < h[0]                                      # ties by root
        mask = res.largest_mask()[s]
        assert mask.sum() == res.largest_count[s] and (mask[:n] == (res.group[s, :n] == res.largest[s])).all() and not mask[n:].any()
        if listed:
            assert np.array_equal(np.flatnonzero(mask), listed[0])
    assert res.largest_mask().shape == (len(counts), 320) and res.largest_mask().dtype == np.bool_


def test_members_from_the_largest_group_returns_members_of_that_group_alone():
    import n_body_problem_amd as nb
    P, V, counts, b = gref.gpu_inputs(128, "a")
    V = np.array(V)
    V[:, :, :3] *= np.float32(0.05)                            # cold: the clumps are bound
    with nb.BatchedSystem(len(counts), 128, counts=counts) as batch:
        batch.set_state(np.array(P), V)
        g = batch.groups(b)
        mask = g.largest_mask()
        bound = batch.members(0.01, initial=mask)
        everything = batch.members(0.01)
    assert not (bound.member & ~mask).any()                    # members only from that group
    assert bound.count[4] > 10 and bound.count[4] <= g.largest_count[4] < counts[4]       # one clump of the split pair
    assert everything.count[4] > bound.count[4]                # without the starting set the other clump is in it too
