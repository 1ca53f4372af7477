"""GPU: the nearest-neighbour lists of batched ensembles (BatchedSystem.neighbours, include/nbody_batch_neighbours.h).  Every
list's indices and r2 bits, every body's found and within and every system word equal the reference (hermite_neighbours_ref: a
stable argsort of the exact r2) exactly, the two means bit for bit, at every workgroup shape, with ragged counts and for lists
of 1, 6 and 8; source masks do what the header says; the lists agree with structure(), spanning_tree() and groups(), which
ship; a system's lists are the same bits wherever it runs and whatever k the handle's buffers were sized for; the call
disturbs no evolve and follows the counts after a merger; and every error is reported.

Capacities: 64 (one wave, one row per lane), 128 (two rows per lane), 320 (four rows per lane, two waves: the tallies and the
nearest indices across waves), 4096 (sixteen waves, 64 KiB of dynamic LDS beside the tallies: the raised limit).  The inputs
lie on a grid, so every r2 is exact and every list a set of integers that Python has too (test_batch_neighbours_cpu.py checks
the premise): the exact agreement asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_neighbours_ref as nref
import hermite_span_ref as sref

pytestmark = pytest.mark.gpu

SYSTEM_INTS = ("bodies", "sources", "listed", "complete", "mutual")
SYSTEM_DOUBLES = ("mean_nearest", "mean_kth")
INF_BITS = int(np.float32(np.inf).view(np.uint32))


def run_neighbours(P, counts, **kw):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))             # copies: the shared inputs are read-only
        return batch.neighbours(**kw)


def system_bits(res, s):
    return np.concatenate([np.array([getattr(res, name)[s] for name in SYSTEM_INTS] + [res.systems["reserved"][s]], dtype=np.int64),
                           np.array([getattr(res, name)[s] for name in SYSTEM_DOUBLES], dtype=np.float64).view(np.int64)])


def body_bits(res, s):
    return (res.index[s], res.r2[s].view(np.uint32), res.found[s], res.within[s])


def check_against_reference(res, refs, counts, k, tag=""):
    for s, (n, ref) in enumerate(zip(counts, refs)):
        print(f"{tag} system {s} (n = {n}): listed {res.listed[s]}, complete {res.complete[s]}, mutual {res.mutual[s]}, means "
              f"{res.mean_nearest[s]!r} {res.mean_kth[s]!r} (reference {ref['listed']}, {ref['complete']}, {ref['mutual']}, "
              f"{ref['mean_nearest']!r}, {ref['mean_kth']!r})")
        for name in SYSTEM_INTS:
            assert getattr(res, name)[s] == ref[name], (s, name, getattr(res, name)[s], ref[name])
        assert res.systems["reserved"][s] == 0
        for name in SYSTEM_DOUBLES:                                # the sum and the quotient, bit for bit
            got = getattr(res, name)[s]
            assert np.float64(got).view(np.uint64) == np.float64(ref[name]).view(np.uint64), (s, name, got, ref[name])
        assert np.array_equal(res.index[s, :n], ref["index"]), (s, np.argwhere(res.index[s, :n] != ref["index"])[:8])
        assert np.array_equal(res.r2[s, :n].view(np.uint32), ref["r2"].view(np.uint32)), s
        assert np.array_equal(res.found[s, :n], ref["found"]) and np.array_equal(res.within[s, :n], ref["within"]), s
        # beyond found and beyond the count: the empty values
        slot = np.arange(k)[None, :]
        empty = slot >= res.found[s][:, None]
        assert (res.index[s][empty] == -1).all() and (res.r2[s].view(np.uint32)[empty] == INF_BITS).all(), s
        assert (res.index[s][~empty] >= 0).all() and np.isfinite(res.r2[s][~empty]).all(), s
        assert not res.found[s, n:].any() and not res.within[s, n:].any(), s
        assert np.array_equal(res.distance[s], np.sqrt(res.r2[s].astype(np.float64)))


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", nref.CAPACITIES)
def test_the_lists_the_counts_and_the_means_equal_the_reference_exactly(capacity):
    P, counts = nref.gpu_inputs(capacity)
    radii = nref.gpu_radii(capacity)
    B = len(counts)
    for k in nref.KS:
        res = run_neighbours(P, counts, k=k, radius=radii)
        assert res.index.shape == (B, capacity, k) and res.index.dtype == np.int32
        assert res.r2.shape == (B, capacity, k) and res.r2.dtype == np.float32
        assert res.distance.shape == (B, capacity, k) and res.distance.dtype == np.float64
        assert res.found.shape == (B, capacity) and res.found.dtype == np.int32 and res.within.dtype == np.int32
        for name in SYSTEM_INTS:
            assert getattr(res, name).shape == (B,) and getattr(res, name).dtype == np.int32
        assert res.mean_nearest.dtype == np.float64 and res.mean_kth.dtype == np.float64 and res.k == k
        check_against_reference(res, nref.gpu_reference(capacity, k), counts, k, f"capacity {capacity} k {k}")
        assert (res.mutual % 2 == 0).all() and res.within.sum() > 0
        if k == 6:
            full = res
    # without a radius nothing is within and nothing else moves
    plain = run_neighbours(P, counts, k=6)
    assert not plain.within.any() and np.array_equal(plain.index, full.index) and np.array_equal(plain.found, full.found)
    for s in range(B):
        assert np.array_equal(system_bits(plain, s), system_bits(full, s)), s
    # without the lists and the per-body records the system records are the same bits, and what survives too
    for kw in (dict(lists=False), dict(bodies=False), dict(lists=False, bodies=False)):
        lean = run_neighbours(P, counts, k=6, radius=radii, **kw)
        assert (lean.index is None and lean.r2 is None and lean.distance is None) == ("lists" in kw)
        assert (lean.found is None and lean.within is None) == ("bodies" in kw)
        for s in range(B):
            assert np.array_equal(system_bits(lean, s), system_bits(full, s)), (kw, s)
        if "lists" not in kw:
            assert np.array_equal(lean.index, full.index) and np.array_equal(lean.r2.view(np.uint32), full.r2.view(np.uint32))
        else:
            with pytest.raises(ValueError, match="lists=True"):
                lean.gather(P)
        if "bodies" not in kw:
            assert np.array_equal(lean.found, full.found) and np.array_equal(lean.within, full.within)
    # gather: the neighbours' positions are at the lists' distances
    near = full.gather(np.asarray(P)[:, :, :3].astype(np.float64))
    assert near.shape == (B, capacity, 6, 3)
    d2 = ((near - np.asarray(P)[:, :, None, :3].astype(np.float64)) ** 2).sum(axis=3)
    filled = full.index >= 0
    assert np.array_equal(d2[filled], full.r2[filled].astype(np.float64)) and np.isnan(near[~filled]).all()
    assert np.array_equal(full.gather(np.arange(B * capacity).reshape(B, capacity), fill=-1)[filled] % capacity, full.index[filled])


# ---- 2. sources -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [64, 320])
def test_one_cluster_in_every_slot_with_a_source_mask_each_equals_the_reference(capacity):
    pos, n, masks = nref.source_inputs(capacity)
    B = len(masks)
    P = np.broadcast_to(pos, (B, capacity, 4))
    for k in (1, 6):
        res = run_neighbours(P, [n] * B, k=k, radius=3.0, sources=masks)
        refs = [nref.reference(pos, n, k, radius=3.0, sources=mask) for mask in masks]
        check_against_reference(res, refs, [n] * B, k, f"capacity {capacity} k {k} sources")
        for s, mask in enumerate(masks):                           # every listed index is a source and never the row itself
            listed = res.index[s] >= 0
            assert mask[res.index[s][listed]].all() and not (res.index[s] == np.arange(capacity)[:, None]).any(), s
    assert res.sources.tolist() == [0, n, 1, 20, 8]
    # no source: nothing is listed.  A single source: every other row lists it, and the source itself lists nothing
    assert system_bits(res, 0).tolist() == [n, 0, 0, 0, 0, 0, 0, 0] and (res.index[0] == -1).all() and not res.found[0].any()
    one = n // 2
    assert res.listed[2] == n - 1 and res.found[2, one] == 0 and (res.index[2, one] == -1).all() and res.mutual[2] == 0
    assert (np.delete(res.index[2, :n, 0], one) == one).all()
    # the mask of all bodies is no mask, bit for bit; bool masks are the uint8 ones
    none = run_neighbours(P[:1], [n], k=6, radius=3.0)
    assert np.array_equal(system_bits(none, 0), system_bits(res, 1))
    for x, y in zip(body_bits(none, 0), body_bits(res, 1)):
        assert np.array_equal(x, y)
    alone = run_neighbours(P[:1], [n], k=6, radius=3.0, sources=masks[3:4].astype(bool))
    assert np.array_equal(system_bits(alone, 0), system_bits(res, 3))
    for x, y in zip(body_bits(alone, 0), body_bits(res, 3)):
        assert np.array_equal(x, y)


# ---- 3. against code that ships -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [128, 320])
def test_the_lists_agree_with_structure_spanning_tree_and_groups(capacity):
    import n_body_problem_amd as nb
    P, counts = nref.gpu_inputs(capacity)
    B = len(counts)
    clean = [s for s, n in enumerate(counts) if not nref.has_zero_distance(P[s], n)]
    assert len(clean) >= 4 and len(clean) < B
    radii = nref.gpu_radii(capacity)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        tree = batch.spanning_tree()
        friends = batch.groups(radii, min_members=1)
        for k in nref.KS:
            res = batch.neighbours(k=k, radius=radii)
            dense = batch.structure(k=k)
            for s in clean:                                        # without a zero distance the k-th smallest r2 > 0 is slot k - 1
                n = counts[s]
                # neighbour_r2 comes back as neighbour_distance, its fp64 square root, whose square rounds to the fp32 r2 again;
                # +inf on both sides where a row has fewer than k neighbours
                theirs = (dense.neighbour_distance[s, :n] * dense.neighbour_distance[s, :n]).astype(np.float32)
                assert np.array_equal(np.sqrt(theirs.astype(np.float64)), dense.neighbour_distance[s, :n])
                assert np.array_equal(res.r2[s, :n, k - 1].view(np.uint32), theirs.view(np.uint32)), (k, s)
                assert np.array_equal(np.isinf(theirs), res.found[s, :n] < k)
            for s, n in enumerate(counts):                         # the nearest body is the tree's nearest, ties included
                assert np.array_equal(res.index[s, :n, 0], tree.nearest[s, :n]), (k, s)
            assert np.array_equal(res.within == 0, friends.size <= 1), k   # alone in its group iff nobody is within the length
            assert (res.mutual % 2 == 0).all()


# ---- 4. placement -----------------------------------------------------------------------------------------------------------------
def test_a_systems_lists_are_the_same_bits_in_another_slot_batch_size_and_capacity():
    systems = {"lattice": sref.lattice(), "sphere": sref.plummer(37, radius=6.0), "cube": sref.cube(64, side=4)}
    for name, rows in systems.items():
        n = len(rows)
        first = None
        for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (320, 4, 1), (4096, 2, 1)):
            P = np.zeros((B, capacity, 4), np.float32)
            counts = [min(capacity, 11 + 3 * s) for s in range(B)]
            for s in range(B):
                P[s, :counts[s]] = sref.cube(counts[s], seed=40 + s, side=5)
            P[slot, :n], counts[slot] = rows, n
            res = run_neighbours(P, counts, k=6, radius=np.full(B, 4.0, np.float32))
            if first is None:
                first, slot0 = res, slot
                continue
            assert np.array_equal(system_bits(res, slot), system_bits(first, slot0)), (name, capacity, B)
            for x, y in zip(body_bits(res, slot), body_bits(first, slot0)):
                assert np.array_equal(x[:64], y[:64]), (name, capacity, B)
            assert (res.index[slot, 64:] == -1).all() and not res.found[slot, 64:].any()


def test_a_smaller_and_then_a_larger_k_on_one_handle_are_correct():
    """The list buffers are sized by the first call that asks for them and grown by a later, larger k."""
    import n_body_problem_amd as nb
    P, counts = nref.gpu_inputs(128)
    radii = nref.gpu_radii(128)
    with nb.BatchedSystem(len(counts), 128, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        for k in (6, 1, 8, 6):
            res = batch.neighbours(k=k, radius=radii)
            check_against_reference(res, nref.gpu_reference(128, k), counts, k, f"one handle, k {k}")


# ---- 5. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.neighbours(k=8, radius=0.5)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.neighbours(k=2, sources=mask, lists=False, bodies=False)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_neighbours_evolve_is_the_two_evolves_alone_bit_for_bit():
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


def test_after_a_merger_the_lists_follow_the_lowered_counts():
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
        res = b.neighbours(k=6, radius=0.3)
        p, v = b.download()
    for s, n in enumerate(live):
        assert res.bodies[s] == n and res.sources[s] == n and res.listed[s] == n and res.complete[s] == n, s
        assert (res.index[s, :n] >= 0).all() and (res.index[s, :n] < n).all() and (res.index[s, n:] == -1).all(), s
        assert (res.found[s, :n] == 6).all() and not res.found[s, n:].any() and not res.within[s, n:].any(), s
    # and the lists are those of a fresh batch that holds the merged state with the lowered counts
    fresh = run_neighbours(p, live.tolist(), k=6, radius=0.3)
    for s in range(2):
        assert np.array_equal(system_bits(fresh, s), system_bits(res, s)), s
        for x, y in zip(body_bits(fresh, s), body_bits(res, s)):
            assert np.array_equal(x, y), s


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, counts = nref.gpu_inputs(64)
    B = len(counts)
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        before = batch.neighbours(k=6, radius=2.0)
        lib, h, pos = batch._lib, batch._h, _ptr(batch.positions)
        out = (_lib.BatchNeighbourSystem * B)()
        out[2].listed = -7                                         # a refused call writes nothing
        index = (ctypes.c_int * (B * 64 * 8))()
        r2 = (ctypes.c_float * (B * 64 * 8))()
        bad = (ctypes.c_float * B)(*([1.0] * B))
        bad[3] = -0.5
        nan = (ctypes.c_float * B)(*([1.0] * B))
        nan[B - 1] = float("nan")
        cases = [((None, 6, None, None, out, None, None, None), b"NULL argument"),
                 ((pos, 6, None, None, None, None, None, None), b"NULL argument"),
                 ((pos, 0, None, None, out, None, None, None), b"k must be 1 ... 8"),
                 ((pos, 9, None, None, out, None, None, None), b"k must be 1 ... 8"),
                 ((pos, -1, None, None, out, None, None, None), b"k must be 1 ... 8"),
                 ((pos, 6, None, None, out, None, index, None), b"both or neither"),
                 ((pos, 6, None, None, out, None, None, r2), b"both or neither"),
                 ((pos, 6, bad, None, out, None, None, None), b"the radius of system 3 must be >= 0"),
                 ((pos, 6, nan, None, out, None, None, None), f"the radius of system {B - 1} must be >= 0".encode())]
        for args, message in cases:
            assert lib.nbody_batch_neighbours(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_neighbours: ") and message in error, (args, error)
            assert out[2].listed == -7
        assert lib.nbody_batch_neighbours(None, pos, 6, None, None, out, None, None, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_neighbours: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="k must be"):
            batch.neighbours(k=9)
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.neighbours(sources=np.ones((B, 64), np.int32))
        with pytest.raises(ValueError, match="shape"):
            batch.neighbours(sources=np.ones((B, 63), bool))
        with pytest.raises(ValueError, match="one radius"):
            batch.neighbours(radius=np.ones(B + 1))
        with pytest.raises(nb.NBodyError, match="nbody_batch_neighbours: the radius of system 0"):
            batch.neighbours(radius=-1.0)
        assert lib.nbody_batch_neighbours(h, pos, 8, None, None, out, None, index, r2) == _lib.NBODY_OK
        assert out[2].listed == 0 and out[0].listed == before.listed[0] and out[0].mean_nearest == before.mean_nearest[0]
        assert np.array_equal(np.ctypeslib.as_array(index).reshape(B, 64, 8)[:, :, :6], before.index)
        after = batch.neighbours(k=6, radius=2.0)
    for s in range(B):
        assert np.array_equal(system_bits(after, s), system_bits(before, s))
        for x, y in zip(body_bits(after, s), body_bits(before, s)):
            assert np.array_equal(x, y)
