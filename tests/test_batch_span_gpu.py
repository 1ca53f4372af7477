"""GPU: the spanning trees of batched ensembles (BatchedSystem.spanning_tree, include/nbody_batch_span.h).  Every slot's i, j and
r2, every system word and every body word equal the reference (hermite_span_ref: Prim's algorithm over the exact keys for the
edges, a literal mirror of the header's rounds for ``rounds``) exactly, and the fp64 sums bit for bit, at every workgroup shape
and with ragged counts; the edges form a spanning tree; subsets do what the header says; cutting the tree gives what groups()
gives; a system's records are the same bits wherever it runs; the call disturbs no evolve and follows the counts after a
merger; every error is reported; and on one input that is not on the grid the total length is within the fp32 chain's error of
an fp64 Prim.

Capacities: 64 (one wave, one row per lane), 128 (two rows per lane), 320 (four rows per lane, two waves: the minima, the
hooks and the exits across waves; a sort of 512 keys), 4096 (sixteen waves, 96 KiB of dynamic LDS: the raised limit; a sort of
4096 keys).  The inputs lie on a grid, so every r2 is exact and every key an integer that Python has too
(test_batch_span_cpu.py checks the premise): the exact agreement asked here is the kernel's to meet."""
import os
import subprocess

import numpy as np
import pytest

import hermite_span_ref as sref
from conftest import ROOT

pytestmark = pytest.mark.gpu

SYSTEM_INTS = ("edges", "selected", "rounds")
SYSTEM_DOUBLES = ("total_length", "longest", "mean_separation")


def run_span(P, counts, **kw):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))             # copies: the shared inputs are read-only
        return batch.spanning_tree(**kw)


def system_bits(res, s):
    return np.concatenate([np.array([getattr(res, name)[s] for name in SYSTEM_INTS] + [res.systems["reserved"][s]], dtype=np.int64),
                           np.array([getattr(res, name)[s] for name in SYSTEM_DOUBLES], dtype=np.float64).view(np.int64)])


def slot_bits(res, s):
    return (res.i[s], res.j[s], res.r2[s].view(np.uint32), res.edge_records["reserved"][s], res.degree[s], res.nearest[s])


def check_against_reference(res, refs, counts, tag="", separations=True):
    for s, (n, ref) in enumerate(zip(counts, refs)):
        print(f"{tag} system {s} (n = {n}): {res.edges[s]} edges in {res.rounds[s]} rounds, length {res.total_length[s]!r}, longest "
              f"{res.longest[s]!r}, mean separation {res.mean_separation[s]!r} (reference {ref['edges']}, {ref['rounds']}, "
              f"{ref['total_length']!r}, {ref['longest']!r}, {ref['mean_separation']!r})")
        for name in SYSTEM_INTS:
            assert getattr(res, name)[s] == ref[name], (s, name, getattr(res, name)[s], ref[name])
        assert res.systems["reserved"][s] == 0
        E = ref["edges"]
        assert np.array_equal(res.i[s, :E], ref["i"]) and np.array_equal(res.j[s, :E], ref["j"]), \
            (s, np.flatnonzero((res.i[s, :E] != ref["i"]) | (res.j[s, :E] != ref["j"]))[:8])
        assert np.array_equal(res.r2[s, :E].view(np.uint32), ref["r2"].view(np.uint32)), s
        want = dict(ref) if separations else dict(ref, mean_separation=0.0)
        for name in SYSTEM_DOUBLES:                                # sums and the quotient, bit for bit
            got = getattr(res, name)[s]
            assert np.float64(got).view(np.uint64) == np.float64(want[name]).view(np.uint64), (s, name, got, want[name])
        assert np.array_equal(res.degree[s, :n], ref["degree"]) and np.array_equal(res.nearest[s, :n], ref["nearest"]), s
        # beyond the edges and beyond the count: the empty values
        assert (res.i[s, E:] == -1).all() and (res.j[s, E:] == -1).all() and not res.r2[s, E:].view(np.uint32).any(), s
        assert not res.edge_records["reserved"][s].any() and not res.degree[s, n:].any() and (res.nearest[s, n:] == -1).all(), s


# ---- 1. against the reference, 2. the structure ------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", sref.CAPACITIES)
def test_the_edges_equal_prims_tree_and_the_sums_the_references_bit_for_bit(capacity):
    P, counts = sref.gpu_inputs(capacity)
    refs = sref.gpu_reference(capacity)
    B = len(counts)
    res = run_span(P, counts, separations=True)
    assert res.i.shape == (B, capacity) and res.i.dtype == np.int32 and res.j.dtype == np.int32 and res.r2.dtype == np.float32
    assert res.degree.shape == (B, capacity) and res.degree.dtype == np.int32 and res.nearest.dtype == np.int32
    assert res.edges.shape == (B,) and res.edges.dtype == np.int32 and res.total_length.dtype == np.float64
    check_against_reference(res, refs, counts, f"capacity {capacity}")
    assert res.rounds.max() <= 12 and res.rounds.max() >= 2
    for s, n in enumerate(counts):
        E = res.edges[s]
        assert sref.is_spanning_tree(res.i[s, :E], res.j[s, :E], range(n)), s
        assert (res.i[s, :E] < res.j[s, :E]).all() and E == max(n - 1, 0)
        assert res.degree[s].sum() == 2 * E
        if n >= 2:                                                 # the nearest body is a tree neighbour
            pairs = set(zip(res.i[s, :E].tolist(), res.j[s, :E].tolist()))
            assert all((min(a, int(c)), max(a, int(c))) in pairs for a, c in enumerate(res.nearest[s, :n])), s
        else:                                                      # no bodies, or a lone one: nothing but the count
            assert system_bits(res, s).tolist() == [0, n, 0, 0, 0, 0, 0] and (res.nearest[s] == -1).all()
    # without the separations the other words are the same bits and the mean is 0
    plain = run_span(P, counts)
    check_against_reference(plain, refs, counts, f"capacity {capacity} plain", separations=False)
    # without the per-slot and per-body records the system records are the same bits
    for kw in (dict(edges=False), dict(bodies=False), dict(edges=False, bodies=False)):
        lean = run_span(P, counts, separations=True, **kw)
        assert (lean.i is None and lean.j is None and lean.r2 is None) == ("edges" in kw)
        assert (lean.degree is None and lean.nearest is None) == ("bodies" in kw)
        for s in range(B):
            assert np.array_equal(system_bits(lean, s), system_bits(res, s)), (kw, s)
        if "edges" not in kw:
            assert np.array_equal(lean.i, res.i) and np.array_equal(lean.j, res.j) and np.array_equal(lean.r2.view(np.uint32), res.r2.view(np.uint32))
        if "bodies" not in kw:
            assert np.array_equal(lean.degree, res.degree) and np.array_equal(lean.nearest, res.nearest)


# ---- 3. subsets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [64, 320])
def test_one_cluster_in_every_slot_with_a_mask_each_equals_the_reference_and_separate_runs(capacity):
    pos, n, masks = sref.subset_inputs(capacity)
    B = len(masks)
    P = np.broadcast_to(pos, (B, capacity, 4))
    res = run_span(P, [n] * B, subset=masks, separations=True)
    refs = [sref.reference(pos, n, mask) for mask in masks]
    check_against_reference(res, refs, [n] * B, f"capacity {capacity} subsets")
    assert res.selected.tolist() == [int(m[:n].sum()) for m in masks] and res.selected[1] == 0 and res.selected[2] == 1
    assert system_bits(res, 1).tolist() == [0, 0, 0, 0, 0, 0, 0] and system_bits(res, 2).tolist() == [0, 1, 0, 0, 0, 0, 0]
    for s, mask in enumerate(masks):
        E = res.edges[s]
        chosen = np.flatnonzero(mask[:n])
        assert sref.is_spanning_tree(res.i[s, :E], res.j[s, :E], chosen), s         # no unselected endpoint among them
        outside = np.setdiff1d(np.arange(capacity), chosen)
        assert not res.degree[s, outside].any() and (res.nearest[s, outside] == -1).all(), s
    # the mask of all bodies is no mask, bit for bit; bool masks are the uint8 ones
    none = run_span(P[:1], [n], separations=True)
    assert np.array_equal(system_bits(none, 0), system_bits(res, 0))
    for x, y in zip(slot_bits(none, 0), slot_bits(res, 0)):
        assert np.array_equal(x, y)
    # every slot equals a run of its own
    for s in (3, 4, B - 1):
        alone = run_span(P[:1], [n], subset=masks[s:s + 1].astype(bool), separations=True)
        assert np.array_equal(system_bits(alone, 0), system_bits(res, s)), s
        for x, y in zip(slot_bits(alone, 0), slot_bits(res, s)):
            assert np.array_equal(x, y), s


# ---- 4. against code that ships -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [128, 320])
def test_cutting_the_tree_gives_the_groups_of_groups(capacity):
    import n_body_problem_amd as nb
    P, counts = sref.gpu_inputs(capacity)
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        tree = batch.spanning_tree()
        # a ladder of linking lengths through every system's own edge lengths, ties and the ends included
        for q in (0.0, 0.3, 0.5, 0.8, 0.95, 1.0):
            b = np.zeros(B, np.float32)
            for s in range(B):
                E = tree.edges[s]
                if E:
                    b[s] = np.sqrt(tree.r2[s, :E].astype(np.float64))[int(q * (E - 1))]
            b = b * np.float32(1.0 if q in (0.5, 1.0) else 1.001)        # on an edge's length, and just above one
            found = batch.groups(b, min_members=1)
            assert found.converged.all()
            assert np.array_equal(tree.group_count(b), found.groups), (q, tree.group_count(b), found.groups)
            for s in range(B):
                assert np.array_equal(tree.labels_at(s, b), found.group[s]), (q, s)
        assert np.array_equal(tree.group_count(1e6), (np.asarray(counts) > 0).astype(np.int32))
    # the length at which a system falls into k pieces
    for k in (2, 3, 5):
        at = tree.linking_length_for(k)
        for s, n in enumerate(counts):
            if tree.edges[s] >= k - 1:
                assert at[s] == np.sqrt(np.float64(tree.r2[s, tree.edges[s] - (k - 1)]))
                below = np.nextafter(np.float32(at[s]), np.float32(0))
                if np.float32(at[s]) == at[s] and below * below < tree.r2[s, tree.edges[s] - (k - 1)]:
                    assert tree.group_count(below)[s] >= k
            else:
                assert np.isnan(at[s])
    ends, lengths = tree.edges_of(0)
    assert ends.shape == (tree.edges[0], 2) and lengths.dtype == np.float64
    assert sref.sequential_sum(lengths) == tree.total_length[0] and lengths[-1] == tree.longest[0]


def test_the_q_parameter_is_its_formula_and_needs_the_separations():
    P, counts = sref.gpu_inputs(128)
    res = run_span(P, counts, separations=True)
    R = 50.0
    q = res.q_parameter(R)
    for s, n in enumerate(counts):
        if n >= 2:
            m = res.total_length[s] / (n * n * 4.0 * np.pi * R ** 3 / 3.0) ** (1.0 / 3.0)
            assert q[s] == pytest.approx(m / (res.mean_separation[s] / R), rel=1e-14)
        else:
            assert np.isnan(q[s])
    assert np.allclose(res.q_parameter(np.full(len(counts), R))[4:], q[4:], rtol=0, atol=0)
    with pytest.raises(ValueError, match="separations=True"):
        run_span(P, counts).q_parameter(R)
    with pytest.raises(ValueError, match="edges=True"):
        run_span(P, counts, edges=False).group_count(1.0)


# ---- 5. bit invariance ---------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bits_in_another_slot_batch_size_and_capacity():
    systems = {"lattice": sref.lattice(), "sphere": sref.plummer(37, radius=6.0), "chain": sref.chain(64, scale=2.0 ** -7)}
    for name, rows in systems.items():
        n = len(rows)
        first = None
        for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (320, 4, 1), (4096, 2, 1)):
            P = np.zeros((B, capacity, 4), np.float32)
            counts = [min(capacity, 11 + 3 * s) for s in range(B)]
            for s in range(B):
                P[s, :counts[s]] = sref.cube(counts[s], seed=40 + s, side=5)
            P[slot, :n], counts[slot] = rows, n
            res = run_span(P, counts, separations=True)
            if first is None:
                first, slot0 = res, slot
                continue
            assert np.array_equal(system_bits(res, slot), system_bits(first, slot0)), (name, capacity, B)
            for x, y in zip(slot_bits(res, slot), slot_bits(first, slot0)):
                assert np.array_equal(x[:64], y[:64]), (name, capacity, B)
            assert (res.i[slot, 64:] == -1).all() and not res.degree[slot, 64:].any()


# ---- 6. changes nothing ----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.spanning_tree(separations=True)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::3] = True
            b.spanning_tree(subset=mask, edges=False, bodies=False)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_spanning_tree_evolve_is_the_two_evolves_alone_bit_for_bit():
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


def test_after_a_merger_the_tree_follows_the_lowered_counts():
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
        res = b.spanning_tree(separations=True)
        p, v = b.download()
    for s, n in enumerate(live):
        E = res.edges[s]
        assert res.selected[s] == n and E == n - 1 and sref.is_spanning_tree(res.i[s, :E], res.j[s, :E], range(n)), s
        assert (res.i[s, E:] == -1).all() and not res.degree[s, n:].any() and (res.nearest[s, n:] == -1).all(), s
        assert np.array_equal(res.vertices[s], np.arange(64) < n)
    # and the records are those of a fresh batch that holds the merged state with the lowered counts
    fresh = run_span(p, live.tolist(), separations=True)
    for s in range(2):
        assert np.array_equal(system_bits(fresh, s), system_bits(res, s)), s
        for x, y in zip(slot_bits(fresh, s), slot_bits(res, s)):
            assert np.array_equal(x, y), s


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import ctypes
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, counts = sref.gpu_inputs(64)
    B = len(counts)
    with nb.BatchedSystem(B, 64, counts=counts) as batch:
        batch.set_state(np.array(P), np.zeros_like(P))
        before = batch.spanning_tree(separations=True)
        lib, h, pos = batch._lib, batch._h, _ptr(batch.positions)
        out = (_lib.BatchSpanSystem * B)()
        out[2].rounds = -7                                         # a refused call writes nothing
        cases = [((None, None, 0, out, None, None), b"NULL argument"),
                 ((pos, None, 0, None, None, None), b"NULL argument"),
                 ((pos, None, 2, out, None, None), b"separations must be 0 or 1"),
                 ((pos, None, -1, out, None, None), b"separations must be 0 or 1")]
        for args, message in cases:
            assert lib.nbody_batch_span(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_span: ") and message in error, (args, error)
            assert out[2].rounds == -7
        assert lib.nbody_batch_span(None, pos, None, 0, out, None, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_span: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.spanning_tree(subset=np.ones((B, 64), np.int32))
        with pytest.raises(ValueError, match="shape"):
            batch.spanning_tree(subset=np.ones((B, 63), bool))
        assert lib.nbody_batch_span(h, pos, None, 1, out, None, None) == _lib.NBODY_OK
        assert out[2].rounds == 0 and out[0].rounds == before.rounds[0] and out[0].total_length == before.total_length[0]
        after = batch.spanning_tree(separations=True)
    for s in range(B):
        assert np.array_equal(system_bits(after, s), system_bits(before, s))
        for x, y in zip(slot_bits(after, s), slot_bits(before, s)):
            assert np.array_equal(x, y)


# ---- 8. a generic float input ------------------------------------------------------------------------------------------------------
def prim64(x):
    """(total length, edges) of an fp64 Prim over fp64 distances."""
    n = len(x)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    best, parent = d[0].copy(), np.zeros(n, np.int64)
    inside = np.zeros(n, bool)
    inside[0] = True
    best[0] = np.inf
    total, edges = 0.0, []
    for _ in range(n - 1):
        u = int(np.argmin(best))
        total += best[u]
        edges.append((int(parent[u]), u))
        inside[u] = True
        closer = (d[u] < best) & ~inside
        best[closer], parent[closer] = d[u][closer], u
        best[u] = np.inf
    return total, edges


def test_a_sphere_off_the_grid_gives_a_spanning_tree_within_the_chains_error_of_an_fp64_prim(tmp_path):
    """|total_length - L64| <= 8 * 2^-24 * L64, with L64 the total of an fp64 Prim over fp64 distances: the fp32 chain puts at
    most 5 * 2^-24 of relative error on r2 (two roundings of the differences doubled by the squares, one of the product, two of
    the fused adds) and so 2.5 * 2^-24 on a length, and swapping near-tied edges costs at most twice that."""
    import n_body_problem_amd as nb
    n, capacity = 300, 320
    P = np.zeros((1, capacity, 4), np.float32)
    P[0, :n] = nb.plummer(n, seed=4242)[0]
    res = run_span(P, [n], separations=True)
    E = res.edges[0]
    assert E == n - 1 and sref.is_spanning_tree(res.i[0, :E], res.j[0, :E], range(n))
    assert (np.diff(res.r2[0, :E]) >= 0).all()
    L64, _ = prim64(P[0, :n, :3].astype(np.float64))
    # the stand-alone CPU driver on the same input
    exe = str(tmp_path / "driver")
    built = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "n_body_problem_amd", "csrc"),
                            os.path.join(ROOT, "tests", "batch_span_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    text = f"system {n} 1\n" + "".join(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} 1\n" for p in P[0, :n])
    head = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()[0].split()
    driver_length, driver_mean = float(head[4]), float(head[6])
    bound = 8.0 * 2.0 ** -24 * L64
    print(f"total_length {res.total_length[0]!r}, the CPU driver's {driver_length!r}, fp64 Prim {L64!r}: off by "
          f"{abs(res.total_length[0] - L64):.3e} (the driver by {abs(driver_length - L64):.3e}), bound {bound:.3e}")
    assert abs(driver_length - L64) <= bound
    assert abs(res.total_length[0] - L64) <= bound
    assert res.total_length[0] == driver_length and res.mean_separation[0] == driver_mean   # the same functions, the same bits
    d = np.sqrt(((P[0, :n, None, :3].astype(np.float64) - P[0, None, :n, :3].astype(np.float64)) ** 2).sum(axis=2))
    assert res.mean_separation[0] == pytest.approx(d.sum() / (n * (n - 1)), rel=1e-6)
