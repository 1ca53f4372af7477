"""GPU: hierarchies of batched ensembles (BatchedSystem.hierarchy, include/nbody_batch_hierarchy.h).  Every int of the node,
body and system records equals the fp64 reference (hermite_hierarchy_ref) at every workgroup shape and with ragged counts,
with and without a tidal tolerance, and the doubles agree with it to the figure pairs() meets for the same formulas; the
analytic triple and 2 + 2 come out as designed on both sides of the stability threshold; max_levels cuts the nesting where it
says; massive counts restrict the leaves; a system's records are the same bytes wherever it runs; the call disturbs no
evolve and follows the counts after a merger; and every error is reported.

Capacities: 64 (one row per lane), 128 (two), 130 (four rows per lane, one wave), 257 (two waves: the creation order across
waves), 4096 (sixteen waves, 144 KiB of dynamic LDS: the raised limit).  test_batch_hierarchy_cpu.py shows that every input
here keeps the four margins of the inputs condition, so that the exact agreement asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_hierarchy_ref as href

pytestmark = pytest.mark.gpu

ELEMENTS = 1e-9      # relative, the doubles of the pair: the figure pairs() meets for the same formulas
PERTURBATION = 2e-6  # relative: g is a maximum of fp32 m inv^3
NODE_EXACT = ("child", "node_parent", "level", "leaves", "slot", "mass")
NODE_ELEMENTS = ("energy", "semi_major_axis", "eccentricity", "inclination", "separation", "mutual_inclination", "h")


def run_hierarchy(P, V, counts, massive=None, **kw):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts) as b:
        b.set_state(np.array(P), np.array(V))                      # copies: the shared inputs are read-only
        if massive is not None:
            b.set_massive_counts(massive)
        return b.hierarchy(**kw)


def record_bytes(res, s):
    """The three records of system s as bytes."""
    return (res.systems[s:s + 1].tobytes(), None if res.node_records is None else res.node_records[s].tobytes(),
            None if res.body_records is None else res.body_records[s].tobytes())


def check_against_reference(res, refs, counts, tag=""):
    """The checks of one batch, system by system; prints its largest deviations before it asserts."""
    from n_body_problem_amd import batch
    empty_node = np.zeros(1, dtype=batch.HIERARCHY_NODE_DTYPE)
    empty_node["child"], empty_node["parent"] = -1, -1
    empty_body = np.array([(-1, -1, 0, 0)], dtype=batch.HIERARCHY_BODY_DTYPE)
    worst = dict(elements=0.0, perturbation=0.0)
    for s, (n, ref) in enumerate(zip(counts, refs)):
        k = ref["nodes"]
        got = {name: getattr(res, name)[s] for name in href.SYSTEM_FIELDS if name != "converged"}
        print(f"{tag} system {s} (n = {n}): {got}, converged {bool(res.converged[s])}; reference "
              f"{ {name: ref[name] for name in href.SYSTEM_FIELDS} }")
        dev = dict(elements=0.0, perturbation=0.0)
        if res.nodes[s] == k and k:
            for name in NODE_ELEMENTS:
                want, have = ref[name][:k], getattr(res, name)[s, :k]
                scale = np.abs(want).max(axis=-1, keepdims=True) if name == "h" else np.abs(want)   # a vector against its largest
                with np.errstate(invalid="ignore", divide="ignore"):
                    d = np.where(scale > 0, np.abs(have - want) / scale, np.abs(have - want))
                dev["elements"] = max(dev["elements"], float(np.nanmax(d)))
            want, have = ref["perturbation"][:k], res.perturbation[s, :k]
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.where(want > 0, np.abs(have - want) / want, np.abs(have - want))
            dev["perturbation"] = float(d.max())
        print(f"{tag} system {s}: elements {dev['elements']:.2g}, perturbation {dev['perturbation']:.2g} (relative)")
        worst = {name: max(worst[name], dev[name]) for name in worst}
        for name in href.SYSTEM_FIELDS:
            assert int(res.systems[name][s]) == ref[name], (s, name, int(res.systems[name][s]), ref[name])
        for name in NODE_EXACT:
            assert np.array_equal(getattr(res, name)[s], ref[name]), (s, name)
        assert np.array_equal(res.stable[s], ref["stable"] != 0), s
        for name in ("parent", "root", "depth"):
            assert np.array_equal(getattr(res, name)[s], ref[name]), (s, name)
        assert dev["elements"] <= ELEMENTS and dev["perturbation"] <= PERTURBATION, (s, dev)
        # beyond the node count and beyond the body count: the empty records, every byte
        assert res.node_records[s, k:].tobytes() == np.repeat(empty_node, len(res.node_records[s]) - k).tobytes(), s
        assert res.body_records[s, n:].tobytes() == np.repeat(empty_body, len(res.body_records[s]) - n).tobytes(), s
        assert not res.node_records["reserved"][s].any() and not res.body_records["reserved"][s].any() and res.systems["reserved"][s] == 0
        assert res.describe(s) == href.describe(ref), s
    print(f"{tag} largest deviations: {worst}")


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
CASES = [(capacity, tolerance) for capacity, tolerances in href.TOLERANCES.items() for tolerance in tolerances]


@pytest.mark.parametrize("capacity,tolerance", CASES)
def test_the_records_equal_the_reference(capacity, tolerance):
    P, V, counts = href.gpu_inputs(capacity)
    res = run_hierarchy(P, V, counts, tidal_tolerance=tolerance, max_levels=16)
    B = len(counts)
    assert res.child.shape == (B, capacity, 2) and res.h.shape == (B, capacity, 3) and res.parent.shape == (B, capacity)
    assert res.nodes.dtype == np.int32 and res.converged.dtype == np.bool_ and res.energy.dtype == np.float64
    assert res.multiplicity().shape == (B, 4)
    check_against_reference(res, href.reference(capacity, tolerance), counts, f"capacity {capacity}, tolerance {tolerance}")
    lean = run_hierarchy(P, V, counts, tidal_tolerance=tolerance, max_levels=16, nodes=False, bodies=False)
    assert lean.child is None and lean.parent is None and lean.systems.tobytes() == res.systems.tobytes()


# ---- 2. the analytic cases ---------------------------------------------------------------------------------------------------
def hand_batch():
    """Capacity 64: the designed triple, the tight one, the tilted one, the 2 + 2, the nested object."""
    objs = [href.designed_triple(), href.designed_triple(outer_a=0.1), href.designed_triple(tilt=0.7), href.designed_two_plus_two(),
            href.designed_nested()]
    P, V = np.zeros((len(objs), 64, 4), np.float32), np.zeros((len(objs), 64, 4), np.float32)
    for s, obj in enumerate(objs):
        P[s], V[s] = href.place(obj, 64)
    return P, V, [len(obj[0]) for obj in objs]


def test_the_designed_triple_and_two_plus_two_come_out_as_designed():
    P, V, counts = hand_batch()
    res = run_hierarchy(P, V, counts, max_levels=16)
    assert [res.describe(s) for s in range(5)] == ["[[0 1] 2]", "[[0 1] 2]", "[[0 1] 2]", "[[0 1] [2 3]]", "[[[0 1] 2] 3]"]
    assert res.stable[0, :2].tolist() == [True, True] and res.stable[1, :2].tolist() == [True, False]
    assert res.unstable.tolist() == [0, 1, 0, 0, 0]
    assert res.multiplicity().tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1]]
    assert res.mutual_inclination[2, 1, 0] == pytest.approx(0.7, abs=1e-6) and res.mutual_inclination[2, 1, 1] == 0
    assert res.mutual_inclination[0, 1].tolist() == pytest.approx([0.2, 0.0], abs=1e-6)
    assert res.semi_major_axis[0, :2].tolist() == pytest.approx([0.05, 1.0], rel=1e-5)
    assert res.eccentricity[0, :2].tolist() == pytest.approx([0.3, 0.2], rel=1e-5)
    assert res.child[3, :3].tolist() == [[0, 1], [2, 3], [4, 5]] and res.roots_of(3) == [6] and res.roots_of(0) == [4]
    check_against_reference(res, [href.hierarchy(P[s], V[s], n, max_levels=16) for s, n in enumerate(counts)], counts, "designed")


# ---- 3. max_levels -----------------------------------------------------------------------------------------------------------
def test_max_levels_cuts_the_nesting_of_the_nested_object():
    P, V, counts = hand_batch()
    for levels, (made, converged, text) in zip((1, 2, 3), ((1, False, "[0 1] 2 3"), (2, False, "[[0 1] 2] 3"), (3, True, "[[[0 1] 2] 3]"))):
        res = run_hierarchy(P, V, counts, max_levels=levels)
        assert (res.nodes[4], bool(res.converged[4]), res.describe(4), res.levels[4]) == (made, converged, text, levels)
        check_against_reference(res, [href.hierarchy(P[s], V[s], n, max_levels=levels) for s, n in enumerate(counts)], counts,
                                f"max_levels {levels}")


# ---- 4. massive counts -------------------------------------------------------------------------------------------------------
def test_only_the_massive_bodies_are_leaves_and_the_tracers_are_untouched():
    P, V, counts, massive = href.massive_inputs()
    res = run_hierarchy(P, V, counts, massive=massive, max_levels=16)
    refs = [href.hierarchy(P[s], V[s], n, massive=massive[s], max_levels=16) for s, n in enumerate(counts)]
    check_against_reference(res, refs, counts, "massive")
    n = counts[0]
    for s, m in enumerate(massive):
        assert res.roots[s] + res.nodes[s] == m and res.multiplicity()[s].sum() == res.roots[s]
        assert (res.parent[s, m:n] == -1).all() and (res.depth[s, m:n] == 0).all() and res.root[s, m:n].tolist() == list(range(m, n))
    assert res.levels[:2].tolist() == [0, 0] and res.converged.all() and res.nodes[3] > res.nodes[2]
    # the tracers' states times 7: no byte of any record changes
    heavy_P, heavy_V = np.array(P), np.array(V)
    for s, m in enumerate(massive):
        heavy_P[s, m:] *= 7
        heavy_V[s, m:] *= 7
    again = run_hierarchy(heavy_P, heavy_V, counts, massive=massive, max_levels=16)
    for s in range(len(counts)):
        assert record_bytes(again, s) == record_bytes(res, s), s


# ---- 5. invariance -----------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bytes_in_another_slot_batch_and_capacity():
    n = href.INVARIANCE_BODIES
    other_pos, other_vel = href.objects(n, href.SEED0 + 3)
    got = []
    for cap, B, slot in ((130, 1, 0), (130, 5, 3), (257, 2, 1)):
        pos, vel = href.invariance_inputs(cap)
        P, V = np.full((B, cap, 4), href.FILL, dtype=np.float32), np.full((B, cap, 4), href.FILL, dtype=np.float32)
        P[:, :n], V[:, :n] = other_pos, other_vel
        P[slot], V[slot] = pos, vel
        res = run_hierarchy(P, V, [n] * B, max_levels=16)
        got.append((res.systems[slot:slot + 1].tobytes(), res.node_records[slot, :130].tobytes(), res.body_records[slot, :130].tobytes()))
        if cap == 130 and B == 1:
            assert res.levels[0] >= 3 and res.nodes[0] > 40
            lean = run_hierarchy(P, V, [n] * B, max_levels=16, nodes=False, bodies=False)
            only_nodes = run_hierarchy(P, V, [n] * B, max_levels=16, bodies=False)
            only_bodies = run_hierarchy(P, V, [n] * B, max_levels=16, nodes=False)
            assert lean.systems.tobytes() == only_nodes.systems.tobytes() == only_bodies.systems.tobytes() == res.systems.tobytes()
            assert only_nodes.node_records.tobytes() == res.node_records.tobytes() and only_nodes.parent is None
            assert only_bodies.body_records.tobytes() == res.body_records.tobytes() and only_bodies.child is None
    assert got[1] == got[0] and got[2] == got[0]


# ---- 6. changes nothing ------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.0)
        binaries = None
        if between:
            before = b.download()
            binaries = b.pairs().binaries
            b.hierarchy()
            b.hierarchy(tidal_tolerance=0.01, max_levels=16, nodes=False, bodies=False)
            after = b.download()
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
            assert np.array_equal(b.pairs().binaries, binaries)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.0)
        p, v = b.download()
        return p, v, b.evolve_stats()


def test_evolve_hierarchy_evolve_is_the_two_evolves_alone_bit_for_bit():
    import hermite_pairs_ref as pref
    counts = [40, 17, 64]
    P, V = pref.ragged(64, counts, 6300)
    pa, va, ra = two_evolves(P, V, counts, False)
    pb, vb, rb = two_evolves(P, V, counts, True)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    for name in ("steps", "min_level", "max_level", "clamped", "ticks"):
        assert np.array_equal(getattr(ra, name), getattr(rb, name)), name
    assert ra.steps.sum() > 0


# ---- 7. after a merger -------------------------------------------------------------------------------------------------------
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
        res = b.hierarchy(max_levels=16)
        p, v = b.download()
    assert np.array_equal(res.counts, live)
    for s, n in enumerate(live):
        assert (res.root[s, n:] == -1).all() and (res.parent[s, n:] == -1).all() and res.roots[s] + res.nodes[s] == n
        assert res.child[s, :res.nodes[s]].max(initial=-1) < n + res.nodes[s]
    # and the records are those of a fresh batch that holds the merged state with the lowered counts
    fresh = run_hierarchy(p, v, live.tolist(), max_levels=16)
    for s in range(2):
        assert record_bytes(fresh, s) == record_bytes(res, s), s


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    P, V, counts = href.gpu_inputs(64)
    inf = float("inf")
    with nb.BatchedSystem(len(counts), 64, counts=counts) as b:
        b.set_state(np.array(P), np.array(V))
        before = b.hierarchy()
        lib, h, pos, vel = b._lib, b._h, _ptr(b.positions), _ptr(b.velocities)
        out = (_lib.BatchHierarchySystem * len(counts))()
        out[5].levels = -7                                         # a refused call writes nothing
        cases = [((None, vel, inf, 8, out, None, None), b"NULL argument"), ((pos, None, inf, 8, out, None, None), b"NULL argument"),
                 ((pos, vel, inf, 8, None, None, None), b"NULL argument"),
                 ((pos, vel, inf, 0, out, None, None), b"max_levels must be 1 ... 16"),
                 ((pos, vel, inf, 17, out, None, None), b"max_levels must be 1 ... 16"),
                 ((pos, vel, inf, -1, out, None, None), b"max_levels must be 1 ... 16"),
                 ((pos, vel, float("nan"), 8, out, None, None), b"tidal_tolerance must be"),
                 ((pos, vel, -0.5, 8, out, None, None), b"tidal_tolerance must be"),
                 ((pos, vel, -inf, 8, out, None, None), b"tidal_tolerance must be")]
        for args, message in cases:
            assert lib.nbody_batch_hierarchy(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_hierarchy: ") and message in error, (args, error)
            assert out[5].levels == -7
        assert lib.nbody_batch_hierarchy(None, pos, vel, inf, 8, out, None, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_hierarchy: batch is NULL" in lib.nbody_batch_last_error(None)
        for bad in (dict(max_levels=0), dict(max_levels=17), dict(tidal_tolerance=-1.0), dict(tidal_tolerance=float("nan"))):
            with pytest.raises(nb.NBodyError):
                b.hierarchy(**bad)
        assert lib.nbody_batch_hierarchy(h, pos, vel, 0.0, 16, out, None, None) == _lib.NBODY_OK     # 0 and 16 are in range
        assert lib.nbody_batch_hierarchy(h, pos, vel, inf, 8, out, None, None) == _lib.NBODY_OK
        assert out[5].levels == before.levels[5] and out[5].nodes == before.nodes[5]
        after = b.hierarchy()
    for s in range(len(counts)):
        assert record_bytes(after, s) == record_bytes(before, s), s
    assert ctypes.sizeof(_lib.BatchHierarchySystem) == 40
