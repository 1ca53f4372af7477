"""GPU: the cluster structure of batched ensembles (BatchedSystem.structure, include/nbody_batch_structure.h).  The k-th
neighbour distances, the bodies inside them and their weight agree with the fp64 reference (hermite_structure_ref) at every
workgroup shape and with ragged counts; the densities, the system records, the radii, the enclosed weights and the Lagrangian
radii follow the header's formulas from what the call itself returned, to fp64 round-off or exactly; inversion-symmetric
shells have their closed values; degenerate systems fall back as the header says; massive counts and removed tracers change
nothing; a system's records are the same bits wherever it runs; the call disturbs no evolve; and every error is reported.

Capacities: 64 (one row per lane), 128 (two), 130 (four rows per lane, one wave), 257 (two waves: the sums and minima across
waves), 4096 (sixteen waves, 64 KiB of dynamic LDS beside the reduction words: the raised limit).  The inputs are Plummer
spheres about (3, -2, 1.5) with masses uniform in [0.5, 2] / n; test_batch_structure_cpu.py shows that the float32 search
finds the fp64 neighbours on them and that their radii are apart, so that the agreement asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_structure_ref as sref

pytestmark = pytest.mark.gpu


def run_structure(P, counts, k=6, weight="mass", fractions=sref.FRACTIONS, bodies=True, massive=None):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts) as b:
        b.set_state(np.array(P), np.zeros_like(P))                 # a copy: the shared inputs are read-only
        if massive is not None:
            b.set_massive_counts(massive)
        return b.structure(k=k, weight=weight, fractions=fractions, bodies=bodies)


def r2_of(res):
    """The records' neighbour_r2 back from neighbour_distance: the square of an fp64 root of a float32 rounds to that float32."""
    return (res.neighbour_distance * res.neighbour_distance).astype(np.float32)


def rel(got, want):
    """max |got - want| / |want| over the entries (0 where both are equal, infinities included)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(err, initial=0.0))


def system_bits(res, s):
    return np.concatenate([res.centre[s], [res.core_radius[s], res.core_density[s], res.total_weight[s]], res.lagrangian[s]]).view(np.uint64)


def check_against_reference(res, P, counts, k, weight, refs, fractions=sref.FRACTIONS):
    """The checks of one batch, system by system; prints its figures before it asserts."""
    r2 = r2_of(res)
    for s, (n, ref) in enumerate(zip(counts, refs)):
        w = sref.weights(P[s], n, weight)
        # the search against the fp64 reference
        e_r2 = rel(r2[s, :n], ref["r2_k"])
        ok = ref["gap_ok"]
        e_nw = rel(res.neighbour_weight[s, :n][ok], ref["neighbour_weight"][ok])
        wrong = int((res.inside[s, :n][ok] != ref["inside"][ok]).sum())
        # the formulas from what the call returned
        e_rho = rel(res.density[s, :n], sref.density_of(r2[s, :n], res.neighbour_weight[s, :n]))
        want = sref.system_from(P[s], n, weight, res.density[s], r2[s])
        d_centre = np.abs(res.centre[s] - want["centre"])
        e_core = max(rel(res.core_radius[s], want["core_radius"]), rel(res.core_density[s], want["core_density"]))
        e_radius = rel(res.radius[s, :n], sref.radii_from(P[s], n, res.centre[s])[1])
        enclosed = sref.enclosed_from(res.radius[s, :n], w)
        lagrange = sref.lagrange_from(res.radius[s, :n], res.enclosed[s, :n], res.total_weight[s], fractions)
        print(f"system {s} (n = {n}): r2_k {e_r2:.2g}, {n - int(ok.sum())} rows left out, inside wrong on {wrong}, weight {e_nw:.2g}, "
              f"density {e_rho:.2g}, centre {d_centre.max():.2g} (scale {want['scale'].max():.2g}), core {e_core:.2g}, "
              f"radius {e_radius:.2g}; against the reference: centre {np.abs(res.centre[s] - ref['centre']).max():.2g}, "
              f"core radius {rel(res.core_radius[s], ref['core_radius']):.2g}, lagrange {rel(res.lagrangian[s], ref['lagrange']):.2g}")
        assert e_r2 <= 1e-6, (s, e_r2)
        assert np.array_equal(np.isinf(r2[s, :n]), np.isinf(ref["r2_k"])), s
        assert n - int(ok.sum()) <= 0.01 * n, s
        assert wrong == 0 and e_nw <= 1e-6, (s, wrong, e_nw)
        assert e_rho <= 1e-14, (s, e_rho)
        assert np.all(d_centre <= 1e-12 * want["scale"]), (s, d_centre, want["scale"])
        assert e_core <= 1e-11, (s, e_core)
        assert res.total_weight[s] == want["total_weight"] and res.estimated[s] == want["estimated"] == ref["estimated"], s
        assert e_radius <= 1e-12, (s, e_radius)
        assert np.array_equal(res.enclosed[s, :n], enclosed), s
        assert np.array_equal(res.lagrangian[s], lagrange), (s, res.lagrangian[s], lagrange)
        # beyond the count: the empty record
        for name in ("density", "radius", "enclosed", "neighbour_distance", "neighbour_weight", "inside"):
            assert not getattr(res, name)[s, n:].any(), (s, name)
    assert np.array_equal(res.lagrangian_radii(fractions), res.lagrangian)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity,k,weight", list(sref.all_cases()))
def test_the_records_agree_with_the_reference_and_follow_the_formulas(capacity, k, weight):
    P, counts = sref.gpu_inputs(capacity, k, weight)
    res = run_structure(P, counts, k, weight)
    assert res.centre.shape == (len(counts), 3) and res.lagrangian.shape == (len(counts), 3) and res.estimated.dtype == np.int32
    assert res.density.shape == (len(counts), capacity) and res.density.dtype == np.float64 and res.inside.dtype == np.int32
    check_against_reference(res, P, counts, k, weight, sref.reference(capacity, k, weight))
    lean = run_structure(P, counts, k, weight, bodies=False)
    assert lean.density is None and lean.radius is None and lean.inside is None
    assert np.array_equal(lean.estimated, res.estimated)
    for s in range(len(counts)):
        assert np.array_equal(system_bits(lean, s), system_bits(res, s)), s


# ---- 2. the symmetric shells -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", sref.KS)
def test_inversion_symmetric_shells_have_their_closed_values(k):
    pos, closed = sref.shells()
    n = closed["n"]
    P = np.full((2, 64, 4), sref.FILL, dtype=np.float32)
    P[:, :n] = pos
    res = run_structure(P, [n, n], k, fractions=(0.25, 0.5))
    ref = sref.structure(pos, n, k, fractions=(0.25, 0.5))
    print(res.centre[0] - closed["centre"], res.lagrangian[0], res.core_radius[0], ref["core_radius"], res.core_density[0])
    for s in (0, 1):
        assert np.abs(res.centre[s] - closed["centre"]).max() <= 1e-13
        assert abs(res.lagrangian[s, 0] - 1.0) <= 1e-12 and abs(res.lagrangian[s, 1] - 2.0) <= 1e-12
        assert res.estimated[s] == n and res.total_weight[s] == n / 32.0
        # every r2 is exact in fp32, so the search is the reference's and the core follows to round-off
        assert np.array_equal(r2_of(res)[s, :n].astype(np.float64), ref["r2_k"]) and np.array_equal(res.inside[s, :n], ref["inside"])
        assert np.array_equal(res.neighbour_weight[s, :n].astype(np.float64), ref["neighbour_weight"])
        assert rel(res.core_radius[s], ref["core_radius"]) <= 1e-11 and rel(res.core_density[s], ref["core_density"]) <= 1e-11
        assert np.array_equal(res.density[s, :n // 2], res.density[s, n // 2:n])        # mirrored bodies
    assert np.array_equal(system_bits(res, 0), system_bits(res, 1))


# ---- 3. degenerate cases -------------------------------------------------------------------------------------------------
def test_too_few_bodies_fall_back_to_the_centre_of_weight():
    k = 6
    counts = [1, 3, 6]                                           # n <= k: nobody has a k-th neighbour
    P = sref.ragged(64, counts, 7700)
    res = run_structure(P, counts, k)
    for s, n in enumerate(counts):
        x, w = P[s, :n, :3].astype(np.float64), P[s, :n, 3].astype(np.float64)
        cow = (w[:, None] * x).sum(0) / w.sum()
        assert res.estimated[s] == 0 and res.core_radius[s] == 0 and res.core_density[s] == 0 and not res.density[s].any()
        # r2_k = +inf: every neighbour pair is inside it, and the density is 0 all the same
        assert np.all(np.isinf(res.neighbour_distance[s, :n])) and np.all(res.inside[s, :n] == n - 1) and not res.inside[s, n:].any()
        others = [np.cumsum(np.delete(P[s, :n, 3], i), dtype=np.float32)[-1] if n > 1 else 0.0 for i in range(n)]
        assert np.array_equal(res.neighbour_weight[s, :n], np.asarray(others, dtype=np.float32))
        assert np.all(np.abs(res.centre[s] - cow) <= 1e-12 * np.abs(x).max(0)), s
        assert res.total_weight[s] == w.sum()
        assert np.array_equal(res.enclosed[s, :n], sref.enclosed_from(res.radius[s, :n], w))
        assert np.array_equal(res.lagrangian[s], sref.lagrange_from(res.radius[s, :n], res.enclosed[s, :n], res.total_weight[s], sref.FRACTIONS))
    assert res.radius[0, 0] == 0 and res.lagrangian[0].tolist() == [0, 0, 0]       # one body is its own centre


def test_coincident_bodies_are_not_each_others_neighbours_and_ties_are_not_inside():
    P = np.full((2, 64, 4), sref.FILL, dtype=np.float32)
    P[0, :3] = [[2, 0, 0, 1], [2, 0, 0, 1], [5, 0, 0, 1]]      # bodies 0 and 1 coincide
    P[1, :3] = [[0, 0, 0, 1], [1, 0, 0, 1], [-1, 0, 0, 1]]     # body 0 has two neighbours at the same distance
    one = run_structure(P, [3, 3], k=1)
    assert one.neighbour_distance[0, :3].tolist() == [3, 3, 3] and one.estimated[0] == 3 and not one.inside[0].any()
    two = run_structure(P, [3, 3], k=2)
    assert np.isinf(two.neighbour_distance[0, :2]).all() and two.neighbour_distance[0, 2] == 3 and two.estimated[0] == 1
    # bodies 0 and 1 have one neighbour each, inside their infinite second distance; body 2's two neighbours tie: neither is inside
    assert two.inside[0, :3].tolist() == [1, 1, 0]
    for res, k in ((one, 1), (two, 2)):
        for s in (0, 1):
            ref = sref.structure(P[s], 3, k)
            assert np.array_equal(r2_of(res)[s, :3].astype(np.float64), ref["r2_k"]) and np.array_equal(res.inside[s, :3], ref["inside"])
            assert np.array_equal(res.neighbour_weight[s, :3].astype(np.float64), ref["neighbour_weight"]) and res.estimated[s] == ref["estimated"]
    assert two.neighbour_distance[1, :3].tolist() == [1, 2, 2] and two.inside[1, :3].tolist() == [0, 1, 1]
    assert two.density[1, 0] == 0 and two.neighbour_weight[1, :3].tolist() == [0, 1, 1]


def test_a_zero_state_returns_all_zeros():
    P = np.zeros((2, 130, 4), dtype=np.float32)
    for weight in sref.WEIGHTS:
        res = run_structure(P, [130, 0], k=6, weight=weight)
        assert not system_bits(res, 1).any() and not res.estimated.any()
        assert np.isinf(res.neighbour_distance[0]).all() and not res.neighbour_distance[1].any()
        for name in ("density", "radius", "neighbour_weight", "inside"):
            assert not getattr(res, name).any(), name
        if weight == "mass":                                     # no weight at all: everything is 0
            assert not system_bits(res, 0).any() and not res.enclosed.any()
        else:                                                    # 130 bodies of weight 1 at the origin
            assert res.total_weight[0] == 130 and not res.centre[0].any() and not res.lagrangian[0].any()
            assert np.all(res.enclosed[0] == 130)


# ---- 4. massive counts and removed tracers ---------------------------------------------------------------------------------
def test_massive_counts_and_removed_tracers_change_nothing():
    import n_body_problem_amd as nb
    n, m, B = 60, 3, 2
    P, V = np.zeros((B, 64, 4), np.float32), np.zeros((B, 64, 4), np.float32)
    for s in range(B):
        pos, vel = nb.plummer(n, seed=7800 + s)
        order = np.argsort((pos[:, :3].astype(np.float64) ** 2).sum(1))          # the innermost bodies are the massive ones
        P[s, :n], V[s, :n] = pos[order], vel[order]
        P[s, :n, 3] = sref.cluster(n, 7800 + s)[:, 3]
    assert np.all((P[:, :m, :3].astype(np.float64) ** 2).sum(-1) < 1.0)
    with nb.BatchedSystem(B, 64, counts=[n] * B, integrator="hermite") as b:
        b.set_massive_counts([m] * B)
        b.set_tracer_action("remove")
        b.set_stop_conditions(escape_radius=1.5)
        b.set_state(P, V)
        b.evolve(2, 1.0 / 256.0, levels=6, softening=0.01)
        removed = b.fates().escaped
        with_them = b.structure(k=6), b.structure(k=6, weight="number")
        p, v = b.download()
    assert np.all(removed > 0)                                   # tracers beyond 1.5 were removed: frozen where they are
    without = run_structure(p, [n] * B, 6), run_structure(p, [n] * B, 6, "number")
    for a, c in zip(with_them, without):
        assert np.array_equal(a.estimated, c.estimated) and a.estimated[0] == n
        for s in range(B):
            assert np.array_equal(system_bits(a, s), system_bits(c, s)), s
        for name in ("density", "radius", "enclosed", "neighbour_distance"):
            assert np.array_equal(getattr(a, name).view(np.uint64), getattr(c, name).view(np.uint64)), name
        assert np.array_equal(a.inside, c.inside) and np.array_equal(a.neighbour_weight.view(np.uint32), c.neighbour_weight.view(np.uint32))


# ---- 5. invariance ---------------------------------------------------------------------------------------------------------
def test_a_system_gives_the_same_bits_in_another_slot_batch_and_capacity():
    n = 60
    pos, other = sref.cluster(n, 4242), sref.cluster(n, 4243)
    body, system = [], []
    for cap, B, slot in ((64, 1, 0), (64, 5, 3), (130, 2, 1), (257, 3, 2)):
        P = np.full((B, cap, 4), sref.FILL, dtype=np.float32)
        P[:, :n] = other
        P[slot, :n] = pos
        res = run_structure(P, [n] * B)
        body.append((r2_of(res)[slot, :n].view(np.uint32), res.inside[slot, :n], res.neighbour_weight[slot, :n].view(np.uint32),
                     res.density[slot, :n].view(np.uint64)))
        system.append((system_bits(res, slot), res.estimated[slot]))
    for rec in body[1:]:
        for a, b in zip(body[0], rec):
            assert np.array_equal(a, b)
    assert np.array_equal(system[0][0], system[1][0])           # another slot and B at one capacity: the same bits
    for bits, estimated in system[1:]:
        assert estimated == system[0][1] == n
        assert rel(bits.view(np.float64), system[0][0].view(np.float64)) <= 1e-12


# ---- 6. non-interference ---------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between, stop=None):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        if stop:
            b.set_stop_conditions(**stop)
        b.set_state(P, V)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.structure()
            b.structure(k=1, weight="number", fractions=(), bodies=False)
        r = b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        st = b.stops() if stop else None
        return p, v, r, st


@pytest.mark.parametrize("stop", [None, dict(escape_radius=4.5)], ids=["plain", "with a stop recorded"])
def test_evolve_structure_evolve_is_the_two_evolves_alone_bit_for_bit(stop):
    import n_body_problem_amd as nb
    counts = [40, 17, 64]
    P = sref.ragged(64, counts, 6100)
    V = np.full_like(P, sref.FILL)
    for s, n in enumerate(counts):
        V[s, :n] = nb.plummer(n, seed=6100 + s)[1]
    pa, va, ra, sa = two_evolves(P, V, counts, False, stop)
    pb, vb, rb, sb = two_evolves(P, V, counts, True, stop)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(ra.steps, rb.steps) and np.array_equal(ra.ticks, rb.ticks)
    if stop:
        assert sa.stopped.any()                                  # the clusters' centre is 3.9 from the origin: bodies are beyond 4.5
        assert np.array_equal(sa.reason, sb.reason) and np.array_equal(sa.ticks, sb.ticks) and np.array_equal(sa.escaper, sb.escaper)


# ---- 7. errors -------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    n = 50
    P = sref.ragged(64, [n, n], 6300)
    with nb.BatchedSystem(2, 64, counts=[n, n]) as b:
        b.set_state(P, np.zeros_like(P))
        before = b.structure()
        lib, h, pos = b._lib, b._h, _ptr(b.positions)
        out = (_lib.BatchStructureSystem * 2)()
        good = (ctypes.c_double * 3)(0.1, 0.5, 0.9)

        def fractions(*values):
            return (ctypes.c_double * len(values))(*values)

        cases = [((None, 6, 0, good, 3, out, None), b"NULL argument"), ((pos, 6, 0, good, 3, None, None), b"NULL argument"),
                 ((pos, 0, 0, good, 3, out, None), b"k must be 1 ... 8"), ((pos, 9, 0, good, 3, out, None), b"k must be 1 ... 8"),
                 ((pos, 6, 2, good, 3, out, None), b"weight must be"), ((pos, 6, -1, good, 3, out, None), b"weight must be"),
                 ((pos, 6, 0, good, -1, out, None), b"n_fractions must be 0 ... 8"),
                 ((pos, 6, 0, fractions(*[0.1] * 9), 9, out, None), b"n_fractions must be 0 ... 8"),
                 ((pos, 6, 0, None, 1, out, None), b"fractions is NULL"),
                 ((pos, 6, 0, fractions(0.5, 0.0), 2, out, None), b"a fraction must be in (0, 1]"),
                 ((pos, 6, 0, fractions(1.0000001), 1, out, None), b"a fraction must be in (0, 1]"),
                 ((pos, 6, 0, fractions(-0.5), 1, out, None), b"a fraction must be in (0, 1]"),
                 ((pos, 6, 0, fractions(float("nan")), 1, out, None), b"a fraction must be in (0, 1]")]
        for args, message in cases:
            assert lib.nbody_batch_structure(h, *args) == _lib.NBODY_ERR_INVALID, args
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_structure: ") and message in error, (args, error)
        with pytest.raises(nb.NBodyError):
            b.structure(k=9)
        with pytest.raises(ValueError):
            b.structure(weight="light")
        assert lib.nbody_batch_structure(h, pos, 6, 0, None, 0, out, None) == _lib.NBODY_OK   # no fractions at all is a call
        assert out[0].lagrange[0] == 0 and out[0].centre[0] == before.centre[0, 0]
        assert b.structure(fractions=(1.0,)).lagrangian[0, 0] == before.radius[0, :n].max()  # f = 1 is in (0, 1]
        after = b.structure()
    for s in range(2):
        assert np.array_equal(system_bits(after, s), system_bits(before, s))
    assert np.array_equal(after.density.view(np.uint64), before.density.view(np.uint64))
