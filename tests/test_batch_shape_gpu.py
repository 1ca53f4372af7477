"""GPU: the shapes of batched ensembles (BatchedSystem.shape, include/nbody_batch_shape.h).

1. Against the reference (hermite_shape_ref, IEEE doubles in the pinned two-level order) at capacities 64, 128, 256 (one wave
   with one, two and four rows per lane), 1024 (four waves) and 4096 (eight waves with eight rows per lane, the raised LDS
   limit), counts 0, 1, 3, 9, 63, 64, 65, 129, 257, 1025 and 4096 as far as the capacity holds them, in one batch; 1, 3 and 8
   apertures, the latter two with an ellipsoidal shell; the reduced and the plain tensor; both weights; a subset mask;
   per-system radii; one body with a NaN coordinate.  A case is compared only if the reference's margin -- how far, relatively,
   the nearest body stayed from changing sides in any pass -- is at least 1e-9, and no case is left out: the smallest margin
   of these inputs is 2.1e-6.  Then the integers (status, iterations, count, the membership masks, selected, unmeasured,
   converged) are equal, the words made of +, - and x alone (weight, D, M, L, total_weight) are bit-equal, and the words that
   pass through the device's division and square root (q, s, change, eigenvalues, axes) are held to hermite_shape_ref.BOUND =
   2.28e-11: four times the spread 5.7e-12 that the reference itself shows when every quotient and root is moved by up to one
   ulp at random (test_batch_shape_cpu.py measures it again).  Whether the device was in fact bit-equal is printed, not asserted.
   Observed on an MI355X: largest error 0 at every capacity and case -- the device was bit-equal to the reference, these words
   included.  The bound stays.
2. Placement: a system's records are the same bytes in another slot, batch size and capacity.
3. Identities: count is the population of the aperture's bit; a sphere that is never deformed has radial_profile()'s count,
   weight, M and L over the same edge; the face-on view of a tilted disc puts the peak of surface_map() at the map's centre and
   makes the disc thin along the line of sight; members() accepts the mask.
4. evolve, shape, evolve is the two evolves alone bit for bit, plain and with a stop recorded; 8 apertures after 1 agree with a
   fresh handle.
5. Every error is raised with the function named, and leaves the state and a later call untouched."""
import ctypes

import numpy as np
import pytest

import hermite_shape_ref as sref

pytestmark = pytest.mark.gpu

SYSTEM_WORDS = ("selected", "unmeasured", "apertures", "reduced", "converged", "reserved", "total_weight", "centre", "velocity")


def call(batch, kw, **more):
    return batch.shape(kw["radii"], inner=kw["inner"], centre=kw["centre"], velocity=kw["velocity"], weight=kw["weight"],
                       subset=kw["subset"], reduced=kw["reduced"], **more)


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", sref.CAPACITIES)
def test_every_word_against_the_reference(capacity):
    import n_body_problem_amd as nb
    worst, equal, compared = 0.0, True, 0
    pos, vel, counts = sref.gaussian_batch(capacity)
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(pos), np.array(vel))                  # copies: the shared inputs are read-only
        for case in sref.CASES:
            name = case[0]
            p, v, c, kw, (systems, apertures, bodies, margin) = sref.reference(capacity, name)
            assert p.tobytes() == pos.tobytes() and list(c) == list(counts)
            print(f"capacity {capacity} {name}: margin {margin:.3g}")
            assert margin >= sref.LEAST_MARGIN, (name, margin)          # no case is left out
            compared += 1
            res = call(batch, kw, bodies=True)
            A = len(case[1])
            assert res.apertures == A and res.q.shape == (B, A) and res.axes.shape == (B, A, 3, 3) and res.inside.shape == (B, capacity)
            for word in SYSTEM_WORDS:
                assert res.systems[word].tobytes() == systems[word].tobytes(), (name, word, res.systems[word], systems[word])
            for word in sref.INTEGER_WORDS + ("radius", "inner"):
                assert res.aperture_records[word].tobytes() == apertures[word].tobytes(), (name, word, res.aperture_records[word], apertures[word])
            assert res.body_records.tobytes() == bodies.tobytes(), name
            for word in sref.EXACT_WORDS:
                assert res.aperture_records[word].tobytes() == apertures[word].tobytes(), (name, word)
            error = sref.rooted_error(res.aperture_records, apertures)
            worst = max(worst, error)
            same = all(res.aperture_records[w].tobytes() == apertures[w].tobytes() for w in sref.ROOTED_WORDS)
            equal = equal and same
            print(f"capacity {capacity} {name}: largest error of q, s, change, eigenvalues, axes {error:.3g} (bound {sref.BOUND:.3g}); "
                  f"{'bit-equal' if same else 'not bit-equal'}")
            assert error <= sref.BOUND, (name, error)
            # lean calls: the remaining records are the same bits
            lean = call(batch, kw, apertures=False)
            assert lean.q is None and lean.inside is None and lean.systems.tobytes() == res.systems.tobytes(), name
            only = call(batch, kw)
            assert only.body_records is None and only.systems.tobytes() == res.systems.tobytes()
            assert only.aperture_records.tobytes() == res.aperture_records.tobytes(), name
        # a torch mask and a (3,) frame are the numpy ones
        import torch
        p, v, c, kw, (systems, apertures, bodies, margin) = sref.reference(capacity, "3-shell-unreduced-number-sparse")
        res = batch.shape(torch.as_tensor(kw["radii"]), inner=kw["inner"], centre=sref.CENTRE, velocity=sref.VELOCITY, weight="number",
                          subset=torch.as_tensor(np.array(kw["subset"])).bool(), reduced=False)
        assert res.systems.tobytes() == systems.tobytes() and res.aperture_records["M"].tobytes() == apertures["M"].tobytes()
    assert compared == len(sref.CASES)
    print(f"capacity {capacity}: worst error {worst:.3g} of the bound {sref.BOUND:.3g}; the device was "
          f"{'bit-equal' if equal else 'not bit-equal'} to the reference")


# ---- 2. placement -----------------------------------------------------------------------------------------------------------------
def test_a_systems_records_are_the_same_bytes_in_another_slot_batch_size_and_capacity():
    n = 60
    import n_body_problem_amd as nb
    body, speed = sref.gaussian_system(n, n, seed=5100)
    rng = np.random.default_rng(5101)
    mask = rng.random(n) < 0.9
    mine, mine_inner = np.array([1.0, 2.5, 1.75]), np.array([0.0, 0.5, 0.0])
    centre, velocity = np.array(sref.CENTRE) + 0.01, np.array(sref.VELOCITY)
    for reduced in (True, False):
        first = None
        for capacity, B, slot in ((64, 1, 0), (64, 5, 3), (128, 3, 2), (256, 4, 1), (1024, 2, 0), (4096, 2, 1)):
            P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
            counts = [min(capacity, 40 + 30 * s) for s in range(B)]
            for s in range(B):
                P[s], V[s] = sref.gaussian_system(capacity, counts[s], seed=5200 + s)
            P[slot, :n], V[slot, :n], counts[slot] = body, speed, n
            S = rng.random((B, capacity)) < 0.8
            S[slot, :n] = mask
            radii = np.array([1.5, 2.0, 3.0])[None, :] * (1.0 + 0.1 * np.arange(B))[:, None]
            inner = np.zeros_like(radii)
            radii[slot], inner[slot] = mine, mine_inner
            C, U = rng.normal(size=(B, 3)) * 0.1, rng.normal(size=(B, 3)) * 0.1
            C[slot], U[slot] = centre, velocity
            with nb.BatchedSystem(B, capacity, counts=counts) as batch:
                batch.set_state(P, V)
                res = batch.shape(radii, inner=inner, centre=C, velocity=U, subset=S, reduced=reduced, bodies=True)
            assert not res.inside[slot, n:].any()
            got = res.systems[slot].tobytes() + res.aperture_records[slot].tobytes() + res.body_records[slot, :n].tobytes()
            assert res.count[slot].max() > n // 2 and res.selected[slot] == mask.sum() and (res.status[slot] <= 1).any()
            if first is None:
                first = got
            assert got == first, (reduced, capacity, B, slot)


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------
def test_count_is_the_population_of_the_bit_and_an_undeformed_sphere_is_radial_profiles_shell():
    """max_iterations=1 alone does not keep the sphere: the one pass deforms the ellipsoid and the final walk runs under the
    deformed one, as the header states.  With min_members above every count the pass ends FEW, the identity stays, and the
    final walk is radial_profile()'s shell (inner, R]: count, M and L bit for bit for the systems of at most 64 bodies, whose
    two-level order is radial_profile()'s, and count and the number weight for all."""
    import n_body_problem_amd as nb
    capacity = 256
    pos, vel, counts, kw, (systems, apertures, bodies, _) = sref.reference(capacity, "8-shell-reduced-mass-own")
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(pos), np.array(vel))
        res = call(batch, kw, bodies=True)
        for a in range(8):
            assert np.array_equal(res.members_mask(a).sum(axis=1), res.count[:, a]), a
        assert res.count.sum() > 0 and np.array_equal(res.converged, (res.status == 0).sum(axis=1))
        for weight in ("mass", "number"):
            sphere = batch.shape([2.0], inner=[0.5], centre=kw["centre"], velocity=kw["velocity"], weight=weight, reduced=False,
                                 max_iterations=1, min_members=1 << 20)
            shell = batch.radial_profile([0.5, 2.0], centre=kw["centre"], velocity=kw["velocity"], weight=weight)
            assert (sphere.status == 2).all() and (sphere.iterations == 1).all() and (sphere.q == 1.0).all()
            assert np.array_equal(sphere.axes[:, 0], np.broadcast_to(np.eye(3), (B, 3, 3)))
            assert np.array_equal(sphere.count[:, 0], shell.count[:, 0]) and shell.count.sum() > 0
            small = np.asarray(counts) <= 64
            for word, theirs in (("weight", shell.weight_sum), ("M", shell.M), ("L", shell.L)):
                assert getattr(sphere, word)[small, 0].tobytes() == theirs[small, 0].tobytes(), (weight, word)
                assert np.allclose(getattr(sphere, word)[:, 0], theirs[:, 0], rtol=1e-12, atol=1e-12)
            if weight == "number":
                assert np.array_equal(sphere.weight[:, 0], shell.weight_sum[:, 0])
            assert sphere.total_weight[small].tobytes() == shell.total_weight[small].tobytes()


def test_the_face_on_view_of_a_tilted_disc_peaks_at_the_map_centre_and_members_accepts_the_mask():
    import n_body_problem_amd as nb
    n, capacity, B = 1000, 1024, 3
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    rots = []
    for s in range(B):
        rot = sref.rotation(np.random.default_rng(5300 + s))
        rots.append(rot)
        P[s], V[s] = sref.gaussian_system(capacity, n, seed=5310 + s, sigmas=(1.0, 0.8, 0.05), rot=rot)
    with nb.BatchedSystem(B, capacity, counts=[n] * B) as batch:
        batch.set_state(P, V)
        res = batch.shape([2.0], centre=sref.CENTRE, velocity=sref.VELOCITY, bodies=True)
        assert (res.status == 0).all() and (res.s < 0.15).all() and (res.q > 0.6).all()
        for s in range(B):                                             # the minor axis is the disc's normal, up to its sign
            assert abs(float(res.axes[s, 0, 2] @ rots[s][2])) > 0.999
        tilt = res.misalignment()
        assert ((tilt < 0.2) | (tilt > np.pi - 0.2)).all(), tilt      # it turns about its minor axis, whichever way e3 points
        # 3 x 3 cells 1.5 wide: of 1000 bodies with dispersions 1 and 0.8 the centre cell expects 356 and the next one 139, far
        # beyond the sampling noise (a finer grid's neighbouring cells differ by less than their square roots)
        edges = nb.SurfaceMapResult.grid(2.25, 3)
        face = batch.surface_map(edges, centre=sref.CENTRE, velocity=sref.VELOCITY, axes=res.view(0, "face_on"))
        edge = batch.surface_map(edges, centre=sref.CENTRE, velocity=sref.VELOCITY, axes=res.view(0, "edge_on"))
        assert (face.peak == 1 * 3 + 1).all(), face.peak                # the centre cell of 3 x 3
        thin, thick = face.depth_dispersion()[:, 1, 1], edge.depth_dispersion()[:, 1, 1]
        assert (thin < 0.08).all() and (thick > 0.3).all(), (thin, thick)
        assert (edge.count[:, [0, 2], :].sum(axis=(1, 2)) == 0).all()  # edge-on nothing lies far above or below the plane
        mask = res.members_mask(0)
        assert mask.shape == (B, capacity) and mask.dtype == np.bool_ and np.array_equal(mask.sum(axis=1), res.count[:, 0])
        bound = batch.members(0.01, initial=mask)
        assert not (bound.member & ~mask).any() and (bound.count <= res.count[:, 0]).all()   # nobody outside the ellipsoid
        again = batch.shape([2.0], centre=sref.CENTRE, velocity=sref.VELOCITY, subset=mask, bodies=True)
        assert np.array_equal(again.selected, res.count[:, 0]) and not (again.members_mask(0) & ~mask).any()


# ---- 4. changes nothing -----------------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between, stop=None):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        if stop:
            b.set_stop_conditions(**stop)
        b.set_state(np.array(P), np.array(V))
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        if between:
            b.shape([0.5, 1.0, 2.0, 4.0], centre="density", bodies=True)
            mask = np.zeros((P.shape[0], P.shape[1]), bool)
            mask[:, ::2] = True
            b.shape([1.5], inner=[0.25], weight="number", subset=mask, reduced=False, apertures=False)
        r = b.evolve(2, 1.0 / 256.0, levels=8, softening=0.01)
        p, v = b.download()
        return p, v, r, b.stops() if stop else None


@pytest.mark.parametrize("stop", [None, dict(escape_radius=2.5)], ids=["plain", "with a stop recorded"])
def test_evolve_shape_evolve_is_the_two_evolves_alone_bit_for_bit(stop):
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


def test_a_call_with_8_apertures_after_one_with_1_agrees_with_a_fresh_handle():
    """The aperture buffers are sized by the first call and grown by a later, larger one."""
    import n_body_problem_amd as nb
    capacity = 128
    p, v, counts, kw1, (systems1, apertures1, _, _) = sref.reference(capacity, "1-reduced-mass")
    _, _, _, kw8, _ = sref.reference(capacity, "8-shell-reduced-mass-own")
    with nb.BatchedSystem(len(counts), capacity, counts=counts) as batch:
        batch.set_state(np.array(p), np.array(v))
        small = call(batch, kw1, bodies=True)
        grown = call(batch, kw8, bodies=True)
        again = call(batch, kw1, bodies=True)
    with nb.BatchedSystem(len(counts), capacity, counts=counts) as fresh:
        fresh.set_state(np.array(p), np.array(v))
        alone = call(fresh, kw8, bodies=True)
    assert grown.systems.tobytes() == alone.systems.tobytes() and grown.aperture_records.tobytes() == alone.aperture_records.tobytes()
    assert grown.body_records.tobytes() == alone.body_records.tobytes() and grown.count.sum() > 0
    assert again.aperture_records.tobytes() == small.aperture_records.tobytes() and again.systems.tobytes() == small.systems.tobytes()
    assert again.body_records.tobytes() == small.body_records.tobytes()
    for word in sref.EXACT_WORDS + sref.INTEGER_WORDS:
        assert small.aperture_records[word].tobytes() == apertures1[word].tobytes(), word


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------
def test_every_error_is_refused_with_its_message_and_leaves_the_state_and_a_later_call_unaffected():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    capacity = 64
    P, V, counts, kw, _ = sref.reference(capacity, "1-reduced-mass")
    B = len(counts)
    with nb.BatchedSystem(B, capacity, counts=counts) as batch:
        batch.set_state(np.array(P), np.array(V))
        before = call(batch, kw, bodies=True)
        lib, h, pos, vel = batch._lib, batch._h, _ptr(batch.positions), _ptr(batch.velocities)
        out = (_lib.BatchShapeSystem * B)()
        out[2].selected = -7                                       # a refused call writes nothing
        doubles = lambda values: (ctypes.c_double * len(values))(*values)   # noqa: E731
        good = doubles([1.0, 2.0])
        nan, inf = float("nan"), float("inf")
        own = np.tile(np.array([1.0, 2.0]), (B, 1))
        own_inner = np.zeros((B, 2))
        own_inner[3, 1] = 2.0
        zeros = [0.0] * (3 * B)
        bad_centre, bad_velocity = list(zeros), list(zeros)
        bad_centre[3 * 2 + 1], bad_velocity[3 * 4] = nan, -inf
        #   pos, vel, apertures, radii, inner, per_system, centre, velocity, weight, reduced, tol, max_iterations, min_members, subset,
        #   systems, apertures_out, bodies
        def args(**change):
            a = dict(pos=pos, vel=vel, apertures=2, radii=good, inner=None, per_system=0, centre=None, velocity=None, weight=0,
                     reduced=1, tol=1e-3, max_iterations=64, min_members=10, subset=None, systems=out, apertures_out=None, bodies=None)
            a.update(change)
            return tuple(a.values())
        cases = [(args(pos=None), b"NULL argument"), (args(vel=None), b"NULL argument"), (args(radii=None), b"NULL argument"),
                 (args(systems=None), b"NULL argument"),
                 (args(apertures=0), b"apertures must be 1 ... 8"), (args(apertures=9), b"apertures must be 1 ... 8"),
                 (args(radii=doubles([1.0, 0.0])), b"the radius of aperture 1 of all systems must be finite and > 0"),
                 (args(radii=doubles([-1.0, 2.0])), b"the radius of aperture 0 of all systems must be finite and > 0"),
                 (args(radii=doubles([nan, 2.0])), b"the radius of aperture 0 of all systems must be finite and > 0"),
                 (args(radii=doubles([1.0, inf])), b"the radius of aperture 1 of all systems must be finite and > 0"),
                 (args(inner=doubles([-0.5, 0.0])), b"the inner radius of aperture 0 of all systems must be finite, >= 0 and below its radius"),
                 (args(inner=doubles([0.0, nan])), b"the inner radius of aperture 1 of all systems must be finite"),
                 (args(inner=doubles([1.0, 0.0])), b"the inner radius of aperture 0 of all systems must be finite, >= 0 and below its radius"),
                 (args(radii=doubles(own.ravel().tolist()), inner=doubles(own_inner.ravel().tolist()), per_system=1),
                  b"the inner radius of aperture 1 of system 3 must be finite"),
                 (args(weight=2), b"weight must be"), (args(weight=-1), b"weight must be"),
                 (args(tol=nan), b"tol must be finite and >= 0"), (args(tol=inf), b"tol must be finite and >= 0"),
                 (args(tol=-1e-3), b"tol must be finite and >= 0"),
                 (args(max_iterations=0), b"max_iterations must be 1 ... 64"), (args(max_iterations=65), b"max_iterations must be 1 ... 64"),
                 (args(min_members=3), b"min_members must be >= 4"),
                 (args(centre=doubles(bad_centre)), b"the centre of system 2 must be finite"),
                 (args(velocity=doubles(bad_velocity)), b"the velocity of system 4 must be finite")]
        for a, message in cases:
            assert lib.nbody_batch_shape(h, *a) == _lib.NBODY_ERR_INVALID, a
            error = lib.nbody_batch_last_error(h)
            assert error.startswith(b"nbody_batch_shape: ") and message in error, (a, error)
            assert out[2].selected == -7
        assert lib.nbody_batch_shape(None, *args()) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_shape: batch is NULL" in lib.nbody_batch_last_error(None)
        with pytest.raises(ValueError, match="apertures must be"):
            batch.shape(np.arange(1.0, 10.0))
        with pytest.raises(ValueError, match="radii must have shape"):
            batch.shape(np.ones((B + 1, 3)))
        with pytest.raises(ValueError, match="inner must have shape"):
            batch.shape([1.0, 2.0], inner=[0.0])
        with pytest.raises(ValueError, match="weight must be"):
            batch.shape([1.0], weight="charge")
        with pytest.raises(ValueError, match="centre must"):
            batch.shape([1.0], centre="mass")
        with pytest.raises(ValueError, match="centre must have shape"):
            batch.shape([1.0], centre=np.zeros((B, 2)))
        with pytest.raises(ValueError, match="bool or uint8"):
            batch.shape([1.0], subset=np.ones((B, capacity), np.int32))
        with pytest.raises(ValueError, match="subset must have shape"):
            batch.shape([1.0], subset=np.ones((B, capacity - 1), bool))
        with pytest.raises(nb.NBodyError, match="nbody_batch_shape: the inner radius of aperture 0 of all systems"):
            batch.shape([1.0], inner=[1.0])
        with pytest.raises(nb.NBodyError, match="nbody_batch_shape: the centre of system 0 must be finite"):
            batch.shape([1.0], centre=(0.0, np.inf, 0.0))
        with pytest.raises(nb.NBodyError, match="nbody_batch_shape: min_members must be >= 4"):
            batch.shape([1.0], min_members=1)
        assert lib.nbody_batch_shape(h, *args()) == _lib.NBODY_OK
        assert out[2].selected == counts[2] and out[2].apertures == 2 and out[2].reduced == 1
        after = call(batch, kw, bodies=True)
        p, v = batch.download()
    assert after.systems.tobytes() == before.systems.tobytes() and after.aperture_records.tobytes() == before.aperture_records.tobytes()
    assert after.body_records.tobytes() == before.body_records.tobytes()
    assert np.array_equal(np.asarray(p).view(np.uint32), P.view(np.uint32)) and np.array_equal(np.asarray(v).view(np.uint32), V.view(np.uint32))
