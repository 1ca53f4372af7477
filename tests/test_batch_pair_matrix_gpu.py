"""GPU: every batch force loop, one source at a time (tests/pair_matrix_ref.py states the inputs, the reference and the
tolerance).  B copies of one configuration, copy s with a mass word on column c_s alone: one launch returns the n x n matrix
of single pair terms, and every entry is held to a few ulp of its own term against the fp64 one-source step -- a dropped,
doubled or mis-indexed column, a wrong guard or a wrong jerk term shows at its (row, column).

Every family takes one step of DT: step_n(1) with kick-drift, KDK and Hermite, evolve(1, DT, levels=0) for the evolve
families (conditions set so that nothing triggers, and asserted), the massive siblings with n // 2 + 1 massive bodies.  The
source's own row, every row of a system whose source is a tracer and the row lying on top of the source are the null
system's rows bit for bit; mass words, fourth velocity words and slots beyond the counts come back untouched.  The worst
|gpu - ref| / tol of every case is printed; profiles/batch_pair_matrix.txt records them."""
import numpy as np
import pytest

import pair_matrix_ref as pm

pytestmark = pytest.mark.gpu

CAPACITIES = pm.CAPACITIES_FULL + (pm.CAPACITY_LARGE,)     # 1, 2, 4 rows per lane; 128, 256 and 1024 threads
COLLISION_RADIUS = 1e-6                                    # below every separation
ESCAPE_RADIUS = 1e3                                        # beyond every body

#: family: (scheme, step or evolve, massive counts, collision watching, setup)
FAMILIES = {
    "step_kick_drift": ("kick_drift", "step", False, False, None),
    "step_kdk": ("kdk", "step", False, False, None),
    "hermite": ("hermite", "step", False, False, None),
    "step_massive_kick_drift": ("kick_drift", "step", True, False, None),
    "step_massive_kdk": ("kdk", "step", True, False, None),
    "hermite_massive": ("hermite", "step", True, False, None),
    "adaptive": ("hermite", "evolve", False, False, None),
    "field": ("hermite", "evolve", False, False, "field"),
    "stop": ("hermite", "evolve", False, True, "stop"),
    "merge": ("hermite", "evolve", False, True, "merge"),
    "radii": ("hermite", "evolve", False, True, "radii"),
    "radii_merge": ("hermite", "evolve", False, True, "radii_merge"),
    "adaptive_massive": ("hermite", "evolve", True, False, None),
    "fate": ("hermite", "evolve", True, True, "fate"),
    "fate_accrete": ("hermite", "evolve", True, True, "fate_accrete"),
}

_references = {}


def reference(scheme, capacity, eps):
    """The fp64 reference of (capacity, scheme, eps), computed once per session and never written to."""
    key = (scheme, capacity, eps)
    if key not in _references:
        lay = pm.Layout(capacity)
        R = pm.Reference(scheme, capacity, eps, None if capacity in pm.CAPACITIES_FULL else lay.all_sources())
        R.ref.setflags(write=False)
        R.drift.setflags(write=False)
        _references[key] = R
    return _references[key]


def run_family(family, lay, P, V, massive, eps):
    """One step of DT of the batch under `family`; (positions, velocities) as downloaded."""
    import n_body_problem_amd as nb
    scheme, how, _, watching, setup = FAMILIES[family]
    B, cap = lay.num_systems, lay.capacity
    with nb.BatchedSystem(B, cap, counts=lay.counts, integrator=scheme) as b:
        b.set_state(P, V)
        if massive is not None:
            b.set_massive_counts(massive)
        if how == "step":
            b.step_n(1, pm.DT, eps)
            return b.download()
        if setup == "field":
            b.set_external_field([("plummer", 0.0, 1.0)])         # runs the field sibling, adds exactly zero
        if watching:
            radii = setup in ("radii", "radii_merge")
            b.set_stop_conditions(collision_radius=0.0 if radii else COLLISION_RADIUS, escape_radius=ESCAPE_RADIUS)
            if setup in ("merge", "radii_merge"):
                b.set_collision_action("merge", log_capacity=2)
            if setup in ("fate", "fate_accrete"):
                b.set_tracer_action("remove")
            if setup == "fate_accrete":
                b.set_hit_action("accrete")
            if radii:
                b.set_radii(np.full((B, cap), COLLISION_RADIUS, dtype=np.float32))
        r = b.evolve(1, pm.DT, levels=0, softening=eps)
        assert (r.steps == 1).all() and (r.min_level == 0).all() and (r.max_level == 0).all(), (family, r)
        if watching:
            assert not b.stops().reason.any(), (family, "a stopping condition triggered")
            if setup in ("merge", "radii_merge"):
                assert not b.mergers().count.any() and np.array_equal(b.counts, lay.counts), (family, "a merger")
            if setup in ("fate", "fate_accrete"):
                f = b.fates()
                assert not f.fate.any() and not f.hit.any() and not f.escaped.any(), (family, "a fate")
            if setup == "fate_accrete":
                assert not b.accretions().count.any(), (family, "an accretion")
        return b.download()


def state6(p, v, rows):
    return np.concatenate([p[:, :rows, :3], v[:, :rows, :3]], axis=-1)


def check_case(family, capacity, eps):
    scheme, _, with_massive, watching, _ = FAMILIES[family]
    lay = pm.Layout(capacity, coincident=not watching)
    massive = lay.counts // 2 + 1 if with_massive else None
    P, V = lay.batch(massive)
    p, v = run_family(family, lay, P, V, massive, eps)
    where = f"{family} capacity {capacity} eps {eps}: "
    assert np.isfinite(p).all() and np.isfinite(v).all(), where + "a state that is not finite"
    R = reference(scheme, capacity, eps)
    worst = 0.0
    for first, length, count in lay.blocks:
        sl = slice(first, first + length)
        src = lay.sources[sl].copy()
        acting = src.copy()
        if with_massive:
            acting[src >= massive[first]] = -1                 # a tracer's mass word is never read
        ref, tol = R.rows(acting, count)
        got = state6(p[sl], v[sl], count)
        null = got[int(lay.null_of[first]) - first]
        for s in lay.coincident:
            if first <= s < first + length:                    # the row on top of the source: held bit for bit below
                k = s - first
                ref[k, count - 3], tol[k, count - 3] = null[7], 0.0
                mism = pm.bitwise_mismatches(got[k:k + 1, count - 3:count - 2], null[7:8], [0])
                assert not mism, where + f"system {s} source column 7 row {count - 3}, on top of the source, differs from the null row"
        w, fails = pm.check(got, ref, tol, src)
        worst = max(worst, w)
        assert not fails, where + pm.describe([dict(f, system=f["system"] + first) for f in fails])
        mism = pm.bitwise_mismatches(got, null, acting, whole=(acting < 0) & (src >= 0))
        assert not mism, where + "rows that differ from the null system's bit for bit (system, row): " + \
            str([(s + first, i) for s, i in mism[:8]]) + f", sources {[int(src[s]) for s, _ in mism[:8]]}"
    kt = R.kt[R.kt > 0.0]
    print(f"pair-matrix {family} capacity {capacity} eps {eps}: worst |gpu - ref| / tol = {worst:.3f} "
          f"(K_term median {np.median(kt):.1f} max {kt.max():.0f}, K_round {R.kr})")
    assert np.array_equal(p[..., 3].view(np.uint32), P[..., 3].view(np.uint32)), where + "a mass word changed"
    assert np.array_equal(v[..., 3].view(np.uint32), V[..., 3].view(np.uint32)), where + "a fourth velocity word changed"
    beyond = np.arange(capacity)[None, :] >= lay.counts[:, None]
    assert np.array_equal(p[beyond].view(np.uint32), P[beyond].view(np.uint32)) and \
        np.array_equal(v[beyond].view(np.uint32), V[beyond].view(np.uint32)), where + "a slot beyond a count changed"
    assert worst <= 1.0


@pytest.mark.parametrize("eps", pm.SOFTENINGS, ids=["guard", "soft"])
@pytest.mark.parametrize("capacity", CAPACITIES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_pair_term(family, capacity, eps):
    check_case(family, capacity, eps)


# ---- the analysis calls on the same inputs: every row's acceleration, potential and tidal tensor is one term -------------

ANALYSIS_CAPACITIES = (64, 128, 320, pm.CAPACITY_LARGE)
TIDAL_WORDS = (np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2]))


def held(name, got, ref, tol, src, where):
    """pm.check on (S, n, k) arrays of one quantity: the worst ratio, or an AssertionError naming the entry."""
    worst, fails = pm.check(got, ref, tol, src, limit=1)
    if fails:
        f = fails[0]
        raise AssertionError(where + f"{name}: system {f['system']} source column {f['source']} row {f['row']} word "
                             f"{pm.COMPONENTS.index(f['component'])}: got {f['got']!r} ref {f['ref']!r} tol {f['tol']:.3g} "
                             f"(x{f['ratio']:.3g})")
    return worst


@pytest.mark.parametrize("eps", pm.SOFTENINGS, ids=["guard", "soft"])
@pytest.mark.parametrize("capacity", ANALYSIS_CAPACITIES)
def test_gravity_members_and_energy_are_single_terms(capacity, eps):
    import n_body_problem_amd as nb
    lay = pm.Layout(capacity, coincident=False)
    P, V = lay.batch()
    where = f"analysis capacity {capacity} eps {eps}: "
    with nb.BatchedSystem(lay.num_systems, capacity, counts=lay.counts) as b:
        b.set_state(P, V)
        g = b.gravity_at(softening=eps, tidal=True)
        mem = b.members(eps, max_iterations=1)
        energy = b.energy(eps)
    assert (energy[:, 1] == 0.0).all(), where + f"a one-source system has potential energy: {energy[:, 1][energy[:, 1] != 0.0][:4]}"
    worst = {}
    for first, length, count in lay.blocks:
        sl = slice(first, first + length - 1)                      # the block without its null system
        src = lay.sources[sl]
        t = pm.single_terms(capacity, src, eps)
        rows = slice(0, count)
        for name, got, ref, tol in (
                ("acceleration", g.acceleration[sl, rows], t["acc"][:, rows], t["tol_acc"][:, rows]),
                ("potential", g.potential[sl, rows, None], t["pot"][:, rows, None], t["tol_pot"][:, rows, None]),
                ("tidal", g.tidal[sl, rows][..., TIDAL_WORDS[0], TIDAL_WORDS[1]], t["tid"][:, rows], t["tol_tid"][:, rows]),
                ("member potential", mem.potential[sl, rows, None], t["pot"][:, rows, None], t["tol_pot"][:, rows, None])):
            worst[name] = max(worst.get(name, 0.0), held(name, got, ref, tol, src, where))
        null = first + length - 1
        assert not g.acceleration[null].any() and not g.potential[null].any() and not g.tidal[null].any() and \
            not mem.potential[null].any(), where + "the null system has a field"
        assert not g.acceleration[sl, count:].any() and not g.tidal[sl, count:].any() and not g.potential[sl, count:].any()
        assert np.array_equal(g.tidal, np.swapaxes(g.tidal, -1, -2))
    print(f"pair-matrix {where}worst |gpu - ref| / tol: " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))


@pytest.mark.parametrize("eps", pm.SOFTENINGS, ids=["guard", "soft"])
@pytest.mark.parametrize("capacity", ANALYSIS_CAPACITIES)
def test_potential_energy_of_two_massive_columns(capacity, eps):
    """Systems with mass on columns c and c + 1 alone: the potential energy is that pair's."""
    import n_body_problem_amd as nb
    cols = [c for c in pm.large_sources(capacity) if c + 1 < capacity - 5] if capacity == pm.CAPACITY_LARGE \
        else list(range(0, capacity - 6))
    counts = np.array([capacity if k % 2 == 0 else capacity - 5 for k in range(len(cols))], dtype=np.int64)
    m = pm.probe_mass(capacity)
    P, V = pm.probe_batch(capacity, counts, cols, m)
    for s, c in enumerate(cols):
        P[s, c + 1, 3] = m
    with nb.BatchedSystem(len(cols), capacity, counts=counts) as b:
        b.set_state(P, V)
        pe = b.energy(eps)[:, 1]
    x = pm.configuration(capacity)[0].astype(np.float64)
    c = np.array(cols)
    want = -m * m / np.sqrt(((x[c + 1] - x[c]) ** 2).sum(-1) + float(np.float32(eps)) ** 2)
    err = np.abs(pe - want) / np.abs(want)
    print(f"pair-matrix energy capacity {capacity} eps {eps}: worst relative error {err.max():.3g}")
    assert err.max() <= 1e-6, (capacity, eps, int(c[np.argmax(err)]), float(err.max()))
