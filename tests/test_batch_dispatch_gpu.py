"""GPU: every kernel family of the batch path at every workgroup shape, against digests recorded before the kernel choice
moved into csrc/nbody_batch_choice.h (tests/golden/batch_dispatch_digests.json, tests/golden/README.md says how).

The batch kernels are siblings instantiated for <rows per lane, guard>: 1, 2 or 4 rows per lane (capacities 64, 128 and 192
are the smallest with each) and the eps = 0 guard on or off.  A wrong case label in the dispatch would launch another
instantiation, which at these capacities either leaves rows unstepped or steps them with the other guard.  The kernels are
bitwise deterministic by construction, so the comparison is of SHA-256 digests: positions, velocities, counts, what evolve
reports, and the stops, mergers and fates where the family keeps them.

Two systems per case: one full, one five bodies short.  The full one carries an approaching pair (bodies 0 and n - 1), the
short one a body about to leave the escape radius (its last), so that the conditions of the families that have them find
something after a few steps: a stop, a merger, a tracer that hits, one that escapes.  Inputs come from integer hashes, not
from a random generator."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAPACITIES = (64, 128, 192)       # 1, 2 and 4 rows per lane
SOFTENINGS = (0.0, 0.01)          # guard on, guard off
STEP_FAMILIES = ("step", "step_massive", "hermite", "hermite_massive")
#: evolve families: (massive counts, collision radius, radii, collision action, tracer action)
EVOLVE_FAMILIES = {
    "adaptive": (False, 0.0, False, "stop", "refuse"),
    "stop": (False, 0.05, False, "stop", "refuse"),
    "merge": (False, 0.05, False, "merge", "refuse"),
    "radii": (False, 0.0, True, "stop", "refuse"),
    "radii_merge": (False, 0.0, True, "merge", "refuse"),       # the radii kernel again, with the merger buffers
    "adaptive_massive": (True, 0.0, False, "stop", "refuse"),
    "fate": (True, 0.05, False, "stop", "remove"),
    "fate_radii": (True, 0.0, True, "stop", "remove"),          # the fate kernel again, judging by radii
}
ESCAPE_RADIUS = 10.0
RADIUS = 0.02                     # per body: the close pair comes to touch, lattice neighbours (>= 0.15 apart) do not


def cases():
    out = []
    for cap in CAPACITIES:
        for eps in SOFTENINGS:
            for fam in STEP_FAMILIES:
                for integ in (("kick_drift", "kdk") if fam.startswith("step") else ("hermite",)):
                    out.append((fam, integ, cap, eps))
            for fam in EVOLVE_FAMILIES:
                out.append((fam, "hermite", cap, eps))
    return out


def case_id(case):
    fam, integ, cap, eps = case
    return f"{fam}-{integ}-{cap}-{'guard' if eps == 0.0 else 'soft'}"


def _hash01(i, salt):
    """[0, 1) from an integer hash (Knuth's multiplicative constant), exact in fp64."""
    i = np.asarray(i, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + np.uint64(salt) * np.uint64(40503)) % np.uint64(1 << 32)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(2246822519) % np.uint64(1 << 32)
    return h.astype(np.float64) / float(1 << 32)


def inputs(cap):
    """(pos, vel, counts): (2, cap, 4) float32.  Bodies on a 6 x 6 x 6 lattice of spacing 0.25, each moved by less than 0.05
    per axis (distinct positions, no pair closer than 0.15), masses 1 / n, small velocities, w = 7."""
    counts = np.array([cap, cap - 5], dtype=np.int64)
    pos = np.zeros((2, cap, 4), dtype=np.float32)
    vel = np.zeros((2, cap, 4), dtype=np.float32)
    for s, n in enumerate(counts):
        i = np.arange(n)
        cell = np.stack([i % 6, (i // 6) % 6, i // 36], axis=1).astype(np.float64)
        for c in range(3):
            pos[s, :n, c] = 0.25 * (cell[:, c] - 2.5) + 0.05 * _hash01(i, 10 * s + c)
            vel[s, :n, c] = 0.2 * (_hash01(i, 10 * s + 3 + c) - 0.5)
        pos[s, :n, 3] = 1.0 / n
        vel[s, :n, 3] = 7.0
    n0, n1 = counts
    # the close pair of the full system: 0.06 apart and closing at speed 1, within 0.05 after 0.01 and within 0.04 after 0.02
    pos[0, n0 - 1, :3] = pos[0, 0, :3] + np.array([0.06, 0.0, 0.0], dtype=np.float32)
    vel[0, n0 - 1, :3] = vel[0, 0, :3] - np.array([1.0, 0.0, 0.0], dtype=np.float32)
    # the far body of the short one: leaves ESCAPE_RADIUS after 0.005
    pos[1, n1 - 1, :3] = [ESCAPE_RADIUS - 0.01, 0.0, 0.0]
    vel[1, n1 - 1, :3] = [2.0, 0.0, 0.0]
    return pos, vel, counts


def run_case(case):
    """The SHA-256 digest of everything the case's run returns."""
    import n_body_problem_amd as nb
    fam, integ, cap, eps = case
    pos, vel, counts = inputs(cap)
    h = hashlib.sha256()

    def feed(*arrays):
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())

    with nb.BatchedSystem(2, cap, counts=counts, integrator=integ) as b:
        b.set_state(pos, vel)
        massive = counts // 2
        if fam in STEP_FAMILIES:
            if fam.endswith("massive"):
                b.set_massive_counts(massive)
            b.step_n(3, 1.0 / 256.0, eps)
        else:
            with_massive, rc, radii, action, tracers = EVOLVE_FAMILIES[fam]
            conditions = rc > 0.0 or radii
            if with_massive:
                b.set_massive_counts(massive)
            if conditions:
                b.set_stop_conditions(collision_radius=rc, escape_radius=ESCAPE_RADIUS)
                b.set_collision_action(action, log_capacity=4)
                b.set_tracer_action(tracers)
            if radii:
                b.set_radii(np.full((2, cap), RADIUS, dtype=np.float32))
            r = b.evolve(2, 1.0 / 64.0, levels=4, eta=0.01, eta_start=0.01, softening=eps)
            feed(r.steps, r.min_level, r.max_level, r.clamped, r.ticks)
            if conditions:
                st = b.stops()
                feed(st.reason, st.ticks, st.pair, st.separation, st.escaper)
            if action == "merge":
                m = b.mergers()
                feed(m.count, m.events)
            if radii:
                feed(b.radii())
            if tracers == "remove":
                f = b.fates()
                feed(f.fate, f.ticks, f.target, f.separation, f.relative_speed, f.hit, f.escaped)
        p, v = b.download()
        feed(p, v, b.counts)
    return h.hexdigest()


def run_diag(cap):
    """The diagnostics' three instantiations (energy with and without the guard, momentum), which share the batch's LDS layout."""
    import n_body_problem_amd as nb
    pos, vel, counts = inputs(cap)
    with nb.BatchedSystem(2, cap, counts=counts) as b:
        b.set_state(pos, vel)
        out = [b.energy(0.0), b.energy(0.01), b.momentum()]
    h = hashlib.sha256()
    for a in out:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record():
    """{case id: digest} of every case: what tests/golden/batch_dispatch_digests.json holds."""
    out = {case_id(c): run_case(c) for c in cases()}
    out.update({f"diag-{cap}": run_diag(cap) for cap in CAPACITIES})
    return out


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "batch_dispatch_digests.json")) as f:
        return json.load(f)["digests"]


def test_golden_covers_every_case(golden):
    assert sorted(golden) == sorted([case_id(c) for c in cases()] + [f"diag-{cap}" for cap in CAPACITIES])
    # the two step families under both of their integrators, the other eight (two of them twice), each at six <RPL, GUARD>
    assert len(cases()) == (2 * 2 + 2 + len(EVOLVE_FAMILIES)) * len(CAPACITIES) * len(SOFTENINGS) == 84
    assert len(set(golden.values())) == len(golden)   # no two cases ran alike: each guard and each shape shows


def test_conditions_find_something():
    """The inputs do what the module's docstring says: the families with conditions do not run as the plain ones."""
    import n_body_problem_amd as nb
    pos, vel, counts = inputs(64)
    with nb.BatchedSystem(2, 64, counts=counts, integrator="hermite") as b:
        b.set_state(pos, vel)
        b.set_stop_conditions(collision_radius=0.05, escape_radius=ESCAPE_RADIUS)
        b.evolve(2, 1.0 / 64.0, levels=4, softening=0.01)
        st = b.stops()
        assert st.reason.tolist() == [1, 2] and st.pair[0].tolist() == [0, 63] and st.escaper[1] == 58
        assert (st.ticks > 0).all() and (st.ticks < 32).all()      # after some steps, before the end
        b.set_massive_counts(counts // 2)
        b.set_tracer_action("remove")
        b.set_state(pos, vel)
        b.evolve(2, 1.0 / 64.0, levels=4, softening=0.01)
        f = b.fates()
        assert f.hit.tolist() == [1, 0] and f.escaped.tolist() == [0, 1] and not b.stops().stopped.any()
        b.set_massive_counts(None)
        b.set_tracer_action("refuse")
        b.set_collision_action("merge", log_capacity=4)
        b.set_state(pos, vel)
        b.evolve(2, 1.0 / 64.0, levels=4, softening=0.01)
        assert b.mergers().count.tolist() == [1, 0] and b.counts.tolist() == [63, 59]


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_family_and_shape(case, golden):
    assert run_case(case) == golden[case_id(case)]


@pytest.mark.parametrize("cap", CAPACITIES)
def test_diagnostics(cap, golden):
    assert run_diag(cap) == golden[f"diag-{cap}"]
