"""CPU: the pair-matrix tests' own parts (tests/pair_matrix_ref.py) -- the one-source reference against hermite_ref and the
fp64 oracle on two-body subsystems, the conditions on the inputs that the tolerance's derivation assumes and that make a
dropped, doubled or jerkless term show, an fp32 restatement of the loops held under the derived tolerance, and the checker
on emulated subtly wrong kernels.

Jerk resolved (|ref - jerkless| >= 8 tol in a component), share of the probed entries, both softenings alike to four digits:
1.0000 (64), 0.9999 (128), 0.9999 (192), 0.9998 (320), 0.9998 (1024), 0.9978 (4096, 64 sources); no row and no source column
without a resolved entry."""
import numpy as np
import pytest

import hermite_ref
import pair_matrix_ref as pm

EPS32 = float(np.float32(1e-2))


def two_body(x, v, c, i, m):
    pos = np.zeros((2, 4))
    vel = np.zeros((2, 4))
    pos[0, :3], pos[1, :3], pos[0, 3] = x[c], x[i], m
    vel[0, :3], vel[1, :3] = v[c, :3], v[i, :3]
    return pos, vel


SAMPLES = [(0, 1), (7, 61), (63, 0), (33, 34), (5, 59), (62, 63)]


@pytest.mark.parametrize("eps", [0.0, EPS32])
def test_reference_equals_hermite_ref_on_two_body_subsystems(eps):
    x, v = pm.configuration(64)
    m = pm.probe_mass(64)
    x1, v1 = pm.one_step("hermite", x, v, np.arange(64), m, pm.DT, eps)
    for c, i in SAMPLES:
        p, w = hermite_ref.step(*two_body(x, v, c, i, m), pm.DT, eps)
        assert np.abs(x1[c, i] - p[1, :3]).max() <= 1e-13 and np.abs(v1[c, i] - w[1, :3]).max() <= 1e-13, (c, i)
        assert np.abs(x1[c, c] - p[0, :3]).max() <= 1e-13 and np.abs(v1[c, c] - w[0, :3]).max() <= 1e-13, (c, "source")


@pytest.mark.parametrize("eps", [0.0, EPS32])
def test_reference_equals_the_fp64_oracle_on_two_body_subsystems(oracle_mod, eps):
    x, v = pm.configuration(64)
    m = pm.probe_mass(64)
    kd = pm.one_step("kick_drift", x, v, np.arange(64), m, pm.DT, eps)
    kdk = pm.one_step("kdk", x, v, np.arange(64), m, pm.DT, eps)
    h = pm.DT
    for c, i in SAMPLES:
        pos, vel = two_body(x, v, c, i, m)
        p, w = oracle_mod.step_f64(pos, vel, h, eps)
        assert np.abs(kd[0][c, i] - p[1, :3]).max() <= 1e-13 and np.abs(kd[1][c, i] - w[1, :3]).max() <= 1e-13, (c, i)
        assert np.abs(kd[0][c, c] - p[0, :3]).max() <= 1e-13 and np.abs(kd[1][c, c] - w[0, :3]).max() <= 1e-13, (c, "source")
        a0 = oracle_mod.accel_f64(pos, eps=eps)
        vh = vel[:, :3] + a0 * (h / 2)
        q = pos.copy()
        q[:, :3] += vh * h
        w1 = vh + oracle_mod.accel_f64(q, eps=eps) * (h / 2)
        assert np.abs(kdk[0][c, i] - q[1, :3]).max() <= 1e-13 and np.abs(kdk[1][c, i] - w1[1]).max() <= 1e-13, (c, i)
        assert np.abs(kdk[0][c, c] - q[0, :3]).max() <= 1e-13 and np.abs(kdk[1][c, c] - w1[0]).max() <= 1e-13, (c, "source")


def test_guard_and_null_system():
    x, v = pm.configuration(64)
    x = x.copy()
    v = v.copy()
    x[61], v[61] = x[7], v[7]                      # a coincident pair, moving together
    for scheme in pm.SCHEMES:
        for eps in pm.SOFTENINGS:
            ref = pm.stack(*pm.one_step(scheme, x, v, [7, -1], 1.0, pm.DT, eps))
            drift = pm.stack(*pm.one_step(scheme, x, v, [7, -1], 1.0, pm.DT, eps, variant="drift"))
            assert np.isfinite(ref).all()
            assert np.array_equal(ref[1], drift[1]) and np.array_equal(ref[0, 7], drift[0, 7])       # null, self pair
            assert np.array_equal(ref[0, 61], ref[0, 7])                                            # on top of the source
            assert np.abs(ref[0, 0] - drift[0, 0]).max() > 1e-3
    with pytest.raises(ValueError):
        pm.one_step("kdk", x, v, [7], 1.0, pm.DT, 0.0, variant="jerkless")


@pytest.mark.parametrize("capacity", pm.CAPACITIES_FULL + (pm.CAPACITY_LARGE,))
def test_configuration_and_probe_batch(capacity):
    x, v = pm.configuration(capacity)
    lo, hi = pm.separation_range(x)
    blo, bhi = pm.separation_bounds(capacity)
    assert 0.13 <= blo <= lo and hi <= bhi <= 6.1, (lo, hi, blo, bhi)
    speed = np.linalg.norm(v[:, :3].astype(np.float64), axis=1)
    assert 0.03 <= speed.min() and speed.max() <= 1.8 and 0.4 <= np.median(speed) <= 1.0, (speed.min(), speed.max())
    assert (v[:, 3] == 7.0).all()
    assert np.array_equal(pm.configuration(capacity)[0], x) and not np.array_equal(pm.configuration(capacity, 1)[0], x)
    lay = pm.Layout(capacity)
    massive = lay.counts // 2 + 1
    for mc in (None, massive):
        P, V = lay.batch(mc)
        assert P.shape == V.shape == (lay.num_systems, capacity, 4) and P.dtype == V.dtype == np.float32
        for s in range(lay.num_systems):
            n, c = lay.counts[s], lay.sources[s]
            want = np.zeros(n, np.float32)
            if c >= 0:
                want[c] = 1.0 if mc is not None and c >= mc[s] else pm.probe_mass(capacity)
            assert np.array_equal(P[s, :n, 3], want), s
            assert (V[s, :n, 3] == 7.0).all()
            assert (P[s, n:] == np.asarray(pm.FILL_POS, np.float32)).all() and (V[s, n:] == np.asarray(pm.FILL_VEL, np.float32)).all()
            if s in lay.coincident:
                assert c == 7 and np.array_equal(P[s, n - 3, :3], P[s, 7, :3]) and np.array_equal(V[s, n - 3, :3], V[s, 7, :3])
            else:
                assert np.array_equal(P[s, :n, :3], x[:n]) and np.array_equal(V[s, :n, :3], v[:n, :3])
        assert (lay.sources[lay.null_of] == -1).all() and (lay.counts[lay.null_of] == lay.counts).all()
    first, length, count = lay.blocks[1]
    assert count == capacity - 5 and lay.num_systems == first + length
    if capacity in pm.CAPACITIES_FULL:
        assert lay.num_systems == 2 * capacity - 5 + 4 and lay.all_sources() == list(range(capacity))
    else:
        want = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4094, 4095, 4089, 4090}
        assert want <= set(lay.all_sources()) and 56 <= len(lay.all_sources()) <= 72


def shape_sources(capacity):
    return None if capacity in pm.CAPACITIES_FULL else pm.Layout(capacity).all_sources()


@pytest.mark.parametrize("capacity", pm.CAPACITIES_FULL + (pm.CAPACITY_LARGE,))
def test_inputs_meet_the_derivation_and_every_term_shows(capacity):
    src = shape_sources(capacity)
    x_min, x_max, drift_share = pm.conditions(capacity)
    assert 0.5 <= x_min and x_max <= 4.5 and drift_share <= pm.DRIFT_SHARE, (x_min, x_max, drift_share)
    for scheme in pm.SCHEMES:
        for eps in pm.SOFTENINGS:
            R = pm.Reference(scheme, capacity, eps, src, jerkless=scheme == "hermite")
            p = R.probed()
            assert R.resolved(R.drift[None])[p].all(), (scheme, eps)         # a dropped term (and so a doubled one) shows
            if scheme == "hermite":
                r = R.resolved(R.jerkless) & p
                share = r.sum() / p.sum()
                print(f"capacity {capacity} eps {eps}: jerk resolved in {share:.4f} of {p.sum()} entries, "
                      f"K_term median {np.median(R.kt[p]):.0f} max {R.kt[p].max():.0f}")
                assert share >= pm.JERK_RESOLVED_SHARE, share
                assert r.any(0).all() and r.any(1).all()


@pytest.mark.parametrize("capacity", (64, 128, 192, 320, pm.CAPACITY_LARGE))
def test_a_correct_fp32_kernel_is_within_the_derived_tolerance(capacity):
    x, v = pm.configuration(capacity)
    src = np.arange(capacity) if capacity in pm.CAPACITIES_FULL else np.array(shape_sources(capacity))
    for scheme in pm.SCHEMES:
        for eps in pm.SOFTENINGS:
            R = pm.Reference(scheme, capacity, eps, src)
            ref, tol = R.rows(src, capacity)
            worst, fails = pm.check(pm.emulate_fp32(scheme, x, v, src, pm.probe_mass(capacity), pm.DT, eps), ref, tol, src)
            print(f"{scheme} capacity {capacity} eps {eps}: fp32 restatement worst ratio {worst:.3f}")
            assert not fails and worst <= 1.0, pm.describe(fails)


def test_k_term_is_the_derived_count():
    x, v = pm.configuration(64)
    m = pm.probe_mass(64)
    for scheme in pm.SCHEMES:
        x1, v1, d = pm.one_step(scheme, x, v, [3, -1], m, pm.DT, 0.0, detail=True)
        kt = pm.k_term(scheme, d, x1, v1, *pm.one_step(scheme, x, v, [-1], m, pm.DT, 0.0))
        assert kt.shape == (2, 64) and kt[0, 3] == 0.0 and not kt[1].any()          # the self pair, the null system
        rows = np.arange(64) != 3
        if scheme == "kick_drift":
            assert (kt[0, rows] == pm.K_A + 1.0).all()
            continue
        # a far row: little more than the operation count; the closest row pays for its conditioning
        r0 = np.linalg.norm(x.astype(np.float64) - x[3].astype(np.float64), axis=1)
        far, near = int(np.argmax(r0)), int(np.argmin(np.where(rows, r0, np.inf)))
        assert pm.K_A + 1.0 < kt[0, far] < 3.0 * pm.K_A + 0.2 * pm.K_J, (scheme, kt[0, far])
        assert kt[0, near] > 2.0 * kt[0, far] and np.isfinite(kt).all() and kt.max() * pm.U * 8.0 < 1.0
        if scheme == "kdk":                                   # the formula, by hand, at the far row
            h = d["h"]
            n0, n1 = np.linalg.norm(d["a0"][0, far]), np.linalg.norm(d["a1"][0, far])
            kc = 4 * np.sqrt(3.0) * d["big"][0, far] / d["r1"][0, far]
            amp = h * h * m / d["r1"][0, far] ** 3 * n0 / (n0 + n1)
            xd, vd = pm.one_step(scheme, x, v, [-1], m, pm.DT, 0.0)
            kappa = max(h / 2 * (n0 + n1) / np.linalg.norm(v1[0, far] - vd[0, far]),
                        h * h / 2 * n0 / np.linalg.norm(x1[0, far] - xd[0, far]))
            assert abs(kt[0, far] - (kappa * (pm.K_A * (1 + amp) + kc) + 2.0)) <= 1e-9 * kt[0, far]
    assert all(1.0 < pm.K_ROUND[s] <= 4 * 2.0 for s in pm.SCHEMES)


# ---- the checker on emulated subtly wrong kernels ------------------------------------------------------------------------

CAP = 64


@pytest.fixture(scope="module")
def hermite_case():
    x, v = pm.configuration(CAP)
    R = pm.Reference("hermite", CAP, 0.0, jerkless=True)
    src = np.concatenate([np.arange(CAP), [-1]])
    ref, tol = R.rows(src, CAP)
    got = ref.astype(np.float32).astype(np.float64)            # the reference's own output, as an fp32 kernel would return it
    return x, v, R, src, ref, tol, got


def reported(got, ref, tol, src):
    worst, fails = pm.check(got, ref, tol, src)
    return worst, [(f["system"], f["row"]) for f in fails], fails


def test_unaltered_output_passes(hermite_case):
    x, v, R, src, ref, tol, got = hermite_case
    worst, where, _ = reported(got, ref, tol, src)
    assert where == [] and worst <= 0.5 + 1e-9       # one rounding against K_round = 2
    assert pm.bitwise_mismatches(got[:CAP], got[CAP], src[:CAP]) == []


@pytest.mark.parametrize("s,i", [(1, 63), (62, 0), (31, 33), (17, 40)])
@pytest.mark.parametrize("fault", ["dropped", "doubled", "column_plus", "column_minus", "jerk_zeroed"])
def test_one_wrong_entry_is_reported_where_it_is(hermite_case, fault, s, i):
    x, v, R, src, ref, tol, got = hermite_case
    bad = got.copy()
    m = pm.probe_mass(CAP)
    if fault == "dropped":
        bad[s, i] = R.drift[i]
    elif fault == "doubled":
        bad[s, i] = pm.stack(*pm.one_step("hermite", x, v, [s], 2.0 * m, pm.DT, 0.0))[0, i]
    elif fault in ("column_plus", "column_minus"):
        c = s + 1 if fault == "column_plus" else s - 1
        assert 0 <= c < CAP and c != i
        bad[s, i] = ref[c, i]
    else:
        assert R.resolved(R.jerkless)[s, i]
        bad[s, i] = R.jerkless[s, i]
    bad = bad.astype(np.float32).astype(np.float64)
    worst, where, fails = reported(bad, ref, tol, src)
    assert set(where) == {(s, i)} and worst >= 8.0, (fault, where, worst)
    assert fails[0]["source"] == s and f"source column {s} row {i}" in pm.describe(fails)


def test_a_self_term_that_is_not_zero_is_reported(hermite_case):
    x, v, R, src, ref, tol, got = hermite_case
    bad = got.copy()
    bad[12, 12] = got[13, 12]                      # the source's own row moved as if a body at the next column pulled it
    worst, where, _ = reported(bad, ref, tol, src)
    assert set(where) == {(12, 12)}
    assert pm.bitwise_mismatches(bad[:CAP], bad[CAP], src[:CAP]) == [(12, 12)]
    bad = got.copy()
    bad[12, 12, 4] = np.nextafter(np.float32(bad[12, 12, 4]), np.float32(np.inf))     # one ulp: within tol, not bit for bit
    assert reported(bad, ref, tol, src)[1] == [] and pm.bitwise_mismatches(bad[:CAP], bad[CAP], src[:CAP]) == [(12, 12)]


def test_a_tracers_mass_word_that_acts_is_reported(hermite_case):
    x, v, R, src, ref, tol, got = hermite_case
    massive = CAP // 2 + 1
    acting = np.where(np.arange(CAP) >= massive, -1, np.arange(CAP))          # what the massive families must do
    want, wtol = R.rows(np.concatenate([acting, [-1]]), CAP)
    ok = want.astype(np.float32).astype(np.float64)
    assert reported(ok, want, wtol, src)[1] == []
    bad = ok.copy()
    c = 50                                                                     # a tracer's column whose mass word 1.0 acts
    bad[c] = pm.stack(*pm.one_step("hermite", x, v, [c], 1.0, pm.DT, 0.0))[0].astype(np.float32)
    worst, fails = pm.check(bad, want, wtol, src, limit=6 * CAP)
    assert {f["system"] for f in fails} == {c} and {f["row"] for f in fails} == set(range(CAP)) - {c}
    rows = pm.bitwise_mismatches(bad[:CAP], bad[CAP], acting, whole=acting < 0)
    assert {s for s, _ in rows} == {c} and len(rows) == CAP - 1


def test_single_terms_are_the_derivatives_they_claim():
    x, v = pm.configuration(64)
    src = np.arange(64)
    m = pm.probe_mass(64)
    for eps in pm.SOFTENINGS:
        t = pm.single_terms(64, src, eps)
        x1, v1 = pm.one_step("kick_drift", x, v, src, m, pm.DT, eps)
        assert np.abs((v1 - v[None, :, :3].astype(np.float64)) / pm.DT - t["acc"]).max() <= 1e-12
        xs = x.astype(np.float64)
        e2 = float(np.float32(eps)) ** 2
        r2 = ((xs[src][:, None] - xs[None]) ** 2).sum(-1) + e2
        off = ~np.eye(64, dtype=bool)
        assert np.abs(t["pot"][off] + m / np.sqrt(r2[off])).max() <= 1e-14 and (t["pot"][~off] == 0.0).all()
        d = 1e-5
        for b in range(3):
            step = np.zeros(3)
            step[b] = d
            ap = pm.acc_jerk(xs[None] + step, 0.0 * xs[None], xs[src][:, None], 0.0, m, e2)[0]
            am = pm.acc_jerk(xs[None] - step, 0.0 * xs[None], xs[src][:, None], 0.0, m, e2)[0]
            fd = (ap - am) / (2 * d)
            for a in range(3):
                k = [[0, 1, 2], [1, 3, 4], [2, 4, 5]][a][b]
                assert np.abs(fd[..., a] - t["tid"][..., k])[off].max() <= 1e-6 * np.abs(t["tid"][off]).max()
        assert (t["tol_tid"][off] > 0).all() and (t["tid"][~off] == 0.0).all()
