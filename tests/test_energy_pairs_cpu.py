"""CPU: the energy and momentum tests' own parts (tests/energy_pair_ref.py) -- the reference summed over all pairs against the
fp64 oracle, a numpy fp32 restatement of energy_tile held under the counted tolerance with the rsq moved by up to an ulp, the
probes and shapes of the cases against what they claim to reach, and the checks on emulated subtly wrong kernels.

Worst |fp32 restatement - ref| / tol over n = 805 and 549, eps = 1e-2 and 0, the rsq exact, moved up, down and at random:
0.892 (K 5.5); with softening lengths 0.772 (K 6)."""
import numpy as np
import pytest

import energy_pair_ref as er
import force_pair_ref as fp

SIZES = (805, 549)


def all_pairs(n):
    r, c = np.divmod(np.arange(n * n), n)
    keep = r != c
    return r[keep], c[keep]


@pytest.mark.parametrize("n", SIZES)
def test_reference_summed_over_all_pairs_is_the_oracle(oracle_mod, n):
    x = er.configuration(n)
    assert np.array_equal(x[fp.coincident_row(n)], x[fp.COINCIDENT]) and not x[er.origin_body(n)].any()
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = x
    pos[:, 3] = 1.0
    r, c = all_pairs(n)
    mine = -0.5 * er.pair_terms(x, r, c, er.EPS).sum() / (er.M_R * er.M_C)
    want = oracle_mod.energy(pos, np.zeros((n, 4), np.float32), float(np.float32(er.EPS)))[1]
    assert abs(mine - want) <= 1e-12 * abs(want)
    # nothing to soften the coincident pair: exactly nothing, with the lengths too (both of its bodies carry 0)
    k = int(np.flatnonzero((r == fp.COINCIDENT) & (c == fp.coincident_row(n)))[0])
    for eps_pp in (None, er.softening_lengths(n)):
        t = er.pair_terms(x, r, c, 0.0, eps_pp)
        assert np.isfinite(t).all() and t[k] == 0.0 and np.count_nonzero(t == 0.0) == 2
        assert er.pair_terms(x, r, c, er.EPS, eps_pp)[k] == pytest.approx(er.M_R * er.M_C / float(np.float32(er.EPS)), rel=1e-12)


@pytest.mark.parametrize("pps", [False, True], ids=["eps", "pps"])
def test_fp32_restatement_stays_under_the_counted_tolerance(pps):
    worst = 0.0
    rng = np.random.default_rng(7)
    for n in SIZES:
        x = er.configuration(n)
        e = er.softening_lengths(n) if pps else None
        r, c = all_pairs(n)
        for eps in (er.EPS, 0.0):
            ref = er.pair_terms(x, r, c, eps, e)
            tol = er.k_of(pps) * er.U * ref
            for wobble in (0, 1, -1, rng.integers(-1, 2, size=len(r))):
                got = er.numpy_term(x, r, c, eps, e, wobble)
                assert np.isfinite(got).all()
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.abs(got - ref) / tol
                ratio[(ref == 0.0) & (got == 0.0)] = 0.0          # the guarded pair: exactly nothing
                k = int(np.argmax(ratio))
                assert ratio[k] <= 1.0, (n, eps, int(r[k]), int(c[k]), got[k], ref[k], ratio[k])
                worst = max(worst, float(ratio[k]))
    print(f"energy pairs: fp32 restatement{' with softening lengths' if pps else ''}: worst ratio {worst:.3f} (K {er.k_of(pps)})")
    assert 0.05 < worst < 1.0


def test_the_count_is_the_sum_of_its_parts():
    """r2 carries 2 + 3 u (6 u with softening lengths), the rsq halves that and adds its own 2 u, the fma one more."""
    assert er.K_ENERGY == (2 + 3) / 2 + 2 + 1 and er.K_ENERGY_PPS == (3 + 3) / 2 + 2 + 1
    assert er.k_of(False) == er.K_ENERGY and er.k_of(True) == er.K_ENERGY_PPS


def test_probes_cover_what_they_claim():
    for case in er.CASES:
        n, lo, cnt = case["n"], case["row_lo"], case["row_count"]
        r, c = er.probes(case)
        edges = er.edge_bodies(case)
        pairs = set(zip(r.tolist(), c.tolist()))
        assert len(pairs) == len(r) and (r != c).all() and r.min(initial=0) >= 0 and max(r.max(initial=0), c.max(initial=0)) < n
        assert {(a, b) for a in edges for b in edges if a != b} <= pairs                       # the edge set is never thinned
        if n >= 1500:
            assert set(er.EDGES) | {n - 2, n - 1, er.origin_body(n), fp.COINCIDENT, fp.coincident_row(n)} <= set(edges)
            assert {lo, lo + cnt - 1} <= set(edges) and (lo == 0 or lo - 1 in edges) and (lo + cnt == n or lo + cnt in edges)
            assert len(r) == len(edges) * (len(edges) - 1) + er.HASHED_PAIRS <= 900
            # a shard's probes hold pairs with both bodies owned, one owned (each way) and none
            own = er.owned(r, lo, cnt) + 2 * er.owned(c, lo, cnt)
            assert set(own.tolist()) == ({3.0} if cnt == n else {0.0, 1.0, 2.0, 3.0}), case["name"]
        else:
            assert len(r) == n * (n - 1)
    assert [c["kernel"] for c in er.CASES[:4]] == ["energy_kernel<false, false>", "energy_kernel<false, true>",
                                                    "energy_kernel<true, false>", "energy_kernel<true, true>"]
    assert {c["kernel"] for c in er.CASES} == set(c["kernel"] for c in er.CASES[:4])


def test_shapes_reach_what_they_claim():
    by = {c["name"]: c for c in er.CASES}
    whole, a, b = by["whole_1500_soft"], by["shard_320_2600_soft"], by["shard_1920_2600_soft"]
    assert whole["row_count"] > er.ROWS_PER_WORKGROUP and whole["n"] % er.TILE != 0             # rows past 1024, a ragged last tile
    for s in (a, b):
        assert s["row_lo"] % s["split_len"] == 0 and s["row_lo"] % 64 == 0 and s["row_lo"] % er.TILE != 0
    assert a["row_count"] > er.ROWS_PER_WORKGROUP and a["row_lo"] + a["row_count"] < a["n"]
    assert b["row_lo"] + b["row_count"] == b["n"] and b["n"] % er.TILE != 0 and b["row_count"] % er.TILE != 0
    # a workgroup's 1024 rows from a start that is a multiple of 64 and not of 256 overlap five tiles
    lo = a["row_lo"]
    assert len({j // er.TILE for j in range(lo, lo + er.ROWS_PER_WORKGROUP)}) == 5
    assert {c["n"] for c in er.CASES} == {1500, 2600, 1, 2}


def test_kinetic_reference_and_inputs():
    for n in er.KINETIC_SIZES:
        mass, vel = er.kinetic_inputs(n)
        assert mass.dtype == vel.dtype == np.float32 and (vel[:, 3] == np.float32(er.FOURTH_WORD)).all()
        want, tol = er.expected_kinetic(mass, vel, 0, n)
        m, v = mass.astype(np.float64), vel[:, :3].astype(np.float64)
        assert want[0] == pytest.approx(0.5 * (m * (v ** 2).sum(1)).sum(), rel=1e-13) and want[4] == pytest.approx(m.sum(), rel=1e-13)
        assert np.allclose(want[1:4], (m[:, None] * v).sum(0), rtol=0, atol=1e-12)
        assert (tol > 0).all() and (tol < 1e-9).all() and np.isfinite(want).all()          # the fourth word did not enter
    mass, vel = er.kinetic_inputs(2600)
    part = er.expected_kinetic(mass, vel, 320, 1100)[0] + er.expected_kinetic(mass, vel, 1420, 1180)[0] + er.expected_kinetic(mass, vel, 0, 320)[0]
    assert np.allclose(part, er.expected_kinetic(mass, vel, 0, 2600)[0], rtol=1e-13, atol=1e-12)


# ---- subtly wrong kernels: each must leave the tolerance --------------------------------------------------------------------

def test_every_injected_fault_leaves_the_tolerance():
    case = next(c for c in er.CASES if c["name"] == "shard_320_2600_soft")
    n, lo, cnt = case["n"], case["row_lo"], case["row_count"]
    x = er.configuration(n)
    r, c = er.probes(case)
    want, tol = er.expected_potential(x, r, c, case["eps"], None, lo, cnt)
    t = er.numpy_term(x, r, c, case["eps"])
    own_r, own_c = er.owned(r, lo, cnt), er.owned(c, lo, cnt)
    good = -0.5 * (own_r + own_c) * t
    assert (np.abs(good - want) <= tol).all()
    neither = (own_r + own_c) == 0
    assert neither.any() and (want[neither] == 0.0).all() and (tol[neither] == 0.0).all()
    faults = {
        "the direction (c, r) dropped": -0.5 * own_r * t,
        "the direction (r, c) doubled": -0.5 * (2 * own_r + own_c) * t,
        "owned taken from 0 instead of row_lo": -0.5 * (er.owned(r, 0, cnt) + er.owned(c, 0, cnt)) * t,
        "one row more than row_count": -0.5 * (er.owned(r, lo, cnt + 1) + er.owned(c, lo, cnt + 1)) * t,
        "a self term leaks in": good - 0.5 * own_r * er.M_R ** 2 / er.EPS,
        "the softening left out": -0.5 * (own_r + own_c) * er.numpy_term(x, r, c, 0.0),
    }
    for name, got in faults.items():
        bad = np.abs(got - want) > tol
        assert bad.any(), name
        if name == "the softening left out":
            assert bad[(own_r + own_c) > 0].all(), name
    # one ulp of the fp32 term more than the count allows is seen on some entry, too: the tolerance is no loose one
    assert (np.abs(good * (1.0 + 8 * er.U) - want) > tol).any()
