"""GPU: bound pairs of batched ensembles (BatchedSystem.pairs, include/nbody_batch_pairs.h).  The partners, the fp64 records,
the mutual flags and the binaries agree with the fp64 reference (hermite_pairs_ref) at every workgroup shape and with ragged
counts; a known binary has its elements at three phases; massive counts restrict the candidates and the mass; a system's
records are the same bits wherever it runs; the call disturbs no evolve; records follow the counts after a merger; and the
errors are reported.

Capacities: 64 (one row per lane), 128 (two), 130 (four rows per lane, one wave), 257 (two waves: the cross-wave count of the
binaries), 4096 (sixteen waves, 128 KiB of LDS: the raised limit).  The inputs are hard binaries plus a few singles
(hermite_pairs_ref.binaries_and_singles); test_batch_pairs_cpu.py shows that the float32 search chooses the fp64 partner on
them, so that the agreement asked here is the kernel's to meet."""
import ctypes

import numpy as np
import pytest

import hermite_pairs_ref as pref

pytestmark = pytest.mark.gpu

#: the second branch of the partner check: eight fp32 ulps of the two terms v^2/2 and mu/r, rounded up
ENERGY_TIE = 2e-6
MASSIVE_N, MASSIVE_SEED, MASSIVE_COUNTS = 96, 77, [0, 1, 3, 96]


def all_inputs():
    """Every (name, P, V, counts, massive) the reference checks below run: the inputs condition of the CPU suite walks them."""
    for cap in pref.CAPACITIES:
        P, V, counts = pref.gpu_inputs(cap)
        yield f"capacity {cap}", P, V, counts, None
    P, V = pref.ragged(MASSIVE_N, [MASSIVE_N] * len(MASSIVE_COUNTS), MASSIVE_SEED)
    P[:], V[:] = P[0], V[0]                                   # the same system under every massive count
    yield "massive", P, V, [MASSIVE_N] * len(MASSIVE_COUNTS), MASSIVE_COUNTS


def run_pairs(P, V, counts, massive=None, capacity=None):
    import n_body_problem_amd as nb
    cap = capacity or P.shape[1]
    with nb.BatchedSystem(P.shape[0], cap, counts=counts) as b:
        b.set_state(P, V)
        if massive is not None:
            b.set_massive_counts(massive)
        return b.pairs()


def rel_err(got, want):
    """max |got - want| / |want| over the entries (0 where both are equal, infinities included)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = got == want
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(same, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(err, initial=0.0))


def check_against_reference(res, P, V, counts, massive=None):
    """The check of one batch against the reference, system by system; prints its figures."""
    cap = P.shape[1]
    for s, n in enumerate(counts):
        ms = None if massive is None else massive[s]
        ref = pref.pairs(P[s], V[s], n, ms)
        got = res.partner[s]
        same = got == ref["partner"]
        other = np.nonzero(~same)[0]
        for i in other:                                       # the second branch: an energy tie in fp32
            assert 0 <= got[i] < (n if ms is None else min(ms, n)) and got[i] != i and i < n, (s, i, got[i])
            eps, scale, valid = pref.pair_energies(P[s], V[s], n, ms, rows=[i])
            assert valid[0, got[i]], (s, i, got[i])
            assert eps[0, got[i]] - eps[0, ref["partner"][i]] <= ENERGY_TIE * scale[0, got[i]], (s, i, got[i], ref["partner"][i])
        print(f"system {s} (n = {n}): {len(other)} rows on the energy branch")
        assert len(other) <= 0.01 * n, (s, len(other))
        # records, given the same partner
        errs = {k: rel_err(getattr(res, k)[s][same], ref[k][same]) for k in pref.FIELDS}
        print(f"  records: " + ", ".join(f"{k} {v:.2g}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-9, (s, errs)
        # mutual where the row's partner and the partner's partner are the reference's
        settled = same & np.where(got >= 0, same[np.clip(got, 0, cap - 1)], True)
        assert np.array_equal(res.mutual[s][settled], ref["mutual"][settled]), s
        if same.all():
            assert res.binaries[s] == ref["binaries"], (s, res.binaries[s], ref["binaries"])
            rows = res.bound_pairs(s)
            assert rows.shape == (ref["binaries"], 5) and np.all(rows[:, 0] < rows[:, 1]) and np.all(rows[:, 4] < 0)
        # beyond the count: the empty record
        assert np.all(got[n:] == -1) and not res.mutual[s][n:].any(), s
        for k in pref.FIELDS:
            assert not getattr(res, k)[s][n:].any(), (s, k)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", list(pref.CAPACITIES))
def test_partners_records_mutual_flags_and_binaries_agree_with_the_reference(capacity):
    P, V, counts = pref.gpu_inputs(capacity)
    res = run_pairs(P, V, counts)
    assert res.partner.shape == (len(counts), capacity) and res.partner.dtype == np.int32 and res.mutual.dtype == bool
    assert res.binaries.shape == (len(counts),) and res.binaries.dtype == np.int64 and res.energy.dtype == np.float64
    check_against_reference(res, P, V, counts)
    big = int(np.argmax(counts))
    assert res.binaries[big] >= (counts[big] - counts[big] % 2 - 2 * (counts[big] // 20)) // 2   # every generated binary is found


# ---- 2. analytic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", list(pref.KNOWN_PHASES))
def test_a_known_binary_and_a_distant_single(phase):
    P, V, want = pref.known_binary(pref.KNOWN_PHASES[phase])
    res = run_pairs(P, V, [3], capacity=64)
    assert res.partner[0, :3].tolist() == [2, 0, 0] and res.mutual[0, :3].tolist() == [True, False, True]
    assert res.binaries[0] == 1
    rows = res.bound_pairs(0)
    assert rows.shape == (1, 5) and rows[0, 0] == 0 and rows[0, 1] == 2
    for i in (0, 2):
        got = (res.semi_major_axis[0, i], res.eccentricity[0, i], res.inclination[0, i], res.energy[0, i], res.separation[0, i])
        print(i, got, want)
        assert np.allclose(got, want, rtol=1e-6, atol=0), (i, got, want)
    assert np.allclose(rows[0, 2:], [want[0], want[1], want[3]], rtol=1e-6, atol=0)


# ---- 3. massive counts -------------------------------------------------------------------------------------------------------
def test_massive_counts_restrict_the_candidates_and_the_mass():
    name, P, V, counts, massive = list(all_inputs())[-1]
    assert name == "massive"
    res = run_pairs(P, V, counts, massive)
    check_against_reference(res, P, V, counts, massive)
    for s, m in enumerate(massive):
        assert np.all(res.partner[s] < m), s                   # every partner is a massive body (-1 < 0 at m = 0)
        assert not res.mutual[s, m:].any(), s                 # tracers are never mutual
    assert np.all(res.partner[0] == -1) and res.binaries[0] == 0          # m = 0: no candidate at all
    assert np.all(res.partner[1, 1:] == 0) and res.partner[1, 0] == -1   # m = 1: the one massive body has no candidate
    # mu follows the rule: a tracer's mass word changes nothing in its record, and nothing in anybody else's
    P2 = P.copy()
    P2[:, 3:, 3] *= 7.0
    res2 = run_pairs(P2, V, counts, massive)
    for s in (0, 1, 2):                                       # every body from 3 on is a tracer there
        assert np.array_equal(res.partner[s], res2.partner[s])
        for k in pref.FIELDS:
            assert np.array_equal(getattr(res, k)[s].view(np.uint64), getattr(res2, k)[s].view(np.uint64)), (s, k)
    assert not np.array_equal(res.energy[3], res2.energy[3])  # without tracers the masses count


# ---- 4. invariance ---------------------------------------------------------------------------------------------------------
def test_a_system_gives_the_same_bits_in_another_slot_batch_and_capacity():
    n = 60
    pos, vel = pref.binaries_and_singles(n, 4242)
    other = pref.binaries_and_singles(n, 4243)
    records = []
    for cap, B, slot in ((64, 1, 0), (64, 5, 3), (130, 2, 1), (257, 3, 2)):
        P, V = pref.ragged(cap, [n] * B, 5000)
        P[:, :n], V[:, :n] = other
        P[slot, :n], V[slot, :n] = pos, vel
        res = run_pairs(P, V, [n] * B)
        records.append((res.partner[slot, :n], res.mutual[slot, :n], res.binaries[slot]) +
                       tuple(getattr(res, k)[slot, :n].view(np.uint64) for k in pref.FIELDS))
    for r in records[1:]:
        for a, b in zip(records[0], r):
            assert np.array_equal(a, b)
    assert records[0][2] >= 20


# ---- 5. non-interference ---------------------------------------------------------------------------------------------------
def two_evolves(P, V, counts, between, stop=None):
    import n_body_problem_amd as nb
    with nb.BatchedSystem(P.shape[0], P.shape[1], counts=counts, integrator="hermite") as b:
        if stop:
            b.set_stop_conditions(**stop)
        b.set_state(P, V)
        b.evolve(2, 1.0 / 256.0, levels=8, softening=0.0)
        if between:
            b.pairs()
        r = b.evolve(2, 1.0 / 256.0, levels=8, softening=0.0)
        p, v = b.download()
        st = b.stops() if stop else None
        return p, v, r, st


@pytest.mark.parametrize("stop", [None, dict(collision_radius=0.02)], ids=["plain", "with a stop recorded"])
def test_evolve_pairs_evolve_is_the_two_evolves_alone_bit_for_bit(stop):
    counts = [40, 17, 64]
    P, V = pref.ragged(64, counts, 6100)
    pa, va, ra, sa = two_evolves(P, V, counts, False, stop)
    pb, vb, rb, sb = two_evolves(P, V, counts, True, stop)
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(ra.steps, rb.steps) and np.array_equal(ra.ticks, rb.ticks)
    if stop:
        assert sa.stopped.any()                                # the binaries come within 0.02 at pericentre: a stop is on record
        assert np.array_equal(sa.reason, sb.reason) and np.array_equal(sa.ticks, sb.ticks) and np.array_equal(sa.pair, sb.pair)


# ---- 6. after a merge --------------------------------------------------------------------------------------------------------
def test_after_a_merger_the_records_follow_the_lowered_counts():
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
        res = b.pairs()
        p, v = b.download()
    check_against_reference(res, p, v, live.tolist())


# ---- 7. errors -------------------------------------------------------------------------------------------------------------
def test_null_arguments_and_binaries_before_any_pairs_are_refused():
    import n_body_problem_amd as nb
    from n_body_problem_amd import _lib
    from n_body_problem_amd.system import _ptr
    with nb.BatchedSystem(2, 64) as b:
        lib, h = b._lib, b._h
        out = np.zeros(2, dtype=np.int64)
        i64 = out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        assert lib.nbody_batch_pairs_binaries(h, i64) == _lib.NBODY_ERR_STATE
        assert b"nbody_batch_pairs_binaries" in lib.nbody_batch_last_error(h)
        rec = (_lib.BatchPairRecord * (2 * 64))()
        for args in ((None, _ptr(b.velocities), rec), (_ptr(b.positions), None, rec), (_ptr(b.positions), _ptr(b.velocities), None)):
            assert lib.nbody_batch_pairs(h, *args) == _lib.NBODY_ERR_INVALID
            assert b"nbody_batch_pairs: NULL argument" in lib.nbody_batch_last_error(h)
        assert lib.nbody_batch_pairs_binaries(h, None) == _lib.NBODY_ERR_INVALID
        assert b"nbody_batch_pairs_binaries: NULL argument" in lib.nbody_batch_last_error(h)
        assert lib.nbody_batch_pairs_binaries(h, i64) == _lib.NBODY_ERR_STATE     # the refused calls were no calls
        b.pairs()
        assert lib.nbody_batch_pairs_binaries(h, i64) == _lib.NBODY_OK and not out.any()  # the zero state: coincident bodies
