"""GPU: energy_kernel pair by pair, its kinetic half and momentum_kernel (tests/energy_pair_ref.py states the inputs, the fp64
reference, the counted tolerance and the table of cases; tests/test_energy_pairs_cpu.py holds the reference to the oracle and
the count to a wobbled numpy restatement).

One NBodySystem per case, the all-dark base state kept on the device; per probe two mass words are written, energy() is
read (a 16-byte read-back) and the two words are cleared.  Every probed pair must lie within K u of its fp64 term -- a pair
no row of which the context owns, a lone lit body at every edge row and the all-dark system give exactly 0.0, the coincident
pair its full softened term or, with nothing to soften it, exactly 0.0.  The worst |gpu - ref| / tol, the entries and the
seconds of every case are printed; profiles/finish_and_energy_pairs.txt records them."""
import time

import numpy as np
import pytest

import energy_pair_ref as er
import force_pair_ref as fp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nb():
    import torch
    import n_body_problem_amd as nb
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    return nb


def system(nb, case_or_n, row_lo=0, row_count=None, split_len=0):
    if isinstance(case_or_n, dict):
        c = case_or_n
        return nb.NBodySystem(c["n"], row_lo=c["row_lo"], row_count=c["row_count"], split_len=c["split_len"])
    return nb.NBodySystem(case_or_n, row_lo=row_lo, row_count=row_count, split_len=split_len)


@pytest.mark.parametrize("case", er.CASES, ids=[c["name"] for c in er.CASES])
def test_every_probed_pair_of_the_potential(nb, case):
    t0 = time.perf_counter()
    n, lo, cnt, eps = case["n"], case["row_lo"], case["row_count"], case["eps"]
    x = er.configuration(n)
    eps_pp = er.softening_lengths(n) if case["pps"] else None
    rows, cols = er.probes(case)
    want, tol = er.expected_potential(x, rows, cols, eps, eps_pp, lo, cnt)
    with system(nb, case) as s:
        if case["pps"]:
            s.set_particle_softening(eps_pp)
        dark = np.zeros((n, 4), np.float32)
        dark[:, :3] = x
        s.setParticlesPosition(dark)
        s.setParticlesVelocity(np.zeros((n, 4), np.float32))
        mass = s.positions[:, 3]
        e = s.energy(eps)
        assert e[1] == 0.0 and e[0] == 0.0 and np.isfinite(e).all(), f"{case['name']}: the all-dark system: {e!r}"
        lone = er.edge_bodies(case)
        for i in lone:                                          # a lone lit body: no self term
            mass[i] = er.M_R
            e = s.energy(eps)
            mass[i] = 0.0
            assert e[1] == 0.0 and e[0] == 0.0, f"{case['name']}: body {i} alone has the potential {e[1]!r}"
        got = np.empty(len(rows))
        for k, (r, c) in enumerate(zip(rows.tolist(), cols.tolist())):
            mass[r] = er.M_R
            mass[c] = er.M_C
            e = s.energy(eps)
            mass[r] = 0.0
            mass[c] = 0.0
            assert e[0] == 0.0 and e[2] == e[1], f"{case['name']}: pair ({r}, {c}): kinetic energy of bodies at rest: {e!r}"
            got[k] = e[1]
        assert not s.positions[:, 3].any().item()               # the base state is dark again
    assert np.isfinite(got).all(), f"{case['name']}: a potential that is not finite"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.abs(got - want) / tol
    ratio[(got == want) & (tol == 0.0)] = 0.0                   # entries that are exactly their reference: nothing owned, the guard
    worst = float(ratio.max()) if len(ratio) else 0.0
    special = ""
    if er.has_coincident_pair(n):
        k = int(np.flatnonzero((rows == fp.COINCIDENT) & (cols == fp.coincident_row(n)))[0])
        softened = eps > 0                                      # both of its bodies carry the softening length 0
        assert (want[k] != 0.0) == (softened and er.owned(fp.COINCIDENT, lo, cnt) + er.owned(fp.coincident_row(n), lo, cnt) > 0)
        if not softened:
            assert got[k] == 0.0, f"{case['name']}: the coincident pair with nothing to soften it: {got[k]!r}"
        special = f", the coincident pair {got[k]!r} (ref {want[k]!r})"
    seconds = time.perf_counter() - t0
    print(f"energy pairs {case['name']}: {case['kernel']} n {n} rows [{lo}, {lo + cnt}): {len(rows)} pairs, {len(lone)} lone bodies and "
          f"the dark system: worst |gpu - ref| / tol {worst:.3f} (K {er.k_of(case['pps'])}){special}; {seconds:.2f} s")
    bad = np.argsort(-ratio)[:8]
    assert worst <= 1.0, "; ".join(f"{case['name']}: pair ({rows[k]}, {cols[k]}): got {got[k]!r} ref {want[k]!r} tol {tol[k]:.3g} "
                                   f"(x{ratio[k]:.3g})" for k in bad if ratio[k] > 1.0)


def kinetic_contexts():
    """(name, n, row_lo, row_count, split_len): the contexts of the potential's cases and the whole contexts of KINETIC_SIZES."""
    seen, out = set(), []
    for c in er.CASES:
        key = (c["n"], c["row_lo"], c["row_count"], c["split_len"])
        if key not in seen:
            seen.add(key)
            out.append((c["name"].rsplit("_", 1)[0].replace("_soft", "").replace("_guard", ""),) + key)
    return out + [(f"whole_{n}", n, 0, n, 0) for n in er.KINETIC_SIZES if (n, 0, n, 0) not in seen]


@pytest.mark.parametrize("ctx", kinetic_contexts(), ids=[c[0] for c in kinetic_contexts()])
def test_kinetic_energy_and_momentum_of_the_owned_rows(nb, ctx):
    t0 = time.perf_counter()
    name, n, lo, cnt, L = ctx
    mass, vel = er.kinetic_inputs(n)
    want, tol = er.expected_kinetic(mass, vel, lo, cnt)
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = er.configuration(n)
    pos[:, 3] = mass
    with system(nb, n, lo, cnt, L) as s:
        s.setParticlesPosition(pos)
        s.setParticlesVelocity(vel)
        e = s.energy(er.EPS)
        p = s.momentum()
    got = np.concatenate([e[:1], p])
    assert np.isfinite(e).all() and np.isfinite(p).all() and e[2] == e[0] + e[1] and (e[1] < 0.0 or n == 1)
    ratio = np.abs(got - want) / tol
    print(f"kinetic energy and momentum {name}: n {n} rows [{lo}, {lo + cnt}): |gpu - ref| / tol kinetic {ratio[0]:.3f}, "
          f"momentum {ratio[1]:.3f} {ratio[2]:.3f} {ratio[3]:.3f}, mass {ratio[4]:.3f}; {time.perf_counter() - t0:.2f} s")
    for k, what in enumerate(("kinetic energy", "px", "py", "pz", "mass")):
        assert ratio[k] <= 1.0, f"{name}: {what}: got {got[k]!r} ref {want[k]!r} tol {tol[k]:.3g} (x{ratio[k]:.3g})"
