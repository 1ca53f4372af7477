"""GPU: what a single-system step does behind its force pass, bit for bit (tests/finish_ref.py states the probe, the numpy
reference, what the bit test cannot distinguish and the table of cases; tests/test_finish_bits_cpu.py holds the reference to
the compiled FMA and ties each case to its finish kernels).

Per case and integrator: the expected states are built from acceleration probes of the context under test and numpy alone,
then the run itself starts from the same initial state -- one kick-drift step, or two kick-drift-kick steps (a whole context
through step(), a shard through the calls) -- and positions and velocities must match on their uint32 views after every step.
Mass words and fourth velocity words come back untouched, a shard's position rows outside its own too, the state is finite,
and some row differs in bits from the unfused fp32 `v + a dt`.  The fused and the unfused 5000-body cases must also give each
other's bits.  Entries compared and seconds are printed; profiles/finish_and_energy_pairs.txt records them."""
import time

import numpy as np
import pytest

import finish_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nb():
    import torch
    import n_body_problem_amd as nb
    assert torch.cuda.is_available(), "the gpu suite needs an MI355X"
    return nb


class Rig:
    """The contexts of one case (one, or two pair-once shards that exchange by copies) and its state on the device."""

    def __init__(self, nb, case):
        import torch
        self.torch, self.case = torch, case
        self.n, self.eps = case["n"], case["eps"]
        self.ctx = []
        for lo, cnt in fr.shards_of(case):
            s = nb.NBodySystem(self.n, row_lo=lo, row_count=cnt, split_len=case["split_len"])
            s.set_force_mode(case["mode"])
            if case["parts"]:
                s.set_summation_parts(case["parts"])
            assert s.split_len == case["split_len"]
            self.ctx.append(s)
        self.lo = self.ctx[0].row_lo
        self.rows = slice(self.lo, self.ctx[-1].row_lo + self.ctx[-1].row_count)       # every row some context owns
        self.pos0, self.vel0 = fr.inputs(case)
        self.still = np.zeros((self.n, 4), np.float32)
        self.still[:, 3] = fr.W_WORD
        self.probes = 0

    def close(self):
        for s in self.ctx:
            s.close()

    # -- state ------------------------------------------------------------------------------------------------------------------
    def set_state(self, x, vel4):
        """Positions x (n, 3) with the case's masses and velocities vel4 (n, 4) into every context; cached forces dropped."""
        p = self.pos0.copy()
        p[:, :3] = x
        for s in self.ctx:
            s.setParticlesPosition(p)
            s.setParticlesVelocity(vel4)
            s.invalidate_forces()

    def download(self):
        """(pos (n, 4) as the LAST context holds it, vel (rows, 4) of every owned row, [pos of each context])."""
        states = [s.download() for s in self.ctx]
        return states[-1][0], np.concatenate([v for _, v in states]), [p for p, _ in states]

    # -- the pieces of a step ---------------------------------------------------------------------------------------------------
    def forces(self):
        if len(self.ctx) == 1:
            self.ctx[0].forces(0, self.n, self.eps)
            return
        for s in self.ctx:                                # own columns first, then the rest, as the sharded host does
            s.forces(s.row_lo, s.row_count, self.eps)
            s.forces_complement(s.row_lo, s.row_count, self.eps)
            s.sym_reduce()
        for s in self.ctx:                                # the exchange of the column sums: every other context's groups
            for o in self.ctx:
                if o is not s:
                    lo, cnt, _ = o.sym_groups()
                    s.colparts[lo:lo + cnt].copy_(o.colparts[lo:lo + cnt])

    def exchange_positions(self):
        for s in self.ctx:
            for o in self.ctx:
                if o is not s:
                    s.positions[o.row_lo:o.row_lo + o.row_count].copy_(o.positions[o.row_lo:o.row_lo + o.row_count])

    def kick_drift_step(self, dt):
        if self.case["rig"] == "whole":
            self.ctx[0].step(dt, self.eps)
            return
        self.forces()
        for s in self.ctx:
            s.update(dt)

    def kdk_steps(self, dt, steps, after, exchanged):
        """`steps` kick-drift-kick steps; after(k) behind a shard's kick-drift (before the positions are exchanged) and behind
        every closing kick, exchanged() behind every exchange of positions."""
        if self.case["rig"] == "whole":
            for k in range(steps):
                self.ctx[0].step(dt, self.eps)
                after(k)
            return
        self.forces()
        for s in self.ctx:
            s.kdk_prepare()
        for k in range(steps):
            for s in self.ctx:
                s.kdk_kick_drift(dt)
            after(k)
            self.exchange_positions()
            exchanged()
            self.forces()
            for s in self.ctx:
                s.kdk_kick(dt)
            after(k)

    # -- the acceleration probe ---------------------------------------------------------------------------------------------------
    def probe(self, x):
        """The fp32 accelerations (rows, 3) of the owned rows at positions x, as this configuration sums them."""
        for s in self.ctx:
            s.set_integrator("kick_drift")
        self.set_state(x, self.still)
        self.kick_drift_step(1.0)
        _, vel, _ = self.download()
        assert (vel[:, 3] == fr.W_WORD).all()
        for s in self.ctx:
            s.invalidate_forces()
        self.probes += 1
        return vel[:, :3].copy()


RESULTS = {}


def run_case(nb, case):
    """{integrator: [(pos (n, 4), vel (rows, 4))] after every step}, every check of the case made on the way."""
    if case["name"] in RESULTS:
        return RESULTS[case["name"]]
    t0 = time.perf_counter()
    rig = Rig(nb, case)
    try:
        n, rows = case["n"], rig.rows
        x0, v0 = rig.pos0[:, :3].copy(), rig.vel0[rows, :3].copy()
        expected = {"kick_drift": fr.expected_kick_drift(rig.probe, x0, v0, fr.DT, rows),
                    "kdk": fr.expected_kdk(rig.probe, x0, v0, fr.DT, rows)}
        a0 = rig.probe(x0)
        assert np.isfinite(a0).all() and a0.any(axis=1).all()
        assert (fr.bits(fr.unfused_fp32(a0, fr.DT, v0)) != fr.bits(expected["kick_drift"][0][1])).any(axis=1).any(), \
            f"{case['name']}: no row tells the fp64 FMA from the unfused fp32 v + a dt"
        got, entries = {}, 0
        for integrator in fr.INTEGRATORS:
            for s in rig.ctx:
                s.set_integrator(integrator)
            rig.set_state(x0, rig.vel0)
            before = [s.download()[0] for s in rig.ctx]
            states = []

            def after(k, states=states, before=before, integrator=integrator):
                pos, vel, each = rig.download()
                for s, mine, was in zip(rig.ctx, each, before):       # a context moves its own rows' positions alone
                    outside = np.ones(n, bool)
                    outside[s.row_lo:s.row_lo + s.row_count] = False
                    assert np.array_equal(fr.bits(mine[outside]), fr.bits(was[outside])), \
                        f"{case['name']} {integrator} step {k}: a position row outside [{s.row_lo}, {s.row_lo + s.row_count}) changed"
                    was[:] = mine
                if len(rig.ctx) > 1:                                  # the whole state: each context's own rows
                    pos = pos.copy()
                    for s, mine in zip(rig.ctx, each):
                        pos[s.row_lo:s.row_lo + s.row_count] = mine[s.row_lo:s.row_lo + s.row_count]
                if len(states) == k + 1:
                    states[k] = (pos, vel)                            # a shard's second look at step k: behind the closing kick
                else:
                    states.append((pos, vel))

            if integrator == "kick_drift":
                rig.kick_drift_step(fr.DT)
                after(0)
            else:
                def exchanged(before=before):                         # the exchange wrote the other rows: take them as they are
                    for s, was in zip(rig.ctx, before):
                        was[:] = s.download()[0]

                rig.kdk_steps(fr.DT, fr.KDK_STEPS, after, exchanged)
            assert len(states) == len(expected[integrator])
            for k, ((pos, vel), (x, v)) in enumerate(zip(states, expected[integrator])):
                where = f"{case['name']} {integrator} step {k}"
                assert np.isfinite(pos).all() and np.isfinite(vel).all(), f"{where}: a state that is not finite"
                assert np.array_equal(fr.bits(pos[:, 3]), fr.bits(rig.pos0[:, 3])), f"{where}: a mass word changed"
                assert (vel[:, 3] == fr.W_WORD).all(), f"{where}: a fourth velocity word changed"
                own = pos[rows, :3]
                bad = np.argwhere(fr.bits(vel[:, :3]) != fr.bits(v))
                assert not len(bad), f"{where}: velocity of row {rows.start + bad[0][0]} word {bad[0][1]}: got " \
                    f"{vel[bad[0][0], bad[0][1]]!r} expected {v[bad[0][0], bad[0][1]]!r} ({len(bad)} words differ)"
                bad = np.argwhere(fr.bits(own) != fr.bits(x[rows]))
                assert not len(bad), f"{where}: position of row {rows.start + bad[0][0]} word {bad[0][1]}: got " \
                    f"{own[bad[0][0], bad[0][1]]!r} expected {x[rows][bad[0][0], bad[0][1]]!r} ({len(bad)} words differ)"
                outside = np.ones(n, bool)
                outside[rows] = False
                assert np.array_equal(fr.bits(pos[outside, :3]), fr.bits(x0[outside])), f"{where}: a row no context owns moved"
                entries += 6 * (rows.stop - rows.start)
            got[integrator] = states
        seconds = time.perf_counter() - t0
        print(f"finish bits {case['name']}: n {n} rows [{rows.start}, {rows.stop}) split {case['split_len']} parts {case['parts']}: " +
              "; ".join(f"{i}: {', '.join(case['kernels'][i])}" for i in fr.INTEGRATORS) +
              f"; {entries} words bit-equal, {rig.probes} probes, {seconds:.2f} s")
        RESULTS[case["name"]] = got
        return got
    finally:
        rig.close()


@pytest.mark.parametrize("case", fr.CASES, ids=[c["name"] for c in fr.CASES])
def test_every_finish_is_the_numpy_state_bit_for_bit(nb, case):
    run_case(nb, case)


def test_the_fused_and_the_unfused_finish_give_the_same_bits(nb):
    by_name = {c["name"]: c for c in fr.CASES}
    fused, unfused = (run_case(nb, by_name[k]) for k in fr.FUSED_AND_UNFUSED)
    for integrator in fr.INTEGRATORS:
        assert len(fused[integrator]) == len(unfused[integrator]) > 0
        for k, (a, b) in enumerate(zip(fused[integrator], unfused[integrator])):
            assert np.array_equal(fr.bits(a[0]), fr.bits(b[0])) and np.array_equal(fr.bits(a[1]), fr.bits(b[1])), (integrator, k)
