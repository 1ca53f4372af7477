"""CPU-only: pins the oracle (oracle/nbody_oracle.c) with analytic known answers and the committed
fixtures.  The reference has no tests or golden vectors for this path, so these
known answers are what stands between the restatement and a typo."""
import glob
import os

import numpy as np
import pytest

from conftest import rel_state_error


def two_bodies(d=1.0, m0=1.0, m1=1.0):
    pos = np.array([[0, 0, 0, m0], [d, 0, 0, m1]], dtype=np.float32)
    vel = np.zeros((2, 4), dtype=np.float32)
    return pos, vel


def test_unit_pair_known_answer(oracle_mod):
    # unit masses at distance 1 -> |a| = (1+eps^2)^(-3/2), pointing at the other body
    for eps in (0.0, 1e-3, 1e-2, 0.5):
        pos, _ = two_bodies()
        a = oracle_mod.accel_f32(pos, eps=eps, threads=1)
        want = (1.0 + eps * eps) ** -1.5
        assert a[0, 0] == pytest.approx(want, rel=3e-7) and a[1, 0] == pytest.approx(-want, rel=3e-7)
        assert np.all(a[:, 1:] == 0)
        a64 = oracle_mod.accel_f64(pos, eps=eps, threads=1)
        assert a64[0, 0] == pytest.approx(want, rel=1e-14)


def test_mass_weighting_and_newton_third_law(oracle_mod):
    pos, _ = two_bodies(d=2.0, m0=3.0, m1=5.0)
    a = oracle_mod.accel_f64(pos, eps=0.0, threads=1)
    assert a[0, 0] == pytest.approx(5.0 / 4.0) and a[1, 0] == pytest.approx(-3.0 / 4.0)
    # m0*a0 + m1*a1 = 0
    assert 3.0 * a[0, 0] + 5.0 * a[1, 0] == pytest.approx(0.0, abs=1e-15)


def test_coincident_and_self_pairs_contribute_zero(oracle_mod):
    pos = np.array([[0.5, 0.5, 0.5, 1.0], [0.5, 0.5, 0.5, 2.0]], dtype=np.float32)
    for eps in (0.0, 1e-3):
        assert np.all(oracle_mod.accel_f32(pos, eps=eps, threads=1) == 0)
        assert np.all(oracle_mod.accel_f64(pos, eps=eps, threads=1) == 0)


def test_zero_mass_padding_changes_nothing(oracle_mod):
    # the reference pads to roundup(n,256)+1 with zero-mass bodies at the origin (kernel.cu:260-278)
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.uniform_cube(100, seed=3)
    ppos, pvel = ic.pad_reference_style(pos, vel)
    assert ppos.shape[0] == 257 == ic.padded_count(100)
    a = oracle_mod.accel_f32(pos, eps=1e-3, threads=1)
    ap = oracle_mod.accel_f32(ppos, eps=1e-3, threads=1)
    assert np.array_equal(a, ap[:100])
    p1, v1 = oracle_mod.step_f32(pos, vel, 1e-3, 1e-3, nsteps=3, threads=1)
    p2, v2 = oracle_mod.step_f32(ppos, pvel, 1e-3, 1e-3, nsteps=3, threads=1)
    assert np.array_equal(p1, p2[:100]) and np.array_equal(v1, v2[:100])


def test_reference_pair_functions_match_general_form(oracle_mod):
    # VERSION 3's pair function (0.1 pre-scale, EPSILON=1e-6) is the general form with eps = 1e-2;
    # VERSION 1's (sqrtf + divide) is the general form with eps = 1e-3.
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = rng.uniform(-1, 1, 4).astype(np.float32)
        b = rng.uniform(-1, 1, 4).astype(np.float32)
        b[3] = abs(b[3]) + 0.1
        pos = np.stack([a, b])
        f3 = oracle_mod.pair_v3(a, b) * b[3]
        g3 = oracle_mod.accel_f64(pos, 0, 1, eps=1e-2, threads=1)[0]
        assert np.allclose(f3, g3, rtol=2e-6, atol=1e-9)
        f1 = oracle_mod.pair_v1(a, b)
        g1 = oracle_mod.accel_f64(pos, 0, 1, eps=1e-3, threads=1)[0]
        assert np.allclose(f1, g1, rtol=2e-6, atol=1e-9)


def test_version3_step_matches_general_step_with_reference_constants(oracle_mod):
    # the parity target: reference VERSION 3 (pair-once, +/- application, dt=0.008) vs step(dt=0.008, eps=1e-2)
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(300, seed=9)
    ppos, pvel = ic.pad_reference_style(pos, vel)
    p3, v3 = oracle_mod.step_v3(ppos, pvel, nsteps=5)
    pg, vg = oracle_mod.step_f32(pos, vel, 0.008, 1e-2, nsteps=5, threads=1)
    assert rel_state_error(p3[:300], pg) < 2e-6
    assert rel_state_error(v3[:300], vg) < 2e-6
    pt, vt = oracle_mod.step_v3_tiled(ppos, pvel, nsteps=5)       # the same step in the reference's own summation order
    assert rel_state_error(pt[:300], pg) < 2e-6 and rel_state_error(vt[:300], vg) < 2e-6
    # and VERSION 2 (Gauss-Seidel, in place) is NOT the same step
    p2, _ = oracle_mod.step_v2_serial(pos, vel, nsteps=5)
    pg1, _ = oracle_mod.step_f32(pos, vel, 0.008, 1e-3, nsteps=5, threads=1)
    assert rel_state_error(p2, pg1) > 1e-7


def test_update_is_kick_then_drift_with_new_velocity(oracle_mod):
    pos = np.array([[1, 2, 3, 1]], dtype=np.float32)
    vel = np.array([[0.5, 0, -1, 7]], dtype=np.float32)
    acc = np.array([[2, 4, 8]], dtype=np.float32)
    oracle_mod.update_f32(pos, vel, acc, 0.25)
    assert np.allclose(vel[0], [1.0, 1.0, 1.0, 7.0])           # v + a*dt ; .w untouched
    assert np.allclose(pos[0], [1.25, 2.25, 3.25, 1.0])        # x + v_new*dt ; mass untouched


def test_f32_path_tracks_f64_truth(oracle_mod):
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(2048, seed=21)
    a32 = oracle_mod.accel_f32(pos, eps=1e-3)
    a64 = oracle_mod.accel_f64(pos, eps=1e-3)
    err = np.linalg.norm(a32 - a64) / np.linalg.norm(a64)
    assert err < 1e-6
    p32, v32 = oracle_mod.step_f32(pos, vel, 1e-3, 1e-3, nsteps=10)
    p64, v64 = oracle_mod.step_f64(pos, vel, 1e-3, 1e-3, nsteps=10)
    assert rel_state_error(p32, p64) < 1e-6 and rel_state_error(v32, v64) < 1e-5


def test_threads_do_not_change_results(oracle_mod):
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(777, seed=2)
    a1 = oracle_mod.accel_f32(pos, eps=1e-3, threads=1)
    a8 = oracle_mod.accel_f32(pos, eps=1e-3, threads=8)
    assert np.array_equal(a1, a8)
    # column ranges add up to the whole (fp64, order-insensitive to 1e-13)
    a = oracle_mod.accel_f64(pos, eps=1e-3)
    b = oracle_mod.accel_f64(pos, j0=0, j1=300, eps=1e-3) + oracle_mod.accel_f64(pos, j0=300, j1=777, eps=1e-3)
    assert np.allclose(a, b, rtol=1e-12, atol=1e-15)


def test_momentum_and_energy_conservation(oracle_mod):
    # BASELINE.json configs[0]: N=1024, softening=1e-3, dt=1e-3, 100 leapfrog steps, scalar CPU path
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(1024, seed=ic.CONFIG_SEED[1])
    e0 = oracle_mod.energy(pos, vel, 1e-3)
    m0 = oracle_mod.momentum(pos, vel)
    p, v = oracle_mod.step_f32(pos, vel, 1e-3, 1e-3, nsteps=100)
    e1 = oracle_mod.energy(p, v, 1e-3)
    m1 = oracle_mod.momentum(p, v)
    assert abs(e1[2] - e0[2]) / abs(e0[2]) < 2e-4     # symplectic Euler: bounded drift
    assert np.abs(m1[:3] - m0[:3]).max() < 1e-6        # sum m a = 0 up to fp32 rounding
    assert e0[0] / abs(e0[1]) == pytest.approx(0.5, abs=0.05)   # virial equilibrium of the Plummer model


def test_energy_known_answer(oracle_mod):
    pos, vel = two_bodies(d=2.0, m0=3.0, m1=5.0)
    vel[0, :3] = [1, 0, 0]
    e = oracle_mod.energy(pos, vel, 0.0)
    assert e[0] == pytest.approx(1.5) and e[1] == pytest.approx(-7.5) and e[2] == pytest.approx(-6.0)


def test_golden_fixtures_reproduce(oracle_mod, golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "f1_*.npz")))
    assert len(files) >= 4
    for f in files:
        g = np.load(f)
        dt, eps = float(g["dt"]), float(g["softening"])
        for k in g["steps"]:
            if k > 10 and g["pos0"].shape[0] > 300:
                continue  # keep the CPU suite short; K=100 at n=1024 is covered by the conservation test
            p, v = oracle_mod.step_f32(g["pos0"], g["vel0"], dt, eps, nsteps=int(k), threads=1)
            assert np.array_equal(p, g[f"p32_{k}"]) and np.array_equal(v, g[f"v32_{k}"]), (f, k)
            assert rel_state_error(p, g[f"p64_{k}"]) < (1e-6 if k <= 10 else 1e-5)


def test_kdk_is_second_order_and_time_reversible(oracle_mod):
    """Velocity Verlet: energy error falls 4x when dt halves (kick-drift: 2x), and stepping
    forward then backward returns to the start to rounding."""
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(512, seed=17)
    e0 = oracle_mod.energy(pos, vel, 5e-2)[2]

    def err(stepper, dt, nsteps):
        p, v = stepper(pos, vel, dt, 5e-2, nsteps=nsteps)
        return abs(oracle_mod.energy(p, v, 5e-2)[2] - e0) / abs(e0)

    k1, k2 = err(oracle_mod.step_kdk_f32, 2e-2, 50), err(oracle_mod.step_kdk_f32, 1e-2, 100)
    d1, d2 = err(oracle_mod.step_f32, 2e-2, 50), err(oracle_mod.step_f32, 1e-2, 100)
    assert k1 < d1 and k2 < d2                      # better than kick-drift at the same dt
    assert 2.5 < k1 / k2 < 6.0                      # ~ dt^2
    p, v = oracle_mod.step_kdk_f32(pos, vel, 1e-2, 5e-2, nsteps=20)
    v[:, :3] *= -1
    p, v = oracle_mod.step_kdk_f32(p, v, 1e-2, 5e-2, nsteps=20)
    assert rel_state_error(p, pos) < 1e-5


def test_per_particle_softening_oracle_known_answers(oracle_mod):
    """eps_ij^2 = eps^2 + eps_i^2 + eps_j^2: two unit masses at distance 1 with lengths 0.3 and 0.4 and eps = 0 feel
    1/(1 + 0.25)^1.5; equal lengths e are a global softening of sqrt(eps^2 + 2 e^2)."""
    pos = np.array([[0, 0, 0, 1], [1, 0, 0, 1]], dtype=np.float64)
    a = oracle_mod.accel_f64_pps(pos, [0.3, 0.4], 0.0)
    assert np.allclose(a[0], [1.25 ** -1.5, 0, 0], rtol=1e-14) and np.allclose(a[1], -a[0])
    assert np.isclose(oracle_mod.potential_pps(pos, [0.3, 0.4], 0.0), -1.25 ** -0.5, rtol=1e-14)
    rng = np.random.default_rng(8)
    p = rng.normal(size=(200, 4))
    p[:, 3] = rng.uniform(0.5, 1.5, 200)
    e = 0.02
    want = oracle_mod.accel_f64(p, eps=np.sqrt(1e-3 ** 2 + 2 * e * e), threads=1)
    assert np.allclose(oracle_mod.accel_f64_pps(p, np.full(200, e), 1e-3), want, rtol=1e-12, atol=1e-14)
    # an unsoftened coincident pair contributes nothing, as in pair_f64
    p[1, :3] = p[0, :3]
    assert np.isfinite(oracle_mod.accel_f64_pps(p, np.zeros(200), 0.0)).all()


# ---- VERSION 3 in the reference's own tile order (oracle_step_v3_tiled) ----------------------------------------------------

TOL = 1e-5          # the suite's stated tolerance (BASELINE.json configs; tests/test_parity_gpu.py)


def test_v3_tiled_visits_cover_every_pair_exactly_once(oracle_mod):
    """kernel.cu:640-661, 717-718, 738-743, 761: over all blocks, the visits are the pairs x < y of 0..n-1, each once, and
    nothing else; a block's visits come in the order the numpy restatement walks (step by step, thread by thread)."""
    import v3_tiled_ref as ref
    for k in (1, 2, 3, 5):
        n = 256 * k + 1
        blocks = oracle_mod.v3_tiled_blocks(n)
        assert blocks == k * (k + 1) // 2
        per_block = [oracle_mod.v3_tiled_visits(n, b) for b in range(blocks)]
        for b in {0, 1 % blocks, blocks - 1}:
            assert np.array_equal(per_block[b], ref.visits(n, b)), (n, b)
        diagonal = sum(len(v) == 256 * 257 // 2 for v in per_block)
        assert diagonal == k and all(len(v) in (256 * 257 // 2, 65536) for v in per_block)
        v = np.concatenate(per_block).astype(np.int64)
        row, col = v[:, 0], v[:, 1]
        assert row.min() == 0 and row.max() == n - 2 and col.min() == 1 and col.max() == n - 1
        assert np.all(row < col)
        key = np.sort(row * n + col)
        x, y = np.triu_indices(n, 1)
        assert len(key) == n * (n - 1) // 2 and np.array_equal(key, x.astype(np.int64) * n + y)
        with pytest.raises(ValueError):
            oracle_mod.v3_tiled_visits(n, blocks)
        with pytest.raises(ValueError):
            oracle_mod.v3_tiled_visits(n, -1)


def test_v3_tiled_block_counts(oracle_mod):
    for h in (0, 1, 2, 7, 32, 79, 172):
        assert oracle_mod.v3_tiled_blocks(256 * h + 1) == h * (h + 1) // 2
    assert oracle_mod.v3_tiled_blocks(20225) == 3160       # what the reference prints for galaxy_20K.bin (kernel.cu:1229)
    assert oracle_mod.v3_tiled_blocks(44033) == 14878      # stars.dat whole


def test_v3_tiled_refuses_other_body_counts(oracle_mod):
    for n in (2, 255, 256, 258, 512, 1000, 20224):
        state = np.zeros((n, 4), np.float32)
        for call in (lambda: oracle_mod.accel_v3_tiled(state), lambda: oracle_mod.step_v3_tiled(state, state),
                     lambda: oracle_mod.v3_tiled_blocks(n), lambda: oracle_mod.v3_tiled_visits(n, 0)):
            with pytest.raises(ValueError, match="256 k"):
                call()
    with pytest.raises(ValueError, match="256 k"):
        oracle_mod.accel_v3_tiled(np.zeros((0, 4), np.float32))
    # n = 1: no block, no pair, no acceleration; a step is the drift alone
    pos = np.array([[1, 2, 3, 5]], np.float32)
    vel = np.array([[0.5, 0, -1, 7]], np.float32)
    assert oracle_mod.v3_tiled_blocks(1) == 0 and np.all(oracle_mod.accel_v3_tiled(pos) == 0)
    p, v = oracle_mod.step_v3_tiled(pos, np.zeros_like(vel), nsteps=3)
    assert np.array_equal(p, pos) and np.all(v == 0)
    p, v = oracle_mod.step_v3_tiled(pos, vel, nsteps=1)
    import finish_ref
    assert np.array_equal(v, vel) and np.array_equal(p[:, :3], finish_ref.drift(vel[:, :3], 0.008, pos[:, :3])) and p[0, 3] == 5


@pytest.mark.parametrize("n", [257, 513, 769])
def test_v3_tiled_equals_the_numpy_restatement_bit_for_bit_and_sees_every_wrong_order(oracle_mod, n):
    """One diagonal block; two diagonal blocks and an off-diagonal one; three and three.  The C pass against
    tests/v3_tiled_ref.py, every bit; and each way of getting the order wrong changes at least one."""
    import v3_tiled_ref as ref
    pos = ref.inputs(n)
    assert len(np.unique(pos[:, 3])) == 4 and np.all(pos[-37:, 3] == 0)
    got = oracle_mod.accel_v3_tiled(pos, threads=1)
    assert np.all(np.isfinite(got)) and np.abs(got).max() > 1
    assert np.array_equal(got.view(np.uint32), ref.accel(pos).view(np.uint32))
    for flags in ref.MUTATIONS:
        wrong = ref.accel(pos, **flags)
        seen = not np.array_equal(got.view(np.uint32), wrong.view(np.uint32))
        # one block adding to accelerations that are all +0 commutes: columns_first has nothing to change at n = 257
        assert seen == (not (n == 257 and "columns_first" in flags)), flags
    # a frame is that pass and the shared update
    vel = np.zeros_like(pos)
    vel[:, :3] = 0.1 * (pos[:, :3] - 2.5)
    import finish_ref
    p, v = oracle_mod.step_v3_tiled(pos, vel, nsteps=1, threads=1)
    want_v = finish_ref.kick(got, 0.008, vel[:, :3])              # TIME_TICK, the double literal (kernel.cu:63)
    want_p = finish_ref.drift(want_v, 0.008, pos[:, :3])
    assert np.array_equal(v[:, :3], want_v) and np.array_equal(p[:, :3], want_p)
    assert np.array_equal(p[:, 3], pos[:, 3]) and np.array_equal(v[:, 3], vel[:, 3])


def test_v3_threads_do_not_change_results(oracle_mod):
    """Blocks are summed in parallel and added serially in block order, 256 blocks at a time: 1, 3, 8 and 16 threads give
    the same bits, also across a batch boundary (n = 5889: 276 blocks); and the single chain walked body by body on several
    threads equals the pair-once walk of one thread."""
    import v3_tiled_ref as ref
    for n, nsteps in ((769, 3), (5889, 1)):
        pos = ref.inputs(n, seed=1)
        vel = np.zeros_like(pos)
        vel[:, :3] = 0.05 * (pos[:, :3] - 2.5)
        a1 = oracle_mod.accel_v3_tiled(pos, threads=1)
        s1 = oracle_mod.step_v3_tiled(pos, vel, nsteps=nsteps, threads=1)
        for threads in (3, 8, 16):
            assert np.array_equal(a1, oracle_mod.accel_v3_tiled(pos, threads=threads))
            s = oracle_mod.step_v3_tiled(pos, vel, nsteps=nsteps, threads=threads)
            assert np.array_equal(s1[0], s[0]) and np.array_equal(s1[1], s[1])
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.pad_reference_style(*ic.plummer(777, seed=2))
    c1 = oracle_mod.step_v3(pos, vel, nsteps=3, threads=1)
    for threads in (2, 8, 16):
        c = oracle_mod.step_v3(pos, vel, nsteps=3, threads=threads)
        assert np.array_equal(c1[0], c[0]) and np.array_equal(c1[1], c[1])


def test_v3_tiled_zero_mass_padding_changes_no_real_bodys_bits(oracle_mod):
    """The chain oracle's padding test allows a real body no changed bit, and the same holds in tile order: a block's row sum
    over zero-mass columns is fmaf(f, 0, +0) = +0 whatever f's sign (a row never sees a column twice, so it stays +0), and
    x + (+0) = x for every x but -0.  400 real bodies padded to 513 and to 769: the real bodies' accelerations, and their
    states after five frames (the padding bodies move, but carry no mass), are the same bits."""
    from n_body_problem_amd import initial_conditions as ic
    pos, vel = ic.plummer(400, seed=11)

    def padded(n):
        p, v = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        p[:400], v[:400] = pos, vel
        return p, v

    (p2, v2), (p3, v3) = padded(513), padded(769)
    assert np.array_equal(p2, ic.pad_reference_style(pos, vel)[0])            # 513 is the reference's own padding of 400
    a2, a3 = oracle_mod.accel_v3_tiled(p2), oracle_mod.accel_v3_tiled(p3)
    assert np.all(a2[:400] != 0) and np.array_equal(a2[:400], a3[:400])
    s2, s3 = oracle_mod.step_v3_tiled(p2, v2, nsteps=5), oracle_mod.step_v3_tiled(p3, v3, nsteps=5)
    assert np.array_equal(s2[0][:400], s3[0][:400]) and np.array_equal(s2[1][:400], s3[1][:400])
    assert np.any(s2[0][400:, :3] != 0)                                       # the padding bodies fell in


@pytest.mark.parametrize("name,n,padded", [("stars_8192.dat", 8192, 8193), ("galaxy_20K.bin", 20000, 20225)])
def test_v3_tile_order_is_nearer_the_truth_than_the_single_chain(oracle_mod, golden_dir, name, n, padded):
    """The reference's inputs, padded its way, one frame at its dt and softening.  Prototype figures, velocities against the
    fp64 truth: stars_8192.dat tile order 2.84e-7, chain 2.92e-6; galaxy_20K.bin 3.9e-8 and 1.75e-6.  Asserted: the
    reference's association is inside the stated tolerance and nearer the truth than the single chain, which bounds from
    above what fp32 summation costs here."""
    import n_body_problem_amd as nb
    from n_body_problem_amd import datasets as ds
    pos, vel = ds.read_any(os.path.join(golden_dir, name))
    ppos, pvel = nb.pad_reference_style(pos, vel)
    assert pos.shape[0] == n and ppos.shape[0] == padded
    pt, vt = oracle_mod.step_v3_tiled(ppos, pvel, nsteps=1)
    pc, vc = oracle_mod.step_v3(ppos, pvel, nsteps=1)
    p64, v64 = oracle_mod.step_f64(ppos, pvel, nb.TIME_TICK, nb.SOFTENING_VERSION3, nsteps=1)
    tile = (rel_state_error(pt[:n], p64[:n]), rel_state_error(vt[:n], v64[:n]))
    chain = (rel_state_error(pc[:n], p64[:n]), rel_state_error(vc[:n], v64[:n]))
    print(f"{name}, one frame: positions / velocities vs fp64 truth: tile order {tile[0]:.3e} / {tile[1]:.3e}, single chain "
          f"{chain[0]:.3e} / {chain[1]:.3e}; tile order vs chain {rel_state_error(vt[:n], vc[:n]):.3e}")
    assert tile[0] < TOL and tile[1] < TOL
    assert tile[1] < chain[1]
