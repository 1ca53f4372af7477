#!/usr/bin/env python3
"""Measured parity on the reference's own inputs (tests/golden: galaxy_20K.bin, k17hp.snap, k17c.snap, stars_8192.dat, stars.dat),
the reference's way: padded to roundup(n, 256) + 1 (kernel.cu:260-278), dt = 0.008, VERSION 3's effective softening 1e-2
(kernel.cu:63-66, 665-692), K frames of the bracket kernel.cu:1225-1242.

For every input, force mode and body order, the HIP path's state against three CPU results: VERSION 3 restated in the
reference's own tile order (oracle.step_v3_tiled: 256 x 256 blocks, fresh sums per block, blocks added in ascending number --
one legal order of its atomics, and the partner of the stated 1e-5), the fp64 truth (oracle.step_f64), and VERSION 3 summed
as one ascending fp32 chain per body (oracle.step_v3: the upper envelope, no order the reference takes).  Per input, next
to them: tile order and chain against the truth, and the wall time of each CPU path at oracle.host_threads() threads (the
chain also on one thread, as it ran before it was threaded).
rel = max_i |x_i - ref_i|_inf / max_i |ref_i|_inf over the real bodies.  Run on an MI355X; the output is
committed as profiles/parity_tile_order.txt and quoted in README.md / DESIGN.md next to the 1e-5 tolerance.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

import n_body_problem_amd as nb
import oracle
from conftest import rel_state_error
from n_body_problem_amd import datasets as ds


def run(ppos, pvel, frames, mode, order):
    n = ppos.shape[0]
    with nb.NBodySystem(n, split_len=(256 if n < 8192 else nb.pair_once_split_len(n)) if mode == "pair_once" else 0,
                        body_order=order) as s:
        s.set_force_mode(mode)
        s.setParticlesPosition(ppos)
        s.setParticlesVelocity(pvel)
        s.step_n(frames, nb.TIME_TICK, nb.SOFTENING_VERSION3)
        return s.download()


def timed(fn, *args, **kw):
    t0 = time.perf_counter()
    out = fn(*args, **kw)
    return out, time.perf_counter() - t0


def main():
    oracle.build()
    golden = os.path.join(ROOT, "tests", "golden")
    err = rel_state_error
    print(f"oracle threads: {oracle.host_threads()}; every entry: positions / velocities")
    for name, frame_list in (("galaxy_20K.bin", (1, 10)), ("k17hp.snap", (1, 10)), ("k17c.snap", (3,)), ("stars_8192.dat", (1,)),
                             ("stars.dat", (1,))):
        pos, vel = ds.read_any(os.path.join(golden, name))
        ppos, pvel = nb.pad_reference_style(pos, vel)
        n = pos.shape[0]
        for frames in frame_list:
            (pt, vt), t_tiled = timed(oracle.step_v3_tiled, ppos, pvel, nsteps=frames)
            (p3, v3), t_chain = timed(oracle.step_v3, ppos, pvel, nsteps=frames)
            (p1, v1), t_chain1 = timed(oracle.step_v3, ppos, pvel, nsteps=frames, threads=1)
            assert np.array_equal(p1, p3) and np.array_equal(v1, v3)
            (p64, v64), t_f64 = timed(oracle.step_f64, ppos, pvel, nb.TIME_TICK, nb.SOFTENING_VERSION3, nsteps=frames)
            print(f"\n{name}: {n} bodies padded to {ppos.shape[0]} ({oracle.v3_tiled_blocks(ppos.shape[0])} blocks), {frames} frame(s)")
            print(f"  tile order vs truth {err(pt[:n], p64[:n]):.3e} / {err(vt[:n], v64[:n]):.3e} | single chain vs truth "
                  f"{err(p3[:n], p64[:n]):.3e} / {err(v3[:n], v64[:n]):.3e} | tile order vs chain {err(pt[:n], p3[:n]):.3e} / "
                  f"{err(vt[:n], v3[:n]):.3e}")
            print(f"  CPU seconds: tile order {t_tiled:.2f}, single chain {t_chain:.2f} (one thread, the same bits: {t_chain1:.2f}), "
                  f"fp64 truth {t_f64:.2f}")
            print(f"  {'mode':10s} {'order':7s} | {'HIP vs tile order':>21s} | {'HIP vs truth':>21s} | {'HIP vs single chain':>21s}")
            for mode in ("one_sided", "pair_once"):
                for order in ("given", "morton"):
                    p, v = run(ppos, pvel, frames, mode, order)
                    print(f"  {mode:10s} {order:7s} | {err(p[:n], pt[:n]):10.3e} {err(v[:n], vt[:n]):10.3e} | "
                          f"{err(p[:n], p64[:n]):10.3e} {err(v[:n], v64[:n]):10.3e} | {err(p[:n], p3[:n]):10.3e} "
                          f"{err(v[:n], v3[:n]):10.3e}", flush=True)


if __name__ == "__main__":
    main()
