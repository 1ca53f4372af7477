#!/usr/bin/env python3
"""Host side of nbody_step_n at small N, where the work per step on the host shows: wall ms per step through the bare C ABI.

    NBODY_AMD_LIBRARY=<library> tools/ctx_rate.py [--sizes 1024 20225] [--repeats 7] > rate.jsonl

One JSON line per case: force mode (one_sided, pair_once) x integrator (kick_drift, kdk) x graph replay (0 off, -1 automatic) x
size, with the wall time of each repeat of step_n(k) (which ends in one synchronisation) divided by k.  Run it once per library
in alternation and compare the medians with the other library's spread (profiles/ctx_ownership_rate.txt).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from n_body_problem_amd import _lib  # noqa: E402

MODES = {"one_sided": 0, "pair_once": 2}   # pair_once: NBODY_FORCE_AUTO, with the split length that mode wants
INTEGRATORS = {"kick_drift": 0, "kdk": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 20225])
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    lib = _lib.load()
    for n in args.sizes:
        rng = np.random.default_rng(7)
        pos = np.concatenate([rng.normal(0, 1, (n, 3)), np.full((n, 1), 1.0 / n)], axis=1).astype(np.float32)
        vel = np.zeros((n, 4), np.float32)
        k = max(200, 2_000_000 // n)
        for mode, integrator, replay in ((m, i, r) for m in MODES for i in INTEGRATORS for r in (0, -1)):
            h = ctypes.c_void_p()
            _lib.check(lib.nbody_create(ctypes.byref(h), 0, n))
            for status in (lib.nbody_set_force_mode(h, MODES[mode]), lib.nbody_set_integrator(h, INTEGRATORS[integrator]),
                           lib.nbody_set_graph_replay(h, replay), lib.nbody_set_positions(h, pos.ctypes.data),
                           lib.nbody_set_velocities(h, vel.ctypes.data), lib.nbody_step_n(h, 50, 1e-3, 1e-2)):
                _lib.check(status, h)
            ms = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                _lib.check(lib.nbody_step_n(h, k, 1e-3, 1e-2), h)
                ms.append((time.perf_counter() - t0) * 1e3 / k)
            _lib.check(lib.nbody_destroy(h))
            print(json.dumps({"n": n, "mode": mode, "integrator": integrator, "graph_replay": replay, "k": k,
                              "ms_per_step": ms}), flush=True)


if __name__ == "__main__":
    main()
