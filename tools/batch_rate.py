"""Batched ensembles against the status quo: B independent systems of n bodies stepped by one BatchedSystem, and the same
systems stepped one NBodySystem each (timed on a subset, scaled to B).  One JSON line per (n, B, integrator):
python tools/batch_rate.py [--cases 1024x1024 ...] [--integrators kick_drift kdk hermite] [--repeats 5] [--subset 8]

Rates use the one-sided convention: n^2 ordered interactions per system and step, against the 157.3 TFLOP/s fp32 vector
peak at 20 flop per interaction for kick_drift and kdk (a force) and 60 flop per interaction for hermite (a force and a
jerk, the convention of the Hermite GPU literature); the line names its convention.  Times are HIP events around
step_n(k) after a warm-up, the median of repeats that alternate the batched and the status-quo measurement.  Hermite
exists for batches only, so its lines have no status-quo figures."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import n_body_problem_amd as nb  # noqa: E402

PEAK_FP32 = 157.3e12
FLOP_PER_INTERACTION = {"kick_drift": 20, "kdk": 20, "hermite": 60}
CASES = [(64, 16384), (256, 4096), (1024, 1024), (4096, 256), (4096, 512)]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="*", default=[f"{n}x{b}" for n, b in CASES], help="n x B")
ap.add_argument("--integrators", nargs="*", default=["kick_drift", "kdk"])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--subset", type=int, default=8, help="systems the status quo is timed on")
ap.add_argument("--dt", type=float, default=1e-3)
ap.add_argument("--eps", type=float, default=1e-2)
args = ap.parse_args()


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def ensemble(n, B):
    """B Plummer spheres of n bodies: one sphere per seed for the first 64 systems, then copies jittered by 1e-4."""
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    rng = np.random.default_rng(n * 7 + B)
    for s in range(B):
        if s < 64:
            P[s], V[s] = nb.plummer(n, seed=1000 + s)
        else:
            P[s], V[s] = P[s % 64], V[s % 64]
            P[s, :, :3] += rng.normal(0, 1e-4, (n, 3)).astype(np.float32)
    return P, V


for case in args.cases:
    n, B = (int(x) for x in case.lower().split("x"))
    P, V = ensemble(n, B)
    inter = B * n * n
    k = int(min(400, max(10, 2e11 // inter)))   # ~60 ms per batched call at 3e12 interactions/s
    for integrator in args.integrators:
        batch = nb.BatchedSystem(B, n, integrator=integrator)
        batch.set_state(P, V)
        subset = min(args.subset, B) if integrator != "hermite" else 0
        singles = []
        for s in range(subset):
            one = nb.NBodySystem(n)
            one.set_force_mode("auto")          # the faster force mode at this size (the pair-once kernels at every size)
            one.set_integrator(integrator)
            one.setParticlesPosition(P[s])
            one.setParticlesVelocity(V[s])
            singles.append(one)
        k_single = max(5, k // 4)

        def run_batch():
            batch.step_n(k, args.dt, args.eps)

        def run_singles():
            for one in singles:
                one.step_n(k_single, args.dt, args.eps)

        run_batch()
        run_singles()
        torch.cuda.synchronize()
        tb, ts = [], []
        for _ in range(args.repeats):          # alternated
            tb.append(timed(run_batch) / k)
            if singles:
                ts.append(timed(run_singles) / k_single * B / subset)
        batch.sync()
        ms = statistics.median(tb)
        rate = inter / (ms * 1e-3)
        flop = FLOP_PER_INTERACTION[integrator]
        line = {
            "n": n, "B": B, "integrator": integrator, "k": k, "ms_per_step": round(ms, 5),
            "ms_per_step_repeats": [round(x, 5) for x in tb],
            "interactions_per_s": float(f"{rate:.4g}"),
            "flop_per_interaction": flop,
            "frac_of_fp32_peak": round(flop * rate / PEAK_FP32, 4)}
        if ts:
            ms_sq = statistics.median(ts)
            line.update({
                "status_quo_ms_per_step": round(ms_sq, 4), "status_quo_systems_timed": subset, "status_quo_k": k_single,
                "status_quo_interactions_per_s": float(f"{inter / (ms_sq * 1e-3):.4g}"),
                "speedup_vs_status_quo": round(ms_sq / ms, 1)})
        print(json.dumps(line), flush=True)
        batch.close()
        for one in singles:
            one.close()
