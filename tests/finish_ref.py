"""Inputs, the numpy reference and the table of cases of the finish tests (no HIP, no GPU): what a single-system step does
behind its force pass -- update_kernel<64|256>, update_sym_kernel<64|256>, sym_finish_update_kernel<0|1|2>, sym_combine_kernel +
kdk_kick_kernel<0|1> and kdk_kick_drift_kernel -- held bit for bit.

The acceleration probe.  On the context under test, in its own configuration (force mode, split length, summation parts,
shard): integrator kick_drift, the positions in place, every velocity zero, one step of dt = 1.  The kick
`(float)fma((double)a, 1.0, 0.0)` returns the fp32 acceleration itself, so the new velocities ARE the sums this configuration
forms (tests/force_pair_ref.py holds those sums pair by pair).  The positions are restored and the cached forces invalidated.

The reference, numpy.  h = f64(f32(dt)), or half of it (exact) for a half kick;
    kick:   v' = f32(f64(a) h + f64(v)),        drift:   x' = f32(f64(v') h + f64(x)).
The product of two 24-bit significands has at most 48 bits and is exact in fp64, so the sum is rounded once to fp64 -- exactly
what `__builtin_fma((double)a, h, (double)v)` returns -- and once more to fp32 by the cast.  tests/test_finish_bits_cpu.py
holds `kick` to that against a compiled C++ program, bit for bit, on 10^5 hashed inputs (`fma_inputs`).

Expected states, from probes and that arithmetic alone (`expected_kick_drift`, `expected_kdk`):
    kick-drift, one step:       a0 = probe(x0), v1 = kick(a0, dt, v0), x1 = drift(v1, dt, x0);
    kick-drift-kick, two steps: a0 = probe(x0), vh = kick(a0, dt/2, v0), x1 = drift(vh, dt, x0), a1 = probe(x1),
                                v1 = kick(a1, dt/2, vh); the second step opens with the CACHED a1 -- vh' = kick(a1, dt/2, v1),
                                x2 = drift(vh', dt, x1) -- and closes with a2 = probe(x2), v2 = kick(a2, dt/2, vh').
A half kick taken with dt, a drift that reads the old velocity, an acceleration that is stale (a0 where a1 belongs) or summed
in another association by one of the three paths, a shard's row_lo applied to the wrong array and a tail row past row_count all
change bits of these states; the CPU test injects each into a numpy device and sees the comparison fail.

What the bit test cannot distinguish.
  * An fp64 FMA rounded to fp32 (what the kernels do, and the reference) from a true fp32 FMA: the two differ only where the
    fp64 result lies within 2^-53 of a midpoint between two floats, about one input in 2^29.  The acceleration is computed,
    not chosen, so such an input cannot be built, and no test here proves which of the two a kernel uses.  It does tell both
    from the unfused fp32 `v + a * dt` (two roundings), and asserts that its inputs do.
  * The summation order across splits and groups.  The probe runs the same configuration, so an order that is wrong in the
    probe and in the step alike is invisible here; with strips the row sums are chained in registers across splits and cannot
    be separated by zeroing masses.  That order is held by the shard, parts and blocking bit-identity tests
    (tests/test_parity_gpu.py) and, term by term, by tests/test_force_pair_matrix_gpu.py.  What IS held: that the kick-drift,
    the half-kick and the acceleration-only finishes of one configuration, fused or not, sum the SAME acceleration.

Inputs (`inputs(case)`): pair_matrix_ref.configuration(n) positions; masses hashed in [0.5, 2) or all 1; velocities hashed in
[-1, 1), every 17th row scaled by 2^-20 and every 19th by 2^20; the fourth velocity word W_WORD.  dt = 0.008, eps = 1e-2 (one
case eps = 0).  `CASES` names, per case and integrator, the finish kernels it must land on; the CPU test asks
csrc/nbody_launch_choice.h (tests/launch_choice_driver.cpp) for each."""
import numpy as np

import pair_matrix_ref as pm

W_WORD = pm.W_WORD
DT = 0.008
EPS = 1e-2
INTEGRATORS = ("kick_drift", "kdk")
KDK_STEPS = 2


# ---- the arithmetic --------------------------------------------------------------------------------------------------------

def step_h(dt, half=False):
    """The step as the kernels see it: the fp32 argument widened, halved exactly for a half kick."""
    h = float(np.float32(dt))
    return 0.5 * h if half else h


def kick(a, h, v):
    """f32(f64(a) h + f64(v)), the fp64 sum rounded once.  The drift is the same function: drift(v, h, x) = kick(v, h, x)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.float64(h) + np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


drift = kick


def unfused_fp32(a, dt, v):
    """The arithmetic the kernels do NOT use: fp32 product, fp32 sum."""
    a, v = np.asarray(a, np.float32), np.asarray(v, np.float32)
    return (a * np.float32(dt)).astype(np.float32) + v


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected_kick_drift(probe, x0, v0, dt, rows=None):
    """One kick-drift step of the rows `rows` (a slice; None: every row).  probe(x (n, 3) float32) -> (rows, 3) float32.
    Returns [(x (n, 3), v (rows, 3))]: the positions of every body, those outside the rows untouched."""
    rows = slice(None) if rows is None else rows
    a0 = probe(x0)
    v1 = kick(a0, step_h(dt), v0)
    x1 = x0.copy()
    x1[rows] = drift(v1, step_h(dt), x0[rows])
    return [(x1, v1)]


def expected_kdk(probe, x0, v0, dt, rows=None, steps=KDK_STEPS):
    """`steps` kick-drift-kick steps with the closing acceleration of one step cached for the next: [(x, v)] after each."""
    rows = slice(None) if rows is None else rows
    h, hh = step_h(dt), step_h(dt, half=True)
    out = []
    x, v = x0, v0
    a = probe(x)
    for _ in range(steps):
        vh = kick(a, hh, v)
        x = x.copy()
        x[rows] = drift(vh, h, x[rows])
        a = probe(x)
        v = kick(a, hh, vh)
        out.append((x, v))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def inputs(case):
    """(pos (n, 4), vel (n, 4)) float32 of a case: the fourth words are the mass and W_WORD."""
    n = case["n"]
    i = np.arange(n)
    pos = np.empty((n, 4), np.float32)
    pos[:, :3] = pm.configuration(n)[0]
    pos[:, 3] = (0.5 + 1.5 * pm._hash01(i, 71)).astype(np.float32) if case["masses"] == "hashed" else np.float32(1.0)
    vel = np.full((n, 4), W_WORD, np.float32)
    v = np.stack([2.0 * pm._hash01(i, 72 + c) - 1.0 for c in range(3)], axis=1)
    v[::17] *= 2.0 ** -20
    v[::19] *= 2.0 ** 20
    vel[:, :3] = v
    return pos, vel


def fma_inputs(count=100000):
    """(a, v) float32 and the list of steps h for the FMA-equivalence proof: hashed accelerations over 2^-30 .. 2^12 with
    both signs, subnormal accelerations, -0.0 and +0.0, and velocities from 2^-24 to 2^24 times a h, both signs."""
    i = np.arange(count)
    sign = np.where(pm._hash01(i, 81) < 0.5, -1.0, 1.0)
    a = sign * (1.0 + pm._hash01(i, 82)) * 2.0 ** np.floor(-30.0 + 42.0 * pm._hash01(i, 83))
    scale = 2.0 ** np.round(-24.0 + 48.0 * pm._hash01(i, 84))
    v = np.where(pm._hash01(i, 85) < 0.5, -1.0, 1.0) * (1.0 + pm._hash01(i, 86)) * np.abs(a) * DT * scale
    a, v = a.astype(np.float32), v.astype(np.float32)
    a[0::50] = (sign[0::50] * (1 + (i[0::50] % 8388607)) * 2.0 ** -149).astype(np.float32)     # subnormal accelerations
    a[1::50] = np.float32(-0.0)
    a[2::50] = np.float32(0.0)
    v[3::50] = np.float32(-0.0)
    v[4::50] = np.float32(0.0)
    v[5::50] = (a[5::50].astype(np.float64) * DT * 2.0 ** 24).astype(np.float32)
    v[6::50] = (-a[6::50].astype(np.float64) * DT * 2.0 ** -24).astype(np.float32)
    v[7::50] = (-a[7::50].astype(np.float64) * step_h(DT)).astype(np.float32)                  # cancellation
    return a, v, [step_h(DT), step_h(DT, half=True), 1.0, step_h(1e-3)]


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------

def _case(name, mode, n, split_len, reaches, rows=None, parts=0, masses="hashed", eps=EPS, rig="whole", kernels=None):
    row_lo, row_count = rows if rows else (0, n)
    return {"name": name, "mode": mode, "n": n, "split_len": split_len, "row_lo": row_lo, "row_count": row_count, "parts": parts,
            "masses": masses, "eps": eps, "rig": rig, "reaches": reaches, "kernels": kernels}


#: per integrator, the finish kernels in the order a run launches them ("sym_combine_kernel + x": the combination in front);
#: kdk_kick_drift_kernel is not a choice: every kick-drift-kick step opens with it.
_ONE_SIDED_KDK = ["kdk_kick_kernel<0>", "kdk_kick_drift_kernel", "kdk_kick_kernel<1>"]
_COMBINED_KDK = ["sym_combine_kernel + kdk_kick_kernel<0>", "kdk_kick_drift_kernel", "sym_combine_kernel + kdk_kick_kernel<1>"]
_FUSED_KDK = ["sym_finish_update_kernel<2>", "kdk_kick_drift_kernel", "sym_finish_update_kernel<1>"]

CASES = [
    _case("one_sided_1000", "one_sided", 1000, 256, "update_kernel<64>, kdk_kick_kernel, kdk_kick_drift_kernel",
          kernels={"kick_drift": ["update_kernel<64>"], "kdk": _ONE_SIDED_KDK}),
    _case("one_sided_65613", "one_sided", 65613, 768, "update_kernel<256> with a ragged last block", masses="equal",
          kernels={"kick_drift": ["update_kernel<256>"], "kdk": _ONE_SIDED_KDK}),
    _case("one_sided_shard_3000", "one_sided", 3000, 320, "row_lo != 0 in the update and all three kick-drift-kick kernels",
          rows=(640, 1000), eps=0.0, rig="shard", kernels={"kick_drift": ["update_kernel<64>"], "kdk": _ONE_SIDED_KDK}),
    _case("pair_once_fused_5000", "pair_once", 5000, 256, "the fused sym_finish_update_kernel<0>, <1> and <2>",
          kernels={"kick_drift": ["sym_finish_update_kernel<0>"], "kdk": _FUSED_KDK}),
    _case("pair_once_parts_5000", "pair_once", 5000, 256, "update_sym_kernel<64>, and sym_combine + kdk_kick_kernel", parts=2,
          kernels={"kick_drift": ["update_sym_kernel<64>"], "kdk": _COMBINED_KDK}),
    _case("pair_once_parts_65613", "pair_once", 65613, 512, "update_sym_kernel<256>", parts=2, masses="equal",
          kernels={"kick_drift": ["update_sym_kernel<256>"], "kdk": _COMBINED_KDK}),
    _case("pair_once_shards_4096", "pair_once", 4096, 256, "update_sym_kernel with row_lo != 0 (two shards, a manual exchange)",
          rows=(2048, 2048), rig="shard_pair", kernels={"kick_drift": ["update_sym_kernel<64>"], "kdk": _COMBINED_KDK}),
]

#: the two cases that must also give each other's bits: the source's claim that the fused finish changes none
FUSED_AND_UNFUSED = ("pair_once_fused_5000", "pair_once_parts_5000")

OPS = {"kick_drift": ["update"], "kdk": ["prepare", "kick"]}


def shards_of(case):
    """[(row_lo, row_count)] of the contexts a case creates: the rows under test last."""
    if case["rig"] == "shard_pair":
        return [(0, case["row_lo"]), (case["row_lo"], case["row_count"])]
    return [(case["row_lo"], case["row_count"])]


def driver_commands(case, integrator):
    """The `finish` commands of tests/launch_choice_driver.cpp for the finishing calls of one run, in the order of OPS."""
    pair_once = int(case["mode"] == "pair_once")
    summed = int(case["rig"] == "shard_pair")        # a pair-once shard has called nbody_sym_reduce before its finish
    return [f"finish {op} {pair_once} {case['n']} {case['split_len']} {case['row_lo']} {case['row_count']} {case['parts']} 0 {summed}"
            for op in OPS[integrator]]


def kernels_from_driver(lines):
    """The driver's answers `kernel|threads|combine` as the table spells them."""
    out = []
    for line in lines:
        kernel, threads, combine = line.split("|")
        out.append(("sym_combine_kernel + " if int(combine) else "") + kernel)
    return out


def chosen_of(case, integrator):
    """The table's kernels of a run without kdk_kick_drift_kernel, which no choice precedes."""
    return [k for k in case["kernels"][integrator] if k != "kdk_kick_drift_kernel"]
