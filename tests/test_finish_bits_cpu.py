"""CPU: the finish tests' own parts (tests/finish_ref.py) -- the numpy kick against the kernels' expression compiled for the host
(tests/finish_fma_driver.cpp), bit for bit; the expected states against a numpy device with one fault at a time, each of which
the comparison must see; and the table of GPU cases against the finish kernels csrc/nbody_launch_choice.h chooses for them
(tests/launch_choice_driver.cpp), with every family and block size the function can return."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import finish_ref as fr
from conftest import ROOT

CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------

def test_numpy_kick_is_the_compiled_fma_bit_for_bit(tmp_path):
    exe = str(tmp_path / "finish_fma_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "finish_fma_driver.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    a, v, steps = fr.fma_inputs()
    n = len(a)
    assert n == 100000
    # what the inputs claim to hold
    sub = (a != 0) & (np.abs(a) < np.float32(2.0 ** -126))
    assert sub.sum() >= n // 50 - 1 and (fr.bits(a) == 0x80000000).sum() >= n // 50 and (fr.bits(v) == 0x80000000).sum() >= n // 50
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.abs(v.astype(np.float64)) / np.abs(a.astype(np.float64) * fr.step_h(fr.DT))
    ratio = ratio[np.isfinite(ratio) & (ratio > 0)]
    assert ratio.max() >= 2.0 ** 24 and ratio.min() <= 2.0 ** -24
    blob = struct.pack("<QQ", n, len(steps)) + a.tobytes() + v.tobytes() + np.asarray(steps, np.float64).tobytes()
    res = subprocess.run([exe], input=blob, capture_output=True)
    assert res.returncode == 0 and len(res.stdout) == 4 * n * len(steps)
    want = np.frombuffer(res.stdout, np.float32).reshape(len(steps), n)
    differs_from_unfused = 0
    for k, h in enumerate(steps):
        got = fr.kick(a, h, v)
        bad = np.flatnonzero(fr.bits(got) != fr.bits(want[k]))
        assert not len(bad), (h, int(bad[0]), float(a[bad[0]]), float(v[bad[0]]), float(got[bad[0]]), float(want[k][bad[0]]))
        differs_from_unfused += int((fr.bits(fr.unfused_fp32(a, h, v)) != fr.bits(got)).sum())
    assert differs_from_unfused > n // 20          # the two-rounding arithmetic is told apart on these inputs
    assert fr.step_h(fr.DT, half=True) * 2.0 == fr.step_h(fr.DT) == float(np.float32(0.008)) != 0.008


# ---- a numpy device, correct or with one fault --------------------------------------------------------------------------------

N_DEVICE = 333


def numpy_probe(pos4, eps, rows):
    """(x (n, 3)) -> (rows, 3) float32: the fp64 direct sum rounded to fp32 -- any fixed function of the positions serves."""
    m = pos4[:, 3].astype(np.float64)

    def probe(x):
        x = np.asarray(x, np.float32).astype(np.float64)
        d = x[None, :, :] - x[rows][:, None, :]
        r2 = (d * d).sum(-1) + eps * eps
        with np.errstate(divide="ignore"):
            s = np.where(r2 > 0, m[None, :] / np.where(r2 > 0, r2, 1.0) ** 1.5, 0.0)
        idx = np.arange(len(x))[rows]
        s[np.arange(len(idx)), idx] = 0.0
        return (s[..., None] * d).sum(1).astype(np.float32)
    return probe


FAULTS = ("half kick with dt", "drift reads the old velocity", "stale cached acceleration", "row_lo on the wrong side",
          "tail row beyond row_count")


def device_run(probe, x0, v0, dt, integrator, rows, fault=None):
    """What a device leaves after the run of `integrator` ([(x, v)] like the expected states), the kernels' way: the state in
    arrays, the shard's rows addressed through row_lo."""
    lo, cnt = rows.start, rows.stop - rows.start
    h, hh = fr.step_h(dt), fr.step_h(dt, half=True)
    x, v = x0.copy(), v0.copy()                       # x: every body; v: the rows
    out = []

    def drift_rows(vel_for_drift):
        for r in range(cnt + (1 if fault == "tail row beyond row_count" and lo + cnt < len(x) else 0)):
            src = vel_for_drift[min(r, cnt - 1)]
            at = r if fault == "row_lo on the wrong side" else lo + r
            x[at] = fr.drift(src, h, x[at])

    if integrator == "kick_drift":
        old = v.copy()
        v[:] = fr.kick(probe(x), h, v)
        drift_rows(old if fault == "drift reads the old velocity" else v)
        return [(x.copy(), v.copy())]
    acc = probe(x)
    for step in range(fr.KDK_STEPS):
        old = v.copy()
        v[:] = fr.kick(acc, h if fault == "half kick with dt" else hh, v)
        drift_rows(old if fault == "drift reads the old velocity" else v)
        new = probe(x)
        v[:] = fr.kick(new, hh, v)
        if fault != "stale cached acceleration":
            acc = new
        out.append((x.copy(), v.copy()))
    return out


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(fr.bits(g[0]), fr.bits(w[0])) and np.array_equal(fr.bits(g[1]), fr.bits(w[1]))
                                         for g, w in zip(got, want))


@pytest.mark.parametrize("rows", [slice(0, N_DEVICE), slice(64, 64 + 200)], ids=["whole", "shard"])
def test_the_expected_states_see_every_fault(rows):
    pos, vel = fr.inputs({"n": N_DEVICE, "masses": "hashed"})
    x0, v0 = pos[:, :3].copy(), vel[rows, :3].copy()
    probe = numpy_probe(pos, fr.EPS, rows)
    expected = {"kick_drift": fr.expected_kick_drift(probe, x0, v0, fr.DT, rows), "kdk": fr.expected_kdk(probe, x0, v0, fr.DT, rows)}
    assert len(expected["kick_drift"]) == 1 and len(expected["kdk"]) == fr.KDK_STEPS
    for integrator in fr.INTEGRATORS:
        assert same(device_run(probe, x0, v0, fr.DT, integrator, rows), expected[integrator]), integrator
        for x, v in expected[integrator]:
            assert np.isfinite(x).all() and np.isfinite(v).all()
            outside = np.ones(N_DEVICE, bool)
            outside[rows] = False
            assert np.array_equal(fr.bits(x[outside]), fr.bits(x0[outside]))
    seen = {f: [i for i in fr.INTEGRATORS if not same(device_run(probe, x0, v0, fr.DT, i, rows, f), expected[i])] for f in FAULTS}
    whole = rows.stop - rows.start == N_DEVICE
    for f in FAULTS:
        if f in ("half kick with dt", "stale cached acceleration"):
            assert seen[f] == ["kdk"], (f, seen[f])                      # faults of the kick-drift-kick path alone
        elif whole and f in ("row_lo on the wrong side", "tail row beyond row_count"):
            assert seen[f] == [], (f, seen[f])                           # no such fault without a shard ...
        else:
            assert seen[f] == list(fr.INTEGRATORS), (f, seen[f])         # ... and both integrators show it on one
    # the second step is what tells a stale cache: after one step the states agree
    stale = device_run(probe, x0, v0, fr.DT, "kdk", rows, "stale cached acceleration")
    assert same(stale[:1], expected["kdk"][:1]) and not same(stale[1:], expected["kdk"][1:])
    # and the inputs tell the fp64 FMA from the unfused fp32 arithmetic
    a0 = probe(x0)
    assert (fr.bits(fr.unfused_fp32(a0, fr.DT, v0)) != fr.bits(fr.kick(a0, fr.step_h(fr.DT), v0))).any()


def test_inputs_are_what_the_module_says():
    for case in fr.CASES:
        pos, vel = fr.inputs(case)
        n = case["n"]
        assert pos.dtype == vel.dtype == np.float32 and pos.shape == vel.shape == (n, 4)
        assert (vel[:, 3] == fr.W_WORD).all() and np.isfinite(pos).all() and np.isfinite(vel).all()
        m = pos[:, 3]
        assert (len(np.unique(m)) > n // 2 and 0.5 <= m.min() and m.max() < 2.0) if case["masses"] == "hashed" else (m == 1.0).all()
        speed = np.abs(vel[:, :3]).max(1)
        slow, fast = np.arange(n) % 17 == 0, np.arange(n) % 19 == 0
        assert speed[~slow & ~fast].max() < 1.0 and speed[slow & ~fast].max() < 2.0 ** -20 and speed[fast & ~slow].max() > 2.0 ** 19
    assert {c["masses"] for c in fr.CASES} == {"hashed", "equal"} and sorted({c["eps"] for c in fr.CASES}) == [0.0, fr.EPS]
    by_name = {c["name"]: c for c in fr.CASES}
    a, b = (by_name[k] for k in fr.FUSED_AND_UNFUSED)
    assert all(a[k] == b[k] for k in ("mode", "n", "split_len", "row_lo", "row_count", "masses", "eps")) and a["parts"] != b["parts"]


# ---- the case table lands where it claims ------------------------------------------------------------------------------------

#: every outcome of finish_choice: family, block size or mode, and the combination in front
EXPECTED_OUTCOMES = [
    "update_kernel<64>", "update_kernel<256>", "update_sym_kernel<64>", "update_sym_kernel<256>",
    "sym_finish_update_kernel<0>", "sym_finish_update_kernel<1>", "sym_finish_update_kernel<2>",
    "kdk_kick_kernel<0>", "kdk_kick_kernel<1>", "sym_combine_kernel + kdk_kick_kernel<0>", "sym_combine_kernel + kdk_kick_kernel<1>",
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("finish") / "launch_choice_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(ROOT, "tests", "launch_choice_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == len(commands)
        return lines
    return run


def everything_the_function_returns(driver):
    """finish_choice over its own inputs: both sides of every condition it reads."""
    commands = [f"choice {op} {po} {whole} {one} {splits} {strip} {rows}"
                for op, po, whole, one, splits, strip, rows in itertools.product(
                    ("update", "prepare", "kick"), (0, 1), (0, 1), (0, 1), (1, 20, 320, 321, 4096), (1, 2, 4, 8),
                    (1, 1000, 65535, 65536, 65613, 1 << 20))]
    return set(fr.kernels_from_driver(driver(commands)))


def test_every_case_lands_on_the_finish_kernels_it_names(driver):
    reached = set()
    for case in fr.CASES:
        one_sided, pair_once = driver([f"split {case['n']}"])[0].split("|")
        if case["mode"] == "one_sided" and case["rig"] == "whole":
            assert case["split_len"] == int(one_sided), case["name"]           # the default split length
        if case["mode"] == "pair_once":
            assert case["split_len"] in (256, int(pair_once)), case["name"]
        assert case["row_lo"] % case["split_len"] == 0 and case["row_lo"] + case["row_count"] <= case["n"]
        for integrator in fr.INTEGRATORS:
            got = fr.kernels_from_driver(driver(fr.driver_commands(case, integrator)))
            assert got == fr.chosen_of(case, integrator), (case["name"], integrator, got)
            reached |= set(got)
            assert ("kdk_kick_drift_kernel" in case["kernels"][integrator]) == (integrator == "kdk")
    assert len(EXPECTED_OUTCOMES) == len(set(EXPECTED_OUTCOMES))
    assert reached == set(EXPECTED_OUTCOMES) == everything_the_function_returns(driver)
    # the shapes: a ragged last block in every case but the shards of whole splits; the 256-thread variants from 256 x 256 rows on
    for case in fr.CASES:
        rows = case["row_count"]
        assert rows % 64 != 0 or case["rig"] == "shard_pair", case["name"]
        block = int(case["kernels"]["kick_drift"][0].split("<")[1].rstrip(">")) if "update_" in case["kernels"]["kick_drift"][0] else 0
        assert block in (0, 64 if rows < 256 * 256 else 256), case["name"]
    shards = [c for c in fr.CASES if c["row_lo"] != 0]
    assert {c["mode"] for c in shards} == {"one_sided", "pair_once"}
    assert fr.shards_of(shards[-1]) == [(0, 2048), (2048, 2048)]
