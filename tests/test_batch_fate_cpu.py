"""CPU-only: tracer fates for Hermite batches (nbody_batch_fate_set, include/nbody_batch_fate.h).  The three entry points are
declared by that header alone, reachable through nbody.h, mirrored in _lib in a list of their own, exported by the library and
by the RCCL test-double build and wrapped by BatchedSystem and nbody::Batch; NULL handles and bad actions are refused without
a device; the ABI stays at version 5.  The fp64 reference (hermite_fate_ref) is checked against hermite_adaptive_ref and
against itself, and every input of test_batch_fate_gpu.py is run through it here: each decision must lie at least MARGIN
relative from its radius, the non-events one evaluation earlier included."""
import ctypes
import glob
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hermite_adaptive_ref as aref
import hermite_fate_ref as fref
import test_batch_fate_gpu as cases
from conftest import ROOT

FATE_NAMES = ["nbody_batch_fate_set", "nbody_batch_fate_read", "nbody_batch_fate_count"]
H, RE, RP, ETA = cases.H, cases.RE, cases.RP, cases.ETA


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def test_the_entry_points_are_declared_by_their_header_alone_and_reachable_through_nbody_h():
    include = os.path.join(ROOT, "include")
    assert declared(open(os.path.join(include, "nbody_batch_fate.h")).read()) == set(FATE_NAMES)
    for header in glob.glob(os.path.join(include, "*.h")):
        if os.path.basename(header) != "nbody_batch_fate.h":
            assert not declared(open(header).read()) & set(FATE_NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(include, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(FATE_NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(include, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_massive.h"') < nbody_h.index('#include "nbody_batch_fate.h"')


def test_the_headers_state_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(ROOT, "include", "nbody_batch_fate.h")).read().replace(" *", " ").split())
    for phrase in ("NBODY_BATCH_TRACERS_REFUSE (0", "NBODY_BATCH_TRACERS_REMOVE (1)", "ABI version 5", "Two tracers never collide",
                   "fmaf(S, S, eps^2)", "fmaf(z, z, fmaf(y, y, x x)) > R_e R_e", "has fate HIT", "does not vote",
                   "0, 0, -1, 0, 0", "NBODY_ERR_STATE", "Out of scope", "first tracer event", "mass word into the body it hits",
                   "mergers among massive bodies", "compacting dead tracers", "centre-of-mass escape test",
                   "evolve(a) followed by evolve(b) is evolve(a + b)", "nbody_batch_evolve_launch_steps"):
        assert phrase in text, phrase
    massive = " ".join(open(os.path.join(ROOT, "include", "nbody_batch_massive.h")).read().replace(" *", " ").split())
    assert "nbody_batch_fate.h" in massive and "NBODY_BATCH_TRACERS_REMOVE" in massive


def test_the_names_are_mirrored_in_a_list_of_their_own_and_exported_by_both_builds(lib):
    from n_body_problem_amd import _lib
    assert set(_lib.fate_names()) == set(FATE_NAMES)
    assert not set(FATE_NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                                  set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()))
    assert (_lib.BATCH_TRACERS_REFUSE, _lib.BATCH_TRACERS_REMOVE) == (0, 1)
    assert (_lib.BATCH_FATE_ALIVE, _lib.BATCH_FATE_HIT, _lib.BATCH_FATE_ESCAPED) == (0, 1, 2)
    for name in FATE_NAMES:
        assert hasattr(lib, name), name
    sys.path.insert(0, os.path.join(ROOT, "tests", "fake_rccl"))
    import build_fake_rccl
    fake = ctypes.CDLL(build_fake_rccl.build())
    for name in FATE_NAMES:
        assert hasattr(fake, name), name


def test_the_abi_stays_at_version_5_and_null_handles_and_bad_actions_are_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    good, bad = _lib.BatchFateConfig(1), _lib.BatchFateConfig(7)
    assert lib.nbody_batch_fate_set(None, ctypes.byref(good)) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_fate_set: batch is NULL" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_fate_set(None, None) == _lib.NBODY_ERR_INVALID
    assert lib.nbody_batch_fate_set(None, ctypes.byref(bad)) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_fate_set: unknown tracer action" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_fate_read(None, None, None, None, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_fate_read: batch is NULL" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_fate_count(None, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_fate_count: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_signatures():
    import n_body_problem_amd as nb
    assert list(inspect.signature(nb.BatchedSystem.set_tracer_action).parameters) == ["self", "action"]
    assert list(inspect.signature(nb.BatchedSystem.fates).parameters) == ["self"]
    assert list(inspect.signature(nb.FateResult.__init__).parameters) == ["self", "fate", "ticks", "target", "separation",
                                                                          "relative_speed", "hit", "escaped"]
    for word in ("refuse", "remove", "merge", "fates"):
        assert word in nb.BatchedSystem.set_tracer_action.__doc__


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_fate.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
int main() {
    try {
        nbody::Batch b(16, 64);
        b.setMassiveCounts(std::vector<std::int64_t>(16, 2));
        b.setTracerAction(true);
        nbody::Batch::Fates f = b.fates();
        b.setTracerAction(false);
        std::printf("%lld %lld\n", (long long)f.fate.size(), (long long)f.hit.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_fate"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.join(ROOT, "n_body_problem_amd"), "-lnbody_amd", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ---- the reference ----------------------------------------------------------------------------------------------------
def test_the_reference_with_conditions_that_never_trigger_is_the_adaptive_reference_with_zero_mass_tracers():
    p, v, R, _ = cases.scene(50, 3, hit_steps=(), escape_steps=())
    z = p.copy()
    z[3:, 3] = 0.0
    for eps in (0.0, 1e-2):
        want = aref.evolve(z, v, 4, H, levels=6, eta=ETA, eta_start=ETA, eps=eps)
        for kw in (dict(), dict(collision_radius=1e-7, escape_radius=1e6), dict(radii=np.full(50, 1e-8), escape_radius=1e6)):
            got = fref.evolve(p, v, 3, 4, H, levels=6, eta=ETA, eta_start=ETA, eps=eps, **kw)
            assert got.level_seq == want.level_seq and got.tick_seq == want.tick_seq and got.ticks == want.ticks
            assert got.steps > 4 and not got.fate.any() and got.reason == 0
            # the same sums over three columns and over fifty of which 47 add zero: equal up to the order of the fp64 sums
            assert np.allclose(got.pos[:, :3], want.pos[:, :3], rtol=1e-12, atol=1e-13)
            assert np.allclose(got.vel[:, :3], want.vel[:, :3], rtol=1e-12, atol=1e-13)
            assert np.array_equal(got.pos[:, 3], p[:, 3].astype(np.float64)) and np.array_equal(got.vel[:, 3], v[:, 3].astype(np.float64))


@pytest.mark.parametrize("cap,n,m", [s for s in cases.SHAPES if s[1] <= 700])
def test_with_a_fixed_step_live_bodies_are_the_plain_run_and_dead_tracers_that_run_at_their_fate_tick(cap, n, m):
    p, v, R, plan, _ = cases.fixed_step_case(cap, n, m)
    kw = dict(levels=0, eta=ETA, eta_start=ETA, eps=0.0, round_state=True)
    ref = fref.evolve(p, v, m, 5, H, radii=R if m else None, escape_radius=RE, **kw)
    plain = {k: fref.evolve(p, v, m, 5, H, max_steps=k, **kw) for k in range(0, 6)}
    alive = ref.fate == 0
    assert np.array_equal(ref.pos[alive], plain[5].pos[alive]) and np.array_equal(ref.vel[alive], plain[5].vel[alive])
    assert (~alive).sum() == len(plan)
    for i in np.nonzero(~alive)[0]:
        k = int(ref.fate_step[i])
        assert ref.fate_tick[i] == plain[k].ticks == k
        assert np.array_equal(ref.pos[i], plain[k].pos[i]) and np.array_equal(ref.vel[i], plain[k].vel[i])


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,n,m", cases.SHAPES)
def test_the_fixed_step_inputs_decide_clearly(cap, n, m):
    p, v, R, plan, _ = cases.fixed_step_case(cap, n, m)
    ref = cases.reference(p, v, m, 5, H, 0, 0.0, radii=R if m else None, escape_radius=RE)
    assert ref.reason == 0
    assert {int(i): int(ref.fate_step[i]) for i in np.nonzero(ref.fate)[0]} == {r: s for r, (_, s) in plan.items()}
    assert cases.decisions_are_clear(ref, m, collide=m > 0)
    for levels, chunk in ((0, 7), (0, 3)):                             # the runs of the frozen-and-forgotten and refusal tests
        ref = cases.reference(p, v, m, chunk, H, levels, 0.0, radii=R if m else None, escape_radius=RE)
        assert cases.decisions_are_clear(ref, m, collide=m > 0) and ref.reason == 0


def test_the_never_triggering_inputs_come_nowhere_near_their_radii():
    for n, m in ((50, 3), (100, 1), (700, 3), (50, 0), (5, 5), (50, 50)):
        p, v, R, _ = cases.scene(n, m, hit_steps=(), escape_steps=())
        for eps in (0.0, 1e-2):
            ref = cases.reference(p, v, m, 2, H, 6, eps, collision_radius=1e-7, escape_radius=1e6)
            assert not ref.fate.any() and ref.reason == 0
            # with eps the ratio sqrt((d.d + eps^2) / (S^2 + eps^2)) is at most about d / eps
            assert min(t[np.isfinite(t)].min(initial=np.inf) for t in ref.touch_seq) > 10.0 and min(ref.massive_touch_seq) > 10.0
            assert max(d.max() for d in ref.dist_seq) < 1e3


def test_the_mask_inputs_decide_clearly():
    for cap, n, row in ((64, 50, 40), (1024, 700, 600)):
        p, v, R = cases.mask_case(cap, n, row, False)
        for kw in (dict(radii=R), dict(collision_radius=2 * float(RP))):
            ref = cases.reference(p, v, 3, 2, H, 0, 0.0, **kw)
            assert np.nonzero(ref.fate)[0].tolist() == [row] and ref.fate_target[row] == 1 and ref.fate_step[row] == 0 and ref.reason == 0
            assert cases.decisions_are_clear(ref, 3, escape_radius=0.0)
        p, v, R = cases.mask_case(cap, n, row, True)
        ref = cases.reference(p, v, 3, 2, H, 0, 0.0, radii=R)
        assert ref.reason == fref.COLLISION and ref.pair == (1, 2) and ref.steps == 0 and not ref.fate.any()
        assert cases.decisions_are_clear(ref, 3, escape_radius=0.0)


def test_the_adaptive_start_coincident_and_massive_stop_inputs_decide_clearly():
    p, v, R, n, m = cases.adaptive_case()
    ref = cases.reference(p, v, m, 24, H, 8, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and cases.decisions_are_clear(ref, m)
    assert ref.hit >= 3 and ref.escaped >= 1
    p, v, R, n, m = cases.start_case()
    ref = cases.reference(p, v, m, 2, H, 8, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and cases.decisions_are_clear(ref, m) and sorted(np.nonzero(ref.fate)[0].tolist()) == [20, 21, 22]
    p, v, R, _ = cases.scene(50, 3, hit_steps=(), escape_steps=())
    p[30, :3], v[30, :3] = p[31, :3], v[31, :3]
    R[:] = 0.01
    ref = cases.reference(p, v, 3, 3, H, 6, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and not ref.fate.any() and cases.decisions_are_clear(ref, 3)
    p, v, R, n, m = cases.massive_stop_case()
    ref = cases.reference(p, v, m, 8, H, 0, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == fref.COLLISION and ref.pair == (1, 2) and ref.steps == 3 and cases.decisions_are_clear(ref, m)
    alone = cases.reference(p[:m], v[:m], m, 8, H, 0, 0.0, radii=R[:m], escape_radius=RE)
    assert (alone.reason, alone.pair, alone.steps) == (ref.reason, ref.pair, ref.steps)
