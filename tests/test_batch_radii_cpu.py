"""CPU-only: per-body collision radii for Hermite batches (nbody_batch_radii_set, include/nbody_batch_radii.h).  The entry
points are declared by nbody.h (through the header it includes), mirrored in _lib in a list of their own, exported by the
library and by the RCCL test-double build and wrapped by BatchedSystem and nbody::Batch; NULL handles and bad radii are
refused without a device; the fp64 reference (hermite_radii_ref) with radii R_c / 2 everywhere is the uniform rule's
reference up to the first merger, conserves mass and momentum across mergers, and tells the GPU tests' inputs from the uniform
rule with R_c = 2 max R and with R_c = 2 min R."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hermite_merge_ref as mref
import hermite_radii_ref as rref
import hermite_ref
import hermite_stop_ref as sref
import test_batch_radii_gpu as cases
from conftest import ROOT

RADII_NAMES = ["nbody_batch_radii_set", "nbody_batch_radii_read"]
ETA = cases.ETA


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def preprocessed_header():
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(ROOT, "include", "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return res.stdout


def test_the_entry_points_are_declared_mirrored_exported_and_refuse_null_handles_without_a_device(lib):
    from n_body_problem_amd import _lib
    text = open(os.path.join(ROOT, "include", "nbody_batch_radii.h")).read()
    assert set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == set(RADII_NAMES)
    assert set(_lib.radii_names()) == set(RADII_NAMES)
    assert set(RADII_NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", preprocessed_header()))
    assert not set(RADII_NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                                   set(_lib.merge_exported_names()))
    for name in RADII_NAMES:
        assert hasattr(lib, name), name
    sys.path.insert(0, os.path.join(ROOT, "tests", "fake_rccl"))
    import build_fake_rccl
    fake = ctypes.CDLL(build_fake_rccl.build())
    for name in RADII_NAMES:
        assert hasattr(fake, name), name
    buf = (ctypes.c_float * 4)()
    assert lib.nbody_batch_radii_set(None, buf) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_radii_set: batch is NULL" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_radii_set(None, None) == _lib.NBODY_ERR_INVALID
    assert lib.nbody_batch_radii_read(None, buf) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_radii_read: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_abi_stays_at_version_5_and_the_headers_no_longer_call_radii_out_of_scope(lib):
    assert lib.nbody_abi_version() == 5
    nbody_h = open(os.path.join(ROOT, "include", "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_merge.h"') < nbody_h.index('#include "nbody_batch_radii.h"')
    for header in ("nbody.h", "nbody_batch_stop.h", "nbody_batch_merge.h"):
        text = " ".join(open(os.path.join(ROOT, "include", header)).read().replace(" *", " ").split())
        assert "no per-body radii" not in text and "Out of scope: per-body radii" not in text, header
        assert not re.search(r"Per-body radii[^.]*are out of scope", text), header
        assert "nbody_batch_radii.h" in text, header


def test_bad_radii_below_the_count_are_refused_with_a_message_and_the_same_values_beyond_it_are_accepted(tmp_path):
    """nbody_batch_radii_set's check is a HIP-free header of its own: a program that needs no device runs it."""
    src = tmp_path / "radii_check.cpp"
    src.write_text(r'''
#include "nbody_batch_radii_check.h"
#include <cstdio>
#include <limits>
#include <vector>
int main() {
    const int counts[3] = {4, 2, 0};
    const float bad[3] = {-1.0f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    std::vector<float> ok(12, 0.5f);
    ok[3] = 0.0f;
    std::string msg = "untouched";
    bool good = nbody::batch_radii_ok(ok.data(), counts, 3, 4, &msg);
    std::printf("%d %s\n", (int)good, msg.c_str());
    for (float b : bad) {
        std::vector<float> r = ok;
        r[4 + 1] = b;   // system 1, slot 1: below its count of 2
        msg.clear();
        good = nbody::batch_radii_ok(r.data(), counts, 3, 4, &msg);
        std::printf("%d %s\n", (int)good, msg.c_str());
        r = ok;
        r[4 + 2] = b;   // system 1, slot 2 and system 2, slot 0: beyond their counts
        r[8] = b;
        msg.clear();
        good = nbody::batch_radii_ok(r.data(), counts, 3, 4, &msg);
        std::printf("%d %s\n", (int)good, msg.c_str());
    }
    std::printf("%d\n", (int)nbody::batch_radii_ok(bad, counts, 1, 4, nullptr));
    return 0;
}
''')
    exe = tmp_path / "radii_check"
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "n_body_problem_amd", "csrc"), str(src),
                          "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "1 untouched"
    for k in range(3):
        assert out[1 + 2 * k].startswith("0 radius of system 1, slot 1 (") and "finite and >= 0" in out[1 + 2 * k], out
        assert out[2 + 2 * k] == "1 ", out
    assert out[7] == "0"


def test_the_python_wrapper_has_the_documented_signatures():
    import inspect
    import n_body_problem_amd as nb
    assert list(inspect.signature(nb.BatchedSystem.set_radii).parameters) == ["self", "radii"]
    assert list(inspect.signature(nb.BatchedSystem.radii).parameters) == ["self"]
    for method in (nb.BatchedSystem.set_stop_conditions, nb.BatchedSystem.set_collision_action):
        assert "set_radii" in method.__doc__


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_radii.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
int main() {
    try {
        nbody::Batch b(16, 64);
        b.setIntegrator(NBODY_INTEGRATOR_HERMITE);
        b.setCollisionAction(true, 4);
        b.setRadii(std::vector<float>(16 * 64, 0.01f));
        std::vector<float> r = b.radii();
        b.setRadii(std::vector<float>());
        std::printf("%lld\n", (long long)r.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_radii"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.join(ROOT, "n_body_problem_amd"), "-lnbody_amd", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def merge_triple():
    """test_batch_merge_cpu's triple: a Kepler pair (e = 0.9) and a bound third body on a wide orbit; dyadic masses."""
    pos, vel, period = hermite_ref.kepler(e=0.9)
    p = np.zeros((3, 4))
    v = np.zeros((3, 4))
    p[:2], v[:2] = pos, vel
    p[2] = [0.0, 5.0, 0.0, 0.25]
    v[2, 0] = -np.sqrt(1.25 / 5.0)
    v[:, 3] = [7.0, 8.0, 9.0]
    return p, v, period


def test_without_radii_the_reference_is_the_merge_reference_itself():
    p, v, period = merge_triple()
    for kw in (dict(collision_radius=0.3), dict(collision_radius=0.3, merge=False), dict(escape_radius=5.5), dict()):
        a = rref.evolve(p, v, 16, period / 64, levels=12, eps=1e-2, radii=None, **kw)
        b = mref.evolve(p, v, 16, period / 64, levels=12, eps=1e-2, **kw)
        assert np.array_equal(a.pos, b.pos) and np.array_equal(a.vel, b.vel) and (a.steps, a.ticks, a.reason) == (b.steps, b.ticks, b.reason)


def test_radii_of_half_the_collision_radius_reproduce_the_uniform_references_exactly_up_to_the_first_merger():
    p, v, period = merge_triple()
    rc = 0.25                                                                       # 0.125 + 0.125 == 0.25 exactly
    half = np.full(3, rc / 2)
    for rounded in (False, True):
        for eps in (0.0, 1e-2):
            kw = dict(levels=12, eps=eps, round_state=rounded)
            # STOP: the whole run
            a = rref.evolve(p, v, 64, period / 64, radii=half, merge=False, **kw)
            b = sref.evolve(p, v, 64, period / 64, collision_radius=rc, **kw)
            assert a.reason == b.reason == 1 and (a.steps, a.ticks, a.level_seq, a.pair, a.separation) == \
                (b.steps, b.ticks, b.level_seq, b.pair, b.separation)
            assert np.array_equal(a.pos, b.pos) and np.array_equal(a.vel, b.vel)
            # MERGE: the merger itself, and every step up to it
            a = rref.evolve(p, v, 64, period / 64, radii=half, **kw)
            b = mref.evolve(p, v, 64, period / 64, collision_radius=rc, **kw)
            ma, mb = a.mergers[0], b.mergers[0]
            assert (ma.tick, ma.survivor, ma.absorbed, ma.count_before, ma.separation, ma.relative_speed, ma.mass_survivor) == \
                (mb.tick, mb.survivor, mb.absorbed, mb.count_before, mb.separation, mb.relative_speed, mb.mass_survivor)
            k = b.tick_seq.index(next(t for t in b.tick_seq if t >= mb.tick))
            assert a.tick_seq[:k] == b.tick_seq[:k] and a.level_seq[:k] == b.level_seq[:k] and k > 10
            assert np.array_equal(ma.momentum_after, mb.momentum_after)
            want = np.cbrt(2.0 * (rc / 2) ** 3)
            assert ma.radius_after == (float(np.float32(want)) if rounded else want)
            # nothing else comes near: the runs stay the same to the end, the grown radius notwithstanding
            assert np.array_equal(a.pos, b.pos) and a.count == b.count == 2 and a.radii.tolist() == [ma.radius_after, rc / 2, rc / 2]


def test_the_reference_conserves_mass_exactly_and_momentum_to_rounding_and_moves_the_radii_with_their_bodies():
    P, V, R = cases.growth_case()
    runs = [rref.evolve(P, V, 2, 1e-2, levels=6, radii=R)]
    P, V, R, dt_max = cases.triple_radii_case()
    runs.append(rref.evolve(P, V, 64, dt_max, levels=12, radii=R))
    P, V, R = cases.per_pair_case(65, (63, 64), (5, 40))
    runs.append(rref.evolve(P, V, 1, 1e-3, levels=4, eps=1e-2, radii=R))
    for r, n_mergers in zip(runs, (2, 1, 1)):
        assert len(r.mergers) == n_mergers
        for mg in r.mergers:
            assert abs(mg.mass_after - mg.mass_before) <= 1e-14 * mg.mass_before
            assert np.abs(mg.momentum_after - mg.momentum_before).max() <= 1e-14 * max(mg.momentum_scale, 1e-3)
            assert mg.survivor < mg.absorbed < mg.count_before
            assert mg.radius_after ** 3 == pytest.approx(mg.radius_survivor ** 3 + mg.radius_absorbed ** 3, rel=1e-14)
        n0, k = r.pos.shape[0], len(r.mergers)
        assert r.count == n0 - k
        for q, mg in enumerate(reversed(r.mergers)):                               # slots n0 - k .. n0 - 1: the most recent first
            assert r.radii[n0 - k + q] == mg.radius_absorbed and r.pos[n0 - k + q, 3] == mg.mass_absorbed


def outcome(r):
    """What tells two runs apart: the pair, the tick and the count."""
    return (r.reason, tuple(r.pair), r.ticks, r.count, [(m.tick, m.survivor, m.absorbed) for m in r.mergers])


def uniform_outcome(P, V, n_intervals, dt_max, rc, merge, **kw):
    r = mref.evolve(P, V, n_intervals, dt_max, collision_radius=rc, merge=merge, **kw)
    if not merge:
        r.count, r.mergers = P.shape[0], []
    else:
        r.pair = (0, 0)
    return outcome(r)


def radii_outcome(P, V, n_intervals, dt_max, R, merge, **kw):
    return outcome(rref.evolve(P, V, n_intervals, dt_max, radii=R, merge=merge, **kw))


def test_the_inputs_of_the_gpu_tests_tell_the_per_pair_rule_from_the_uniform_rule_with_the_largest_and_the_smallest_radius():
    inputs = []
    n, cap, wide, close = cases.PER_PAIR[0]
    P, V, R = cases.per_pair_case(n, wide, close)
    inputs.append(("per pair", P, V, R, 1, 1e-3, dict(levels=4, eps=1e-2)))
    P, V, R = cases.growth_case()
    inputs.append(("growth", P, V, R, 2, 1e-2, dict(levels=6)))                       # told apart by its mergers only
    P, V, R, dt_max = cases.kepler_radii_case()
    inputs.append(("kepler", P, V, R, 64, dt_max, dict(levels=12)))
    P, V, R, dt_max = cases.triple_radii_case()
    inputs.append(("triple", P, V, R, 64, dt_max, dict(levels=12)))
    P, V, R = cases.head_on_radii()
    inputs.append(("head on", P, V, R, 100, 1e-3, dict(levels=6, eps=1e-3)))
    for name, P, V, R, n_intervals, dt_max, kw in inputs:
        R = R.astype(np.float64)
        for merge in ((True,) if name == "growth" else (False, True)):
            got = radii_outcome(P, V, n_intervals, dt_max, R, merge, **kw)
            for rc in (2.0 * R.max(), 2.0 * R.min()):
                other = uniform_outcome(P, V, n_intervals, dt_max, rc, merge, **kw)
                assert got != other, (name, merge, rc, got)
    # every pair of PER_PAIR names the wide pair; the uniform rule with the largest radius names the close one
    for n, cap, wide, close in cases.PER_PAIR:
        P, V, R = cases.per_pair_case(n, wide, close)
        x = P[:, :3].astype(np.float64)
        assert rref.colliding_pair(x, R.astype(np.float64), 1e-2)[:2] == wide
        assert mref.closest_pair(x, 1e-2)[:2] == close
    # the one-sided pair: inside and outside differ, and a coincident pair of zero radii collides without softening
    for inside in (True, False):
        P, V, R = cases.one_sided_case(inside)
        assert (rref.colliding_pair(P[:, :3].astype(np.float64), R.astype(np.float64), 0.0)[:2] == (0, 2)) == inside
    assert rref.colliding_pair(np.zeros((2, 3)), np.zeros(2), 0.0)[:3] == (0, 1, 0.0)
