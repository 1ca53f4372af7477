"""CPU-only: accreting tracers for Hermite batches (nbody_batch_accrete_set, include/nbody_batch_accrete.h).  The header is
included by nbody.h and its two entry points are exported and bound; the choice header sets `accreting` and `accrete` exactly
where fates act, collisions are watched and the hit action is ACCRETE, with the family and the refusals unchanged; the fp64
reference (hermite_accrete_ref) is hermite_fate_ref with zero mass words, and its merger conserves mass and momentum; and
every scene of test_batch_accrete_gpu.py is run through it here: each decision, at restart evaluations too, must lie at least
MARGIN relative from its radius, and the planted events must come out."""
import ctypes
import glob
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_accrete_ref as aref
import hermite_fate_ref as fref
from conftest import ROOT

ACCRETE_NAMES = ["nbody_batch_accrete_set", "nbody_batch_accrete_read"]
H, RE, RP, ETA = aref.H, aref.RE, aref.RP, aref.ETA


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_the_fates_and_declares_its_entry_points_alone():
    include = os.path.join(ROOT, "include")
    assert declared(open(os.path.join(include, "nbody_batch_accrete.h")).read()) == set(ACCRETE_NAMES)
    for header in glob.glob(os.path.join(include, "*.h")):
        if os.path.basename(header) != "nbody_batch_accrete.h":
            assert not declared(open(header).read()) & set(ACCRETE_NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(include, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(ACCRETE_NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(include, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_fate.h"') < nbody_h.index('#include "nbody_batch_accrete.h"')


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(ROOT, "include", "nbody_batch_accrete.h")).read().replace(" *", " ").split())
    for phrase in ("NBODY_BATCH_ON_HIT_REMOVE (0", "NBODY_BATCH_ON_HIT_ACCRETE (1)", "ABI version 5", "unknown hit action",
                   "ascending index", "fma(m_i, u_i, m_t u_t) / (m_t + m_i)", "cbrt(R_t^3 + R_i^3)", "+0.0f", "not validated",
                   "min(levels, max(L*, L_tick))", "accretes nothing", "NBODY_ERR_STATE", "zeroed exactly where the fates are",
                   "has a zero mass word", "evolve(a) followed by evolve(b) is evolve(a + b)", "nbody_batch_evolve_launch_steps",
                   "Out of scope", "mergers among massive bodies", "nbody_batch_step_n_*", "first accretion", "fragmentation",
                   "a log of accretion events"):
        assert phrase in text, phrase


def test_the_names_are_mirrored_in_a_list_of_their_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert set(_lib.accrete_names()) == set(ACCRETE_NAMES)
    assert not set(ACCRETE_NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                                     set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                                     set(_lib.fate_names()))
    assert (_lib.BATCH_ON_HIT_REMOVE, _lib.BATCH_ON_HIT_ACCRETE) == (0, 1)
    for name in ACCRETE_NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchAccreteConfig) == ctypes.sizeof(ctypes.c_int)


def test_the_abi_stays_at_version_5_and_null_handles_and_bad_actions_are_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    good, bad = _lib.BatchAccreteConfig(1), _lib.BatchAccreteConfig(2)
    assert lib.nbody_batch_accrete_set(None, ctypes.byref(good)) == _lib.NBODY_ERR_INVALID
    assert b"unknown hit action" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_accrete_set(None, None) == _lib.NBODY_ERR_INVALID
    assert lib.nbody_batch_accrete_set(None, ctypes.byref(bad)) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_accrete_set: unknown hit action" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_accrete_read(None, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_accrete_read: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_signatures():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    assert list(inspect.signature(nb.BatchedSystem.set_hit_action).parameters) == ["self", "action"]
    assert list(inspect.signature(nb.BatchedSystem.accretions).parameters) == ["self"]
    assert list(inspect.signature(nb.AccretionResult.__init__).parameters) == ["self", "given", "count"]
    assert "AccretionResult" in batch.__all__ and batch.HIT_ACTIONS == {"remove": 0, "accrete": 1}
    for word in ("remove", "accrete", "mass word", "accretions"):
        assert word in nb.BatchedSystem.set_hit_action.__doc__
    assert "unless :meth:`set_tracer_action` opts in" not in nb.BatchedSystem.set_massive_counts.__doc__


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_accrete.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
int main() {
    try {
        nbody::Batch b(16, 64);
        b.setMassiveCounts(std::vector<std::int64_t>(16, 2));
        b.setTracerAction(true);
        b.setHitAction(true);
        nbody::Batch::Accretions a = b.accretions();
        b.setHitAction(false);
        std::printf("%lld %lld\n", (long long)a.given.size(), (long long)a.count.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_accrete"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
           "-L" + os.path.join(ROOT, "n_body_problem_amd"), "-lnbody_amd", "-L/opt/rocm/lib",
           "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ---- the choice -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("accrete_choice") / "driver"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "n_body_problem_amd", "csrc"),
           os.path.join(ROOT, "tests", "batch_accrete_choice_driver.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def test_the_choice_sets_accreting_and_accrete_exactly_by_the_rule_and_changes_no_family_and_no_refusal(driver):
    settings = list(itertools.product((0, 2), (0, 1), (0, 1), ("0", "0.05"), ("0", "6"), (0, 1), (0, 1), (64, 700, 4096), ("0", "0.01")))
    lines = []
    for integ, massive, radii, rc, re_, coll, tracer, cap, eps in settings:
        for hit in (0, 1):
            lines.append(f"{integ} {massive} {radii} {rc} {re_} {coll} {tracer} {hit} {cap} {eps}")
    res = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = res.stdout.splitlines()
    assert len(out) == len(lines)
    seen = set()
    for k, (integ, massive, radii, rc, re_, coll, tracer, cap, eps) in enumerate(settings):
        remove, accrete = out[2 * k].split("|"), out[2 * k + 1].split("|")
        collisions = float(rc) > 0 or radii == 1
        fates = massive == 1 and tracer == 1 and (collisions or float(re_) > 0)
        want = fates and collisions
        assert remove[:4] == [str(int(fates)), "0", str(int(fates)), "0"], lines[2 * k]
        assert accrete[:4] == [str(int(fates)), str(int(want)), str(int(fates)), str(int(want))], lines[2 * k + 1]
        assert remove[4:] == accrete[4:], lines[2 * k]            # the shape, the LDS and the refusal with its message
        seen.add((want, accrete[8].split(":")[0]))
        if fates and coll == 1 and collisions and integ == 2 and not (radii == 1 and float(rc) > 0):
            assert "MERGE together with massive counts" in accrete[8] and accrete[8] == remove[8]
    assert (True, "0") in seen and (False, "0") in seen and len({status for _, status in seen}) == 2   # run and refused, both


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels,chunk", [(0, 5), (8, 3)])
def test_with_zero_mass_words_the_reference_is_the_fate_reference(levels, chunk):
    p, v, R, plan, _ = aref.fixed_step_case(64, 50, 3, zero=True)
    for eps in (0.0, 1e-2):
        kw = dict(levels=levels, eta=ETA, eta_start=ETA, eps=eps, radii=R, escape_radius=RE, round_state=True)
        want = fref.evolve(p, v, 3, chunk, H, **kw)
        got = aref.evolve(p, v, 3, chunk, H, **kw)
        assert np.array_equal(got.pos, want.pos) and np.array_equal(got.vel, want.vel)
        assert got.level_seq == want.level_seq and got.tick_seq == want.tick_seq and got.clamped == want.clamped
        for name in ("fate", "fate_tick", "fate_target", "fate_separation", "fate_speed", "fate_step"):
            assert np.array_equal(getattr(got, name), getattr(want, name)), name
        assert got.hit == want.hit >= 2 and got.escaped == want.escaped and got.accretions == 0 and not got.given.any()
        assert not got.restart_seq and np.array_equal(got.radii, R.astype(np.float64))


def test_a_merger_conserves_the_pairs_mass_and_momentum():
    rng = np.random.default_rng(3)
    for _ in range(20):
        P, V = rng.normal(size=(2, 4)), rng.normal(size=(2, 4))
        P[:, 3] = [1e-3 * rng.uniform(0.5, 2.0), 1e-5 * rng.uniform(0.5, 2.0)]
        mass, mom, com = P[:, 3].sum(), (P[:, 3:4] * V[:, :3]).sum(0), (P[:, 3:4] * P[:, :3]).sum(0)
        tracer = (P[1].copy(), V[1].copy())
        aref.merge_onto(P, V, 0, 1, lambda u: u)
        assert abs(P[0, 3] - mass) <= 1e-15 * mass and P[1, 3] == 0.0
        assert np.allclose(P[0, 3] * V[0, :3], mom, rtol=1e-13, atol=1e-18) and np.allclose(P[0, 3] * P[0, :3], com, rtol=1e-13, atol=1e-18)
        assert np.array_equal(P[1, :3], tracer[0][:3]) and np.array_equal(V[1], tracer[1])
    P, V = np.array([[1.0, 0, 0, 2.0], [3.0, 0, 0, -2.0]]), np.zeros((2, 4))
    aref.merge_onto(P, V, 0, 1, lambda u: u)
    assert P[0, 0] == 2.0 and P[0, 3] == 0.0                           # a zero sum of the masses: the arithmetic mean


def test_a_run_conserves_the_total_mass_and_follows_the_planted_order():
    p, v, R, plan, _ = aref.fixed_step_case(64, 50, 3)
    ref = aref.reference(p, v, 3, 5, H, 0, 0.0, radii=R, escape_radius=RE)
    hitters = sorted(r for r, (kind, _) in plan.items() if kind == "hit")
    assert [e[1] for e in ref.events] == hitters and [e[2] for e in ref.events] == [2] * 3 and ref.accretions == 3
    assert abs(ref.pos[:, 3].sum() - p[:, 3].astype(np.float64).sum()) <= 3 * 2.0 ** -24 * 1e-3
    total = np.float32(p[2, 3])
    for r in hitters:
        total = np.float32(total + p[r, 3])
    assert ref.pos[2, 3] == float(total) and np.array_equal(ref.given[hitters], p[hitters, 3].astype(np.float64))
    assert not ref.pos[hitters, 3].any() and np.count_nonzero(ref.given) == 3


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,n,m", [(64, 50, 3), (128, 100, 1), (1024, 700, 3), (4096, 3000, 3)])
def test_the_zero_mass_inputs_decide_clearly(cap, n, m):
    p, v, R, plan, _ = aref.fixed_step_case(cap, n, m, zero=True)
    for eps in (0.0, 1e-2):
        ref = aref.reference(p, v, m, 5, H, 0, eps, radii=R, escape_radius=RE)
        assert ref.reason == 0 and aref.decisions_are_clear(ref) and ref.accretions == 0
        assert {int(i): int(ref.fate_step[i]) for i in np.nonzero(ref.fate)[0]} == {r: s for r, (_, s) in plan.items()}


@pytest.mark.parametrize("cap,n,m", [(64, 50, 3), (128, 100, 3), (1024, 700, 3)])
def test_the_fixed_step_inputs_decide_clearly_at_every_evaluation_and_yield_the_planted_events(cap, n, m):
    p, v, R, plan, _ = aref.fixed_step_case(cap, n, m)
    for chunk in (5, 7, 3):                                            # the runs of the fixed-step, chunking and refusal tests
        ref = aref.reference(p, v, m, chunk, H, 0, 0.0, radii=R, escape_radius=RE)
        assert ref.reason == 0 and aref.decisions_are_clear(ref)
        assert "restart" in ref.eval_kind and len(ref.touch_seq) == chunk + 1 + len(ref.restart_seq)
        assert {int(i): int(ref.fate_step[i]) for i in np.nonzero(ref.fate)[0]} == {r: s for r, (_, s) in plan.items() if s <= chunk}
        assert [e[1] for e in ref.events] == sorted(r for r, (kind, s) in plan.items() if kind == "hit" and s <= chunk)
    for max_steps in (3,):                                             # out of steps in the middle, as the refusal test runs it
        ref = aref.reference(p, v, m, 5, H, 0, 0.0, radii=R, escape_radius=RE, max_steps=max_steps)
        assert aref.decisions_are_clear(ref)


def test_the_pair_input_brings_two_tracers_of_different_waves_to_one_target_at_one_evaluation():
    p, v, R, n, m, rows = aref.pair_case()
    ref = aref.reference(p, v, m, 4, H, 0, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and aref.decisions_are_clear(ref)
    assert [(e[0], e[1], e[2]) for e in ref.events] == [(2, 3, 2), (2, 699, 2)] and len(ref.restart_seq) == 1
    assert rows[0] // 64 != (rows[1] % 256) // 64                      # 256 threads, four rows per lane: waves 0 and 2
    M, a, b = p[2, 3], p[3, 3], p[699, 3]
    assert np.float32(np.float32(M + a) + b) != np.float32(np.float32(M + b) + a)
    assert ref.pos[2, 3] == float(np.float32(np.float32(M + a) + b))


def test_the_adaptive_input_accretes_at_a_tick_no_coarse_step_divides_and_a_dead_vote_would_show():
    p, v, R, n, m = aref.adaptive_case()
    ref = aref.reference(p, v, m, 24, H, 8, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and aref.decisions_are_clear(ref) and ref.ticks == 24 << 8
    assert ref.fate[10] == fref.HIT and ref.fate_tick[10] == 0 and ref.given[10] == 0.0 and ref.accretions == 3 and ref.escaped == 1
    assert any(tick % (1 << 8) for tick, _, _, _ in ref.restart_seq)
    assert all(level >= floor_level and level >= want for _, want, floor_level, level in ref.restart_seq)
    with_vote = aref.reference(p, v, m, 24, H, 8, 0.0, radii=R, escape_radius=RE, dead_votes=True)
    # row 10, dead from the start, asks every restart for the finest level: three levels finer than the live rows at each of
    # the three restarts, and every level costs at least one step on the way back
    assert all(w[1] == 8 and w[3] >= r[3] + 3 for w, r in zip(with_vote.restart_seq, ref.restart_seq))
    assert with_vote.steps >= ref.steps + 9


def test_the_chain_start_and_stop_inputs_decide_clearly():
    p, v, R, n, m, (t, A, B) = aref.chain_case()
    ref = aref.reference(p, v, m, 3, H, 0, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and aref.decisions_are_clear(ref)
    assert [(e[0], e[1], e[2]) for e in ref.events] == [(1, A, t), (1, B, t)] and ref.eval_kind[:4] == ["start", "step", "restart", "restart"]
    assert ref.fate_eval[A] == 1 and ref.fate_eval[B] == 2 and ref.fate_tick[A] == ref.fate_tick[B] == 1
    once = np.float32(np.cbrt(float(R[t]) ** 3 + float(R[A]) ** 3))
    assert ref.radii[t] == float(np.float32(np.cbrt(float(once) ** 3 + float(R[B]) ** 3)))
    removing = aref.reference(p, v, m, 3, H, 0, 0.0, radii=R, escape_radius=RE, accrete=False)
    assert aref.decisions_are_clear(removing) and removing.fate[A] == fref.HIT and removing.fate[B] == 0
    p, v, R, n, m, (t, A, B) = aref.chain_case(shared=True)
    ref = aref.reference(p, v, m, 3, H, 0, 0.0, collision_radius=0.02, escape_radius=RE)
    assert ref.reason == 0 and aref.decisions_are_clear(ref) and ref.fate[A] == fref.HIT and ref.fate[B] == 0 and ref.accretions == 1
    p, v, R, n, m = aref.start_case()
    ref = aref.reference(p, v, m, 2, H, 8, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == 0 and aref.decisions_are_clear(ref)
    assert [(e[0], e[1], e[2]) for e in ref.events] == [(0, 20, 1), (0, 22, 2)] and ref.fate[21] == fref.ESCAPED
    assert ref.restart_seq == [(0, ref.level_seq[0], 0, ref.level_seq[0])]
    voting = aref.reference(p, v, m, 2, H, 8, 0.0, radii=R, escape_radius=RE, dead_votes=True)
    assert voting.level_seq[0] > ref.level_seq[0]                     # tracer 20's |a| / |j| alone would refine the first step
    p, v, R, n, m = aref.massive_stop_case()
    ref = aref.reference(p, v, m, 8, H, 0, 0.0, radii=R, escape_radius=RE)
    assert ref.reason == fref.COLLISION and ref.pair == (1, 2) and ref.steps == 3 and aref.decisions_are_clear(ref)
    assert ref.fate[12] == fref.HIT and ref.fate_step[12] == 3 and ref.fate_step[13] == 1 and ref.accretions == 0 and p[12, 3] > 0
    alone = aref.reference(p[:m], v[:m], m, 8, H, 0, 0.0, radii=R[:m], escape_radius=RE)
    assert (alone.reason, alone.pair, alone.steps) == (ref.reason, ref.pair, ref.steps)
