"""CPU-only: external fields for Hermite batches (nbody_batch_field_set, include/nbody_batch_field.h).  The header is
self-contained C99, included by nbody.h, and its three entry points are exported and bound; the choice header keeps every
choice it made without a field (the recorded table of test_batch_choice_cpu.py), runs a field through the same family, shape
and LDS, and refuses it with conditions and with fixed steps, after the older refusals; batch_field_component_error is walked
over the edges of every domain; the fp64 reference (hermite_field_ref) has accelerations and jerks that are the derivatives of
its potentials, is hermite_adaptive_ref without components, and keeps the energy of the orbit the GPU suite runs."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_adaptive_ref as aref
import hermite_field_ref as fref
from conftest import ROOT
from test_batch_choice_cpu import domain, golden, parse  # noqa: F401  (golden: the fixture with the recorded choices)

FIELD_NAMES = ["nbody_batch_field_set", "nbody_batch_field_read", "nbody_batch_field_potential"]
INCLUDE = os.path.join(ROOT, "include")
F32 = lambda x: float(np.float32(x))  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_the_accretions_and_declares_its_entry_points_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_field.h")).read()) == set(FIELD_NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_field.h":
            assert not declared(open(header).read()) & set(FIELD_NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(FIELD_NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_accrete.h"') < nbody_h.index('#include "nbody_batch_field.h"')


def test_the_header_is_self_contained_c99(tmp_path):
    src = tmp_path / "field.c"
    src.write_text(r'''
#include "nbody.h"
typedef char component_is_16_bytes[sizeof(nbody_batch_field_component) == 16 ? 1 : -1];
int main(void) {
    nbody_batch_field_component c[NBODY_BATCH_FIELD_MAX_COMPONENTS] = {{NBODY_BATCH_FIELD_PLUMMER, {1.0f, 0.1f, 0.0f}},
                                                                       {NBODY_BATCH_FIELD_LOG_HALO, {1.0f, 0.1f, 0.9f}},
                                                                       {NBODY_BATCH_FIELD_MIYAMOTO_NAGAI, {1.0f, 0.5f, 0.05f}},
                                                                       {NBODY_BATCH_FIELD_NONE, {0.0f, 0.0f, 0.0f}}};
    int n = 0;
    return (nbody_batch_field_set(0, c, 4) != NBODY_ERR_INVALID) + (nbody_batch_field_read(0, c, &n) != NBODY_ERR_INVALID) +
           (nbody_batch_field_potential(0, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_field.h")).read().replace(" *", " ").split())
    for phrase in ("NBODY_BATCH_FIELD_MAX_COMPONENTS = 4", "ABI version 5", "no new status", "coordinate origin", "G = 1",
                   "forgets what nbody_batch_massive_set forgets", "names the function, the system, the component and the value",
                   "A refused call changes nothing", "PREDICTED state", "v_rsq_f32", "v_rcp_f32", "b^2 in place of eps^2", ">= NBODY_MIN_SOFTENING", "a = fmaf(d, s, a), j = fmaf(fmaf(-c, d, e), s, j)",
                   "D = fmaf(zw, z, fmaf(y, y, fmaf(x, x, rc rc)))", "mu = (M iD) iD2", "ascending component order",
                   "not added as zero", "bit for bit", "reads no mass word", "nbody_batch_energy stays exactly what it is",
                   "levels = 0 gives fixed steps", "nbody_batch_step_n_*", "Out of scope", "condition, fate and accrete kernels",
                   "KDK and kick-drift", "off-centre, moving, rotating or time-dependent", "Hernquist, NFW or a tidal tensor"):
        assert phrase in text, phrase


def test_the_names_are_mirrored_in_a_list_of_their_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert set(_lib.field_names()) == set(FIELD_NAMES)
    assert not set(FIELD_NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                                   set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                                   set(_lib.fate_names()) | set(_lib.accrete_names()))
    assert (_lib.BATCH_FIELD_NONE, _lib.BATCH_FIELD_PLUMMER, _lib.BATCH_FIELD_LOG_HALO, _lib.BATCH_FIELD_MIYAMOTO_NAGAI) == (0, 1, 2, 3)
    assert _lib.BATCH_FIELD_MAX_COMPONENTS == 4
    for name in FIELD_NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchFieldComponent) == 16


def test_the_abi_stays_at_version_5_and_null_handles_are_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    comp = (_lib.BatchFieldComponent * 1)()
    n = ctypes.c_int(0)
    assert lib.nbody_batch_field_set(None, comp, 1) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_field_set: batch is NULL" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_field_set(None, None, 0) == _lib.NBODY_ERR_INVALID
    assert lib.nbody_batch_field_read(None, comp, ctypes.byref(n)) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_field_read: batch is NULL" in lib.nbody_batch_last_error(None)
    assert lib.nbody_batch_field_potential(None, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_field_potential: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_signatures():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    assert list(inspect.signature(nb.BatchedSystem.set_external_field).parameters) == ["self", "components"]
    for name in ("external_field", "field_potential", "field_energy"):
        assert list(inspect.signature(getattr(nb.BatchedSystem, name)).parameters) == ["self"], name
    assert batch.FIELD_KINDS == {"none": 0, "plummer": 1, "log_halo": 2, "miyamoto_nagai": 3} and "FIELD_KINDS" in batch.__all__
    assert batch.FIELD_KINDS == fref.KINDS
    for word in ("plummer", "log_halo", "miyamoto_nagai", "None", "levels=0", "step_n"):
        assert word in nb.BatchedSystem.set_external_field.__doc__, word


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_field.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
int main() {
    try {
        nbody::Batch b(16, 64);
        std::vector<nbody_batch_field_component> c(16 * 2);
        for (size_t i = 0; i < c.size(); ++i)
            c[i] = i % 2 ? nbody_batch_field_component{NBODY_BATCH_FIELD_LOG_HALO, {1.f, 0.1f, 0.9f}}
                         : nbody_batch_field_component{NBODY_BATCH_FIELD_PLUMMER, {1.f, 0.1f, 0.f}};
        b.setField(c, 2);
        std::vector<nbody_batch_field_component> back = b.field();
        std::vector<double> phi = b.fieldPotential(nullptr);
        b.setField({}, 0);
        std::printf("%lld %lld\n", (long long)back.size(), (long long)phi.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_field"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-L" + os.path.join(ROOT, "n_body_problem_amd"),
           "-lnbody_amd", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ---- the choice -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("field_choice") / "driver")
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "n_body_problem_amd", "csrc"),
           os.path.join(ROOT, "tests", "batch_field_choice_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == len(commands)
        return lines
    return run


def with_field(command, field):
    call, rest = command.split(" ", 1)
    return f"{call} {field} {rest}"


def test_without_a_field_every_choice_is_the_recorded_one(driver, golden):  # noqa: F811
    for section, commands in domain().items():
        for command, line in zip(commands, driver([with_field(c, 0) for c in commands])):
            entry, field = line.rsplit("|", 1)
            assert parse(entry) == golden[section][command] and field == "0", command


def test_with_a_field_evolve_keeps_family_shape_and_lds_and_refuses_conditions_after_the_older_refusals(driver, golden):  # noqa: F811
    commands = domain()["evolve"]
    ran, refused, older = 0, 0, 0
    for command, line in zip(commands, driver([with_field(c, 1) for c in commands])):
        entry, field = line.rsplit("|", 1)
        got, was = parse(entry), golden["evolve"][command]
        _, _, massive, radii, rc, re_, _, _, _, _ = command.split()
        conditions = float(rc) > 0 or float(re_) > 0 or radii == "1"
        assert field == "1", command
        if was["refusal"] != "none":                    # Hermite, radii with a collision radius, merge or conditions with massive
            assert got == was, command
            older += 1
        elif conditions:
            assert got["family"] == "none" and got["refusal"].startswith("-1:nbody_batch_evolve: an external field is set together "
                                                                         "with a collision radius, an escape radius, radii, "), command
            assert "nbody_batch_field_set(b, NULL, 0)" in got["refusal"]
            refused += 1
        else:
            assert got == was and got["family"] == ("adaptive_massive" if massive == "1" else "adaptive"), command
            ran += 1
    assert ran and refused and older
    assert {parse(line.rsplit("|", 1)[0])["refusal"].split(":")[0] for line in driver([with_field(c, 1) for c in commands])} == {"none", "-1"}


def test_with_a_field_fixed_steps_are_refused_for_every_integrator(driver):
    commands = domain()["step"]
    for command, line in zip(commands, driver([with_field(c, 1) for c in commands])):
        got = parse(line.rsplit("|", 1)[0])
        assert got["family"] == "none" and got["refusal"].startswith("-1:nbody_batch_step_n: an external field is set"), command
        assert "nbody_batch_evolve_on with levels = 0" in got["refusal"], command
    assert {c.split()[1] for c in commands} == {"0", "1", "2"}


@pytest.mark.parametrize("kind,p,word", [
    (0, ("nan", "-1", "inf"), None),                                   # NONE: the parameters are not read
    (1, ("1", "0", "0"), None), (1, ("0", "1e-9", "nan"), None), (1, ("1", "0.05", "-3"), None),
    (1, ("nan", "0.1", "0"), "mass"), (1, ("inf", "0.1", "0"), "mass"), (1, ("-1", "0.1", "0"), "mass"),
    (1, ("1", "nan", "0"), "scale b"), (1, ("1", "inf", "0"), "scale b"), (1, ("1", "-0.1", "0"), "scale b"),
    (1, ("1", "5e-10", "0"), "NBODY_MIN_SOFTENING"), (1, ("1", "1e-30", "0"), "NBODY_MIN_SOFTENING"),
    (2, ("1", "0.1", "0.9"), None), (2, ("0", "1e-3", "5"), None),
    (2, ("nan", "0.1", "1"), "v0"), (2, ("inf", "0.1", "1"), "v0"), (2, ("-1", "0.1", "1"), "v0"),
    (2, ("1", "0", "1"), "rc"), (2, ("1", "-0.1", "1"), "rc"), (2, ("1", "nan", "1"), "rc"), (2, ("1", "inf", "1"), "rc"),
    (2, ("1", "0.1", "0"), "q"), (2, ("1", "0.1", "-1"), "q"), (2, ("1", "0.1", "nan"), "q"), (2, ("1", "0.1", "inf"), "q"),
    (3, ("1", "0", "0.1"), None), (3, ("0", "3", "0.1"), None),
    (3, ("nan", "1", "0.1"), "mass"), (3, ("inf", "1", "0.1"), "mass"), (3, ("-1", "1", "0.1"), "mass"),
    (3, ("1", "-1", "0.1"), "scale length"), (3, ("1", "nan", "0.1"), "scale length"), (3, ("1", "inf", "0.1"), "scale length"),
    (3, ("1", "1", "0"), "scale height"), (3, ("1", "1", "-0.1"), "scale height"), (3, ("1", "1", "nan"), "scale height"),
    (3, ("1", "1", "inf"), "scale height"),
    (4, ("1", "1", "1"), "unknown kind"), (-1, ("1", "1", "1"), "unknown kind"), (1 << 20, ("1", "1", "1"), "unknown kind")])
def test_component_domains_at_their_edges(driver, kind, p, word):
    msg = driver([f"component {kind} {' '.join(p)}"])[0]
    if word is None:
        assert msg == "none"
    else:
        assert word in msg and msg != "none", msg
        assert msg.startswith({1: "PLUMMER", 2: "LOG_HALO", 3: "MIYAMOTO_NAGAI"}.get(kind, "unknown kind")), msg


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("components", [[("plummer", 2.0, 0.3, 0.0)], [("log_halo", 1.3, 0.2, 0.8)],
                                        [("miyamoto_nagai", 3.0, 0.7, 0.15)],
                                        [("plummer", 0.5, 0.0, 0.0), ("none", 9, 9, 9), ("miyamoto_nagai", 1.0, 0.0, 0.2),
                                         ("log_halo", 0.7, 0.5, 1.2)]], ids=["plummer", "log_halo", "miyamoto_nagai", "sum"])
def test_accelerations_and_jerks_are_the_derivatives_of_the_potential(components):
    rng = np.random.default_rng(20)
    x, v = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    a, j = fref.field_acc_jerk(x, v, components)
    h = 3e-6
    grad = np.zeros_like(x)
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        grad[:, c] = (fref.potential(x + e, components) - fref.potential(x - e, components)) / (2 * h)
    dadt = (fref.field_acc_jerk(x + h * v, v, components)[0] - fref.field_acc_jerk(x - h * v, v, components)[0]) / (2 * h)
    ea = (np.linalg.norm(-grad - a, axis=1) / np.linalg.norm(a, axis=1)).max()
    ej = (np.linalg.norm(dadt - j, axis=1) / np.linalg.norm(j, axis=1)).max()
    print(f"a against -grad Phi {ea:.3g}, j against da/dt along v {ej:.3g}")
    assert ea <= 1e-8 and ej <= 1e-8, (ea, ej)


def test_a_plummer_term_is_a_body_fixed_at_the_origin_and_the_guard_drops_the_centre():
    rng = np.random.default_rng(21)
    x, v = rng.normal(size=(30, 3)), rng.normal(size=(30, 3))
    X, V = np.vstack([np.zeros((1, 3)), x]), np.vstack([np.zeros((1, 3)), v])
    m = np.zeros(31)
    m[0] = 2.5
    for b in (0.0, 0.05):
        a, j = fref.field_acc_jerk(x, v, [("plummer", 2.5, b, 0.0)])
        pa, pj = fref.hermite_ref.acc_jerk(X, V, m, b)
        assert np.allclose(a, pa[1:], rtol=1e-13, atol=0) and np.allclose(j, pj[1:], rtol=1e-12, atol=1e-15)
    a, j = fref.field_acc_jerk(np.zeros((1, 3)), np.ones((1, 3)), [("plummer", 1.0, 0.0, 0.0)])
    assert not a.any() and not j.any() and fref.potential(np.zeros((1, 3)), [("plummer", 1.0, 0.0, 0.0)])[0] == 0.0


@pytest.mark.parametrize("round_state", [False, True])
def test_without_components_the_reference_is_the_adaptive_reference(round_state):
    rng = np.random.default_rng(22)
    pos, vel = rng.normal(size=(12, 4)), 0.3 * rng.normal(size=(12, 4))
    pos[:, 3] = rng.uniform(0.05, 0.2, size=12)
    for components in ((), [("none", 1.0, 2.0, 3.0)] * 4):
        for eps, levels in ((0.0, 8), (1e-2, 0), (1e-2, 5)):
            kw = dict(levels=levels, eta=0.02, eta_start=0.01, eps=eps, round_state=round_state)
            want = aref.evolve(pos, vel, 3, 1.0 / 64.0, **kw)
            got = fref.evolve(pos, vel, 3, 1.0 / 64.0, components=components, **kw)
            assert np.array_equal(got.pos, want.pos) and np.array_equal(got.vel, want.vel)
            assert got.level_seq == want.level_seq and got.tick_seq == want.tick_seq and got.coarsen_ticks == want.coarsen_ticks
            assert (got.steps, got.clamped, got.ticks, got.level) == (want.steps, want.clamped, want.ticks, want.level)


def test_massive_counts_in_the_reference_are_zero_mass_columns_and_the_field_moves_the_tracers():
    rng = np.random.default_rng(23)
    pos, vel = rng.normal(size=(9, 4)), 0.3 * rng.normal(size=(9, 4))
    pos[:, 3] = 0.1
    zeroed = pos.copy()
    zeroed[3:, 3] = 0.0
    comps = [("miyamoto_nagai", 1.0, 0.5, 0.1)]
    got = fref.evolve(pos, vel, 2, 1.0 / 32.0, levels=6, eps=1e-2, components=comps, massive=3)
    want = fref.evolve(zeroed, vel, 2, 1.0 / 32.0, levels=6, eps=1e-2, components=comps)
    assert np.array_equal(got.pos[:, :3], want.pos[:, :3]) and np.array_equal(got.vel, want.vel) and got.level_seq == want.level_seq
    assert np.array_equal(got.pos[:, 3], pos[:, 3])                                   # the mass words are carried
    off = fref.evolve(pos, vel, 2, 1.0 / 32.0, levels=6, eps=1e-2, massive=3)
    assert np.abs(got.pos[3:, :3] - off.pos[3:, :3]).max() > 1e-5


def test_the_halo_orbit_of_the_gpu_suite_keeps_its_specific_energy_in_the_reference():
    """One tracer (massive count 0) in LOG_HALO(v0 = 1, rc = 0.1, q = 0.9), from (3, 0, 0.6) with (0, 0.3, 0.05) -- apocentre,
    0.3 of the circular speed --, 320 intervals of dt_max = 1/8 (t = 40), levels = 12, eta = eta_start = 0.01: the scheme keeps
    v^2 / 2 + Phi to 1e-5 relative in fp64 (measured 3.8e-7 over 839 steps) and with the fp32 rounding of the state too
    (1.6e-6), so that the 1e-4 the GPU test asks of the kernel is the kernel's to meet."""
    e0 = fref.specific_energy(fref.ORBIT_POS, fref.ORBIT_VEL, fref.HALO)[0]
    assert 1.0 < e0 < 1.3
    radii = []
    for round_state in (False, True):
        r = fref.evolve(fref.ORBIT_POS, fref.ORBIT_VEL, fref.ORBIT_INTERVALS, fref.ORBIT_DT_MAX, levels=fref.ORBIT_LEVELS,
                        eta=F32(fref.ORBIT_ETA), eta_start=F32(fref.ORBIT_ETA), components=fref.HALO, massive=0,
                        round_state=round_state)
        de = abs(fref.specific_energy(r.pos, r.vel, fref.HALO)[0] / e0 - 1.0)
        print(f"round_state {round_state}: {r.steps} steps, levels {min(r.level_seq)}..{max(r.level_seq)}, dE/E {de:.3g}")
        assert r.ticks == fref.ORBIT_INTERVALS << fref.ORBIT_LEVELS and r.clamped == 0
        assert de <= 1e-5, de
        assert max(r.level_seq) - min(r.level_seq) >= 3                                # eccentric: the step really adapts
        radii.append(np.linalg.norm(r.pos[0, :3]))
    assert abs(radii[0] - radii[1]) < 1e-3
