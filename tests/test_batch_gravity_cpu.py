"""CPU-only: gravity at points of batched ensembles (nbody_batch_gravity, include/nbody_batch_gravity.h).  The header is
self-contained C99, included by nbody.h after the hierarchy header, and declares its one entry point alone; it is exported, bound
and listed apart; the arithmetic without a GPU (csrc/nbody_batch_gravity_math.h), built into a stand-alone driver with g++ (and
once more with the address and undefined-behaviour sanitizers), gives the hand-worked field of one source, the Plummer closed
forms, and on a 64-body sphere the numpy reference (hermite_gravity_ref) within the bands of fp32 terms and chains; the launch
plan serves every row exactly once; and the reference's tensor is the derivative of its acceleration, with the trace the header
states."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_gravity_ref as gref
from conftest import ROOT

NAMES = ["nbody_batch_gravity"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
PLAN_ROWS = (1, 63, 64, 65, 1024, 1025, 4097, 1048576)


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_hierarchy_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_gravity.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_gravity.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_hierarchy.h"') < nbody_h.index('#include "nbody_batch_gravity.h"')


def test_the_header_is_self_contained_c99_and_the_record_is_24_bytes(tmp_path):
    src = tmp_path / "gravity.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char record_is_24_bytes[sizeof(nbody_batch_gravity_record) == 24 ? 1 : -1];
typedef char acceleration_at_0[offsetof(nbody_batch_gravity_record, acceleration) == 0 ? 1 : -1];
typedef char reserved_at_12[offsetof(nbody_batch_gravity_record, reserved) == 12 ? 1 : -1];
typedef char potential_at_16[offsetof(nbody_batch_gravity_record, potential) == 16 ? 1 : -1];
typedef char limit[NBODY_BATCH_GRAVITY_MAX_POINTS == 1048576 ? 1 : -1];
int main(void) {
    nbody_batch_gravity_record r;
    return (nbody_batch_gravity(0, 0, 0, 0, 0, 0.0f, &r, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_gravity.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_hierarchy.h", "The sources are the bodies j < m",
                   "m = min(massive[s], counts[s])", "otherwise m = counts[s]", "Test particles are never sources",
                   "their mass words are not read", "n_systems x n_points x 4 floats {x, y, z, ignored}",
                   "[1, NBODY_BATCH_GRAVITY_MAX_POINTS]", "values in [0, n_points]", "NULL means every system has n_points",
                   "feels all m sources", "n_points must be 0 and host_point_counts NULL", "test particles included",
                   "max_bodies entries per system", "skipped by index", "inv = 0 for that column", "All fp32",
                   "every fmaf one fused operation", "r2 = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, eps2)))", "inv = rsq(r2)",
                   "below 2^-84", "adds nothing to any output", "mi = m_j inv", "inv2 = inv inv", "s = mi inv2",
                   "a = fmaf(d, s, a) per component", "in ascending j, starting at +0", "sum += (double)mi in ascending j in fp64",
                   "potential = 0.0 - sum", "only when tidal_out != NULL", "{xx, xy, xz, yy, yz, zz}",
                   "the exact derivative of the softened acceleration", "u = (3.f s) inv2", "p_a = u d_a",
                   "t_ab = fmaf(p_a, d_b, t_ab) for a <= b", "tr = tr + s", "each become t - tr", "the empty record, all zero",
                   "A system with m = 0 gives +0 everywhere", "synchronous", "allocated on first use, grown when a call needs more",
                   "freed in nbody_batch_destroy", "forgets nothing", "bit for bit", "the row's coordinates alone",
                   "the slot, n_systems, max_bodies or the launch shape", "nbody_batch_energy's rule", "names the function",
                   "a NULL handle", "NULL records_out", "n_points outside its range",
                   "n_points or host_point_counts given without points", "a point count outside [0, n_points]", "a bad softening",
                   "refused before any device work", "Out of scope", "the external field of nbody_batch_field.h", "jerks",
                   "device-side outputs", "a frame other than the state's"):
        assert phrase in text, phrase
    # the hierarchy header, which this one follows, is as it was
    assert "nbody_batch_gravity" not in open(os.path.join(INCLUDE, "nbody_batch_hierarchy.h")).read()


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert _lib.gravity_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                             set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                             set(_lib.fate_names()) | set(_lib.accrete_names()) | set(_lib.field_names()) | set(_lib.pairs_names()) |
                             set(_lib.structure_names()) | set(_lib.members_names()) | set(_lib.hierarchy_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchGravityRecord) == 24
    assert [f[0] for f in _lib.BatchGravityRecord._fields_] == ["acceleration", "reserved", "potential"]
    assert _lib.BatchGravityRecord.reserved.offset == 12 and _lib.BatchGravityRecord.potential.offset == 16
    assert _lib.BATCH_GRAVITY_MAX_POINTS == 1048576


def test_the_abi_stays_at_version_5_and_a_null_handle_is_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchGravityRecord * 1)()
    assert lib.nbody_batch_gravity(None, None, None, 0, None, 0.0, out, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_gravity: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_surface():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    sig = inspect.signature(nb.BatchedSystem.gravity_at)
    assert list(sig.parameters) == ["self", "points", "softening", "tidal", "point_counts"]
    assert [sig.parameters[p].default for p in ("points", "softening", "tidal", "point_counts")] == [None, 1e-2, False, None]
    assert {"GravityResult", "GRAVITY_RECORD_DTYPE"} <= set(batch.__all__) and nb.GravityResult is batch.GravityResult
    assert "GravityResult" in nb.__all__ and batch.GravityResult.__doc__
    assert batch.GRAVITY_RECORD_DTYPE.itemsize == 24 and batch.GRAVITY_RECORD_DTYPE.fields["potential"][1] == 16
    # a result built by hand: one system of two rows
    rec = np.zeros((1, 2), dtype=batch.GRAVITY_RECORD_DTYPE)
    rec[0, 0] = ((-0.25, 0.0, 0.5), 0.0, -0.5)
    tid = np.zeros((1, 2, 6), dtype=np.float32)
    tid[0, 0] = [1, 2, 3, 4, 5, 6]
    res = batch.GravityResult(rec, tid)
    assert res.acceleration.shape == (1, 2, 3) and res.acceleration.dtype == np.float32 and res.acceleration[0, 0].tolist() == [-0.25, 0.0, 0.5]
    assert res.potential.shape == (1, 2) and res.potential.dtype == np.float64 and res.potential[0].tolist() == [-0.5, 0.0]
    assert res.tidal.shape == (1, 2, 3, 3) and res.tidal.dtype == np.float32
    assert res.tidal[0, 0].tolist() == [[1, 2, 3], [2, 4, 5], [3, 5, 6]] and not res.tidal[0, 1].any()
    assert batch.GravityResult(rec, None).tidal is None


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_gravity.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
static_assert(sizeof(nbody_batch_gravity_record) == 24, "the record");
int main() {
    try {
        nbody::Batch b(16, 64);
        std::vector<float> tidal;
        std::vector<nbody_batch_gravity_record> own = b.gravityAt(nullptr, 0.01f);
        std::vector<nbody_batch_gravity_record> at = b.gravityAt(nullptr, 0.f, nullptr, 0, nullptr, tidal);
        std::printf("%lld %lld %lld\n", (long long)own.size(), (long long)at.size(), (long long)tidal.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_gravity"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-L" + os.path.join(ROOT, "n_body_problem_amd"),
           "-lnbody_amd", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_gravity_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_gravity.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_gravity_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and "1.f / sqrtf(r2)" in text
    hip = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    assert '#include "nbody_batch_gravity_math.h"' in hip
    # the kernel forms its pairs, sums, rows and empty records with the header's functions, not with copies of them
    kernel = hip[hip.index("void batch_gravity_kernel("):hip.index("hipError_t launch_batch_gravity(")]
    for call in ("gravity_pair<GUARD, TIDAL>(", "GravityRow<TIDAL>", ".add(", ".record()", ".tidal(", "gravity_empty_record()", "gravity_row("):
        assert call in kernel, call
    assert "fmaf" not in kernel and "rsqf" not in kernel and "atomic" not in kernel
    launcher = hip[hip.index("hipError_t launch_batch_gravity("):hip.index("// ---- hierarchies")]
    assert "gravity_plan_own(" in launcher and "gravity_plan_points(" in launcher and "gravity_lds_bytes(" in launcher
    # batch_forces has the callers it had: the step kernels and their massive siblings
    assert len(re.findall(r"\bbatch_forces<", open(os.path.join(CSRC, "nbody_batch.hip")).read())) == 6


# ---- the arithmetic and the plan, through the driver ------------------------------------------------------------------------
def build_driver(exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_gravity_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr, res.stdout + res.stderr
        return [[float(w) for w in line.split()] for line in res.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("gravity") / "driver"))


def field_line(eps, own, sources, rows):
    words = [repr(float(u)) for u in np.asarray(sources, np.float32).reshape(-1)] + \
            [repr(float(u)) for u in np.asarray(rows, np.float32)[:, :3].reshape(-1)]
    return f"field {float(np.float32(eps))!r} {int(own)} {len(sources)} {len(rows)} " + " ".join(words)


def unpack(out):
    out = np.array(out, dtype=np.float64)
    return out[:, :3], out[:, 3], out[:, 4:][:, [[0, 1, 2], [1, 3, 4], [2, 4, 5]]]


def test_one_source_at_the_origin_gives_the_hand_worked_field(driver):
    """Mass 1 at the origin, the point (2, 0, 0), eps = 0: every step is exact in binary.  d = (-2, 0, 0), r2 = 4, inv = 1/2,
    mi = 1/2, inv2 = 1/4, s = 1/8: a = (-1/4, 0, 0), phi = -1/2; u = 3/32, p = (-3/16, 0, 0), t_xx = 3/8, tr = 1/8:
    T = diag(1/4, -1/8, -1/8)."""
    (row,) = driver([field_line(0.0, False, [(0, 0, 0, 1)], [(2, 0, 0)])])
    assert row == [-0.25, 0.0, 0.0, -0.5, 0.25, 0.0, 0.0, -0.125, 0.0, -0.125]
    # with eps = 1/2 the Plummer closed forms, q = r^2 + eps^2 = 4.25: a_x = -2 q^-3/2, phi = -q^-1/2,
    # T_xx = 12 q^-5/2 - q^-3/2, T_yy = T_zz = -q^-3/2; each output is one term (T_xx two), so the band is TERM_BAND of them
    (row,) = driver([field_line(0.5, False, [(0, 0, 0, 1)], [(2, 0, 0)])])
    q = 4.25
    want = [-2 * q ** -1.5, 0, 0, -q ** -0.5, 12 * q ** -2.5 - q ** -1.5, 0, 0, -q ** -1.5, 0, -q ** -1.5]
    scale = [2 * q ** -1.5, 0, 0, q ** -0.5, 12 * q ** -2.5 + q ** -1.5, 0, 0, q ** -1.5, 0, q ** -1.5]
    for got, w, sc in zip(row, want, scale):
        assert abs(got - w) <= gref.TERM_BAND * sc, (got, w)
    # the reference says the same
    ref = gref.gravity(np.array([(0, 0, 0, 1)], np.float32), 1, points=np.array([(2, 0, 0)], np.float32), softening=0.5)
    assert np.allclose(ref["acceleration"][0], want[:3], rtol=1e-14) and ref["potential"][0] == pytest.approx(want[3], rel=1e-14)
    assert np.allclose(np.diag(ref["tidal"][0]), [want[4], want[7], want[9]], rtol=1e-14)
    assert np.allclose(np.diag(ref["tidal_scale"][0]), [scale[4], scale[7], scale[9]], rtol=1e-14)


def test_a_source_at_zero_distance_adds_nothing_and_the_own_row_skips_itself(driver):
    src = [(0, 0, 0, 1), (2, 0, 0, 3), (0, 1, 0, 2)]
    # eps = 0, a point exactly on source 1: the field of the other two, bit for bit
    (on,) = driver([field_line(0.0, False, src, [(2, 0, 0)])])
    (without,) = driver([field_line(0.0, False, [src[0], src[2]], [(2, 0, 0)])])
    assert on == without
    # own-bodies mode: row 1 is that point; with softening the point feels source 1's own m / eps, the body does not
    own = driver([field_line(0.0, True, src, src)])
    assert own[1] == on
    soft_own = driver([field_line(0.25, True, src, src)])
    soft_at = driver([field_line(0.25, False, src, src)])
    for i, s in enumerate(src):
        assert soft_own[i][:3] == soft_at[i][:3]                                  # the self pair has d = 0
        assert soft_own[i][3] - soft_at[i][3] == pytest.approx(s[3] / 0.25, rel=1e-6)
    # no source at all: +0 everywhere
    (empty,) = driver([field_line(0.0, False, [], [(1, 2, 3)])])
    assert empty == [0.0] * 10 and not np.signbit(empty).any()


@pytest.mark.parametrize("eps", gref.SOFTENINGS)
def test_the_drivers_fp32_rows_agree_with_the_reference_on_a_64_body_sphere(driver, eps):
    """The potential within TERM_BAND of the sum of its terms (fp32 terms, fp64 sum); the acceleration and the tensor within
    m 2^-24 + TERM_BAND of theirs (an fp32 chain of m FMAs over such terms).  Own-bodies mode and 37 points off the bodies."""
    from n_body_problem_amd import plummer
    pos = np.array(plummer(64, seed=5)[0], dtype=np.float32)
    points = (np.random.default_rng(3).normal(size=(37, 3)) * 0.8).astype(np.float32)
    for own, rows in ((True, pos), (False, points)):
        a, phi, t = unpack(driver([field_line(eps, own, pos, rows)]))
        ref = gref.gravity(pos, 64, points=None if own else points, softening=eps)
        dev = gref.deviations(a, phi, t, ref)
        print(f"eps {eps}, {'own bodies' if own else 'points'}: largest deviations {dev} of the terms; bands {gref.TERM_BAND:.3g}, {gref.band(64):.3g}")
        assert dev["potential"] <= gref.TERM_BAND and dev["acceleration"] <= gref.band(64) and dev["tidal"] <= gref.band(64)
        assert np.all(phi <= 0) and np.array_equal(t, np.swapaxes(t, 1, 2))


def test_the_plan_serves_every_row_exactly_once(driver):
    for P in PLAN_ROWS:
        (rpl, threads, blocks), (least, most, beyond) = driver([f"plan points {P}", f"cover points {P}"])
        assert rpl in (1, 2, 4) and threads % 64 == 0 and 64 <= threads <= 1024 and blocks >= 1, (P, rpl, threads, blocks)
        assert least == most == 1 and beyond == rpl * threads * blocks - P and (blocks - 1) * rpl * threads < P, P
    assert driver(["plan points 65536"]) == [[4, 1024, 16]] and driver(["plan points 4096", "plan points 4097"]) == [[4, 1024, 1], [4, 1024, 2]]
    # own-bodies mode: batch_shape's workgroup, one block, and 16 bytes of LDS per body of the capacity
    for N, shape in ((1, (1, 64)), (64, (1, 64)), (65, (2, 64)), (128, (2, 64)), (130, (4, 64)), (257, (4, 128)), (4096, (4, 1024))):
        (rpl, threads, blocks, lds), (least, most, beyond) = driver([f"plan own {N}", f"cover own {N}"])
        assert (rpl, threads, blocks, lds) == (*shape, 1, 16 * N) and least == most == 1 and beyond == rpl * threads - N


def test_the_record_layout_and_the_empty_record(driver):
    assert driver(["layout"]) == [[24, 0, 12, 16, 1048576, 0, 0, 0, 0, 0]]


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(driver, tmp_path):
    """The stand-alone driver again, built with -fsanitize=address,undefined: the same lines give the same output."""
    checked = build_driver(str(tmp_path / "driver_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    from n_body_problem_amd import plummer
    pos = np.array(plummer(64, seed=5)[0], dtype=np.float32)
    lines = [field_line(0.0, True, pos, pos), field_line(1e-2, False, pos, pos[:9] * 1.5), field_line(0.0, False, [], pos[:2]),
             "plan points 1", "cover points 4097", "cover points 1048576", "plan own 4096", "cover own 257", "layout"]
    assert checked(lines) == driver(lines)


# ---- the reference itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", (0.0, 0.05))
def test_the_references_tensor_is_the_derivative_of_its_acceleration_and_has_the_stated_trace(eps):
    from n_body_problem_amd import plummer
    pos = np.array(plummer(48, seed=9)[0], dtype=np.float32)
    pts = (np.random.default_rng(4).normal(size=(11, 3)) * 0.7).astype(np.float32)
    ref = gref.gravity(pos, 48, points=pts, softening=eps)
    # a central difference in fp64, stepping float32-exact amounts so that the points stay float32
    h = 2.0 ** -16

    def accel(p):
        # float64 points: the reference reads points as float32, so evaluate the sum here in fp64 directly
        d = pos[None, :, :3].astype(np.float64) - p[:, None, :]
        w3 = pos[None, :, 3].astype(np.float64) * ((d * d).sum(-1) + float(np.float32(eps)) ** 2) ** -1.5
        return (d * w3[..., None]).sum(1)
    x = pts.astype(np.float64)
    assert np.allclose(accel(x), ref["acceleration"], rtol=1e-13, atol=0)
    for b in range(3):
        step = np.zeros(3)
        step[b] = h
        column = (accel(x + step) - accel(x - step)) / (2 * h)             # d a_a / d x_b for every a
        scale = np.abs(ref["tidal_scale"][:, :, b]).max(axis=1, keepdims=True)
        assert np.all(np.abs(column - ref["tidal"][:, :, b]) <= 1e-4 * scale), b      # O(h^2) of the third derivative
    assert np.array_equal(ref["tidal"], np.swapaxes(ref["tidal"], 1, 2))
    d = pos[None, :, :3].astype(np.float64) - x[:, None, :]
    q = (d * d).sum(-1) + float(np.float32(eps)) ** 2
    trace = -3.0 * float(np.float32(eps)) ** 2 * (pos[None, :, 3].astype(np.float64) * q ** -2.5).sum(1)
    got = np.trace(ref["tidal"], axis1=1, axis2=2)
    assert np.all(np.abs(got - trace) <= 1e-12 * np.trace(ref["tidal_scale"], axis1=1, axis2=2))
    if eps == 0.0:
        assert not trace.any()


def test_the_reference_honours_sources_self_and_the_guard():
    pos = np.array([(0, 0, 0, 1), (2, 0, 0, 3), (0, 1, 0, 2), (5, 5, 5, 9)], np.float32)
    own = gref.gravity(pos, 4, m=3)                       # body 3 is a test particle: a row, never a source
    assert own["potential"][0] == pytest.approx(-(3 / 2 + 2 / 1), rel=1e-15) and own["sources"] == 3
    assert own["potential"][3] == pytest.approx(-(1 / np.sqrt(75) + 3 / np.sqrt(59) + 2 / np.sqrt(66)), rel=1e-15)
    at = gref.gravity(pos, 4, m=3, points=pos[:, :3])     # points on the sources at eps = 0: the guard drops them
    for name in ("acceleration", "potential", "tidal"):
        assert np.array_equal(at[name], own[name]), name
    none = gref.gravity(pos, 4, m=0)
    assert not none["potential"].any() and not none["acceleration"].any() and not none["tidal"].any()
    assert gref.gravity(pos, 0)["potential"].shape == (0,)
    assert gref.band(4096) == 4096 * 2.0 ** -24 + 2e-6 and gref.CAPACITIES == (64, 128, 130, 257, 4096)
