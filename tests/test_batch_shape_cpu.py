"""Shapes of batches without a GPU (include/nbody_batch_shape.h): the surface -- header, records, mirrors, export list, C++
wrapper, build dependencies -- every byte of every record that the arithmetic of csrc/nbody_batch_shape_math.h gives on the
CPU (a stand-alone g++ program, tests/batch_shape_driver.cpp, that runs the kernel's phases for any workgroup shape, once more
under the address and undefined-behaviour sanitizers) against the reference tests/hermite_shape_ref.py, independent checks of
that reference (numpy.linalg.eigh, a sampled triaxial Gaussian, a rotated state, radial_profile's reference, the degenerate
ends), the bound of the GPU test measured again, and the derived quantities of ShapeResult on hand-made records."""
import ctypes
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_radial_ref as rref
import hermite_shape_ref as sref
from conftest import ROOT

NAMES = ["nbody_batch_shape"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
APERTURE_WORDS = ("status", "iterations", "count", "radius", "inner", "q", "s", "change", "eigenvalues", "axes", "weight", "D", "M", "L")
APERTURE_OFFSETS = [0, 4, 8, 16, 24, 32, 40, 48, 56, 80, 152, 160, 184, 232]
SYSTEM_WORDS = ("selected", "unmeasured", "apertures", "reduced", "converged", "reserved", "total_weight", "centre", "velocity")
SYSTEM_OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32, 56]
BODY_WORDS = ("inside", "reserved")
BODY_OFFSETS = [0, 4]
HELPERS = ("triaxiality", "ellipticity", "offset", "spin_axis", "misalignment", "view", "members_mask")


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_surface_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_shape.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_shape.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_surface.h"') < nbody_h.index('#include "nbody_batch_shape.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_256_80_and_8_bytes(tmp_path):
    lines = ['#include "nbody.h"', "#include <stddef.h>",
             "typedef char aperture_size[sizeof(nbody_batch_shape_aperture) == 256 ? 1 : -1];",
             "typedef char system_size[sizeof(nbody_batch_shape_system) == 80 ? 1 : -1];",
             "typedef char body_size[sizeof(nbody_batch_shape_body) == 8 ? 1 : -1];",
             "typedef char count_is_long_long[sizeof(((nbody_batch_shape_aperture *)0)->count) == 8 ? 1 : -1];",
             "typedef char limit[NBODY_BATCH_SHAPE_MAX_APERTURES == 8 && NBODY_BATCH_SHAPE_MAX_ITERATIONS == 64 ? 1 : -1];",
             "typedef char words[NBODY_BATCH_SHAPE_CONVERGED == 0 && NBODY_BATCH_SHAPE_MAX == 1 && NBODY_BATCH_SHAPE_FEW == 2 && "
             "NBODY_BATCH_SHAPE_DEGENERATE == 3 ? 1 : -1];"]
    for record, names, offsets in (("aperture", APERTURE_WORDS, APERTURE_OFFSETS), ("system", SYSTEM_WORDS, SYSTEM_OFFSETS),
                                   ("body", BODY_WORDS, BODY_OFFSETS)):
        for name, offset in zip(names, offsets):
            lines.append(f"typedef char {record}_{name}_at_{offset}[offsetof(nbody_batch_shape_{record}, {name}) == {offset} ? 1 : -1];")
    lines += ["int main(void) {", "    nbody_batch_shape_system s;", "    double radii[1] = {1.0};",
              "    return (nbody_batch_shape(0, 0, 0, 1, radii, 0, 0, 0, 0, NBODY_BATCH_WEIGHT_MASS, 1, 1e-3, 64, 10, 0, &s, 0, 0) != NBODY_ERR_INVALID)"
              " + (NBODY_ABI_VERSION != 5);", "}"]
    src = tmp_path / "shape.c"
    src.write_text("\n".join(lines) + "\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_shape.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_surface.h", "nbody_batch_radial.h's rule",
                   "takes part iff i < min(counts[s], max_bodies) and subset is NULL or", "The massive counts play no part",
                   "NBODY_BATCH_WEIGHT_MASS (0)", "NBODY_BATCH_WEIGHT_NUMBER (1)", "widened to fp64", "or NULL for zeros",
                   "d_k = (double)x_k - c_k", "u_k = (double)v_k - v0_k", "unmeasured iff any of its six words",
                   "a member of nothing", "+, -, x, / and sqrt alone, nothing contracted",
                   "1 <= apertures <= NBODY_BATCH_SHAPE_MAX_APERTURES (8)", "finite and > 0", "0 <= inner[a] < radii[a]",
                   "need not be ordered and are independent", "one fp64 product each, on the host", "largest finite double",
                   "starts as the identity with w2 = w3 = 1", "The major axis is kept at R",
                   "a' = (e1_x d_x + e1_y d_y) + e1_z d_z", "r2e = (a'a' + w2 (b'b')) + w3 (c'c')", "in2 < r2e <= out2",
                   "a member always has r2e > 0", "in the state's coordinates, not the rotated ones", "w (d_a d_b)",
                   "(w (d_a d_b)) / r2e", "status FEW", "min_members (>= 4)", "cyclic Jacobi", "(0,1), (0,2), (1,2)", "16 at the most",
                   "g = 100 |a_pq|", "theta = (a_qq - a_pp) / (2 a_pq)", "root = sqrt(theta theta + 1)",
                   "t = theta < 0 ? -1 / (root - theta) : 1 / (theta + root)", "c = 1 / sqrt(t t + 1)", "s = t c",
                   "lambda1 >= lambda2 >= lambda3, ties to the lower original column",
                   "component of largest magnitude positive, ties to the lower index", "e3 = e1 x e2", "right-handed",
                   "status DEGENERATE", "razor-thin disc", "w2 = lambda1 / lambda2", "q = sqrt(lambda2 / lambda1)",
                   "|q - q_prev| <= tol q_prev && |s - s_prev| <= tol s_prev", "q_prev = s_prev = 1 before pass 1",
                   "max_iterations (1 ... 64)", "status MAX", "one more walk runs under the final state",
                   "unreduced whatever the flag", "Every sum is two-level", "64 k ... 64 k + 63", "from +0.0",
                   "in ascending k", "the same bits in any slot, n_systems, max_bodies and workgroup shape",
                   "Adding +0.0 for a non-member is the same bits as skipping it", "nbody_batch_radial_profile's",
                   "not plain ascending index", "256 bytes", "80 bytes", "8 bytes", "nbody_batch_surface_map's axes layout",
                   "Slots from the count on, and bodies not taking part, read 0", "the same bits either way", "synchronous",
                   "forgets nothing", "bit for bit", "freed in nbody_batch_destroy", "names the function", "a NULL handle",
                   "NULL d_positions_xyzm, d_velocities, radii or systems_out", "apertures outside 1 ... 8",
                   "the message names the system and the aperture", "a weight that is not 0 or 1", "not finite or negative",
                   "max_iterations outside 1 ... 64", "min_members < 4", "a centre or velocity that is not finite",
                   "refused before any device work", "Out of scope", "keeping the volume or the middle axis", "cube root",
                   "recentring during the iteration", "shapes of velocity space", "more than 8 apertures", "shapes across systems",
                   "device-side outputs", "the single-system context"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.shape_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.radial_names()) | set(_lib.surface_names()))
    fn = lib.nbody_batch_shape
    assert fn.argtypes is not None and len(fn.argtypes) == 18
    for mirror, size, names, offsets in ((_lib.BatchShapeAperture, 256, APERTURE_WORDS, APERTURE_OFFSETS),
                                         (_lib.BatchShapeSystem, 80, SYSTEM_WORDS, SYSTEM_OFFSETS),
                                         (_lib.BatchShapeBody, 8, BODY_WORDS, BODY_OFFSETS)):
        assert ctypes.sizeof(mirror) == size and [f[0] for f in mirror._fields_] == list(names)
        assert [getattr(mirror, w).offset for w in names] == offsets
    assert _lib.BATCH_SHAPE_MAX_APERTURES == 8 and _lib.BATCH_SHAPE_MAX_ITERATIONS == 64
    assert batch.SHAPE_SYSTEM_DTYPE == sref.SYSTEM_DTYPE and batch.SHAPE_APERTURE_DTYPE == sref.APERTURE_DTYPE
    assert batch.SHAPE_BODY_DTYPE == sref.BODY_DTYPE
    assert [batch.SHAPE_APERTURE_DTYPE.fields[w][1] for w in APERTURE_WORDS] == APERTURE_OFFSETS
    assert [batch.SHAPE_SYSTEM_DTYPE.fields[w][1] for w in SYSTEM_WORDS] == SYSTEM_OFFSETS
    assert [batch.SHAPE_BODY_DTYPE.fields[w][1] for w in BODY_WORDS] == BODY_OFFSETS
    for name in ("ShapeResult", "SHAPE_SYSTEM_DTYPE", "SHAPE_APERTURE_DTYPE", "SHAPE_BODY_DTYPE"):
        assert name in nb.__all__ and getattr(nb, name) is getattr(batch, name), name
    assert batch.ShapeResult.__doc__ and batch.BatchedSystem.shape.__doc__
    for helper in HELPERS:
        assert getattr(batch.ShapeResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_shape") == 1
    assert exports[exports.index("nbody_batch_shape") - 1].startswith("# nbody_batch_shape:")
    names = [line for line in exports if not line.startswith("#")]
    assert names == sorted(names)


def test_the_cpp_wrapper_compiles_with_a_lean_and_a_full_call(tmp_path):
    src = tmp_path / "batch_shape.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_shape_system> both(nbody::Batch &b, const float *pos, const float *vel)
{
    std::vector<nbody_batch_shape_aperture> records;
    std::vector<nbody_batch_shape_body> bodies;
    const std::vector<double> radii{1.0, 2.0, 4.0}, inner{0.0, 0.5, 0.0};
    std::vector<nbody_batch_shape_system> lean = b.shape(pos, vel, radii, nullptr);
    b.shape(pos, vel, 3, radii, &records, inner, std::vector<double>(3 * 16, 0.0), std::vector<double>(3 * 16, 0.0),
            NBODY_BATCH_WEIGHT_NUMBER, false, 1e-4, 32, 20, std::vector<unsigned char>(16 * 64, 1), &bodies);
    return lean;
}
''')
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_every_error_is_refused_before_any_device_work(lib):
    """A NULL handle is refused first, with the function's name, by the library itself.  The other cases need a handle
    (test_batch_shape_gpu.py walks them); here the source shows that each is refused before the first device call."""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchShapeSystem * 1)()
    radii = (ctypes.c_double * 1)(1.0)
    assert lib.nbody_batch_shape(None, None, None, 1, radii, None, 0, None, None, 0, 1, 1e-3, 64, 10, None, out, None, None) == \
        _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_shape: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_shape("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_shape: batch is NULL", "nbody_batch_shape: NULL argument", "nbody_batch_shape: apertures must be 1 ... 8",
                "nbody_batch_shape: weight must be", "nbody_batch_shape: tol must be finite and >= 0",
                "nbody_batch_shape: max_iterations must be 1 ... 64", "nbody_batch_shape: min_members must be >= 4",
                "nbody_batch_shape: the radius", "nbody_batch_shape: the inner radius", "nbody_batch_shape: the centre of system ",
                "nbody_batch_shape: the velocity of system ")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_shape: ') == len(messages)                                # every message names the function


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_other_roots_and_fused_operations():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_shape_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_shape.h" for h in build.HEADERS)
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(CSRC, "nbody_batch_shape_math.h")).read()
    code = re.sub(r"//.*", "", text)
    assert "hip/" not in code and "NBODY_HD inline" in code and "fma(" not in code and "fmaf(" not in code and "float " in code
    assert '#include "nbody_batch_surface_math.h"' in code                                   # the chain of math headers
    assert "cbrt" not in code and "pow(" not in code and "exp(" not in code and "log(" not in code and "hypot" not in code
    assert set(re.findall(r"__builtin_\w+", code)) == {"__builtin_fabs", "__builtin_fabsf", "__builtin_sqrt", "__builtin_nanf"}
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_shape_kernel("):source.index("hipError_t launch_batch_shape(")]
    for call in ("shape_measured(", "shape_image_point(", "shape_image_slot(", "shape_total_step(", "shape_pass_step(", "shape_level2<",
                 "shape_update(", "shape_final_step(", "shape_inside_at(", "shape_record(", "shape_body(", "shape_system(", "shape_start("):
        assert call in kernel, call
    assert "asm" not in kernel and "fma" not in kernel and "sqrt" not in kernel
    launch = source[source.index("hipError_t launch_batch_shape("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "with_rpl(" in launch and "launch_analysis_kernel(" in launch
    assert "shape_threads(sh.threads)" in launch
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchShapeSystem> shape_systems", "DeviceArray<BatchShapeAperture> shape_apertures",
                   "DeviceArray<BatchShapeBody> shape_bodies", "DeviceArray<unsigned char> shape_subset",
                   "DeviceArray<double> shape_aps", "DeviceArray<double> shape_frames"):
        assert member in members, member
    entry = source[source.index("int nbody_batch_shape("):]
    assert "hipFree" not in entry[:entry.index("\n}\n")] and "hipMalloc" not in entry[:entry.index("\n}\n")]


def test_the_lds_of_the_largest_launch_fits_a_gfx950_workgroup():
    """The launcher's sum, recomputed: 16 bytes per image word, two words per body and one more per block of 64, then one
    membership byte per body and four more per block, and the static arrays."""
    dynamic = 16 * (2 * 4096 + 64) + (4096 + 4 * 64)
    static = 8 * 4 * 8 + 6 * 8 + 3 * 4                                                       # 316; 320 with the compiler's padding
    assert dynamic == 136448 and dynamic + static <= 136448 + 320 == 136768 <= 160 * 1024
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    assert "136448 bytes" in source and "320 bytes" in source and "136768 bytes" in source


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_shape_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        return res.stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("shape"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("shape_checked"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def number(v):
    v = float(v)
    return v.hex() if math.isfinite(v) else ("nan" if v != v else ("inf" if v > 0 else "-inf"))


def command(pos, vel, n, shape, radii, inner, centre, velocity, weight, reduced, subset, tol=1e-3, max_iterations=64, min_members=10,
            want=1):
    T, rpl = shape
    A = len(radii)
    inner = [0.0] * A if inner is None else inner
    lines = [f"system {n} {pos.shape[0]} {T} {rpl} {A} {1 if weight == 'number' else 0} {int(reduced)} {max_iterations} {min_members} {want}",
             number(tol), " ".join(number(r) for r in radii), " ".join(number(r) for r in inner),
             " ".join(number(c) for c in list(centre) + list(velocity))]
    for i in range(n):
        take = 1 if subset is None else int(subset[i] != 0)
        lines.append(" ".join(number(w) for w in (*pos[i], *vel[i, :3])) + f" {take}")
    return "\n".join(lines) + "\n"


def run_batch(run, pos, vel, counts, shape, want, radii, inner, centre, velocity, weight, reduced, subset, only=None, **more):
    """The driver's records of the systems `only` (all) of a batch: systems, apertures or None, bodies."""
    text = ""
    radii = np.asarray(radii)
    which = list(range(pos.shape[0])) if only is None else list(only)
    for s in which:
        text += command(pos[s], vel[s], int(counts[s]), shape, radii[s] if radii.ndim == 2 else radii,
                        None if inner is None else (inner[s] if np.ndim(inner) == 2 else inner), centre[s], velocity[s], weight, reduced,
                        None if subset is None else subset[s], want=want, **more)
    out = run(text)
    systems = np.stack([np.frombuffer(bytes.fromhex(out[3 * k]), dtype=sref.SYSTEM_DTYPE)[0] for k in range(len(which))])
    apertures = np.stack([np.frombuffer(bytes.fromhex(out[3 * k + 1]), dtype=sref.APERTURE_DTYPE) for k in range(len(which))]) if want else None
    bodies = np.stack([np.frombuffer(bytes.fromhex(out[3 * k + 2]), dtype=sref.BODY_DTYPE) for k in range(len(which))])
    if not want:
        assert all(out[3 * k + 1] == "" for k in range(len(which)))
    return systems, apertures, bodies


reference = sref.reference


def test_the_layout(driver):
    words = [int(w) for w in driver("layout\n")[0].split()]
    assert words == [256, *APERTURE_OFFSETS, 80, *SYSTEM_OFFSETS, 8, *BODY_OFFSETS]


@pytest.mark.parametrize("capacity", sref.CAPACITIES)
def test_the_inputs_do_their_work(capacity):
    """The shared inputs reach what they are there for: every count the capacity holds; an empty system; systems that end FEW;
    converged ones, and from 128 bodies on one that hits the iteration limit; a shell; a mask; per-system radii; one unmeasured
    body; every margin above the GPU test's cap."""
    assert sref.shape_of(capacity) == sref.SHAPES[sref.CAPACITIES.index(capacity)]
    seen = set()
    for case in sref.CASES:
        pos, vel, counts, kw, (systems, apertures, bodies, margin) = reference(capacity, case[0])
        assert list(counts) == sref.batch_counts(capacity) and counts[0] == 0 and counts[-1] == capacity
        assert margin >= 1000 * sref.LEAST_MARGIN, (case[0], margin)
        assert systems["selected"][0] == 0 and (apertures["status"][0] == sref.FEW).all() and not bodies["inside"][0].any()
        assert (apertures["iterations"][0] == 1).all() and (apertures["q"][0] == 1.0).all()
        assert systems["unmeasured"][-1] == (1 if kw["subset"] is None or kw["subset"][-1, 5] else 0)
        assert np.array_equal(systems["converged"], (apertures["status"] == sref.CONVERGED).sum(axis=1))
        for a in range(apertures.shape[1]):
            assert np.array_equal(((bodies["inside"] >> a) & 1).sum(axis=1), apertures["count"][:, a])
        if case[6] == "none":
            assert np.array_equal(systems["selected"], counts)
        else:
            assert 0 < systems["selected"][-1] < counts[-1]
        seen |= set(apertures["status"].ravel().tolist())
        assert (apertures["status"][-1] == sref.CONVERGED).any() and apertures["count"][-1].max() > capacity // 2
        if case[2] is not None:
            assert (apertures["inner"] > 0).any() and (apertures["count"][-1][apertures["inner"][-1] > 0] > 0).all()
        if case[3]:
            assert apertures["radius"][1, 0] != apertures["radius"][2, 0]
    assert {sref.CONVERGED, sref.FEW} <= seen and (capacity < 128 or sref.MAX in seen)


@pytest.mark.parametrize("capacity", sref.CAPACITIES)
@pytest.mark.parametrize("case", [c[0] for c in sref.CASES])
def test_the_driver_gives_the_references_records_byte_for_byte(driver, capacity, case):
    """Every byte of every record, for the workgroup shape of this capacity, with and without the aperture records."""
    pos, vel, counts, kw, (systems, apertures, bodies, _) = reference(capacity, case)
    shape = sref.shape_of(capacity)
    got = run_batch(driver, pos, vel, counts, shape, 1, **kw)
    assert got[0].tobytes() == systems.tobytes(), (got[0], systems)
    assert got[1].tobytes() == apertures.tobytes()
    assert got[2].tobytes() == bodies.tobytes()
    lean = run_batch(driver, pos, vel, counts, shape, 0, **kw)
    assert lean[0].tobytes() == systems.tobytes() and lean[2].tobytes() == bodies.tobytes()


def test_the_records_do_not_depend_on_the_workgroup_shape(driver):
    pos, vel, counts, kw, (systems, apertures, bodies, _) = reference(64, "8-shell-reduced-mass-own")
    for shape in sref.SHAPES + ((1024, 4),):
        got = run_batch(driver, pos, vel, counts, shape, 1, **kw)
        assert got[0].tobytes() == systems.tobytes() and got[1].tobytes() == apertures.tobytes() and got[2].tobytes() == bodies.tobytes()


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    for capacity, names, only in ((128, [c[0] for c in sref.CASES], None), (64, ["8-shell-reduced-mass-own"], None),
                                  (4096, ["3-shell-unreduced-number-sparse"], (0, 2, 10)), (4096, ["1-reduced-mass"], (9,))):
        for name in names:
            pos, vel, counts, kw, (systems, apertures, bodies, _) = reference(capacity, name)
            which = list(range(len(counts))) if only is None else list(only)
            got = run_batch(checked_driver, pos, vel, counts, sref.shape_of(capacity), 1, only=only, **kw)
            assert got[0].tobytes() == systems[which].tobytes() and got[1].tobytes() == apertures[which].tobytes()
            assert got[2].tobytes() == bodies[which].tobytes()


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def full(T):
    return np.array([[T[0], T[3], T[4]], [T[3], T[1], T[5]], [T[4], T[5], T[2]]])


def test_the_references_eigenvalues_and_axes_are_numpy_linalg_eighs_on_its_own_tensors():
    checked = 0
    for capacity in (128, 1024):
        for case in sref.CASES:
            pos, vel, counts, kw, _ = reference(capacity, case[0])
            radii = np.asarray(kw["radii"])
            for s in (len(counts) - 1, len(counts) - 2):
                out = sref.shape(pos[s], vel[s], counts[s], radii[s] if radii.ndim == 2 else radii,
                                 None if kw["inner"] is None else (kw["inner"][s] if np.ndim(kw["inner"]) == 2 else kw["inner"]),
                                 kw["centre"][s], kw["velocity"][s], kw["weight"], kw["reduced"],
                                 subset=None if kw["subset"] is None else kw["subset"][s])
                for passes in out[4]:
                    for T, lam, e in passes[:4] + passes[-1:]:
                        values, vectors = np.linalg.eigh(full(T))
                        assert np.allclose(lam, values[::-1], rtol=1e-13, atol=1e-13 * abs(values[-1]))
                        E = np.array(e).reshape(3, 3)
                        assert np.allclose(E @ E.T, np.eye(3), atol=1e-14) and np.linalg.det(E) == pytest.approx(1.0, abs=1e-14)
                        gaps = min(values[1] - values[0], values[2] - values[1]) / values[2]
                        for r in range(3):                            # the same axis up to the sign, as far as the gaps resolve it
                            assert abs(E[r] @ vectors[:, 2 - r]) > 1.0 - 1e-12 / max(gaps, 1e-3) ** 2, (r, gaps)
                        for r in range(2):
                            assert E[r][np.argmax(np.abs(E[r]))] > 0.0
                        assert np.allclose(E @ full(T) @ E.T, np.diag(lam), atol=1e-13 * abs(lam[0]))
                        checked += 1
    assert checked > 100


def test_jacobi_sorts_signs_and_handles_the_special_tensors():
    lam, e = sref.jacobi([3.0, 1.0, 2.0, 0.0, 0.0, 0.0])                  # diagonal: no sweep, the sort alone
    assert lam == [3.0, 2.0, 1.0] and e == [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0]   # e3 = x cross z = -y
    lam, e = sref.jacobi([2.0, 2.0, 2.0, 0.0, 0.0, 0.0])                  # ties to the lower original column
    assert lam == [2.0, 2.0, 2.0] and e == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    lam, e = sref.jacobi([1.0, 1.0, 0.0, -1.0, 0.0, 0.0])                 # eigenvalues 2, 0, 0: (1, -1, 0) / sqrt 2 with its sign fixed
    assert lam[0] == pytest.approx(2.0, abs=1e-15) and abs(lam[1]) < 1e-15 and abs(lam[2]) < 1e-15
    assert e[0] == pytest.approx(math.sqrt(0.5)) and e[1] == pytest.approx(-math.sqrt(0.5)) and e[0] > 0.0
    lam, e = sref.jacobi([float("nan")] * 6)                               # ends, and says nothing finite
    assert all(x != x for x in lam)


def test_a_sampled_triaxial_gaussian_gives_back_its_rotation_and_its_ratios():
    """20000 bodies of a Gaussian with dispersions 1 : 0.7 : 0.4 along the rows of a known rotation, at R = 2 sigma_major,
    unit weights.  The iterated reduced tensor of an ellipsoidal aperture similar to the distribution recovers the ratios
    without bias; the sampling error of a ratio of dispersions from N members is about 1 / sqrt(N) (each second moment has
    the relative error sqrt(2 / N), a ratio of two roots of them sqrt(2 / N) too, and the members number about 0.74 N x the
    fraction of a Gaussian within 2 sigma along every axis, ~ 0.74): with N ~ 14800, 0.0082; the bound is four of these, 0.033,
    and for the axes the same over the smallest gap between the squared ratios, 0.49 - 0.16: 0.1 rad."""
    rng = np.random.default_rng(77)
    rot = sref.rotation(rng)
    n = 20000
    pos = np.zeros((n, 4), dtype=np.float32)
    vel = np.zeros((n, 4), dtype=np.float32)
    pos[:, :3] = (rng.normal(size=(n, 3)) * np.array(sref.SIGMAS)) @ rot
    pos[:, 3] = 1.0
    # 20000 bodies are more than a batch holds: the reference takes any count (313 blocks)
    system, apertures, bodies, margin, _ = sref.shape(pos, vel, n, [2.0], weight="number", tol=1e-4)
    a = apertures[0]
    assert a["status"] == sref.CONVERGED and 12000 < a["count"] < 17000
    assert abs(a["q"] - 0.7) < 0.033 and abs(a["s"] - 0.4) < 0.033, (a["q"], a["s"])
    E = a["axes"].reshape(3, 3)
    for r in range(3):
        assert abs(E[r] @ rot[r]) > math.cos(0.1), (r, E[r], rot[r])


def test_rotating_the_state_rotates_the_axes_and_leaves_the_ratios_and_the_members_alone():
    """The same bodies turned by a rotation: q, s and the member sets agree (to the rounding of the rotation itself, which the
    margin covers), and the axes are the turned axes up to the sign convention."""
    pos, vel, counts, kw, (systems, apertures, bodies, margin) = reference(256, "1-reduced-mass")
    s = len(counts) - 2                                                    # 129 bodies, no NaN
    rot = sref.rotation(np.random.default_rng(8))
    turned, turned_v = np.array(pos[s]), np.array(vel[s])
    centre = np.asarray(kw["centre"][s])
    turned[:, :3] = (pos[s][:, :3].astype(np.float64) - centre) @ rot.T + centre
    _, a0, b0, m0, _ = sref.shape(pos[s], vel[s], counts[s], [2.0], centre=centre)
    _, a1, b1, m1, _ = sref.shape(turned, turned_v, counts[s], [2.0], centre=centre)
    assert min(m0, m1) > 1e-5                                              # float32 positions after the turn: 6e-8
    assert np.array_equal(b0["inside"], b1["inside"]) and a0["count"][0] == a1["count"][0] and a0["status"][0] == sref.CONVERGED
    assert abs(a0["q"][0] - a1["q"][0]) < 1e-5 and abs(a0["s"][0] - a1["s"][0]) < 1e-5
    E0, E1 = a0["axes"][0].reshape(3, 3), a1["axes"][0].reshape(3, 3)
    for r in range(3):
        assert abs(abs((E0[r] @ rot.T) @ E1[r]) - 1.0) < 1e-4
    # and started from a turned state instead of the identity, the first pass is the same sphere: the same first tensor
    _, a2, b2, _, t2 = sref.shape(pos[s], vel[s], counts[s], [2.0], centre=centre, start=rot.ravel())
    _, _, _, _, t0 = sref.shape(pos[s], vel[s], counts[s], [2.0], centre=centre)
    assert np.allclose(t2[0][0][0], t0[0][0][0], rtol=1e-12) and np.array_equal(b2["inside"], b0["inside"])


def test_a_spheres_first_unreduced_tensor_is_radial_profiles_m_bit_for_bit_up_to_64_bodies():
    for n, seed in ((64, 1), (63, 2), (17, 3)):
        pos, vel = sref.gaussian_system(64, n, seed)
        for weight in ("mass", "number"):
            out = sref.shape(pos, vel, n, [2.0], inner=[0.5], centre=sref.CENTRE, velocity=sref.VELOCITY, weight=weight, reduced=False)
            T = out[4][0][0][0]
            _, shells, _, _ = rref.profile(pos, vel, n, [0.5, 2.0], centre=sref.CENTRE, velocity=sref.VELOCITY, weight=weight)
            assert shells["count"][0] > 10 and np.array(T).tobytes() == shells["M"][0].tobytes(), (n, weight)
            # and a sphere that is never deformed (FEW at pass 1) has the shell's final sums too
            kept = sref.shape(pos, vel, n, [2.0], inner=[0.5], centre=sref.CENTRE, velocity=sref.VELOCITY, weight=weight,
                              reduced=False, min_members=1000)[1][0]
            assert kept["status"] == sref.FEW and kept["count"] == shells["count"][0]
            for word in ("weight", "M", "L"):
                assert kept[word].tobytes() == shells[word][0].tobytes(), word


def test_the_degenerate_ends():
    rng = np.random.default_rng(12)
    n = 200
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :2] = rng.normal(size=(n, 2))
    pos[:, 3] = 1.0                                                        # a coplanar set: z = 0 exactly
    for reduced in (True, False):
        _, a, b, _, _ = sref.shape(pos, vel, n, [2.0], reduced=reduced)
        assert a["status"][0] == sref.DEGENERATE and a["iterations"][0] == 1 and a["eigenvalues"][0][2] == 0.0
        assert a["eigenvalues"][0][0] > a["eigenvalues"][0][1] > 0.0 and a["q"][0] == 1.0 and a["s"][0] == 1.0
        assert a["axes"][0].tolist() == np.eye(3).ravel().tolist() and a["count"][0] == ((b["inside"] & 1) != 0).sum() > 100
    four, four_v = sref.gaussian_system(64, 4, seed=9)                     # four bodies with min_members = 10
    _, a, b, _, _ = sref.shape(four, four_v, 4, [100.0], centre=sref.CENTRE)
    assert a["status"][0] == sref.FEW and a["iterations"][0] == 1 and a["axes"][0].tolist() == np.eye(3).ravel().tolist()
    assert a["count"][0] == 4 and not a["eigenvalues"][0].any() and a["change"][0] == 0.0
    pos, vel = sref.gaussian_system(256, 256, seed=10)
    _, a, _, _, _ = sref.shape(pos, vel, 256, [2.0], centre=sref.CENTRE, max_iterations=1)
    assert a["status"][0] == sref.MAX and a["iterations"][0] == 1 and a["q"][0] < 1.0
    _, a, _, _, _ = sref.shape(pos, vel, 256, [2.0], centre=sref.CENTRE, max_iterations=1, tol=1.0)
    assert a["status"][0] == sref.CONVERGED and a["iterations"][0] == 1   # already within tol


def test_the_bound_of_the_rooted_words_measured_again():
    """hermite_shape_ref.SPREAD, the spread of q, s, change, eigenvalues and axes when every quotient and root of the reference
    is moved by up to one ulp at random, over all cases of the three smaller capacities (all five: 5.63e-12, the constant):
    no integer and no exact word moves, and the spread stays within the constant that the GPU test's bound is four times of."""
    spread, same = sref.jitter_spread(capacities=(64, 128, 256))
    print(f"spread {spread:.3g}; SPREAD {sref.SPREAD:.3g}; BOUND {sref.BOUND:.3g}")
    assert same and 0.0 < spread <= sref.SPREAD and sref.BOUND == 4.0 * sref.SPREAD


# ---- the derived quantities ----------------------------------------------------------------------------------------------------
def test_the_derived_quantities_of_hand_made_records():
    from n_body_problem_amd.batch import ShapeResult
    systems = np.zeros(2, dtype=sref.SYSTEM_DTYPE)
    systems["apertures"], systems["reduced"] = 2, 1
    ap = np.zeros((2, 2), dtype=sref.APERTURE_DTYPE)
    ap["q"], ap["s"] = [[0.8, 1.0], [0.5, 0.5]], [[0.6, 1.0], [0.5, 0.25]]
    ap["weight"] = [[2.0, 0.0], [4.0, 1.0]]
    ap["D"][0, 0], ap["D"][1, 0] = [1.0, -2.0, 4.0], [0.0, 0.0, 2.0]
    ap["L"][0, 0], ap["L"][1, 0], ap["L"][1, 1] = [0.0, 0.0, 5.0], [0.0, 3.0, 0.0], [0.0, 0.0, -2.0]
    ap["axes"][:] = np.eye(3).ravel()
    ap["axes"][1, 1] = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]).ravel()
    bodies = np.zeros((2, 5), dtype=sref.BODY_DTYPE)
    bodies["inside"] = [[1, 3, 2, 0, 0], [0, 1, 1, 2, 0]]
    res = ShapeResult(systems, ap, bodies, "mass")
    T = res.triaxiality()
    assert T[0, 0] == (1 - 0.8 ** 2) / (1 - 0.6 ** 2) and np.isnan(T[0, 1]) and T[1, 0] == 1.0 and T[1, 1] == 0.75 / (1 - 0.0625)
    assert res.ellipticity().tolist() == [[0.4, 0.0], [0.5, 0.75]]
    assert res.offset()[0, 0].tolist() == [0.5, -1.0, 2.0] and np.isnan(res.offset()[0, 1]).all() and res.offset()[1, 0, 2] == 0.5
    assert res.spin_axis()[0, 0].tolist() == [0.0, 0.0, 1.0] and np.isnan(res.spin_axis()[0, 1]).all()
    assert res.spin_axis()[1, 1].tolist() == [0.0, 0.0, -1.0]
    m = res.misalignment()
    assert m[0, 0] == 0.0 and np.isnan(m[0, 1]) and m[1, 0] == pytest.approx(math.pi / 2) and m[1, 1] == pytest.approx(math.pi / 2)
    assert res.members_mask(0).tolist() == [[True, True, False, False, False], [False, True, True, False, False]]
    assert res.members_mask(1).tolist() == [[False, True, True, False, False], [False, False, False, True, False]]
    assert res.members_mask(0).dtype == np.bool_ and res.axes.shape == (2, 2, 3, 3) and res.reduced is True
    for kind in ("face_on", "edge_on"):
        for a in range(2):
            v = res.view(a, kind)
            assert v.shape == (2, 3, 3) and v.flags["C_CONTIGUOUS"]
            for s in range(2):
                assert np.array_equal(v[s] @ v[s].T, np.eye(3)) and np.linalg.det(v[s]) == 1.0   # orthonormal and right-handed
                assert np.array_equal(np.cross(v[s, 0], v[s, 1]), v[s, 2])
    assert np.array_equal(res.view(1, "face_on")[1, 2], [1.0, 0.0, 0.0])                     # the line of sight is the minor axis
    assert np.array_equal(res.view(1, "edge_on")[1], [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    with pytest.raises(ValueError, match="kind must be"):
        res.view(0, "side")
    with pytest.raises(ValueError, match="a must be"):
        res.members_mask(2)
    lean = ShapeResult(systems, None, None, "mass")
    assert lean.q is None and lean.inside is None
    with pytest.raises(ValueError, match="apertures=True"):
        lean.triaxiality()
    with pytest.raises(ValueError, match="bodies=True"):
        lean.members_mask(0)
    assert "ShapeResult(apertures=2" in repr(res)
