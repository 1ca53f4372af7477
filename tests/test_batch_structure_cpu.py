"""CPU-only: the cluster structure of batched ensembles (nbody_batch_structure, include/nbody_batch_structure.h).  The header is
self-contained C99, included by nbody.h after the pairs header, and declares its one entry point alone; it is exported, bound
and listed apart; the arithmetic without a GPU (csrc/nbody_batch_structure_math.h), built into a stand-alone driver with g++,
keeps the eight smallest of any sequence as std::sort does and gives the density formula; the numpy reference
(hermite_structure_ref) gives the hand-worked numbers of a small system and the closed values of inversion-symmetric shells;
and on every input of the GPU suite the float32 search finds the fp64 neighbours, so that those inputs, not a tolerance,
carry the GPU test."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_structure_ref as sref
from conftest import ROOT

NAMES = ["nbody_batch_structure"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
C = sref.FOUR_PI_OVER_THREE

from n_body_problem_amd import _lib as _bound  # noqa: E402  (the constants of the feature: the reference is held to them)
assert (sref.MAX_NEIGHBOUR, sref.MAX_FRACTIONS) == (_bound.BATCH_STRUCTURE_MAX_NEIGHBOUR, _bound.BATCH_STRUCTURE_FRACTIONS)
assert sref.WEIGHTS == ("mass", "number") and (_bound.BATCH_WEIGHT_MASS, _bound.BATCH_WEIGHT_NUMBER) == (0, 1)


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_pairs_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_structure.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_structure.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_pairs.h"') < nbody_h.index('#include "nbody_batch_structure.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_40_and_120_bytes(tmp_path):
    src = tmp_path / "structure.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char body_is_40_bytes[sizeof(nbody_batch_structure_body) == 40 ? 1 : -1];
typedef char system_is_120_bytes[sizeof(nbody_batch_structure_system) == 120 ? 1 : -1];
typedef char enclosed_at_16[offsetof(nbody_batch_structure_body, enclosed) == 16 ? 1 : -1];
typedef char r2_at_24[offsetof(nbody_batch_structure_body, neighbour_r2) == 24 ? 1 : -1];
typedef char inside_at_32[offsetof(nbody_batch_structure_body, inside) == 32 ? 1 : -1];
typedef char core_radius_at_24[offsetof(nbody_batch_structure_system, core_radius) == 24 ? 1 : -1];
typedef char lagrange_at_48[offsetof(nbody_batch_structure_system, lagrange) == 48 ? 1 : -1];
typedef char estimated_at_112[offsetof(nbody_batch_structure_system, estimated) == 112 ? 1 : -1];
typedef char limits[NBODY_BATCH_STRUCTURE_MAX_NEIGHBOUR == 8 && NBODY_BATCH_STRUCTURE_FRACTIONS == 8 ? 1 : -1];
typedef char weights[NBODY_BATCH_WEIGHT_MASS == 0 && NBODY_BATCH_WEIGHT_NUMBER == 1 ? 1 : -1];
int main(void) {
    nbody_batch_structure_system s;
    double f[1] = {0.5};
    return (nbody_batch_structure(0, 0, 6, NBODY_BATCH_WEIGHT_MASS, f, 1, &s, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_structure.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_pairs.h", "all j < counts[s]", "whatever the massive counts",
                   "as the state holds them", "NBODY_BATCH_WEIGHT_MASS (0): the mass word", "NBODY_BATCH_WEIGHT_NUMBER (1): every body weighs 1",
                   "runs in fp32", "ascending j", "every fmaf one fused operation", "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))",
                   "only where r2 > 0", "the self pair, coincident bodies and NaN", "k-th smallest r2", "+inf where the row has fewer than k",
                   "does not depend on the order it is found in", "a function of the state alone", "the unbiased estimator",
                   "0 < r2 < r2_k(i)", "the fp32 sum, in ascending j", "Exact ties with the k-th distance are not inside",
                   "inside may be below k - 1", "r = sqrt((double)r2_k)", "4 pi / 3 = 4.1887902047863909846", "density is 0 where r2_k is +inf",
                   "the number of bodies with finite r2_k", "sum rho_i x_i / sum rho_i", "sqrt(sum rho_i^2 |x_i - centre|^2 / sum rho_i^2)",
                   "sum rho_i^2 / sum rho_i", "the fp32 weights summed in fp64", "centre is the centre of weight sum w x / sum w",
                   "Where total_weight is also 0: everything is 0", "dx = (double)x_i - centre_x", "radius(i) = sqrt(s_i)",
                   "sum_j w_j [s_j <= s_i]", "a factor 2^17", "do not depend on the summation order", "f in (0, 1]",
                   "enclosed(i) >= f_q total_weight (one fp64 product)", "it is the largest radius", "Unused slots are 0",
                   "the empty body record: all zero, inside 0", "NULL skips the per-body copy", "synchronous", "forgets nothing", "bit for bit",
                   "allocated on first use and freed in nbody_batch_destroy", "names the function", "k outside 1 ... 8", "weight not 0 or 1",
                   "n_fractions outside 0 ... 8", "n_fractions > 0 with fractions NULL", "a fraction outside (0, 1]",
                   "refused before any device work", "Out of scope",
                   "subsets of bodies, softened or velocity-dependent estimators, k > 8, the neighbours' indices, and recentring the state"):
        assert phrase in text, phrase
    # the pairs header, which leaves the neighbour work to this one, is as it was
    assert "neighbour lists" in open(os.path.join(INCLUDE, "nbody_batch_pairs.h")).read()


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert _lib.structure_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                             set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                             set(_lib.fate_names()) | set(_lib.accrete_names()) | set(_lib.field_names()) | set(_lib.pairs_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchStructureBody) == 40 and ctypes.sizeof(_lib.BatchStructureSystem) == 120
    assert [f[0] for f in _lib.BatchStructureBody._fields_] == ["density", "radius", "enclosed", "neighbour_r2", "neighbour_weight",
                                                                "inside", "reserved"]
    assert [f[0] for f in _lib.BatchStructureSystem._fields_] == ["centre", "core_radius", "core_density", "total_weight", "lagrange",
                                                                  "estimated", "reserved"]
    assert _lib.BatchStructureSystem.lagrange.offset == 48 and _lib.BatchStructureSystem.estimated.offset == 112


def test_the_abi_stays_at_version_5_and_a_null_handle_is_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchStructureSystem * 1)()
    assert lib.nbody_batch_structure(None, None, 6, 0, None, 0, out, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_structure: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_surface():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    sig = inspect.signature(nb.BatchedSystem.structure)
    assert list(sig.parameters) == ["self", "k", "weight", "fractions", "bodies"]
    assert [sig.parameters[p].default for p in ("k", "weight", "fractions", "bodies")] == [6, "mass", (0.1, 0.5, 0.9), True]
    assert batch.WEIGHTS == {"mass": 0, "number": 1}
    assert {"StructureResult", "WEIGHTS"} <= set(batch.__all__) and nb.StructureResult is batch.StructureResult
    assert "StructureResult" in nb.__all__
    assert batch.STRUCTURE_BODY_DTYPE.itemsize == 40 and batch.STRUCTURE_SYSTEM_DTYPE.itemsize == 120
    assert batch.STRUCTURE_SYSTEM_DTYPE.fields["lagrange"][1] == 48 and batch.STRUCTURE_BODY_DTYPE.fields["inside"][1] == 32
    # a result built by hand: two systems of capacity 4, the second empty
    systems = np.zeros(2, dtype=batch.STRUCTURE_SYSTEM_DTYPE)
    systems[0] = ((1.0, 2.0, 3.0), 0.5, 7.0, 10.0, (1.0, 3.0, 0, 0, 0, 0, 0, 0), 3, 0)
    bodies = np.zeros((2, 4), dtype=batch.STRUCTURE_BODY_DTYPE)
    bodies[0, :3] = [(2.0, 1.0, 3.0, 4.0, 1.5, 1, 0), (1.0, 2.0, 6.0, np.inf, 0.0, 0, 0), (0.5, 3.0, 10.0, 9.0, 2.0, 2, 0)]
    res = batch.StructureResult(systems, bodies, np.array([0.3, 0.6]), 2, "mass", [3, 0])
    assert res.centre.shape == (2, 3) and res.centre[0].tolist() == [1.0, 2.0, 3.0] and res.lagrangian.shape == (2, 2)
    assert res.lagrangian[0].tolist() == [1.0, 3.0] and res.fractions.tolist() == [0.3, 0.6] and res.estimated.dtype == np.int32
    assert res.neighbour_distance.dtype == np.float64 and res.neighbour_distance[0, :3].tolist() == [2.0, np.inf, 3.0]
    assert res.inside.dtype == np.int32 and res.neighbour_weight.dtype == np.float32 and res.density.dtype == np.float64
    # the host helper follows the header's rule: 0.3 * 10 = 3 -> radius 1; 0.6 -> 2; 1.0 -> 3; empty systems read 0
    assert res.lagrangian_radii([0.3, 0.6, 0.61, 1.0]).tolist() == [[1.0, 2.0, 3.0, 3.0], [0.0, 0.0, 0.0, 0.0]]
    with pytest.raises(ValueError):
        res.lagrangian_radii([0.0])
    none = batch.StructureResult(systems, None, np.array([0.3, 0.6]), 2, "mass", [3, 0])
    assert all(getattr(none, name) is None for name in ("density", "radius", "enclosed", "neighbour_distance", "neighbour_weight", "inside"))
    with pytest.raises(ValueError):
        none.lagrangian_radii([0.5])


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_structure.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
static_assert(sizeof(nbody_batch_structure_body) == 40 && sizeof(nbody_batch_structure_system) == 120, "the records");
int main() {
    try {
        nbody::Batch b(16, 64);
        std::vector<nbody_batch_structure_body> bodies;
        std::vector<nbody_batch_structure_system> s = b.structure(nullptr, 6, NBODY_BATCH_WEIGHT_MASS, {0.1, 0.5, 0.9});
        std::vector<nbody_batch_structure_system> t = b.structure(nullptr, 6, NBODY_BATCH_WEIGHT_NUMBER, {0.5}, bodies);
        std::printf("%lld %lld %lld\n", (long long)s.size(), (long long)t.size(), (long long)bodies.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_structure"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-L" + os.path.join(ROOT, "n_body_problem_amd"),
           "-lnbody_amd", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_structure_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_structure.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_structure_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and "4.1887902047863909846" in text
    assert "lo = fminf(a[t], c)" in text and "c = fmaxf(a[t], c)" in text and "a[t] = lo" in text
    assert '#include "nbody_batch_structure_math.h"' in open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()


# ---- the arithmetic, through the driver ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("structure") / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "batch_structure_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        out = [[float(w) for w in line.split()] if not line.startswith(("ok", "mismatch")) else line for line in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def test_the_list_keeps_the_eight_smallest_as_std_sort_does(driver):
    assert driver(["sorted 1 4000", "sorted 2 4000"]) == ["ok 4000", "ok 4000"]
    inf = float("inf")
    got = driver(["insert", "insert 3 1 2", "insert 5 5 inf 1 5", "insert 9 8 7 6 5 4 3 2 1 0.5 0.25", "insert inf inf",
                  "insert 2 2 2 2 2 2 2 2 2 1"])
    assert got == [[inf] * 8, [1, 2, 3] + [inf] * 5, [1, 5, 5, 5] + [inf] * 4, [0.25, 0.5, 1, 2, 3, 4, 5, 6], [inf] * 8,
                   [1, 2, 2, 2, 2, 2, 2, 2]]
    a = "0.5 1 1 2 3 inf inf inf"
    assert [v[0] for v in driver([f"kth {k} {a}" for k in range(1, 9)])] == [0.5, 1, 1, 2, 3, inf, inf, inf]


def test_the_density_formula_and_zero_without_a_kth_neighbour(driver):
    rng = np.random.default_rng(5)
    r2 = rng.uniform(1e-4, 50.0, size=60).astype(np.float32)
    w = rng.uniform(0.0, 3.0, size=60).astype(np.float32)
    got = np.array([v[0] for v in driver([f"density {float(a)!r} {float(b)!r}" for a, b in zip(r2, w)])])
    want = w.astype(np.float64) / (C * np.sqrt(r2.astype(np.float64)) ** 3)
    assert np.abs(got - want).max() <= 1e-15 * np.abs(want).max() and np.all(np.abs(got - want) <= 4e-16 * want)
    assert np.abs(got - sref.density_of(r2, w)).max() <= 4e-16 * want.max()
    assert driver(["density inf 2.5", "density 4 1", "density 1 0"]) == [[0.0], [1.0 / (C * 8.0)], [0.0]]
    assert abs(C - 4.0 * np.pi / 3.0) < 1e-15


def test_the_record_sizes_offsets_and_the_empty_records(driver):
    assert driver(["layout", "empty"]) == [[40, 0, 8, 16, 24, 28, 32, 120, 0, 24, 32, 40, 48, 112], [0] * 10]


# ---- the reference itself ---------------------------------------------------------------------------------------------------
def line_of_four():
    pos = np.zeros((4, 4), np.float32)
    pos[:, 0], pos[:, 3] = [0.0, 1.0, 3.0, 7.0], [1.0, 2.0, 4.0, 8.0]
    return pos


def test_the_reference_gives_the_hand_worked_numbers_of_four_bodies_on_a_line():
    """Bodies at x = 0, 1, 3, 7 with masses 1, 2, 4, 8, k = 2, in units of 1 / C for the densities (C = 4 pi / 3).
    Squared distances, sorted: body 0 {1, 9, 49}, body 1 {1, 4, 36}, body 2 {4, 9, 16}, body 3 {16, 36, 49}.  So r2_2 = 9, 4, 9,
    36; the one body inside is 1, 0, 1, 2, with weight 2, 1, 2, 4; densities 2/27, 1/8, 2/27, 4/216 = (16, 27, 16, 4) / 216.
    Centre x = (27 * 1 + 16 * 3 + 4 * 7) / 63 = 103 / 63.  Core density = sum rho^2 / sum rho = (1257 / 216) / 63 = 1257 / 13608.
    x - c = (-103, -40, 86, 338) / 63, so the core radius squared is (256 * 10609 + 729 * 1600 + 256 * 7396 + 16 * 114244) /
    (1257 * 3969) = 7603584 / 4989033.  Radii sorted: body 1 (40/63, weight 2), body 2 (86/63, 4), body 0 (103/63, 1), body 3
    (338/63, 8): enclosed 2, 6, 7, 15 of 15.  Fractions 0.1 (1.5), 0.4 (6), 0.5 (7.5), 1 (15): bodies 1, 2, 3, 3."""
    ref = sref.structure(line_of_four(), 4, k=2, fractions=(0.1, 0.4, 0.5, 1.0))
    assert ref["r2_k"].tolist() == [9, 4, 9, 36] and ref["r2_k32"].tolist() == [9, 4, 9, 36]
    assert ref["inside"].tolist() == [1, 1, 1, 1] and ref["neighbour_weight"].tolist() == [2, 1, 2, 4]
    assert ref["inside32"].tolist() == [1, 1, 1, 1] and ref["neighbour_weight32"].tolist() == [2, 1, 2, 4]
    assert np.allclose(ref["density"] * C, [2 / 27, 1 / 8, 2 / 27, 1 / 54], rtol=1e-15)
    assert ref["estimated"] == 4 and ref["total_weight"] == 15.0
    assert np.allclose(ref["centre"], [103 / 63, 0, 0], rtol=1e-15, atol=0)
    assert ref["core_density"] * C == pytest.approx(1257 / 13608, rel=1e-14)
    assert ref["core_radius"] == pytest.approx(np.sqrt(7603584 / 4989033), rel=1e-14)
    assert np.allclose(ref["radius"], np.array([103, 40, 86, 338]) / 63, rtol=1e-14)
    assert ref["enclosed"].tolist() == [7, 2, 6, 15]
    assert np.allclose(ref["lagrange"], np.array([40, 86, 338, 338]) / 63, rtol=1e-14)
    # the number weight: every body weighs 1
    num = sref.structure(line_of_four(), 4, k=2, weight="number", fractions=(0.5,))
    assert num["neighbour_weight"].tolist() == [1, 1, 1, 1] and num["total_weight"] == 4.0 and num["enclosed"].max() == 4.0
    # k = 3: every body has exactly three neighbours; k = 4: none has, and the centre is the centre of weight
    assert sref.structure(line_of_four(), 4, k=3)["r2_k"].tolist() == [49, 36, 16, 49]
    none = sref.structure(line_of_four(), 4, k=4)
    assert np.all(np.isinf(none["r2_k"])) and none["estimated"] == 0 and not none["density"].any()
    assert none["centre"].tolist() == [(2 + 12 + 56) / 15, 0, 0] and none["core_radius"] == 0 and none["core_density"] == 0
    assert none["lagrange"][1] > 0


def test_ties_coincident_bodies_and_empty_systems_in_the_reference():
    pos = np.zeros((3, 4), np.float32)
    pos[:, 0], pos[:, 3] = [0.0, 1.0, -1.0], 1.0
    ref = sref.structure(pos, 3, k=2)
    # body 0 has two neighbours at r2 = 1: the second is the k-th, and its tie is not inside
    assert ref["r2_k"].tolist() == [1, 4, 4] and ref["inside"].tolist() == [0, 1, 1] and ref["density"][0] == 0
    assert ref["inside32"].tolist() == [0, 1, 1]
    twins = np.zeros((3, 4), np.float32)
    twins[:, 0], twins[:, 3] = [2.0, 2.0, 5.0], 1.0             # bodies 0 and 1 coincide: they are not each other's neighbours
    ref = sref.structure(twins, 3, k=1)
    assert ref["r2_k"].tolist() == [9, 9, 9] and ref["inside"].tolist() == [0, 0, 0] and ref["estimated"] == 3
    assert np.all(np.isinf(sref.structure(twins, 3, k=2)["r2_k"][:2]))
    for n in (0, 1):
        e = sref.structure(twins, n, k=1)
        assert e["estimated"] == 0 and e["core_radius"] == 0 and e["total_weight"] == float(n) and e["centre"].tolist() == [2.0 * n, 0, 0]
        assert e["lagrange"].tolist() == [0, 0, 0]
    zero = sref.structure(np.zeros((5, 4), np.float32), 5, k=1)
    assert zero["total_weight"] == 0 and not zero["centre"].any() and not zero["lagrange"].any() and zero["estimated"] == 0


def test_inversion_symmetric_shells_have_their_closed_values_in_the_reference():
    pos, closed = sref.shells()
    n = closed["n"]
    for k in sref.KS:
        for weight in sref.WEIGHTS:
            ref = sref.structure(pos, n, k=k, weight=weight, fractions=(0.25, 0.5))
            print(k, weight, ref["centre"] - closed["centre"], ref["lagrange"], ref["core_radius"])
            assert np.abs(ref["centre"] - closed["centre"]).max() <= 1e-13
            assert abs(ref["lagrange"][0] - 1.0) <= 1e-12 and abs(ref["lagrange"][1] - 2.0) <= 1e-12
            assert ref["estimated"] == n
            assert np.array_equal(ref["r2_k32"].astype(np.float64), ref["r2_k"])      # every r2 is exact in fp32
            assert np.array_equal(ref["density"][:n // 2], ref["density"][n // 2:])   # mirrored bodies


def test_the_inputs_condition():
    """On every input of the GPU suite and k in {1, 6, 8}: (a) the emulated fp32 r2_k is within 1e-6 relative of the fp64 one on
    every row (three fp32 roundings bound it at about 3e-7); (b) the fp32 inside set equals the fp64 one on at least 99 % of
    each system's rows, and so do the rows whose rank gaps exceed 1e-6, which are the rows the GPU test holds to exactness;
    (c) every row's s_i differs from every other's by more than 1e-9 relative at the reference's centre, so that the order of
    the radii, and with it enclosed and the Lagrangian radii, is round-off proof."""
    seen, worst = 0, 0.0
    for capacity, k, weight in sref.all_cases():
        P, counts = sref.gpu_inputs(capacity, k, weight)
        for s, (n, ref) in enumerate(zip(counts, sref.reference(capacity, k, weight))):
            seen += 1
            if n == 0:
                continue
            fin = np.isfinite(ref["r2_k"])
            assert np.array_equal(fin, np.isfinite(ref["r2_k32"]))
            err = float(np.max(np.abs(ref["r2_k32"][fin].astype(np.float64) - ref["r2_k"][fin]) / ref["r2_k"][fin], initial=0.0))
            worst = max(worst, err)
            assert err <= 1e-6, (capacity, k, s, err)                                                       # (a)
            assert ref["same_set"].sum() >= 0.99 * n and ref["gap_ok"].sum() >= 0.99 * n, (capacity, k, s)  # (b)
            assert np.all(ref["same_set"][ref["gap_ok"]]), (capacity, k, s)
            ss = np.sort(ref["s"])
            gap = float(np.min((ss[1:] - ss[:-1]) / ss[1:], initial=1.0))
            assert gap > 1e-9, (capacity, k, s, gap)                                                        # (c)
            mass = P[s, :n, 3]
            assert mass.max() / mass.min() < 2.0 ** 17                                 # the header's premise of exact sums
    print(f"{seen} systems, worst r2_k error {worst:.3g}")
    assert seen == (4 * 6 + 2) * 3 + 6 * 3
