"""Surface maps of batches without a GPU (include/nbody_batch_surface.h): the surface -- header, records, mirrors, export
list, C++ wrapper, build dependencies -- the premises of the shared inputs, every byte of every record that the arithmetic of
csrc/nbody_batch_surface_math.h gives on the CPU (a stand-alone g++ program, tests/batch_surface_driver.cpp, that runs the
kernel's three phases for any workgroup shape, once more under the address and undefined-behaviour sanitizers) against the
Python-float reference tests/hermite_surface_ref.py, and the derived quantities of SurfaceMapResult against closed forms."""
import ctypes
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_surface_ref as sref
from conftest import ROOT

NAMES = ["nbody_batch_surface_map"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
CELL_WORDS = ("count", "weight", "v1", "v2", "pa", "pb", "z1", "z2")
CELL_OFFSETS = [0, 8, 16, 24, 32, 40, 48, 56]
SYSTEM_WORDS = ("selected", "outside", "unmeasured", "columns", "rows", "occupied", "peak", "peak_count", "total_weight", "centre",
                "velocity")
SYSTEM_OFFSETS = [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 64]
BODY_WORDS = ("cell", "reserved", "a", "b")
BODY_OFFSETS = [0, 4, 8, 16]
HELPERS = ("surface_density", "number_density", "mean_velocity", "dispersion", "plane_velocity", "mean_depth", "depth_dispersion",
           "image", "grid", "view", "area")


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_radial_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_surface.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_surface.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_radial.h"') < nbody_h.index('#include "nbody_batch_surface.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_64_88_and_24_bytes(tmp_path):
    lines = ['#include "nbody.h"', "#include <stddef.h>",
             "typedef char cell_size[sizeof(nbody_batch_surface_cell) == 64 ? 1 : -1];",
             "typedef char system_size[sizeof(nbody_batch_surface_system) == 88 ? 1 : -1];",
             "typedef char body_size[sizeof(nbody_batch_surface_body) == 24 ? 1 : -1];",
             "typedef char count_is_long_long[sizeof(((nbody_batch_surface_cell *)0)->count) == 8 ? 1 : -1];",
             "typedef char limit[NBODY_BATCH_SURFACE_MAX_SIDE == 64 ? 1 : -1];",
             "typedef char words[NBODY_BATCH_SURFACE_OUTSIDE == -1 && NBODY_BATCH_SURFACE_UNMEASURED == -2 && "
             "NBODY_BATCH_SURFACE_NOT_TAKING == -3 ? 1 : -1];"]
    for record, names, offsets in (("cell", CELL_WORDS, CELL_OFFSETS), ("system", SYSTEM_WORDS, SYSTEM_OFFSETS),
                                   ("body", BODY_WORDS, BODY_OFFSETS)):
        for name, offset in zip(names, offsets):
            lines.append(f"typedef char {record}_{name}_at_{offset}[offsetof(nbody_batch_surface_{record}, {name}) == {offset} ? 1 : -1];")
    lines += ["int main(void) {", "    nbody_batch_surface_system s;", "    double edges[2] = {0.0, 1.0};",
              "    return (nbody_batch_surface_map(0, 0, 0, 1, 1, edges, edges, 0, 0, 0, 0, NBODY_BATCH_WEIGHT_MASS, 0, &s, 0, 0) != NBODY_ERR_INVALID)"
              " + (NBODY_ABI_VERSION != 5);", "}"]
    src = tmp_path / "surface.c"
    src.write_text("\n".join(lines) + "\n")
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_surface.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_radial.h",
                   "takes part iff i < min(counts[s], max_bodies) and subset is NULL or", "nbody_batch_radial.h's rule",
                   "NBODY_BATCH_WEIGHT_MASS (0", "NBODY_BATCH_WEIGHT_NUMBER (1)", "widened to fp64", "or NULL for zeros",
                   "or NULL for the identity: A = x, B = y, Q = z", "orthonormality is the caller's business",
                   "basic operations only, nothing contracted", "No word passes through a square root or a division",
                   "the same on any IEEE hardware", "d_k = (double)x_k - c_k", "u_k = (double)v_k - v0_k",
                   "a = (A_x d_x + A_y d_y) + A_z d_z", "b = (B_x d_x + B_y d_y) + B_z d_z", "q = (Q_x d_x + Q_y d_y) + Q_z d_z",
                   "ua = (A_x u_x + A_y u_y) + A_z u_z", "ub = (B_x u_x + B_y u_y) + B_z u_z", "uq = (Q_x u_x + Q_y u_y) + Q_z u_z",
                   "1 <= columns, rows <= NBODY_BATCH_SURFACE_MAX_SIDE (64)", "strictly ascending",
                   "unmeasured iff any of a, b, q, ua, ub, uq is not finite",
                   "outside iff otherwise a < ea[0] || a >= ea[columns] || b < eb[0] || b >= eb[rows]",
                   "ea[i] <= a < ea[i + 1] and eb[j] <= b < eb[j + 1]", "half-open on the right",
                   "numpy.histogram2d's rule except that the last edge is not closed", "The cell index is j * columns + i",
                   "outside + sum of count + unmeasured == selected", "64 bytes", "88 bytes", "24 bytes",
                   "v1 (16) sum of w uq", "v2 (24) sum of w (uq uq)", "pa (32) sum of w ua", "pb (40) sum of w ub", "z1 (48) sum of w q",
                   "z2 (56) sum of w (q q)", "in ascending body index", "one fp64 add per member and term",
                   "the parenthesis first and then the product with w",
                   "the same bits in any slot, n_systems, max_bodies and workgroup shape", "An empty cell reads 0 everywhere",
                   "ties to the lower index, -1 if there is none", "outside bodies included",
                   "nbody_batch_radial_profile's total_weight, bit for bit, on finite states",
                   "-1 outside, -2 unmeasured, -3 not taking part", "Slots from the count on hold -3 and zeros",
                   "the same bits either way", "synchronous", "forgets nothing", "bit for bit",
                   "grown when a later call asks for more cells", "freed in nbody_batch_destroy", "names the function",
                   "a NULL handle", "NULL d_positions_xyzm, d_velocities, edges_a, edges_b or systems_out",
                   "columns or rows outside 1 ... 64", "an edge that is NaN or infinite",
                   "the message names the axis, the system and the edge", "a weight that is not 0 or 1",
                   "a centre, velocity or axes value that is not finite", "refused before any device work", "Out of scope",
                   "perspective", "smoothing kernels and cloud-in-cell deposit", "3-D meshes", "position-velocity diagrams",
                   "more than 64 x 64 cells", "maps across systems", "device-side outputs", "the single-system context"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.surface_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.radial_names()) | set(_lib.approaches_names()))
    fn = lib.nbody_batch_surface_map
    assert fn.argtypes is not None and len(fn.argtypes) == 16
    for mirror, size, names, offsets in ((_lib.BatchSurfaceCell, 64, CELL_WORDS, CELL_OFFSETS),
                                         (_lib.BatchSurfaceSystem, 88, SYSTEM_WORDS, SYSTEM_OFFSETS),
                                         (_lib.BatchSurfaceBody, 24, BODY_WORDS, BODY_OFFSETS)):
        assert ctypes.sizeof(mirror) == size and [f[0] for f in mirror._fields_] == list(names)
        assert [getattr(mirror, w).offset for w in names] == offsets
    assert _lib.BATCH_SURFACE_MAX_SIDE == 64
    assert batch.SURFACE_SYSTEM_DTYPE == sref.SYSTEM_DTYPE and batch.SURFACE_CELL_DTYPE == sref.CELL_DTYPE
    assert batch.SURFACE_BODY_DTYPE == sref.BODY_DTYPE
    assert [batch.SURFACE_CELL_DTYPE.fields[w][1] for w in CELL_WORDS] == CELL_OFFSETS
    assert [batch.SURFACE_SYSTEM_DTYPE.fields[w][1] for w in SYSTEM_WORDS] == SYSTEM_OFFSETS
    assert [batch.SURFACE_BODY_DTYPE.fields[w][1] for w in BODY_WORDS] == BODY_OFFSETS
    for name in ("SurfaceMapResult", "SURFACE_SYSTEM_DTYPE", "SURFACE_CELL_DTYPE", "SURFACE_BODY_DTYPE"):
        assert name in nb.__all__ and getattr(nb, name) is getattr(batch, name), name
    assert batch.SurfaceMapResult.__doc__ and batch.BatchedSystem.surface_map.__doc__
    for helper in HELPERS:
        assert getattr(batch.SurfaceMapResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_surface_map") == 1
    assert exports[exports.index("nbody_batch_surface_map") - 1].startswith("# nbody_batch_surface_map:")
    names = [line for line in exports if not line.startswith("#")]
    assert names == sorted(names)


def test_the_cpp_wrapper_compiles_with_a_lean_and_a_full_call(tmp_path):
    src = tmp_path / "batch_surface.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_surface_system> both(nbody::Batch &b, const float *pos, const float *vel)
{
    std::vector<nbody_batch_surface_cell> cells;
    std::vector<nbody_batch_surface_body> bodies;
    const std::vector<double> a{-1.0, 0.0, 0.5, 1.0}, c{-2.0, 0.0, 2.0};
    std::vector<nbody_batch_surface_system> lean = b.surfaceMap(pos, vel, 3, 2, a, c);
    b.surfaceMap(pos, vel, 3, 2, a, c, &cells, std::vector<double>(3 * 16, 0.0), std::vector<double>(3 * 16, 0.0),
                 std::vector<double>(9 * 16, 1.0), NBODY_BATCH_WEIGHT_NUMBER, std::vector<unsigned char>(16 * 64, 1), &bodies);
    return lean;
}
''')
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_every_error_is_refused_before_any_device_work(lib):
    """A NULL handle is refused first, with the function's name, by the library itself.  The other cases need a handle
    (test_batch_surface_gpu.py walks them); here the source shows that each is refused before the first device call."""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchSurfaceSystem * 1)()
    edges = (ctypes.c_double * 2)(0.0, 1.0)
    assert lib.nbody_batch_surface_map(None, None, None, 1, 1, edges, edges, 0, None, None, None, 0, None, out, None, None) == \
        _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_surface_map: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_surface_map("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_surface_map: batch is NULL", "nbody_batch_surface_map: NULL argument",
                "nbody_batch_surface_map: columns and rows must be 1 ... 64", "nbody_batch_surface_map: weight must be",
                '" must be finite"', "the edges must be strictly ascending", "nbody_batch_surface_map: the centre of system ",
                "nbody_batch_surface_map: the velocity of system ", "nbody_batch_surface_map: the axes of system ")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_surface_map: ') == len(messages)                          # every message names the function


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_roots_and_fused_operations():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_surface_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_surface.h" for h in build.HEADERS)
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(CSRC, "nbody_batch_surface_math.h")).read()
    code = re.sub(r"//.*", "", text)
    assert "hip/" not in code and "NBODY_HD inline" in code and "fma(" not in code and "fmaf(" not in code and "float " in code
    assert "sqrt" not in code and " / " not in code                                          # no square root, no division
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_surface_kernel("):source.index("hipError_t launch_batch_surface(")]
    for call in ("surface_words(", "surface_cell(", "surface_word(", "surface_body(", "surface_body_absent(", "surface_key(",
                 "surface_rank_step(", "surface_is_start(", "surface_walk(", "surface_walk_total(", "surface_peak_key(",
                 "surface_system("):
        assert call in kernel, call
    assert "asm" not in kernel and "fma" not in kernel and "sqrt" not in kernel
    launch = source[source.index("hipError_t launch_batch_surface("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "with_rpl(" in launch and "launch_analysis_kernel(" in launch
    assert "2 * kBatchBytesPerBody * (size_t)max_bodies" in kernel                           # launch_batch_pairs' image
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchSurfaceSystem> surface_systems", "DeviceArray<BatchSurfaceCell> surface_cells",
                   "DeviceArray<BatchSurfaceBody> surface_bodies", "DeviceArray<unsigned char> surface_subset",
                   "DeviceArray<double> surface_edges", "DeviceArray<double> surface_frames"):
        assert member in members, member
    entry = source[source.index("int nbody_batch_surface_map("):]
    assert "hipFree" not in entry[:entry.index("\n}\n")] and "hipMalloc" not in entry[:entry.index("\n}\n")]


def test_the_lds_of_the_largest_launch_fits_a_gfx950_workgroup():
    """The launcher's sum, recomputed: 32 bytes per body, two 16-bit words per padded body, one per cell, and the static arrays."""
    dynamic = 32 * 4096 + 2 * 2 * 4096 + 2 * 4096
    static = 2 * 65 * 8 + 15 * 8 + 5 * 4                                                     # 1180; 1216 with the compiler's padding
    assert dynamic == 155648 and dynamic + static <= 155648 + 1216 == 156864 <= 160 * 1024
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    assert "155648 bytes" in source and "1216 bytes" in source and "156864 bytes" in source


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_surface_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        return res.stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("surface"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("surface_checked"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def number(v):
    v = float(v)
    return v.hex() if math.isfinite(v) else ("nan" if v != v else ("inf" if v > 0 else "-inf"))


def command(pos, vel, n, shape, ea, eb, centre, velocity, axes, weight, subset, want=1):
    T, rpl = shape
    head = f"system {n} {pos.shape[0]} {T} {rpl} {len(ea) - 1} {len(eb) - 1} {1 if weight == 'number' else 0} {want}"
    lines = [head, " ".join(number(e) for e in ea), " ".join(number(e) for e in eb),
             " ".join(number(c) for c in list(centre) + list(velocity) + list(np.asarray(axes).ravel()))]
    for i in range(n):
        take = 1 if subset is None else int(subset[i] != 0)
        lines.append(" ".join(number(w) for w in (*pos[i], *vel[i, :3])) + f" {take}")
    return "\n".join(lines) + "\n"


def run_batch(run, pos, vel, counts, shape, want, edges_a, edges_b, centre, velocity, axes, weight, subset, only=None):
    """The driver's records of the systems `only` (all) of a batch: systems, cells (rows, columns) or None, bodies."""
    text = ""
    ea, eb = np.asarray(edges_a), np.asarray(edges_b)
    which = list(range(pos.shape[0])) if only is None else list(only)
    for s in which:
        text += command(pos[s], vel[s], int(counts[s]), shape, ea[s] if ea.ndim == 2 else ea, eb[s] if eb.ndim == 2 else eb, centre[s],
                        velocity[s], axes[s], weight, None if subset is None else subset[s], want)
    out = run(text)
    rows, columns = eb.shape[-1] - 1, ea.shape[-1] - 1
    systems = np.stack([np.frombuffer(bytes.fromhex(out[3 * k]), dtype=sref.SYSTEM_DTYPE)[0] for k in range(len(which))])
    cells = np.stack([np.frombuffer(bytes.fromhex(out[3 * k + 1]), dtype=sref.CELL_DTYPE).reshape(rows, columns)
                      for k in range(len(which))]) if want else None
    bodies = np.stack([np.frombuffer(bytes.fromhex(out[3 * k + 2]), dtype=sref.BODY_DTYPE) for k in range(len(which))])
    if not want:
        assert all(out[3 * k + 1] == "" for k in range(len(which)))
    return systems, cells, bodies


reference = sref.reference


def test_the_layout(driver):
    words = [int(w) for w in driver("layout\n")[0].split()]
    assert words == [64, *CELL_OFFSETS, 88, *SYSTEM_OFFSETS, 24, *BODY_OFFSETS]


@pytest.mark.parametrize("capacity", sref.CAPACITIES)
def test_the_inputs_do_their_work(capacity):
    """The shared inputs reach what they are there for: the identity holds in every case; empty and full systems; the three
    fates besides membership; bodies on the first, the last and an interior edge; masks; and the shapes at which a sort by cell
    can go wrong -- one cell with every body, every body in its own cell, the cells in descending order of the bodies, members of
    one cell in several waves, and a cell whose sum depends on the order of its members."""
    assert sref.shape_of(capacity) == sref.SHAPES[sref.CAPACITIES.index(capacity)]
    generic, one, own, reverse, order = (len(sref.COUNTS) + k for k in range(5))
    for case in sref.CASES:
        pos, vel, counts, kw, (systems, cells, bodies) = reference(capacity, case[0])
        assert list(counts) == sref.batch_counts(capacity)
        assert np.array_equal(systems["outside"] + cells["count"].sum(axis=(1, 2)) + systems["unmeasured"], systems["selected"])
        assert np.array_equal(systems["occupied"], (cells["count"] > 0).sum(axis=(1, 2)))
        assert (bodies["cell"][0] == sref.NOT_TAKING).all() and systems["peak"][0] == -1 and systems["peak_count"][0] == 0
        if case[6] == "none":
            assert np.array_equal(systems["selected"], counts)
            assert systems["unmeasured"][generic] == 3 and bodies["cell"][generic, 3:6].tolist() == [-2, -2, -2]
            assert systems["outside"][generic] > 0
        elif case[6] == "all-false":
            assert not systems["selected"].any() and not cells["count"].any() and (bodies["cell"] == sref.NOT_TAKING).all()
        else:
            assert 0 < systems["selected"][generic] < counts[generic]
    pos, vel, counts, kw, (systems, cells, bodies) = reference(capacity, "64x64-mass")
    n = capacity
    assert bodies["cell"][generic, 6] == 0 and bodies["a"][generic, 6] == -sref.HALF == kw["edges_a"][0]          # on the first edge: inside
    assert bodies["cell"][generic, 7] == sref.OUTSIDE and bodies["a"][generic, 7] == sref.HALF == kw["edges_a"][-1]  # on the last: outside
    assert bodies["cell"][generic, 8] == 33 * 64 + 32 and bodies["a"][generic, 8] == kw["edges_a"][32]             # on an interior edge: above it
    assert bodies["b"][generic, 8] == kw["edges_b"][33]
    assert systems["occupied"][one] == 1 and systems["peak_count"][one] == n and systems["peak"][one] == 32 * 64 + 32
    assert np.array_equal(bodies["cell"][own], np.arange(n)) and systems["occupied"][own] == n and systems["peak"][own] == 0
    assert np.array_equal(bodies["cell"][reverse], n - 1 - np.arange(n)) and systems["peak_count"][reverse] == 1
    pos, vel, counts, kw, (systems, cells, bodies) = reference(capacity, "1x1-mass")
    members = np.flatnonzero(bodies["cell"][order] == 0)
    assert members[0] == 0 and len(members) > n // 2 and members[-1] > n - 8               # in every wave of the workgroup
    assert cells["weight"][order, 0, 0] == sref.BIG                                          # 2^53 + 1 + 1 + ... in ascending index
    backwards = 0.0
    for i in members[::-1]:
        backwards += float(pos[order, i, 3])
    assert backwards >= sref.BIG + len(members) - 2 > sref.BIG                              # any order that adds ones first differs


@pytest.mark.parametrize("capacity", sref.CAPACITIES)
@pytest.mark.parametrize("case", [c[0] for c in sref.CASES])
def test_the_driver_gives_the_references_records_byte_for_byte(driver, capacity, case):
    """Every byte of every record, for the workgroup shape of this capacity, with and without the cell records."""
    pos, vel, counts, kw, (systems, cells, bodies) = reference(capacity, case)
    shape = sref.shape_of(capacity)
    got = run_batch(driver, pos, vel, counts, shape, 1, **kw)
    assert got[0].tobytes() == systems.tobytes(), (got[0], systems)
    assert got[1].tobytes() == cells.tobytes()
    assert got[2].tobytes() == bodies.tobytes()
    lean = run_batch(driver, pos, vel, counts, shape, 0, **kw)
    assert lean[0].tobytes() == systems.tobytes() and lean[2].tobytes() == bodies.tobytes()


def test_the_records_do_not_depend_on_the_workgroup_shape(driver):
    pos, vel, counts, kw, (systems, cells, bodies) = reference(64, "64x64-each-view")
    for shape in sref.SHAPES:
        got = run_batch(driver, pos, vel, counts, shape, 1, **kw)
        assert got[0].tobytes() == systems.tobytes() and got[1].tobytes() == cells.tobytes() and got[2].tobytes() == bodies.tobytes()


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    for capacity, names, only in ((320, [c[0] for c in sref.CASES], None), (64, ["64x64-mass", "1x1-mass"], None),
                                  (4096, ["64x64-mass"], (4, 6, 7)), (4096, ["1x1-mass"], (8,))):
        for name in names:
            pos, vel, counts, kw, (systems, cells, bodies) = reference(capacity, name)
            which = list(range(len(counts))) if only is None else list(only)
            got = run_batch(checked_driver, pos, vel, counts, sref.shape_of(capacity), 1, only=only, **kw)
            assert got[0].tobytes() == systems[which].tobytes() and got[1].tobytes() == cells[which].tobytes()
            assert got[2].tobytes() == bodies[which].tobytes()
            lean = run_batch(checked_driver, pos, vel, counts, sref.shape_of(capacity), 0, only=which[:2], **kw)
            assert lean[0].tobytes() == systems[which[:2]].tobytes()


# ---- the derived quantities ----------------------------------------------------------------------------------------------------
def result_of(pos, vel, edges_a, edges_b, weight="number", axes=None, mass=None):
    from n_body_problem_amd.batch import SurfaceMapResult
    pos4 = np.zeros((1, len(pos), 4), dtype=np.float32)
    pos4[0, :, :3], pos4[0, :, 3] = pos, 1.0 if mass is None else mass
    vel4 = np.zeros((1, len(pos), 4), dtype=np.float32)
    vel4[0, :, :3] = vel
    ea, eb = np.asarray(edges_a, dtype=np.float64), np.asarray(edges_b, dtype=np.float64)
    view = np.eye(3)[None] if axes is None else np.asarray(axes, dtype=np.float64).reshape(1, 3, 3)
    systems, cells, bodies = sref.surface_batch(pos4, vel4, [len(pos)], ea, eb, axes=view, weight=weight)
    return SurfaceMapResult(systems, cells, bodies, ea, eb, view, weight)


def test_a_uniform_lattice_has_a_flat_surface_density_and_the_columns_depth_moments():
    """One body per unit volume at the integer points of -6 ... 5 cubed, seen along z in cells two wide from -6 to 6: every cell
    holds 2 x 2 x 12 bodies, so both densities are 12 per unit area, the mean depth is that of the integers -6 ... 5, -1/2,
    and the depth dispersion theirs, sqrt((12^2 - 1) / 12).  With masses of 2 the surface density doubles and the moments stay."""
    from n_body_problem_amd.batch import SurfaceMapResult
    axis = np.arange(-6, 6)
    pts = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    edges = SurfaceMapResult.grid(6.0, 6)
    assert np.array_equal(edges, np.linspace(-6.0, 6.0, 7)) and np.array_equal(SurfaceMapResult.grid((-6.0, 6.0), 6), edges)
    assert SurfaceMapResult.grid(np.array([[0.0, 1.0], [0.0, 2.0]]), 4).tolist() == [[0, 0.25, 0.5, 0.75, 1.0], [0, 0.5, 1.0, 1.5, 2.0]]
    res = result_of(pts, np.zeros_like(pts), edges, edges)
    assert np.array_equal(res.area(), np.full((1, 6, 6), 4.0)) and np.array_equal(res.count, np.full((1, 6, 6), 48))
    assert np.array_equal(res.surface_density(), np.full((1, 6, 6), 12.0)) and np.array_equal(res.number_density(), res.surface_density())
    assert np.array_equal(res.mean_depth(), np.full((1, 6, 6), -0.5))
    assert np.allclose(res.depth_dispersion(), math.sqrt(143.0 / 12.0), rtol=1e-14)
    assert not res.mean_velocity().any() and not res.dispersion().any()
    assert res.occupied[0] == 36 and res.peak[0] == 0 and res.peak_count[0] == 48 and res.total_weight[0] == 12 ** 3
    heavy = result_of(pts, np.zeros_like(pts), edges, edges, weight="mass", mass=2.0)
    assert np.array_equal(heavy.surface_density(), 2.0 * res.surface_density()) and np.array_equal(heavy.mean_depth(), res.mean_depth())
    array, extent = res.image(0, "count")
    assert array.shape == (6, 6) and extent == (-6.0, 6.0, -6.0, 6.0) and array.dtype == np.int64
    assert np.array_equal(res.image(0)[0], res.surface_density()[0])
    with pytest.raises(ValueError, match="quantity must be"):
        res.image(0, "plane_velocity")
    with pytest.raises(ValueError, match="extent must be"):
        SurfaceMapResult.grid((0.0, 1.0, 2.0), 4)
    assert "SurfaceMapResult(columns=6, rows=6" in repr(res)


def test_a_rigid_rotation_seen_edge_on_has_the_line_of_sight_velocity_omega_a_and_no_dispersion_within_a_column():
    """A disc in the plane z = 0 turning rigidly about z with omega: seen along y (edge-on, A = z x y ... the view of direction y),
    the line-of-sight velocity of a body is omega times its coordinate along the map's first axis up to the sign of that axis,
    whatever its depth.  With one body column per cell the dispersion is 0 and the mean is exact; face-on the line-of-sight
    velocity vanishes and the plane velocity is the rotation's."""
    from n_body_problem_amd.batch import SurfaceMapResult
    omega = 0.5
    axis = np.arange(-4, 5).astype(np.float64)
    pts = np.stack(np.meshgrid(axis, axis, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    vel = omega * np.stack([-pts[:, 1], pts[:, 0], np.zeros(len(pts))], axis=1)
    edges = np.arange(-4.5, 5.0)
    view = SurfaceMapResult.view((0.0, 1.0, 0.0))
    assert np.array_equal(view, [[-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])           # A = up x Q, B = Q x A, Q
    res = result_of(pts, vel, edges, [-0.5, 0.5], axes=view)
    assert res.count.shape == (1, 1, 9) and np.array_equal(res.count[0, 0], np.full(9, 9))
    centres = 0.5 * (edges[1:] + edges[:-1])                                                  # a = -x and uq = vy = omega x = -omega a
    assert np.array_equal(res.mean_velocity()[0, 0], -omega * centres) and not res.dispersion().any()
    assert not res.mean_depth().any() and np.allclose(res.depth_dispersion()[0, 0], math.sqrt(80.0 / 12.0), rtol=1e-14)
    face = result_of(pts, vel, edges, edges)
    assert np.array_equal(face.count[0], np.ones((9, 9))) and not face.mean_velocity().any() and not face.depth_dispersion().any()
    pa, pb = face.plane_velocity()
    assert np.array_equal(pa[0], -omega * centres[:, None] * np.ones(9)) and np.array_equal(pb[0], omega * centres[None, :] * np.ones((9, 1)))


def test_two_streams_in_one_cell_have_their_mean_and_dispersion_and_empty_cells_read_nan():
    """Bodies of weights 1 and 3 with line-of-sight velocities +2 and -2 in one cell: mean (1 * 2 - 3 * 2) / 4 = -1 and
    dispersion sqrt(4 - 1) = sqrt(3); the cell beside it is empty."""
    pts = np.array([[0.5, 0.5, 1.0], [0.25, 0.75, -1.0]])
    vel = np.array([[1.0, 0.0, 2.0], [1.0, 4.0, -2.0]])
    res = result_of(pts, vel, [0.0, 1.0, 2.0], [0.0, 1.0], weight="mass", mass=np.array([1.0, 3.0]))
    assert res.count[0].tolist() == [[2, 0]] and res.weight_sum[0, 0, 0] == 4.0
    assert res.mean_velocity()[0, 0, 0] == -1.0 and res.dispersion()[0, 0, 0] == math.sqrt(3.0)
    pa, pb = res.plane_velocity()
    assert pa[0, 0, 0] == 1.0 and pb[0, 0, 0] == 3.0
    assert res.mean_depth()[0, 0, 0] == -0.5 and res.depth_dispersion()[0, 0, 0] == math.sqrt(1.0 - 0.25)
    for derived in (res.mean_velocity(), res.dispersion(), pa, pb, res.mean_depth(), res.depth_dispersion()):
        assert derived.shape == (1, 1, 2) and np.isnan(derived[0, 0, 1])
    assert res.surface_density()[0, 0, 1] == 0.0 and res.number_density()[0, 0, 0] == 2.0
    from n_body_problem_amd.batch import SurfaceMapResult
    lean = SurfaceMapResult(res.systems, None, None, res.edges_a, res.edges_b, res.axes, "mass")
    assert lean.count is None and lean.body_cell is None and lean.total_weight[0] == 4.0
    with pytest.raises(ValueError, match="cells=True"):
        lean.surface_density()


def test_view_builds_right_handed_orthonormal_triples_for_any_direction():
    from n_body_problem_amd.batch import SurfaceMapResult
    rng = np.random.default_rng(7)
    directions = np.concatenate([rng.normal(size=(50, 3)), np.eye(3), -np.eye(3), [[0.0, 0.0, 5.0]]])
    views = SurfaceMapResult.view(directions)
    assert views.shape == (len(directions), 3, 3)
    for d, v in zip(directions, views):
        assert np.allclose(v @ v.T, np.eye(3), atol=1e-14) and np.linalg.det(v) == pytest.approx(1.0, abs=1e-14)
        assert np.allclose(v[2], d / np.linalg.norm(d), atol=1e-15) and np.allclose(np.cross(v[0], v[1]), v[2], atol=1e-14)
        assert np.array_equal(SurfaceMapResult.view(d), v)
    tilted = SurfaceMapResult.view((1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    assert np.array_equal(tilted, [[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])       # looking along x: y to the right, z up
    with pytest.raises(ValueError, match="direction must"):
        SurfaceMapResult.view((0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="direction must have shape"):
        SurfaceMapResult.view(np.zeros((2, 2)))
