"""CPU-only: the approach lists of batched ensembles (nbody_batch_approaches, include/nbody_batch_approaches.h).  The header is
self-contained C99, included by nbody.h after the contacts header, and declares its one entry point alone; it is exported,
bound and listed apart; the arithmetic without a GPU (csrc/nbody_batch_approaches_math.h), built into a stand-alone driver with
g++ -- once more with the address and undefined-behaviour sanitizers -- that runs the kernel's three steps for any workgroup
shape, gives the reference's records and list on every input of the GPU suite exactly, at list capacities on both sides of the
number of approaches, whether the separation at the horizon is computed for every pair or only where it decides; on every input
every word of every chain and of the predicate is an integer that fp32 holds, which is the premise of all the exact
comparisons; the inputs contain what they are there for, each hand-placed pair in its intended phase; and the helpers of
ApproachesResult do what they say on hand-made records."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_approaches_ref as aref
from conftest import ROOT

NAMES = ["nbody_batch_approaches"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
SYSTEM_WORDS = ("bodies", "approaching", "max_degree", "reserved", "pairs", "stored", "now", "passing", "ending", "reserved2")
BODY_WORDS = ("degree", "upper", "first", "now")
ENTRY_WORDS = ("i", "j", "r2", "rv", "v2", "phase")
SHAPES = aref.SHAPES


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_contacts_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_approaches.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_approaches.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_contacts.h"') < nbody_h.index('#include "nbody_batch_approaches.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_48_16_and_24_bytes(tmp_path):
    src = tmp_path / "approaches.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char system_is_48_bytes[sizeof(nbody_batch_approach_system) == 48 ? 1 : -1];
typedef char bodies_at_0[offsetof(nbody_batch_approach_system, bodies) == 0 ? 1 : -1];
typedef char approaching_at_4[offsetof(nbody_batch_approach_system, approaching) == 4 ? 1 : -1];
typedef char max_degree_at_8[offsetof(nbody_batch_approach_system, max_degree) == 8 ? 1 : -1];
typedef char reserved_at_12[offsetof(nbody_batch_approach_system, reserved) == 12 ? 1 : -1];
typedef char pairs_at_16[offsetof(nbody_batch_approach_system, pairs) == 16 ? 1 : -1];
typedef char stored_at_24[offsetof(nbody_batch_approach_system, stored) == 24 ? 1 : -1];
typedef char now_at_32[offsetof(nbody_batch_approach_system, now) == 32 ? 1 : -1];
typedef char passing_at_36[offsetof(nbody_batch_approach_system, passing) == 36 ? 1 : -1];
typedef char ending_at_40[offsetof(nbody_batch_approach_system, ending) == 40 ? 1 : -1];
typedef char reserved2_at_44[offsetof(nbody_batch_approach_system, reserved2) == 44 ? 1 : -1];
typedef char pairs_is_long_long[sizeof(((nbody_batch_approach_system *)0)->pairs) == 8 ? 1 : -1];
typedef char body_is_16_bytes[sizeof(nbody_batch_approach_body) == 16 ? 1 : -1];
typedef char degree_at_0[offsetof(nbody_batch_approach_body, degree) == 0 ? 1 : -1];
typedef char upper_at_4[offsetof(nbody_batch_approach_body, upper) == 4 ? 1 : -1];
typedef char first_at_8[offsetof(nbody_batch_approach_body, first) == 8 ? 1 : -1];
typedef char now_at_12[offsetof(nbody_batch_approach_body, now) == 12 ? 1 : -1];
typedef char entry_is_24_bytes[sizeof(nbody_batch_approach) == 24 ? 1 : -1];
typedef char i_at_0[offsetof(nbody_batch_approach, i) == 0 ? 1 : -1];
typedef char j_at_4[offsetof(nbody_batch_approach, j) == 4 ? 1 : -1];
typedef char r2_at_8[offsetof(nbody_batch_approach, r2) == 8 ? 1 : -1];
typedef char rv_at_12[offsetof(nbody_batch_approach, rv) == 12 ? 1 : -1];
typedef char v2_at_16[offsetof(nbody_batch_approach, v2) == 16 ? 1 : -1];
typedef char phase_at_20[offsetof(nbody_batch_approach, phase) == 20 ? 1 : -1];
typedef char limit[NBODY_BATCH_APPROACHES_MAX_ENTRIES == 134217728LL ? 1 : -1];
typedef char the_bytes_of_the_contacts_limit[NBODY_BATCH_APPROACHES_MAX_ENTRIES * 24 == NBODY_BATCH_CONTACTS_MAX_ENTRIES * 12 ? 1 : -1];
typedef char phases[NBODY_BATCH_APPROACH_NOW == 0 && NBODY_BATCH_APPROACH_PASSAGE == 1 && NBODY_BATCH_APPROACH_END == 2 ? 1 : -1];
int main(void) {
    nbody_batch_approach_system s;
    float radius[1] = {1.f}, horizon[1] = {1.f};
    return (nbody_batch_approaches(0, 0, 0, horizon, radius, 0, 0, 0, &s, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):                                              # without the comment's own stars and line breaks
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_approaches.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_contacts.h", "Exactly those of nbody_batch_contacts.h",
                   "takes part iff i < min(counts[s], max_bodies) and subset is NULL or", "this is geometry", "whatever the massive counts",
                   "the state is read as it stands", "Exactly one of radius and radii is non-NULL", "t2 = correlation_edge2(radius[s])",
                   "S = R_i + R_j is one fp32 add and t2 = S * S one fp32 product", "the caller passes the radii",
                   "n_systems fp32 values H, each finite and >= 0", "d = x_j - x_i and w = v_j - v_i per component, as fp32 subtractions",
                   "every fmaf one fused operation, nothing else contracted", "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))",
                   "v2 = fmaf(wz, wz, fmaf(wy, wy, wx wx))", "rv = fmaf(dz, wz, fmaf(dy, wy, dx wx))", "bit-symmetric under i <-> j",
                   "no decision reads the sign of a zero", "measured iff r2 <= FLT_MAX, v2 <= FLT_MAX and fabsf(rv) <= FLT_MAX",
                   "with no division anywhere", "0 `now`: r2 <= t2", "the predicate of nbody_batch_contacts", "must be closing: rv < 0",
                   "2 `end`: with vh = v2 * H (one product)", "-rv >= vh", "e = fmaf(w, H, d) per component", "m2 is the r2 chain over e",
                   "an approach iff m2 <= FLT_MAX and m2 <= t2", "1 `passage`: otherwise; then v2 > 0 follows",
                   "g = r2 - t2, lhs = g * v2, rhs = rv * rv", "an approach iff lhs <= rhs", "r2 - rv^2 / v2 <= t2, cross-multiplied",
                   "Products that overflow are compared as computed", "With H == 0, or with all velocities equal",
                   "the approaches are exactly the contacts", "Adding one velocity to every body changes nothing",
                   "(i, j, r2, rv, v2, phase) with i < j", "ascending in i and then in j", "the order is total",
                   "entry k of system s is at s * capacity + k", "stored = min(pairs, capacity)", "hold {-1, -1, +inf, 0, 0, -1}",
                   "pairs is exact whatever the capacity", "{int i; int j; float r2; float rv; float v2; int phase;}, 24 bytes",
                   "16 bytes", "the exclusive sum of upper over the lower rows", "not clamped", "[first, first + upper) cut at stored",
                   "which is its degree in nbody_batch_contacts", "hold {0, 0, first, 0}", "48 bytes", "those with degree >= 1",
                   "now + passing + ending == pairs", "sum(degree) == 2 * pairs == 2 * sum(upper)", "NULL iff capacity == 0",
                   "the same bits either way", "No time or distance is computed on the device", "time -rv / v2",
                   "sqrt(max(0, r2 - rv^2 / v2))", "sqrt(r2 + 2 rv H + v2 H^2)",
                   "no schedule, slot, n_systems, max_bodies or capacity changes a bit", "synchronous", "forgets nothing", "bit for bit",
                   "grown when a later call asks for more", "freed in nbody_batch_destroy", "names the function", "a NULL handle",
                   "NULL d_positions_xyzm, d_velocities, horizon or systems_out", "a horizon that is negative, NaN or infinite",
                   "the message names the system", "both of radius and radii given, or neither", "names the system and the slot",
                   "capacity < 0", "capacity > 0 with list_out NULL, or capacity == 0 with list_out non-NULL", "n_systems * capacity > 2^27",
                   "refused before any device work", "nothing is written to the outputs", "Out of scope", "curved paths (accelerations)",
                   "pairs across systems", "softening", "sorting by time on the device", "device-side outputs", "changing the state"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.approaches_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.contacts_names()) | set(_lib.correlation_names()) |
                             set(_lib.neighbours_names()) | set(_lib.pairs_names()))
    fn = lib.nbody_batch_approaches
    assert fn.argtypes is not None and len(fn.argtypes) == 11 and fn.argtypes[7] is ctypes.c_longlong
    assert ctypes.sizeof(_lib.BatchApproachSystem) == 48 and ctypes.sizeof(_lib.BatchApproachBody) == 16 and ctypes.sizeof(_lib.BatchApproach) == 24
    assert [f[0] for f in _lib.BatchApproachSystem._fields_] == list(SYSTEM_WORDS)
    assert [getattr(_lib.BatchApproachSystem, w).offset for w in SYSTEM_WORDS] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
    assert [f[0] for f in _lib.BatchApproachBody._fields_] == list(BODY_WORDS)
    assert [f[0] for f in _lib.BatchApproach._fields_] == list(ENTRY_WORDS)
    assert [getattr(_lib.BatchApproach, w).offset for w in ENTRY_WORDS] == [0, 4, 8, 12, 16, 20]
    assert _lib.BATCH_APPROACHES_MAX_ENTRIES == 2 ** 27
    assert batch.APPROACH_SYSTEM_DTYPE == aref.SYSTEM_DTYPE and batch.APPROACH_BODY_DTYPE == aref.BODY_DTYPE and batch.APPROACH_DTYPE == aref.ENTRY_DTYPE
    assert [batch.APPROACH_SYSTEM_DTYPE.fields[w][1] for w in SYSTEM_WORDS] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
    for name in ("ApproachesResult", "APPROACH_SYSTEM_DTYPE", "APPROACH_BODY_DTYPE", "APPROACH_DTYPE"):
        assert name in batch.__all__ and name in nb.__all__ and getattr(nb, name) is getattr(batch, name), name
    assert batch.ApproachesResult.__doc__ and batch.BatchedSystem.approaches.__doc__
    for helper in ("pairs_of", "partners_of", "soonest"):
        assert getattr(batch.ApproachesResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_approaches") == 1 and exports[exports.index("nbody_batch_approaches") - 1].startswith("#")
    hpp = open(os.path.join(INCLUDE, "nbody.hpp")).read()
    assert "std::vector<nbody_batch_approach_system> approaches(" in hpp and "nbody_batch_approaches(b_, dPositions, dVelocities," in hpp
    assert hpp.index("> contacts(") < hpp.index("> approaches(")


def test_the_cpp_wrapper_compiles_with_a_call_in_each_mode(tmp_path):
    src = tmp_path / "batch_approaches.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_approach_system> both(nbody::Batch &b, const float *pos, const float *vel)
{
    std::vector<nbody_batch_approach> list;
    std::vector<nbody_batch_approach_body> bodies;
    const std::vector<float> horizon(16, 2.f);
    std::vector<nbody_batch_approach_system> counted = b.approaches(pos, vel, horizon, std::vector<float>(16, 0.5f));
    b.approaches(pos, vel, horizon, std::vector<float>(16 * 64, 0.1f), 8, &list, std::vector<unsigned char>(16 * 64, 1), &bodies);
    return counted;
}
''')
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_every_error_is_refused_without_a_device(lib):
    """A NULL handle is refused first, with the function's name, by the library itself.  The other cases need a handle
    (test_batch_approaches_gpu.py walks them); here the source shows that each is refused before the first device call."""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchApproachSystem * 1)()
    one = (ctypes.c_float * 1)(1.0)
    assert lib.nbody_batch_approaches(None, None, None, one, one, None, None, 0, out, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_approaches: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_approaches("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_approaches: batch is NULL", "nbody_batch_approaches: NULL argument",
                "nbody_batch_approaches: the horizon of system ", "approaches_horizon_valid(",
                "nbody_batch_approaches: exactly one of radius and radii must be given", "must be finite and >= 0",
                "batch_radii_ok(", "nbody_batch_approaches: capacity must be >= 0",
                "nbody_batch_approaches: list_out must be given iff capacity > 0",
                "nbody_batch_approaches: n_systems x capacity must not exceed 2^27")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_approaches: ') == 9                                     # every message names the function


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_and_reuses_the_contacts_functions():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_approaches_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_approaches.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_approaches_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and '#include "nbody_batch_contacts_math.h"' in text
    code = re.sub(r"//.*", "", text)
    for call in ("groups_r2(", "groups_friends(", "correlation_measured(", "contacts_above(", "contacts_stored(", "contacts_row_fills("):
        assert call in code, call
    assert "/" not in re.sub(r"#include.*", "", code)                                        # no division anywhere
    assert code.count("__builtin_fmaf(") == 2 + 3 + 2                                        # rv, e and m2; r2 and v2 are groups_r2
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void approaches_column("):source.index("hipError_t launch_batch_approaches(")]
    for call in ("approaches_words(", "approaches_ends(", "approaches_m2(", "approaches_phase(", "approaches_step(", "approaches_fill(",
                 "approaches_row_fills(", "approaches_pad(", "approaches_body(", "approaches_system(", "contacts_examined(",
                 "contacts_radii_t2(", "contacts_no_radius(", "contacts_wave_scan(", "contacts_unit(", "contacts_units_below(",
                 "contacts_stored(", "readfirstlane(", "img[2 * j + 1]"):
        assert call in kernel, call
    assert "fmaf" not in kernel and "asm" not in kernel
    launch = source[source.index("hipError_t launch_batch_approaches("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "with_rpl(" in launch and "launch_analysis_kernel(" in launch
    assert "2 * kBatchBytesPerBody * (size_t)max_bodies" in launch                           # launch_batch_pairs' image
    assert source.index("hipError_t launch_batch_contacts(") < source.index("void batch_approaches_kernel(") \
        < source.index("hipError_t launch_batch_approaches(") < source.index("void batch_diag_kernel(") < source.index("}  // namespace\n")
    for sibling in ("pairs", "structure", "members", "gravity", "hierarchy", "groups", "span", "neighbours", "correlation", "contacts"):
        cut = source[source.index(f"void batch_{sibling}_kernel("):source.index(f"hipError_t launch_batch_{sibling}(")]
        assert "approach" not in cut, sibling
    assert source.count("NBODY_BATCH_APPROACHES_END_ALWAYS ||") == 1 and source.count("NBODY_BATCH_APPROACHES_FILL_ALWAYS ||") == 1
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchApproachSystem> approaches_systems", "DeviceArray<BatchApproachBody> approaches_bodies",
                   "DeviceArray<BatchApproach> approaches_list", "DeviceArray<unsigned char> approaches_subset",
                   "DeviceArray<float> approaches_radius2", "DeviceArray<float> approaches_radii", "DeviceArray<float> approaches_horizon"):
        assert member in members, member


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_approaches_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("approaches"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("approaches_checked"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def command(pos, vel, n, slots, shape, capacity, H, radius=None, radii=None, subset=None, always=0, end=0):
    T, rpl = shape
    take = np.ones(n, np.uint8) if subset is None else (np.asarray(subset)[:n] != 0).astype(np.uint8)
    R = np.zeros(n, np.float32) if radii is None else np.asarray(radii)[:n]
    lines = [f"system {n} {slots} {T} {rpl} {0 if radii is None else 1} {capacity} {float(radius or 0.0)!r} {float(H)!r} {always} {end}"]
    lines += [" ".join(repr(float(w)) for w in (*p[:3], *v[:3], r)) + f" {int(t)}"
              for p, v, r, t in zip(np.asarray(pos)[:n], np.asarray(vel)[:n], R, take)]
    return "\n".join(lines) + "\n"


def parse(out, slots, capacity):
    """One system's three lines of the driver's output: (system record, body records, list)."""
    system = np.zeros((), aref.SYSTEM_DTYPE)
    for name, word in zip(SYSTEM_WORDS, out[0].split()):
        system[name] = int(word)
    bodies = np.array([int(w) for w in out[1].split()], np.int32).reshape(slots, 4).copy().view(aref.BODY_DTYPE).reshape(slots)
    flat = np.array([int(w) for w in out[2].split()], np.int64).reshape(capacity, 6)
    entries = np.zeros(capacity, aref.ENTRY_DTYPE)
    entries["i"], entries["j"], entries["phase"] = flat[:, 0], flat[:, 1], flat[:, 5]
    for at, name in ((2, "r2"), (3, "rv"), (4, "v2")):
        entries[name] = flat[:, at].astype(np.uint32).view(np.float32)
    return system, bodies, entries


def same(got, ref, capacity, tag):
    system, bodies, entries = got
    assert system.tobytes() == aref.system_record(ref, capacity).tobytes(), (tag, system, aref.system_record(ref, capacity))
    assert bodies.tobytes() == ref["bodies"].tobytes(), (tag, bodies, ref["bodies"])
    assert entries.tobytes() == aref.listed(ref, capacity).tobytes(), (tag, entries, aref.listed(ref, capacity))
    aref.check_identity(bodies, int(system["pairs"]))
    aref.check_phases(system)


def run_cases(driver, cases):
    """cases: (tag, pos, vel, n, slots, shape, capacity, H, keywords, reference); one process runs them all."""
    out = driver("".join(command(pos, vel, n, slots, shape, capacity, H, **kw) for _, pos, vel, n, slots, shape, capacity, H, kw, _ in cases))
    assert len(out) == 3 * len(cases) + 1 and out[-1] == ""
    for at, (tag, _, _, _, slots, _, capacity, _, _, ref) in enumerate(cases):
        same(parse(out[3 * at:3 * at + 3], slots, capacity), ref, capacity, tag)


def cutting_capacity(ref):
    """A capacity that cuts the system in the middle of a row, or one short of all."""
    rows = np.nonzero(ref["bodies"]["upper"] >= 2)[0]
    if len(rows):
        return int(ref["bodies"]["first"][rows[len(rows) // 2]]) + 1
    return max(ref["system"]["pairs"] - 1, 0)


def gpu_cases(capacity, shapes, variants=((0, 0),), systems=range(aref.B)):
    """Every system of the GPU inputs in both modes, with and without the subset, at capacities 0, one cutting a row, and
    full (and three beyond)."""
    P, V, counts, R = aref.gpu_inputs(capacity)
    cases = []
    for mode in aref.MODES:
        for with_subset in (False, True):
            refs = aref.gpu_reference(capacity, mode, with_subset)
            subset = aref.gpu_subset(capacity) if with_subset else None
            for s in systems:
                kw = {"radius": aref.RADIUS[s]} if mode == "radius" else {"radii": R[s]}
                if with_subset:
                    kw["subset"] = subset[s]
                pairs = refs[s]["system"]["pairs"]
                for shape in shapes:
                    for cap in sorted({0, cutting_capacity(refs[s]), pairs, pairs + 3}):
                        for always, end in variants:
                            cases.append(((capacity, mode, with_subset, s, shape, cap, always, end), P[s], V[s], counts[s], capacity,
                                          shape, cap, aref.HORIZON[s], dict(kw, always=always, end=end), refs[s]))
    return cases


def test_the_layout(driver):
    assert [int(w) for w in driver("layout\n")[0].split()] == [48, 0, 4, 8, 12, 16, 24, 32, 36, 40, 44, 16, 0, 4, 8, 12, 24, 0, 4, 8, 12, 16, 20]


@pytest.mark.parametrize("capacity", [64, 128, 320])
def test_the_driver_gives_the_references_records_and_list_exactly(driver, capacity):
    """Every input of the GPU suite in both modes, with and without the subset, at list capacities 0, one cutting a row, all
    and all + 3, with both fills and both ways to the separation at the horizon, for batch_shape's workgroup and for the
    other shapes of the suite that hold the slots."""
    shapes = [shape for shape in ((64, 1), (64, 2), (128, 4), (1024, 4)) if shape[0] * shape[1] >= capacity]
    assert SHAPES[capacity] == shapes[0]
    run_cases(driver, gpu_cases(capacity, shapes[:1], variants=((0, 0), (1, 0), (0, 1), (1, 1))))
    run_cases(driver, gpu_cases(capacity, shapes[1:], systems=(3, 4)))


def test_the_driver_at_4096_bodies(driver):
    cases = [c for c in gpu_cases(4096, [SHAPES[4096]], systems=(4,))]
    assert len(cases) == 4 * 4 and SHAPES[4096] == (1024, 4)
    run_cases(driver, cases)
    assert cases[0][-1]["system"]["pairs"] > 4096


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    run_cases(checked_driver, gpu_cases(128, [(64, 2), (128, 4)], variants=((0, 0), (1, 1))))
    run_cases(checked_driver, gpu_cases(320, [SHAPES[320]], systems=(3, 4)))
    assert checked_driver("layout\n")[0].split()[0] == "48"
    assert checked_driver("pair -4 3 0 1 0 0 9 6\n")[0].split()[0] == "1"


def pair(driver, d, w, t2, H):
    """(phase, bits of r2, rv, v2) of one pair from the driver, checked to be the same phase, r2 and v2 the other way round."""
    words = [int(x) for x in driver("pair " + " ".join(repr(float(x)) for x in (*d, *w, t2, H)) + "\n")[0].split()]
    assert words[0] == words[4], (d, w, words)
    if all(word & 0x7f800000 != 0x7f800000 for word in words[1:4]):                          # measured: the same bits both ways
        assert words[1] == words[5] and words[3] == words[7], (d, w, words)
        assert words[2] == words[6] or words[2] & 0x7fffffff == words[6] & 0x7fffffff == 0   # rv: but for the sign of a zero
    return words[0]


def test_the_hand_placed_pairs_and_the_edges_of_the_predicate_on_the_driver(driver):
    for name, (d, w, phase) in aref.HAND.items():
        assert pair(driver, d, w, 9, 6) == (-1 if phase is None else phase), name
    assert pair(driver, *aref.BEYOND, 9, 6) == -1
    assert pair(driver, (-4, 3, 0), (1, 0, 0), 9, 4) == aref.END                            # -rv == vh now: (0, 3, 0) at the horizon
    assert pair(driver, (-4, 3, 0), (1, 0, 0), 9, 3) == -1                                  # (-1, 3, 0) at the horizon: 10 > 9
    assert pair(driver, (-4, 0, 0), (1, 0, 0), 9, 0) == -1 and pair(driver, (-3, 0, 0), (1, 0, 0), 9, 0) == aref.NOW   # H == 0
    assert pair(driver, (-4, 0, 0), (0, 0, 0), 9, 8) == -1                                  # at rest to each other
    assert pair(driver, (-4, 0, 0), (1, 0, 0), float("nan"), 8) == -1                       # a body that takes no part
    assert pair(driver, (-4, 0, 0), (float("nan"), 0, 0), 9, 8) == -1 and pair(driver, (float("inf"), 0, 0), (-1, 0, 0), 9, 8) == -1
    assert pair(driver, (-2, 0, 0), (float("nan"), 0, 0), 9, 8) == -1                       # within reach, but not measured
    # products that overflow are compared as computed: vh = 1e30 * 1e10 = +inf sends a closing pair to the passage, where
    # lhs = 1e30 * 1e30 = +inf <= rhs = +inf holds (the pair does pass 1 away); an lhs of +inf is within no finite rhs
    assert pair(driver, (-1e15, 1.0, 0), (1e15, 0, 0), 9, 1e10) == aref.PASSAGE
    assert pair(driver, (-1.0, 1e15, 0), (1e10, 0, 0), 9, 1e10) == -1
    # a radius whose square overflowed is FLT_MAX: within reach of every measured pair now
    assert pair(driver, (1e10, 0, 0), (1, 0, 0), 3.4028234663852886e38, 1) == aref.NOW


# ---- the inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", aref.CAPACITIES)
def test_the_inputs_do_their_work(capacity):
    P, V, counts, R = aref.gpu_inputs(capacity)
    assert counts == [0, 1, 2, min(65, capacity), capacity] and aref.HORIZON[4] == 6 and aref.RADIUS[4] == 3 and aref.HORIZON[1] == 0
    m = aref.marks(capacity)
    assert len({row for rows in m.values() for row in rows}) == 2 * len(m) - 1 - (2 if m["wave"] == m["last"] else 0)
    T, rpl = SHAPES[capacity]
    for mode in aref.MODES:
        for with_subset in (False, True):
            refs = aref.gpu_reference(capacity, mode, with_subset)
            pairs = [r["system"]["pairs"] for r in refs]
            assert pairs[0] == pairs[1] == 0 and pairs[2] == 1 and pairs[3] > 0 and pairs[4] > capacity // 4
            assert refs[2]["list"]["phase"].tolist() == [aref.PASSAGE]
            full = refs[4]
            listed = {(int(i), int(j)): int(p) for i, j, p in zip(full["list"]["i"], full["list"]["j"], full["list"]["phase"])}
            for name, (_, _, phase) in aref.HAND.items():
                assert listed.get(m[name]) == phase, (name, mode, with_subset)                 # present, in its intended phase; or absent
            assert m["beyond"] not in listed
            assert listed[m["last"]] == aref.PASSAGE and listed[m["wave"]] == aref.PASSAGE
            assert min(full["system"][k] for k in ("now", "passing", "ending")) > 0, full["system"]   # all three phases occur
            mid = {(int(i), int(j)): int(p) for i, j, p in zip(refs[3]["list"]["i"], refs[3]["list"]["j"], refs[3]["list"]["phase"])}
            assert mid[(2, 20)] == aref.NOW and R[3, 2] == R[3, 20] == 0 and np.array_equal(V[3, 2], V[3, 20])
            assert np.isnan(V[3, 5, 1]) and np.isinf(P[3, 9, 0])
            assert refs[3]["bodies"]["degree"][5] == 0 and refs[3]["bodies"]["degree"][9] == 0   # unmeasured: no approach
            last, wave = m["last"][0], m["wave"][0]
            assert full["bodies"]["upper"][last] > 0 and last // T == (capacity - 1) // T        # the last q that holds rows
            assert full["bodies"]["upper"][wave] > 0 and (wave % T) // 64 == T // 64 - 1         # the last wave
            aref.check_identity(full["bodies"], full["system"]["pairs"])
            cut = cutting_capacity(full)
            row = np.searchsorted(full["bodies"]["first"], cut, side="right") - 1
            assert 0 < cut < full["system"]["pairs"] and full["bodies"]["first"][row] < cut < full["bodies"]["first"][row] + full["bodies"]["upper"][row]
    # the threshold pair sits exactly on lhs == rhs, and the boundary pair on -rv == vh with m2 == t2
    d, w, _ = aref.HAND["threshold"]
    r2, v2, rv = sum(a * a for a in d), sum(a * a for a in w), sum(a * b for a, b in zip(d, w))
    assert (r2 - 9) * v2 == rv * rv and -rv < v2 * 6
    d, w, _ = aref.HAND["boundary"]
    assert -sum(a * b for a, b in zip(d, w)) == sum(a * a for a in w) * 6 and sum((a + 6 * b) ** 2 for a, b in zip(d, w)) == 9


def test_the_phase_counts_of_the_4096_body_cube():
    """The figures the cube of half-width 21 gives at radius 3 and H = 6, all three phases in thousands."""
    system = aref.gpu_reference(4096, "radius", False)[4]["system"]
    print(system)
    assert system["now"] > 10000 and system["passing"] > 20000 and system["ending"] > 2000
    assert system["now"] + system["passing"] + system["ending"] == system["pairs"]


# ---- the premise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", aref.CAPACITIES)
def test_every_word_of_every_chain_and_of_the_predicate_is_an_integer_that_fp32_holds_on_every_input(capacity):
    """Finite coordinates are integers within 32, velocities within 2, horizons integers up to 8 and radii small integers: the
    fp32 operations one by one (numpy has no fused multiply-add, and needs none where nothing rounds) give the reference's
    integers, and the largest of them is far below 2^24."""
    P, V, counts, R = aref.gpu_inputs(capacity)
    for s, n in enumerate(counts):
        H = aref.HORIZON[s]
        assert float(H) == int(H) and 0 <= H <= aref.MAX_HORIZON and float(aref.RADIUS[s]) == int(aref.RADIUS[s])
        x, v = np.asarray(P[s, :n, :3], np.float32), np.asarray(V[s, :n, :3], np.float32)
        xi, vi, finite = aref.integers(P[s], V[s], n)
        assert np.array_equal(x[finite], xi[finite]) and (np.abs(xi) <= aref.LIMIT).all()
        assert np.array_equal(v[finite], vi[finite]) and (np.abs(vi) <= aref.SPEED).all()
        assert np.array_equal(R[s], np.round(R[s])) and (R[s] >= 0).all() and (R[s] <= 2).all()
        rows = np.arange(0, n, max(n // 64, 1))
        r2, v2, rv, m2, _ = aref.pair_words(xi, vi, rows, int(H))
        both = finite[rows][:, None] & finite[None, :]
        h = np.float32(H)
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[None, :, :] - x[rows][:, None, :]
            w = v[None, :, :] - v[rows][:, None, :]
            e = w * h + d
            f_r2 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
            f_v2 = w[..., 2] * w[..., 2] + (w[..., 1] * w[..., 1] + w[..., 0] * w[..., 0])
            f_rv = d[..., 2] * w[..., 2] + (d[..., 1] * w[..., 1] + d[..., 0] * w[..., 0])
            f_m2 = e[..., 2] * e[..., 2] + (e[..., 1] * e[..., 1] + e[..., 0] * e[..., 0])
        top = np.finfo(np.float32).max
        for name, f, exact in (("r2", f_r2, r2), ("v2", f_v2, v2), ("rv", f_rv, rv), ("m2", f_m2, m2)):
            assert f.dtype == np.float32 and np.array_equal(f[both].astype(np.int64), exact[both]), (name, s)
        assert not ((f_r2 <= top) & (f_v2 <= top) & (np.abs(f_rv) <= top))[~both].any()      # not measured
        for mode in aref.MODES:
            t2 = aref.thresholds(n, rows, radius=aref.RADIUS[s]) if mode == "radius" else aref.thresholds(n, rows, radii=R[s])
            if mode == "radii":
                S = R[s, :n][rows][:, None] + R[s, :n][None, :]
                assert S.dtype == np.float32 and np.array_equal((S * S).astype(np.int64), t2)
            else:
                assert float(np.float32(aref.RADIUS[s]) * np.float32(aref.RADIUS[s])) == float(t2)
            f_t2 = np.broadcast_to(np.asarray(t2, np.float32), f_r2.shape)
            with np.errstate(invalid="ignore", over="ignore"):
                products = (("vh", f_v2 * h, v2 * int(H)), ("lhs", (f_r2 - f_t2) * f_v2, (r2 - t2) * v2), ("rhs", f_rv * f_rv, rv * rv))
            for name, f, exact in products:
                assert np.array_equal(f[both].astype(np.int64), np.broadcast_to(exact, f.shape)[both]), (name, s, mode)
    for mode in aref.MODES:
        for with_subset in (False, True):
            largest = max(r["largest"] for r in aref.gpu_reference(capacity, mode, with_subset))
            assert largest < 2 ** 20, largest                                                  # 3 * 64^2 * 48 = 589 824 at the most


# ---- the helpers of the result -------------------------------------------------------------------------------------------------
def test_the_host_methods_of_the_result_on_hand_made_records():
    from n_body_problem_amd import batch
    systems = np.zeros(2, batch.APPROACH_SYSTEM_DTYPE)
    systems["pairs"], systems["stored"] = [3, 4], [3, 2]
    systems["now"], systems["passing"], systems["ending"] = [1, 2], [1, 1], [1, 1]
    systems["approaching"], systems["max_degree"], systems["bodies"] = [3, 4], [2, 3], [4, 4]
    entries = np.zeros((2, 3), batch.APPROACH_DTYPE)
    entries["i"], entries["j"] = [[0, 0, 1], [0, 0, -1]], [[1, 2, 2], [1, 3, -1]]
    entries["phase"] = [[0, 2, 1], [1, 0, -1]]
    entries["r2"] = [[4, 100, 25], [25, 1, np.inf]]
    entries["rv"] = [[-1, -10, -4], [-4, 0, 0]]
    entries["v2"] = [[1, 1, 1], [1, 0, 0]]
    bodies = np.zeros((2, 4), batch.APPROACH_BODY_DTYPE)
    bodies["degree"][0], bodies["upper"][0], bodies["first"][0], bodies["now"][0] = [2, 2, 2, 0], [2, 1, 0, 0], [0, 2, 3, 3], [1, 1, 0, 0]
    res = batch.ApproachesResult(systems, bodies, entries, np.array([8.0, 6.0], np.float32))
    assert res.pairs.tolist() == [3, 4] and res.stored.tolist() == [3, 2] and res.truncated.tolist() == [False, True]
    assert res.now_pairs.tolist() == [1, 2] and res.passing.tolist() == [1, 1] and res.ending.tolist() == [1, 1] and res.capacity == 3
    assert res.horizon.tolist() == [8.0, 6.0]
    assert res.degree[0].tolist() == [2, 2, 2, 0] and res.first[0].tolist() == [0, 2, 3, 3] and res.now[0].tolist() == [1, 1, 0, 0]
    assert res.phase[0].tolist() == [0, 2, 1] and res.rv[0].tolist() == [-1, -10, -4]
    # now: time 0 at sqrt(r2); end: the horizon, sqrt(100 - 2 * 10 * 8 + 64) = 2 there; passage: 4 on, sqrt(25 - 16) = 3 away
    assert res.time[0].tolist() == [0.0, 8.0, 4.0] and res.miss_distance[0].tolist() == [2.0, 2.0, 3.0]
    assert res.time[1].tolist() == [4.0, 0.0, np.inf] and res.miss_distance[1].tolist() == [3.0, 1.0, np.inf]
    assert res.time.dtype == np.float64 and res.miss_distance.dtype == np.float64
    assert res.pairs_of(0).tolist() == [[0, 1], [0, 2], [1, 2]] and res.pairs_of(1).tolist() == [[0, 1], [0, 3]]
    assert res.pairs_of(0).shape == (3, 2)
    assert res.partners_of(0, 0).tolist() == [1, 2] and res.partners_of(0, 2).tolist() == [0, 1] and res.partners_of(0, 3).tolist() == []
    with pytest.raises(ValueError, match="truncated"):
        res.partners_of(1, 0)
    first, time, miss = res.soonest(0)
    assert first["j"].tolist() == [1, 2, 2] and first["i"].tolist() == [0, 1, 0] and time.tolist() == [0.0, 4.0, 8.0] and miss.tolist() == [2.0, 3.0, 2.0]
    first, time, _ = res.soonest(1)
    assert first["phase"].tolist() == [0, 1] and time.tolist() == [0.0, 4.0]                   # the listed ones alone
    lean = batch.ApproachesResult(systems, None, None, np.array([8.0, 6.0], np.float32))
    assert lean.degree is None and lean.i is None and lean.time is None and lean.miss_distance is None and lean.capacity == 0
    for call in (lambda: lean.pairs_of(0), lambda: lean.soonest(0)):
        with pytest.raises(ValueError, match="lists=True"):
            call()
    assert "ApproachesResult(pairs=[3, 4]" in repr(res)
