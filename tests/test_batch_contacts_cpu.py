"""CPU-only: the contact lists of batched ensembles (nbody_batch_contacts, include/nbody_batch_contacts.h).  The header is
self-contained C99, included by nbody.h after the correlation header, and declares its one entry point alone; it is exported,
bound and listed apart; the arithmetic without a GPU (csrc/nbody_batch_contacts_math.h), built into a stand-alone driver with
g++ -- once more with the address and undefined-behaviour sanitizers -- that runs the kernel's three phases for any workgroup
shape, gives the reference's records and list on every input of the GPU suite exactly, at list capacities on both sides of the
number of contacts; on every input the fp32 chain gives the integer r2 and the fp32 operations the exact thresholds, which is
the premise of all the exact comparisons; the inputs contain what they are there for; and the helpers of ContactsResult do what
they say on hand-made records."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_contacts_ref as kref
from conftest import ROOT

NAMES = ["nbody_batch_contacts"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
SYSTEM_WORDS = ("bodies", "touching", "max_degree", "reserved", "pairs", "stored", "closest_i", "closest_j", "closest_r2", "reserved2")
BODY_WORDS = ("degree", "upper", "first", "nearest")
SHAPES = kref.SHAPES


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_correlation_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_contacts.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_contacts.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_correlation.h"') < nbody_h.index('#include "nbody_batch_contacts.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_48_16_and_12_bytes(tmp_path):
    src = tmp_path / "contacts.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char system_is_48_bytes[sizeof(nbody_batch_contact_system) == 48 ? 1 : -1];
typedef char bodies_at_0[offsetof(nbody_batch_contact_system, bodies) == 0 ? 1 : -1];
typedef char touching_at_4[offsetof(nbody_batch_contact_system, touching) == 4 ? 1 : -1];
typedef char max_degree_at_8[offsetof(nbody_batch_contact_system, max_degree) == 8 ? 1 : -1];
typedef char reserved_at_12[offsetof(nbody_batch_contact_system, reserved) == 12 ? 1 : -1];
typedef char pairs_at_16[offsetof(nbody_batch_contact_system, pairs) == 16 ? 1 : -1];
typedef char stored_at_24[offsetof(nbody_batch_contact_system, stored) == 24 ? 1 : -1];
typedef char closest_i_at_32[offsetof(nbody_batch_contact_system, closest_i) == 32 ? 1 : -1];
typedef char closest_j_at_36[offsetof(nbody_batch_contact_system, closest_j) == 36 ? 1 : -1];
typedef char closest_r2_at_40[offsetof(nbody_batch_contact_system, closest_r2) == 40 ? 1 : -1];
typedef char reserved2_at_44[offsetof(nbody_batch_contact_system, reserved2) == 44 ? 1 : -1];
typedef char body_is_16_bytes[sizeof(nbody_batch_contact_body) == 16 ? 1 : -1];
typedef char degree_at_0[offsetof(nbody_batch_contact_body, degree) == 0 ? 1 : -1];
typedef char upper_at_4[offsetof(nbody_batch_contact_body, upper) == 4 ? 1 : -1];
typedef char first_at_8[offsetof(nbody_batch_contact_body, first) == 8 ? 1 : -1];
typedef char nearest_at_12[offsetof(nbody_batch_contact_body, nearest) == 12 ? 1 : -1];
typedef char entry_is_12_bytes[sizeof(nbody_batch_contact) == 12 ? 1 : -1];
typedef char i_at_0[offsetof(nbody_batch_contact, i) == 0 ? 1 : -1];
typedef char j_at_4[offsetof(nbody_batch_contact, j) == 4 ? 1 : -1];
typedef char r2_at_8[offsetof(nbody_batch_contact, r2) == 8 ? 1 : -1];
typedef char limit[NBODY_BATCH_CONTACTS_MAX_ENTRIES == 268435456LL ? 1 : -1];
int main(void) {
    nbody_batch_contact_system s;
    float radius[1] = {1.f};
    return (nbody_batch_contacts(0, 0, radius, 0, 0, 0, &s, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):                                              # without the comment's own stars and line breaks
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_contacts.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_correlation.h", "n_systems x max_bodies bytes",
                   "takes part iff i < min(counts[s], max_bodies) and subset is NULL or", "whatever the massive counts",
                   "this is geometry", "Removed tracers and merged bodies are seen as the state holds them", "r2 is groups_r2",
                   "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))", "There is no softening", "measured iff r2 <= FLT_MAX",
                   "Exactly one of radius and radii is non-NULL", "radius[s] * radius[s] is one fp32 product",
                   "taken as the largest finite fp32 value", "correlation_edge2's rule", "groups_friends: r2 <= t2",
                   "S = R_i + R_j is one fp32 add", "t2 = S * S one fp32 product", "fmaf(S, S, eps^2) at eps = 0",
                   "Contact iff measured and r2 <= t2", "A coincident pair with zero radii is a contact",
                   "they are not the handle's", "i != j, both taking part", "r2 is bit-symmetric", "(i, j) and (j, i) agree",
                   "ascending in i and then in j", "the order is total", "does not depend on schedule, slot, n_systems or max_bodies",
                   "entry k of system s is at s * capacity + k", "stored = min(pairs, capacity)", "hold {-1, -1, +inf}",
                   "pairs is exact whatever the capacity", "calls again with more", "16 bytes", "the exclusive sum of upper over the lower rows",
                   "not clamped", "[first, first + upper) cut at stored", "ties to the lower index", "hold {0, 0, first, -1}",
                   "first is the running sum there too", "48 bytes", "those with degree >= 1", "ties to the smallest i and then the smallest j",
                   "\"Pair\" rule", "-1, -1 and +inf without a contact", "12 bytes", "sum(degree) == 2 * pairs == 2 * sum(upper)",
                   "NULL iff capacity == 0", "the same bits either way", "synchronous", "forgets nothing", "bit for bit",
                   "grown when a later call asks for more", "freed in nbody_batch_destroy",
                   "the same bits in any slot, n_systems and max_bodies", "names the function", "a NULL handle",
                   "NULL d_positions_xyzm or systems_out", "both of radius and radii given, or neither", "negative, NaN or infinite",
                   "the message names the system", "names the system and the slot", "capacity < 0",
                   "capacity > 0 with list_out NULL, or capacity == 0 with list_out non-NULL", "n_systems * capacity > 2^28",
                   "refused before any device work", "nothing is written to the outputs", "Out of scope", "pairs across systems",
                   "softened or periodic distances", "velocity criteria (approaching pairs, impact parameters)", "device-side outputs",
                   "per-system capacities", "a list sorted by distance", "changing the state"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.contacts_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.correlation_names()) | set(_lib.neighbours_names()) |
                             set(_lib.span_names()) | set(_lib.groups_names()))
    fn = lib.nbody_batch_contacts
    assert fn.argtypes is not None and len(fn.argtypes) == 9 and fn.argtypes[5] is ctypes.c_longlong
    assert ctypes.sizeof(_lib.BatchContactSystem) == 48 and ctypes.sizeof(_lib.BatchContactBody) == 16 and ctypes.sizeof(_lib.BatchContact) == 12
    assert [f[0] for f in _lib.BatchContactSystem._fields_] == list(SYSTEM_WORDS)
    assert [getattr(_lib.BatchContactSystem, w).offset for w in SYSTEM_WORDS] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
    assert [f[0] for f in _lib.BatchContactBody._fields_] == list(BODY_WORDS)
    assert [f[0] for f in _lib.BatchContact._fields_] == ["i", "j", "r2"]
    assert _lib.BATCH_CONTACTS_MAX_ENTRIES == 2 ** 28
    assert batch.CONTACT_SYSTEM_DTYPE == kref.SYSTEM_DTYPE and batch.CONTACT_BODY_DTYPE == kref.BODY_DTYPE and batch.CONTACT_DTYPE == kref.ENTRY_DTYPE
    assert [batch.CONTACT_SYSTEM_DTYPE.fields[w][1] for w in SYSTEM_WORDS] == [0, 4, 8, 12, 16, 24, 32, 36, 40, 44]
    assert "ContactsResult" in batch.__all__ and "ContactsResult" in nb.__all__ and nb.ContactsResult is batch.ContactsResult
    assert batch.ContactsResult.__doc__ and batch.BatchedSystem.contacts.__doc__
    for helper in ("pairs_of", "partners_of"):
        assert getattr(batch.ContactsResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_contacts") == 1 and exports[exports.index("nbody_batch_contacts") - 1].startswith("#")
    hpp = open(os.path.join(INCLUDE, "nbody.hpp")).read()
    assert "std::vector<nbody_batch_contact_system> contacts(" in hpp and "nbody_batch_contacts(b_, dPositions," in hpp


def test_the_cpp_wrapper_compiles_with_a_call_in_each_mode(tmp_path):
    src = tmp_path / "batch_contacts.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_contact_system> both(nbody::Batch &b, const float *pos)
{
    std::vector<nbody_batch_contact> list;
    std::vector<nbody_batch_contact_body> bodies;
    std::vector<nbody_batch_contact_system> counted = b.contacts(pos, std::vector<float>(16, 0.5f));
    b.contacts(pos, std::vector<float>(16 * 64, 0.1f), 8, &list, std::vector<unsigned char>(16 * 64, 1), &bodies);
    return counted;
}
''')
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_every_error_is_refused_without_a_device(lib):
    """A NULL handle is refused first, with the function's name, by the library itself.  The other cases need a handle
    (test_batch_contacts_gpu.py walks them); here the source shows that each is refused before the first device call."""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchContactSystem * 1)()
    radius = (ctypes.c_float * 1)(1.0)
    assert lib.nbody_batch_contacts(None, None, radius, None, None, 0, out, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_contacts: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_contacts("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_contacts: batch is NULL", "nbody_batch_contacts: NULL argument",
                "nbody_batch_contacts: exactly one of radius and radii must be given", "must be finite and >= 0",
                "batch_radii_ok(", "nbody_batch_contacts: capacity must be >= 0",
                "nbody_batch_contacts: list_out must be given iff capacity > 0",
                "nbody_batch_contacts: n_systems x capacity must not exceed 2^28")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_contacts: ') == 8                                       # every message names the function


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_and_reuses_the_groups_functions():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_contacts_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_contacts.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_contacts_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and '#include "nbody_batch_groups_math.h"' in text
    code = re.sub(r"//.*", "", text)
    assert "groups_friends(" in code and "correlation_edge2(" in code and "span_key(" in code and "fmaf" not in code
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_contacts_kernel("):source.index("hipError_t launch_batch_contacts(")]
    for call in ("groups_r2(", "contacts_examined(", "contacts_step(", "contacts_row_key(", "contacts_units_below(", "contacts_unit(",
                 "contacts_fill(", "contacts_row_fills(", "contacts_pad(", "contacts_stored(", "contacts_body(", "contacts_system(",
                 "contacts_radii_t2(", "readfirstlane("):
        assert call in kernel, call
    assert "fmaf" not in kernel and "asm" not in kernel
    launch = source[source.index("hipError_t launch_batch_contacts("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "with_rpl(" in launch and "launch_analysis_kernel(" in launch
    assert source.index("hipError_t launch_batch_correlation(") < source.index("void batch_contacts_kernel(") \
        < source.index("hipError_t launch_batch_contacts(") < source.index("void batch_diag_kernel(") < source.index("}  // namespace\n")
    for sibling in ("pairs", "structure", "members", "gravity", "hierarchy", "groups", "span", "neighbours", "correlation"):
        cut = source[source.index(f"void batch_{sibling}_kernel("):source.index(f"hipError_t launch_batch_{sibling}(")]
        assert "contacts" not in cut, sibling
    assert source.count("NBODY_BATCH_CONTACTS_FILL_ALWAYS ||") == 1                        # both fills behind one switch
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchContactSystem> contacts_systems", "DeviceArray<BatchContactBody> contacts_bodies",
                   "DeviceArray<BatchContact> contacts_list", "DeviceArray<unsigned char> contacts_subset",
                   "DeviceArray<float> contacts_radius2", "DeviceArray<float> contacts_radii"):
        assert member in members, member


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_contacts_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("contacts"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("contacts_checked"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def command(pos, n, slots, shape, capacity, radius=None, radii=None, subset=None, always=0):
    T, rpl = shape
    take = np.ones(n, np.uint8) if subset is None else (np.asarray(subset)[:n] != 0).astype(np.uint8)
    R = np.zeros(n, np.float32) if radii is None else np.asarray(radii)[:n]
    lines = [f"system {n} {slots} {T} {rpl} {0 if radii is None else 1} {capacity} {float(radius or 0.0)!r} {always}"]
    lines += [f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {float(r)!r} {int(t)}" for p, r, t in zip(np.asarray(pos)[:n], R, take)]
    return "\n".join(lines) + "\n"


def parse(out, slots, capacity):
    """One system's three lines of the driver's output: (system record, body records, list)."""
    words = out[0].split()
    system = np.zeros((), kref.SYSTEM_DTYPE)
    for name, word in zip(SYSTEM_WORDS, words):
        system[name] = np.array(int(word), np.uint32).view(np.float32) if name == "closest_r2" else int(word)
    bodies = np.array([int(w) for w in out[1].split()], np.int32).reshape(slots, 4).copy().view(kref.BODY_DTYPE).reshape(slots)
    flat = np.array([int(w) for w in out[2].split()], np.int64).reshape(capacity, 3)
    entries = np.zeros(capacity, kref.ENTRY_DTYPE)
    entries["i"], entries["j"], entries["r2"] = flat[:, 0], flat[:, 1], flat[:, 2].astype(np.uint32).view(np.float32)
    return system, bodies, entries


def same(got, ref, capacity, tag):
    system, bodies, entries = got
    assert system.tobytes() == kref.system_record(ref, capacity).tobytes(), (tag, system, kref.system_record(ref, capacity))
    assert bodies.tobytes() == ref["bodies"].tobytes(), (tag, bodies, ref["bodies"])
    assert entries.tobytes() == kref.listed(ref, capacity).tobytes(), (tag, entries, kref.listed(ref, capacity))
    kref.check_identity(bodies, int(system["pairs"]))


def capacities_around(pairs):
    return sorted({0, 1, max(pairs - 1, 0), pairs, pairs + 3})


def run_cases(driver, cases):
    """cases: (tag, pos, n, slots, shape, capacity, keywords, reference); one process runs them all."""
    out = driver("".join(command(pos, n, slots, shape, capacity, **kw) for _, pos, n, slots, shape, capacity, kw, _ in cases))
    assert len(out) == 3 * len(cases) + 1 and out[-1] == ""
    for at, (tag, _, _, slots, _, capacity, _, ref) in enumerate(cases):
        same(parse(out[3 * at:3 * at + 3], slots, capacity), ref, capacity, tag)


def gpu_cases(capacity, shapes, always=(0,)):
    P, counts, R = kref.gpu_inputs(capacity)
    cases = []
    for mode in kref.MODES:
        for with_subset in (False, True):
            refs = kref.gpu_reference(capacity, mode, with_subset)
            subset = kref.gpu_subset(capacity) if with_subset else None
            for s, n in enumerate(counts):
                kw = {"radius": kref.RADIUS[s]} if mode == "radius" else {"radii": R[s]}
                if with_subset:
                    kw["subset"] = subset[s]
                for shape in shapes:
                    for cap in capacities_around(refs[s]["system"]["pairs"]):
                        for a in always:
                            cases.append(((capacity, mode, with_subset, s, shape, cap, a), P[s], n, capacity, shape, cap,
                                          dict(kw, always=a), refs[s]))
    return cases


def test_the_layout(driver):
    assert [int(w) for w in driver("layout\n")[0].split()] == [48, 0, 4, 8, 12, 16, 24, 32, 36, 40, 44, 16, 0, 4, 8, 12, 12, 0, 4, 8]


@pytest.mark.parametrize("capacity", [64, 128, 320])
def test_the_driver_gives_the_references_records_and_list_exactly(driver, capacity):
    """Every input of the GPU suite in both modes, with and without the subset, at list capacities 0, 1, pairs - 1, pairs and
    pairs + 3, with both fills, for batch_shape's workgroup and for others that hold the slots: more waves, more rows per lane."""
    shapes = {64: [(64, 1), (64, 2), (128, 1)], 128: [(64, 2), (128, 1), (64, 4)], 320: [(128, 4), (64, 8), (320 // 64 * 64, 1)]}[capacity]
    assert SHAPES[capacity] == shapes[0]
    run_cases(driver, gpu_cases(capacity, shapes, always=(0, 1)))


def test_the_driver_at_4096_bodies(driver):
    cases = [c for c in gpu_cases(4096, [SHAPES[4096]]) if c[0][3] == 4 and c[0][5] != 1]
    assert len(cases) == 4 * 4
    run_cases(driver, cases)
    assert cases[0][-1]["system"]["pairs"] > 4096


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    run_cases(checked_driver, gpu_cases(128, [(64, 2), (128, 1)], always=(0, 1)))
    run_cases(checked_driver, [c for c in gpu_cases(320, [SHAPES[320]]) if c[0][3] >= 3])
    assert checked_driver("layout\n")[0].split()[0] == "48"


def test_hand_made_systems_on_the_driver(driver):
    def rows_of(xyz):
        out = np.ones((len(xyz), 4), np.float32)
        out[:, :3] = xyz
        return out
    # on a line at 0, 3, 6, 10: radius 3 touches (0, 1) and (1, 2), exactly on the threshold; (2, 3) at 4 does not
    pos = rows_of([(0, 0, 0), (3, 0, 0), (6, 0, 0), (10, 0, 0)])
    system, bodies, entries = parse(driver(command(pos, 4, 4, (64, 1), 4, radius=3.0)), 4, 4)
    assert entries["i"].tolist() == [0, 1, -1, -1] and entries["j"].tolist() == [1, 2, -1, -1] and entries["r2"].tolist() == [9, 9, np.inf, np.inf]
    assert bodies["degree"].tolist() == [1, 2, 1, 0] and bodies["upper"].tolist() == [1, 1, 0, 0] and bodies["first"].tolist() == [0, 1, 2, 2]
    assert bodies["nearest"].tolist() == [1, 0, 1, -1]                                        # a tie: the lower index
    assert (system["pairs"], system["stored"], system["closest_i"], system["closest_j"], system["closest_r2"]) == (2, 2, 0, 1, 9)
    # radii: (0, 1) needs R_0 + R_1 >= 3; coincident bodies of zero radius touch; a NaN body and one at +inf touch nothing
    pos = rows_of([(0, 0, 0), (3, 0, 0), (3, 0, 0), (np.nan, 0, 0), (0, np.inf, 0)])
    R = np.array([1, 2, 0, 50, 50], np.float32)
    system, bodies, entries = parse(driver(command(pos, 5, 5, (64, 1), 3, radii=R)), 5, 3)
    assert entries["i"].tolist() == [0, 1, -1] and entries["j"].tolist() == [1, 2, -1] and entries["r2"].tolist() == [9, 0, np.inf]
    assert (system["closest_i"], system["closest_j"], system["closest_r2"], system["touching"], system["bodies"]) == (1, 2, 0, 3, 5)
    R0 = np.zeros(5, np.float32)
    system, bodies, entries = parse(driver(command(pos, 5, 5, (64, 1), 2, radii=R0)), 5, 2)
    assert entries["i"].tolist() == [1, -1] and system["pairs"] == 1                           # the coincident pair alone
    # a radius whose square overflows is within reach of every measured pair and of no unmeasured one
    system, _, _ = parse(driver(command(pos, 5, 5, (64, 1), 0, radius=3e38)), 5, 0)
    assert system["pairs"] == 3 and system["stored"] == 0
    # the subset: body 1 out, so (0, 1) and (1, 2) go and nothing else comes
    system, bodies, _ = parse(driver(command(pos, 5, 5, (64, 1), 0, radii=R, subset=[1, 0, 1, 1, 1])), 5, 0)
    assert system["pairs"] == 0 and system["bodies"] == 4 and system["closest_i"] == -1 and np.isinf(system["closest_r2"])
    assert bodies.tobytes() == np.array([(0, 0, 0, -1)] * 5, kref.BODY_DTYPE).tobytes()


# ---- the inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", kref.CAPACITIES)
def test_the_inputs_do_their_work(capacity):
    P, counts, R = kref.gpu_inputs(capacity)
    assert counts == [0, 1, 2, min(65, capacity), capacity]
    m = kref.marks(capacity)
    T, rpl = SHAPES[capacity]
    for mode in kref.MODES:
        for with_subset in (False, True):
            refs = kref.gpu_reference(capacity, mode, with_subset)
            pairs = [r["system"]["pairs"] for r in refs]
            assert pairs[0] == pairs[1] == pairs[2] == 0 and pairs[3] > 0 and pairs[4] > capacity // 4   # systems with no contact
            full = refs[4]
            listed = set(zip(full["list"]["i"].tolist(), full["list"]["j"].tolist()))
            a, b, c = m["a"], m["b"], m["c"]
            codes = kref.r2_codes(P[4], capacity)
            t2 = kref.thresholds(capacity, radius=kref.RADIUS[4]) if mode == "radius" else kref.thresholds(capacity, radii=R[4])
            t2 = np.broadcast_to(t2, codes.shape)
            assert (a, b) in listed and codes[a, b] == t2[a, b]                                   # exactly on the threshold
            assert (a, c) not in listed and codes[a, c] == t2[a, c] + 1                           # one beyond it
            assert m["same"] in listed and codes[m["same"]] == 0                                  # coincident bodies
            assert (2, 20) in set(zip(refs[3]["list"]["i"].tolist(), refs[3]["list"]["j"].tolist())) and R[3, 2] == R[3, 20] == 0
            assert np.isnan(P[3, 5, 1]) and np.isinf(P[3, 9, 0])
            assert refs[3]["bodies"]["degree"][5] == 0 and refs[3]["bodies"]["degree"][9] == 0   # unmeasured: no contact
            last, wave = m["last"][0], m["wave"][0]
            assert full["bodies"]["upper"][last] > 0 and last // T == (capacity - 1) // T        # the last q that holds rows
            assert full["bodies"]["upper"][wave] > 0 and (wave % T) // 64 == T // 64 - 1         # the last wave
            assert 0 < full["bodies"]["degree"][:capacity].mean() < 10                           # single digits
            kref.check_identity(full["bodies"], full["system"]["pairs"])
            cut = kref.truncating_capacity(refs)
            row = np.searchsorted(full["bodies"]["first"], cut, side="right") - 1
            assert 0 < cut < full["system"]["pairs"] and full["bodies"]["first"][row] < cut < full["bodies"]["first"][row] + full["bodies"]["upper"][row]
    # non-contacts in radius mode of the no-contact system sit well beyond the threshold
    assert kref.r2_codes(P[2], 2)[0, 1] > 16


# ---- the premise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", kref.CAPACITIES)
def test_the_fp32_chain_gives_the_integer_r2_and_the_fp32_operations_the_exact_thresholds_on_every_input(capacity):
    """Finite coordinates are integers within the limit, so the fp32 operations one by one (numpy has no fused multiply-add,
    and needs none where nothing rounds) give the integer r2 of the reference; the radii are small integers, so the fp32 sum
    and the fp32 products are the exact ones."""
    P, counts, R = kref.gpu_inputs(capacity)
    for s, n in enumerate(counts):
        x = np.asarray(P[s, :n, :3], dtype=np.float32)
        finite = np.isfinite(x).all(axis=1)
        assert np.array_equal(x[finite], np.round(x[finite])) and (np.abs(x[finite]) <= kref.LIMIT).all()
        rows = np.arange(0, n, max(n // 64, 1))
        with np.errstate(invalid="ignore", over="ignore"):
            d = x[None, :, :] - x[rows][:, None, :]
            r2 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
        assert r2.dtype == np.float32
        codes = kref.r2_codes(P[s], n)[rows]
        measured = codes < kref.TOP
        assert np.array_equal(r2[measured].astype(np.int64), codes[measured]) and (codes[measured] < 2 ** 24).all()
        assert not (r2[~measured] <= np.finfo(np.float32).max).any()
        r = R[s, :n]
        S = r[rows][:, None] + r[None, :]
        assert S.dtype == np.float32 and np.array_equal((S * S).astype(np.int64), kref.thresholds(n, radii=r)[rows])
        b = np.float32(kref.RADIUS[s])
        assert float(b * b) == float(kref.thresholds(n, radius=kref.RADIUS[s]))


# ---- the helpers of the result -------------------------------------------------------------------------------------------------
def test_the_host_methods_of_the_result_on_hand_made_records():
    from n_body_problem_amd import batch
    systems = np.zeros(2, batch.CONTACT_SYSTEM_DTYPE)
    systems["pairs"], systems["stored"] = [3, 4], [3, 2]
    systems["closest_i"], systems["closest_j"], systems["closest_r2"] = [0, -1], [2, -1], [4.0, np.inf]
    systems["touching"], systems["max_degree"], systems["bodies"] = [3, 4], [2, 3], [4, 4]
    entries = np.zeros((2, 3), batch.CONTACT_DTYPE)
    entries["i"], entries["j"], entries["r2"] = [[0, 0, 1], [0, 0, -1]], [[1, 2, 2], [1, 3, -1]], [[9, 4, 16], [1, 1, np.inf]]
    bodies = np.zeros((2, 4), batch.CONTACT_BODY_DTYPE)
    bodies["degree"][0], bodies["upper"][0], bodies["first"][0], bodies["nearest"][0] = [2, 2, 2, 0], [2, 1, 0, 0], [0, 2, 3, 3], [2, 0, 0, -1]
    res = batch.ContactsResult(systems, bodies, entries)
    assert res.pairs.tolist() == [3, 4] and res.stored.tolist() == [3, 2] and res.truncated.tolist() == [False, True]
    assert res.closest.tolist() == [[0, 2], [-1, -1]] and res.closest_distance.tolist() == [2.0, np.inf] and res.capacity == 3
    assert res.degree[0].tolist() == [2, 2, 2, 0] and res.first[0].tolist() == [0, 2, 3, 3] and res.nearest[0].tolist() == [2, 0, 0, -1]
    assert res.distance[0].tolist() == [3.0, 2.0, 4.0] and np.isinf(res.distance[1, 2])
    assert res.pairs_of(0).tolist() == [[0, 1], [0, 2], [1, 2]] and res.pairs_of(1).tolist() == [[0, 1], [0, 3]]
    assert res.pairs_of(0).shape == (3, 2)
    assert res.partners_of(0, 0).tolist() == [1, 2] and res.partners_of(0, 2).tolist() == [0, 1] and res.partners_of(0, 3).tolist() == []
    with pytest.raises(ValueError, match="truncated"):
        res.partners_of(1, 0)
    lean = batch.ContactsResult(systems, None, None)
    assert lean.degree is None and lean.i is None and lean.distance is None and lean.capacity == 0
    with pytest.raises(ValueError, match="lists=True"):
        lean.pairs_of(0)
    assert "ContactsResult(pairs=[3, 4]" in repr(res)
