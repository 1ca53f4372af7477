"""CPU-only: the groups of batched ensembles (nbody_batch_groups, include/nbody_batch_groups.h).  The header is self-contained
C99, included by nbody.h after the gravity header, and declares its one entry point alone; it is exported, bound and listed
apart; the arithmetic without a GPU (csrc/nbody_batch_groups_math.h), built into a stand-alone driver with g++, gives the
union-find's labels on every input of the GPU suite and the hand-worked cases as worked; the hook earns its place on permuted
chains; and on every input of the GPU suite no pair comes within 1e-4 of the linking length, so that those inputs, not a
tolerance, carry the GPU test."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_groups_ref as gref
from conftest import ROOT

NAMES = ["nbody_batch_groups"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_gravity_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_groups.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_groups.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_gravity.h"') < nbody_h.index('#include "nbody_batch_groups.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_8_64_and_32_bytes(tmp_path):
    src = tmp_path / "groups.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char body_is_8_bytes[sizeof(nbody_batch_group_body) == 8 ? 1 : -1];
typedef char record_is_64_bytes[sizeof(nbody_batch_group_record) == 64 ? 1 : -1];
typedef char system_is_32_bytes[sizeof(nbody_batch_group_system) == 32 ? 1 : -1];
typedef char group_at_0[offsetof(nbody_batch_group_body, group) == 0 ? 1 : -1];
typedef char size_at_4[offsetof(nbody_batch_group_body, size) == 4 ? 1 : -1];
typedef char weight_at_0[offsetof(nbody_batch_group_record, weight) == 0 ? 1 : -1];
typedef char centre_at_8[offsetof(nbody_batch_group_record, centre) == 8 ? 1 : -1];
typedef char velocity_at_32[offsetof(nbody_batch_group_record, velocity) == 32 ? 1 : -1];
typedef char count_at_56[offsetof(nbody_batch_group_record, count) == 56 ? 1 : -1];
typedef char sources_at_60[offsetof(nbody_batch_group_record, sources) == 60 ? 1 : -1];
typedef char groups_at_0[offsetof(nbody_batch_group_system, groups) == 0 ? 1 : -1];
typedef char grouped_at_4[offsetof(nbody_batch_group_system, grouped) == 4 ? 1 : -1];
typedef char singles_at_8[offsetof(nbody_batch_group_system, singles) == 8 ? 1 : -1];
typedef char largest_at_12[offsetof(nbody_batch_group_system, largest) == 12 ? 1 : -1];
typedef char largest_count_at_16[offsetof(nbody_batch_group_system, largest_count) == 16 ? 1 : -1];
typedef char sweeps_at_20[offsetof(nbody_batch_group_system, sweeps) == 20 ? 1 : -1];
typedef char converged_at_24[offsetof(nbody_batch_group_system, converged) == 24 ? 1 : -1];
typedef char reserved_at_28[offsetof(nbody_batch_group_system, reserved) == 28 ? 1 : -1];
typedef char limit[NBODY_BATCH_GROUPS_MAX_SWEEPS == 64 ? 1 : -1];
int main(void) {
    nbody_batch_group_system s;
    float b = 1.0f;
    return (nbody_batch_groups(0, 0, 0, &b, 2, NBODY_BATCH_WEIGHT_MASS, 64, &s, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_groups.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_gravity.h", "The rows are all i < counts[s]",
                   "whatever the massive counts", "this is geometry", "as the state holds them",
                   "friends iff r2 <= b2", "every fmaf one fused operation", "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))",
                   "b2 = b[s] b[s], one fp32 product formed on the host", "There is no softening", "bit-symmetric in i and j",
                   "A NaN coordinate links to nothing", "b[s] == 0 links only coincident bodies", "L_i starts as i",
                   "all reads before any write", "c_i = min L_j over the friends of i",
                   "L[L_i] = min(L[L_i], c_i) and L_i = c_i", "L_i is a root here", "Min commutes",
                   "L_i <- L[L_i] for all rows at once, repeated until a pass changes nothing",
                   "its Link step lowered no label: converged = 1", "t == max_sweeps: converged = 0",
                   "it is a function of the state alone", "L_i is the lowest index of i's group",
                   "NBODY_BATCH_GROUPS_MAX_SWEEPS (64) keeps a launch bounded", "NBODY_BATCH_WEIGHT_MASS", "NBODY_BATCH_WEIGHT_NUMBER",
                   "m = min(massive[s], counts[s])", "otherwise m = counts[s]", "w_j = 0 for a test particle",
                   "mass word is read by nothing here", "w_j = 1 for every body", "fp64 from the fp32 state",
                   "in ascending index", "Each product is exact", "Nothing is summed across lanes",
                   "-1 and 0 from the count on", "filled at slot r where L_r == r", "0 where the weight is 0",
                   "count (all members) and sources (the members j < m)", "is the all-zero record",
                   "groups with count >= min_members", "ties to the lower root", "-1 for a system without bodies",
                   "largest = -1, sweeps = 0 and converged = 1", "NULL skips that copy", "the same bits either way", "synchronous",
                   "forgets nothing", "bit for bit", "allocated on first use and freed in nbody_batch_destroy",
                   "the same bits in any slot, n_systems and max_bodies", "names the function", "a NULL handle",
                   "a negative or non-finite linking length", "min_members < 1", "an unknown weight", "max_sweeps outside 1 ... 64",
                   "refused before any device work", "Out of scope", "linking in velocity (6-D FoF)", "unbinding of the groups",
                   "periodic boxes", "groups across systems", "second moments", "changing the state"):
        assert phrase in text, phrase
    # the gravity header, which this one follows, is as it was
    assert "nbody_batch_groups" not in open(os.path.join(INCLUDE, "nbody_batch_gravity.h")).read()


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert _lib.groups_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                             set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                             set(_lib.fate_names()) | set(_lib.accrete_names()) | set(_lib.field_names()) | set(_lib.pairs_names()) |
                             set(_lib.structure_names()) | set(_lib.members_names()) | set(_lib.hierarchy_names()) |
                             set(_lib.gravity_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchGroupBody) == 8 and ctypes.sizeof(_lib.BatchGroupRecord) == 64
    assert ctypes.sizeof(_lib.BatchGroupSystem) == 32
    assert [f[0] for f in _lib.BatchGroupBody._fields_] == ["group", "size"]
    assert [f[0] for f in _lib.BatchGroupRecord._fields_] == ["weight", "centre", "velocity", "count", "sources"]
    assert [f[0] for f in _lib.BatchGroupSystem._fields_] == ["groups", "grouped", "singles", "largest", "largest_count", "sweeps",
                                                              "converged", "reserved"]
    assert _lib.BatchGroupRecord.count.offset == 56 and _lib.BatchGroupSystem.converged.offset == 24
    assert _lib.BATCH_GROUPS_MAX_SWEEPS == gref.MAX_SWEEPS == 64


def test_the_abi_stays_at_version_5_and_a_null_handle_is_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchGroupSystem * 1)()
    b = (ctypes.c_float * 1)(1.0)
    assert lib.nbody_batch_groups(None, None, None, b, 2, 0, 64, out, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_groups: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_surface():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    sig = inspect.signature(nb.BatchedSystem.groups)
    assert list(sig.parameters) == ["self", "linking_length", "min_members", "weight", "max_sweeps", "records", "bodies"]
    assert sig.parameters["linking_length"].default is inspect.Parameter.empty
    assert [sig.parameters[p].default for p in ("min_members", "weight", "max_sweeps", "records", "bodies")] == [2, "mass", 64, True, True]
    assert {"BatchGroups", "GROUP_BODY_DTYPE", "GROUP_RECORD_DTYPE", "GROUP_SYSTEM_DTYPE"} <= set(batch.__all__)
    assert nb.BatchGroups is batch.BatchGroups and "BatchGroups" in nb.__all__
    assert batch.GROUP_BODY_DTYPE.itemsize == 8 and batch.GROUP_RECORD_DTYPE.itemsize == 64 and batch.GROUP_SYSTEM_DTYPE.itemsize == 32
    assert batch.GROUP_RECORD_DTYPE.fields["count"][1] == 56 and batch.GROUP_SYSTEM_DTYPE.fields["sweeps"][1] == 20
    # a result built by hand: two systems of capacity 5, the second empty.  System 0: {0, 2, 3}, {1, 4} -- no, {1}, {4}: a
    # group of three and two singles
    systems = np.zeros(2, dtype=batch.GROUP_SYSTEM_DTYPE)
    systems[0] = (1, 3, 2, 0, 3, 2, 1, 0)
    systems[1] = (0, 0, 0, -1, 0, 0, 1, 0)
    bodies = np.zeros((2, 5), dtype=batch.GROUP_BODY_DTYPE)
    bodies[0] = [(0, 3), (1, 1), (0, 3), (0, 3), (4, 1)]
    bodies[1] = [(-1, 0)] * 5
    records = np.zeros((2, 5), dtype=batch.GROUP_RECORD_DTYPE)
    records[0, 0] = (1.5, (1.0, 2.0, 3.0), (0.1, 0.2, 0.3), 3, 2)
    records[0, 1] = (0.5, (4.0, 4.0, 4.0), (0.0, 0.0, 0.0), 1, 1)
    records[0, 4] = (0.25, (5.0, 5.0, 5.0), (0.0, 0.0, 0.0), 1, 0)
    res = batch.BatchGroups(systems, records, bodies, [0.5, 0.5], 2, "mass")
    assert res.groups.tolist() == [1, 0] and res.grouped.tolist() == [3, 0] and res.singles.tolist() == [2, 0]
    assert res.largest.tolist() == [0, -1] and res.largest_count.tolist() == [3, 0] and res.sweeps.tolist() == [2, 0]
    assert res.converged.tolist() == [True, True] and res.converged.dtype == np.bool_ and res.groups.dtype == np.int32
    assert res.group[0].tolist() == [0, 1, 0, 0, 4] and res.size[0].tolist() == [3, 1, 3, 3, 1] and res.group.dtype == np.int32
    assert res.weight[0].tolist() == [1.5, 0.5, 0.0, 0.0, 0.25] and res.centre.shape == (2, 5, 3) and res.velocity[0, 0].tolist() == [0.1, 0.2, 0.3]
    assert res.count[0].tolist() == [3, 1, 0, 0, 1] and res.sources[0].tolist() == [2, 1, 0, 0, 0]
    assert res.roots(0).tolist() == [0, 1, 4] and res.roots(1).tolist() == []
    assert [g.tolist() for g in res.groups_of(0)] == [[0, 2, 3]] and res.groups_of(1) == []
    assert res.largest_mask().tolist() == [[True, False, True, True, False], [False] * 5]
    one = batch.BatchGroups(systems, records, bodies, [0.5, 0.5], 1, "mass")           # min_members = 1: the singles too, by root
    assert [g.tolist() for g in one.groups_of(0)] == [[0, 2, 3], [1], [4]]
    lean = batch.BatchGroups(systems, None, None, [0.5, 0.5], 2, "mass")
    assert all(getattr(lean, name) is None for name in ("group", "size", "weight", "centre", "velocity", "count", "sources"))
    assert lean.groups.tolist() == [1, 0]
    with pytest.raises(ValueError, match="bodies=True"):
        lean.largest_mask()


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_groups.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
static_assert(sizeof(nbody_batch_group_body) == 8 && sizeof(nbody_batch_group_record) == 64 &&
              sizeof(nbody_batch_group_system) == 32, "the records");
int main() {
    try {
        nbody::Batch b(16, 64);
        std::vector<float> length(16, 0.5f);
        std::vector<nbody_batch_group_record> groups;
        std::vector<nbody_batch_group_body> bodies;
        std::vector<nbody_batch_group_system> s = b.groups(nullptr, nullptr, length);
        std::vector<nbody_batch_group_system> t = b.groups(nullptr, nullptr, length, 3, NBODY_BATCH_WEIGHT_NUMBER, 8, &groups, &bodies);
        std::printf("%lld %lld %lld %lld\n", (long long)s.size(), (long long)t.size(), (long long)groups.size(), (long long)bodies.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_groups"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-L" + os.path.join(ROOT, "n_body_problem_amd"),
           "-lnbody_amd", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_groups_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_groups.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_groups_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and "return r2 <= b2;" in text
    assert "__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx))" in text
    hip = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    assert '#include "nbody_batch_groups_math.h"' in hip
    # the kernel links, hooks, compresses and sums with the header's functions, not with copies of them
    kernel = hip[hip.index("void batch_groups_kernel("):hip.index("hipError_t launch_batch_groups(")]
    for call in ("groups_link(", "groups_lowered(", "groups_hook(", "groups_compress(", "groups_weight(", "groups_add_position(",
                 "groups_add_velocity(", "groups_record(", "groups_tally_root(", "groups_summary(", "groups_empty_record()",
                 "groups_empty_body()", "atomicMin("):
        assert call in kernel, call
    assert "fmaf" not in kernel and "<=" not in kernel          # no second copy of the predicate


# ---- the arithmetic, through the driver ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("groups") / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_groups_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


def drive(driver, pos, vel, n, b, m=None, weight=0, min_members=2, max_sweeps=64):
    """One system through the driver: a dict shaped like hermite_groups_ref.groups'."""
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    lines = [f"system {n} {n if m is None else m} {weight} {min_members} {max_sweeps} {float(np.float32(b))!r}"]
    lines += [" ".join(repr(float(u)) for u in (*pos[i], *vel[i, :3])) for i in range(n)]
    out = driver("\n".join(lines) + "\n")
    head = [int(w) for w in out[0].split()]
    res = dict(zip(("sweeps", "converged", "groups", "grouped", "singles", "largest", "largest_count", "reserved"), head))
    res["group"], res["size"] = np.array(out[1].split(), dtype=np.int32), np.array(out[2].split(), dtype=np.int32)
    roots = int(out[3])
    assert len(out) == 4 + roots
    res.update({"weight": np.zeros(n), "centre": np.zeros((n, 3)), "velocity": np.zeros((n, 3)), "count": np.zeros(n, np.int32),
                "sources": np.zeros(n, np.int32)})
    for line in out[4:]:
        w = line.split()
        r = int(w[0])
        res["weight"][r], res["centre"][r], res["velocity"][r] = float(w[1]), [float(u) for u in w[2:5]], [float(u) for u in w[5:8]]
        res["count"][r], res["sources"][r] = int(w[8]), int(w[9])
    return res


def same(got, ref, truth=True):
    """The driver's (or the library's) system against the reference: integers equal, doubles bit for bit."""
    for name in ("sweeps", "converged", "groups", "grouped", "singles", "largest", "largest_count"):
        assert got[name] == ref[name], (name, got[name], ref[name])
    for name in ("group", "size", "count", "sources"):
        assert np.array_equal(got[name], ref[name]), name
    for name in ("weight", "centre", "velocity"):
        assert np.array_equal(got[name].view(np.int64), ref[name].view(np.int64)), name
    if truth:
        assert np.array_equal(got["group"], ref["true_group"]) and np.array_equal(got["size"], ref["true_size"])


def gpu_suite_inputs():
    """Every (tag, pos, vel, n, b, m) of the GPU suite."""
    for capacity in gref.CAPACITIES:
        for which in "ab":
            P, V, counts, b = gref.gpu_inputs(capacity, which)
            for s, n in enumerate(counts):
                yield (capacity, which, s), P[s], V[s], n, b[s], None
    P, V, counts, massive, b = gref.massive_inputs()
    for s, n in enumerate(counts):
        yield ("massive", s), P[s], V[s], n, b[s], massive[s]
    for k, (pos, vel, b) in enumerate(gref.invariance_inputs()):
        yield ("invariance", k), pos, vel, gref.INVARIANCE_BODIES, b, None
    pos, vel, lengths = gref.ladder_inputs()
    for k, b in enumerate(lengths):
        yield ("ladder", k), pos, vel, gref.LADDER_BODIES, b, None


def test_the_record_sizes_offsets_and_the_empty_records(driver):
    out = driver("layout\nempty\n")
    assert [int(w) for w in out[0].split()] == [8, 0, 4, 64, 0, 8, 32, 56, 60, 32, 0, 4, 8, 12, 16, 20, 24, 28]
    assert [float(w) for w in out[1].split()] == [-1, 0, 0, 0, 0, 0, 0, 0, -1, 0, 0, 1, 0, 64]


def test_the_shared_math_gives_the_union_finds_labels_on_every_input_of_the_gpu_suite(driver):
    """The functions the kernel calls, in sequential loops: the labels and sizes are the union-find's, the sweeps the schedule
    mirror's, the records the sequential fp64 sums, bit for bit."""
    seen = 0
    for tag, pos, vel, n, b, m in gpu_suite_inputs():
        if tag[0] in gref.CAPACITIES:
            ref = gref.reference(tag[0], tag[1])[tag[2]]
        else:
            ref = gref.groups(pos, vel, n, b, m=m)
        same(drive(driver, pos, vel, n, b, m=m), ref)
        assert ref["converged"] == 1 and ref["sweeps"] <= 16, tag
        seen += 1
    assert seen == 4 * 11 + 4 + 2 + 6


def test_hand_worked_cases_come_out_as_worked(driver):
    zero = np.zeros((8, 4), np.float32)

    def system(xs, b, masses=None, **kw):
        n = len(xs)
        pos = np.zeros((n, 4), np.float32)
        pos[:, :3] = xs
        pos[:, 3] = 1.0 if masses is None else masses
        return drive(driver, pos, zero[:n], n, b, **kw)

    # two bodies at distance 1: friends at b = 1 (r2 <= b2 holds with equality), not at the float below 1
    inside = system([[0, 0, 0], [1, 0, 0]], 1.0)
    assert inside["group"].tolist() == [0, 0] and inside["size"].tolist() == [2, 2] and inside["sweeps"] == 2 and inside["groups"] == 1
    assert inside["weight"][0] == 2.0 and inside["centre"][0].tolist() == [0.5, 0, 0] and inside["largest_count"] == 2
    outside = system([[0, 0, 0], [1, 0, 0]], np.nextafter(np.float32(1), np.float32(0)))
    assert outside["group"].tolist() == [0, 1] and outside["sweeps"] == 1 and outside["groups"] == 0 and outside["singles"] == 2
    assert outside["largest"] == 0 and outside["largest_count"] == 1 and outside["grouped"] == 0        # the tie goes to the lower root
    # a lone body: one sweep that lowers nothing
    lone = system([[3, 4, 5]], 10.0, masses=[2.5])
    assert lone["group"].tolist() == [0] and lone["sweeps"] == 1 and lone["converged"] == 1 and lone["singles"] == 1
    assert lone["weight"][0] == 2.5 and lone["centre"][0].tolist() == [3, 4, 5] and lone["count"][0] == 1 and lone["groups"] == 0
    # b = 0 links coincident bodies alone
    coincident = system([[1, 1, 1], [2, 2, 2], [1, 1, 1], [2, 2, 2.0000002]], 0.0)
    assert coincident["group"].tolist() == [0, 1, 0, 3] and coincident["groups"] == 1 and coincident["singles"] == 2
    # a NaN coordinate links to nothing, not even to a body at the same place
    nan = system([[0, 0, 0], [np.nan, 0, 0], [0.5, 0, 0], [np.nan, 0, 0]], 1.0)
    assert nan["group"].tolist() == [0, 1, 0, 3] and nan["size"].tolist() == [2, 1, 2, 1] and np.isnan(nan["centre"][1][0])
    # a chain of three whose ends are no friends: the middle body joins them; its index is the highest
    three = system([[0, 0, 0], [2, 0, 0], [1, 0, 0]], 1.25, masses=[1, 2, 1])
    assert three["group"].tolist() == [0, 0, 0] and three["size"].tolist() == [3, 3, 3] and three["converged"] == 1
    assert three["weight"][0] == 4.0 and three["centre"][0].tolist() == [1.25, 0, 0] and three["count"].tolist() == [3, 0, 0]
    # ... and with the ends first: body 1 reaches label 0 only through body 2, in a second lowering sweep or by the hook
    assert system([[0, 0, 0], [2, 0, 0], [1, 0, 0]], 1.25, max_sweeps=1)["converged"] == 0
    # weights: with one massive body the others weigh nothing; by number all weigh 1
    massive = system([[0, 0, 0], [1, 0, 0], [2, 0, 0]], 1.25, masses=[4, np.nan, np.nan], m=1)
    assert massive["weight"][0] == 4.0 and massive["centre"][0].tolist() == [0, 0, 0] and massive["sources"][0] == 1 and massive["count"][0] == 3
    number = system([[0, 0, 0], [1, 0, 0], [2, 0, 0]], 1.25, masses=[0, 0, 0], m=0, weight=1)
    assert number["weight"][0] == 3.0 and number["centre"][0].tolist() == [1, 0, 0] and number["sources"][0] == 0
    weightless = system([[0, 0, 0], [1, 0, 0]], 1.25, masses=[0, 0])
    assert weightless["weight"][0] == 0.0 and weightless["centre"][0].tolist() == [0, 0, 0] and weightless["count"][0] == 2
    # min_members moves groups and grouped alone
    for k, (groups, grouped) in {1: (2, 4), 2: (1, 3), 3: (1, 3), 4: (0, 0)}.items():
        res = system([[0, 0, 0], [1, 0, 0], [2, 0, 0], [9, 9, 9]], 1.25, min_members=k)
        assert (res["groups"], res["grouped"], res["singles"], res["largest_count"]) == (groups, grouped, 1, 3)
    empty = system(np.zeros((0, 3)), 1.0)
    assert (empty["sweeps"], empty["converged"], empty["largest"], empty["groups"]) == (0, 1, -1, 0)


def test_the_hook_earns_its_place_on_permuted_chains():
    """Unit spacing, b = 1.25, seeds 0 to 4: with the hook the schedule converges within 16 sweeps at every size of the GPU
    suite (8 to 10 at 4096 bodies); without it, 4096 bodies are not done after 64.  So a GPU run that equals this mirror cannot
    hide a failure behind converged = 0."""
    for n in (64, 128, 320, 4096):
        for seed in range(5):
            pos, _ = gref.chain(n, seed)
            pairs = gref.edges(pos, n, gref.CHAIN_B)
            labels, sweeps, converged = gref.schedule(pos, n, gref.CHAIN_B, pairs=pairs)
            print(n, seed, sweeps)
            assert converged == 1 and sweeps <= 16 and not labels.any(), (n, seed, sweeps)
            if n == 4096:
                assert 8 <= sweeps <= 10, (seed, sweeps)
                plain = gref.schedule(pos, n, gref.CHAIN_B, hook=False, pairs=pairs)
                assert plain[1] == 64 and plain[2] == 0 and plain[0].any(), seed
    # one sweep alone leaves the chain in pieces: the labels of the GPU suite's max_sweeps = 1 case are no single group
    pos, _ = gref.chain(64, 64)
    labels, sweeps, converged = gref.schedule(pos, 64, gref.CHAIN_B, max_sweeps=1)
    assert (sweeps, converged) == (1, 0) and labels.any()


def test_the_inputs_condition():
    """On every input of the GPU suite no pair has |r2 / b2 - 1| < 1e-4 in fp64, so the fp32 predicate (three roundings, a few
    1e-7) and the fp64 union-find cannot disagree: the GPU test needs no tolerance.  The inputs also do what they are for: the
    clumps are one group with the bridge's middle body and two without it, and the cube has many groups of many sizes."""
    seen, worst = 0, np.inf
    for tag, pos, vel, n, b, m in gpu_suite_inputs():
        mg = gref.margin(pos, n, b)
        worst = min(worst, mg)
        seen += 1
        assert mg >= gref.MARGIN, (tag, mg)
    print(f"{seen} systems, smallest margin {worst:.3g}")
    assert seen == 4 * 11 + 4 + 2 + 6 and gref.MARGIN == 1e-4
    for capacity in gref.CAPACITIES:
        a, b = gref.reference(capacity, "a"), gref.reference(capacity, "b")
        assert [r["count"].sum() for r in a] == [capacity, 0, capacity - 1, 1, capacity - 2, 2]
        assert [r["count"].sum() for r in b] == [2, capacity, 0, 1, capacity - 3]
        joined, split = a[2], a[4]
        assert split["groups"] == joined["groups"] + 1 and joined["largest_count"] > split["largest_count"] + capacity // 4
        assert a[0]["groups"] == 1 and a[0]["largest_count"] == capacity and b[4]["largest_count"] == capacity - 3
        cube = b[1]
        assert cube["groups"] >= capacity // 16 and len(set(cube["size"].tolist())) >= 5 and cube["singles"] >= 5
