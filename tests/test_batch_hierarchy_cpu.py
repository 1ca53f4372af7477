"""CPU-only: hierarchies of batched ensembles (nbody_batch_hierarchy, include/nbody_batch_hierarchy.h).  The header is
self-contained C99, included by nbody.h after the members header, and declares its one entry point alone; it is exported,
bound and listed apart; the fp64 arithmetic without a GPU (csrc/nbody_batch_hierarchy_math.h), built into a stand-alone
driver with g++, gives closed forms; the numpy reference (hermite_hierarchy_ref) gives the hand-worked hierarchies; and every
input of the GPU suite keeps the four margins of the inputs condition, so that those inputs, not a tolerance, carry the
GPU test's exact comparisons."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_hierarchy_ref as href
import hermite_pairs_ref as pref
from conftest import ROOT

NAMES = ["nbody_batch_hierarchy"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


def result_of(refs):
    """A HierarchyResult built by hand from references of one capacity."""
    from n_body_problem_amd import batch
    cap = len(refs[0]["parent"])
    systems = np.zeros(len(refs), dtype=batch.HIERARCHY_SYSTEM_DTYPE)
    nodes = np.zeros((len(refs), cap), dtype=batch.HIERARCHY_NODE_DTYPE)
    bodies = np.zeros((len(refs), cap), dtype=batch.HIERARCHY_BODY_DTYPE)
    for s, ref in enumerate(refs):
        for name in href.SYSTEM_FIELDS:
            systems[name][s] = ref[name]
        for name in nodes.dtype.names:
            if name != "reserved":
                nodes[name][s] = ref["node_parent" if name == "parent" else name]
        for name in ("parent", "root", "depth"):
            bodies[name][s] = ref[name]
    return batch.HierarchyResult(systems, nodes, bodies, [ref["count"] for ref in refs])


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_members_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_hierarchy.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_hierarchy.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_members.h"') < nbody_h.index('#include "nbody_batch_hierarchy.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_128_16_and_40_bytes(tmp_path):
    src = tmp_path / "hierarchy.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char node_is_128_bytes[sizeof(nbody_batch_hierarchy_node) == 128 ? 1 : -1];
typedef char body_is_16_bytes[sizeof(nbody_batch_hierarchy_body) == 16 ? 1 : -1];
typedef char system_is_40_bytes[sizeof(nbody_batch_hierarchy_system) == 40 ? 1 : -1];
typedef char parent_at_8[offsetof(nbody_batch_hierarchy_node, parent) == 8 ? 1 : -1];
typedef char stable_at_24[offsetof(nbody_batch_hierarchy_node, stable) == 24 ? 1 : -1];
typedef char mass_at_32[offsetof(nbody_batch_hierarchy_node, mass) == 32 ? 1 : -1];
typedef char energy_at_40[offsetof(nbody_batch_hierarchy_node, energy) == 40 ? 1 : -1];
typedef char perturbation_at_80[offsetof(nbody_batch_hierarchy_node, perturbation) == 80 ? 1 : -1];
typedef char mutual_at_88[offsetof(nbody_batch_hierarchy_node, mutual_inclination) == 88 ? 1 : -1];
typedef char h_at_104[offsetof(nbody_batch_hierarchy_node, h) == 104 ? 1 : -1];
typedef char depth_at_8[offsetof(nbody_batch_hierarchy_body, depth) == 8 ? 1 : -1];
typedef char singles_at_16[offsetof(nbody_batch_hierarchy_system, singles) == 16 ? 1 : -1];
typedef char unstable_at_32[offsetof(nbody_batch_hierarchy_system, unstable) == 32 ? 1 : -1];
typedef char limit[NBODY_BATCH_HIERARCHY_MAX_LEVELS == 16 ? 1 : -1];
int main(void) {
    nbody_batch_hierarchy_system s;
    return (nbody_batch_hierarchy(0, 0, 0, 1.0, 8, &s, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_hierarchy.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_members.h", "The leaves are the bodies j < m",
                   "m = min(massive[s], counts[s])", "Test particles take no part", "counted in nothing",
                   "a node's slot is its smallest leaf index", "dead from then on", "the fp32 search of nbody_batch_pairs.h",
                   "mu = m_j + m_i", "r2 == 0 is no candidate", "ties go to the lower slot", "NaN or +inf eps is never chosen",
                   "mass word in LDS is NaN", "without a branch", "choose each other and whose fp64 energy is < 0",
                   "g = max over live roots k not in {i, j}", "s_k = (m_k inv)(inv inv)", "is 0 with no other root",
                   "perturbation = 2 (double)g Q^3 / mu, Q = a (1 + e)", "accepted unless perturbation > tidal_tolerance",
                   "+inf accepts every candidate", "all of them at once, in ascending lower slot", "has the id counts[s] + k",
                   "a leaf's id is its index", "the merged body of nbody_batch_merge.h, exactly", "fma(m_j, u_j, m_i u_i) / (m_i + m_j)",
                   "rounded once to fp32", "the arithmetic mean", "The state arrays in global memory are never written",
                   "q = m_o / m_c", "0 where a norm is 0",
                   "a (1 - e) / a_c > 2.8 ((1 + q)(1 + e) / sqrt(1 - e))^(2/5) (1 - 0.3 i_mut / pi)", "Mardling & Aarseth (2001)",
                   "A node of two leaves is stable", "after a level that made no node (converged = 1)",
                   "when fewer than two roots live (converged = 1", "a system of one leaf evaluates no level",
                   "after max_levels levels (converged = 0 if the last level still made a node and two or more roots live)",
                   "except that child and parent are -1", "child[0] is the lower slot's id", "beyond the count {-1, -1, 0, 0}",
                   "all zero with converged = 1", "they skip 128 and 16 bytes per slot", "keep the same bits", "synchronous",
                   "forgets nothing", "bit for bit", "allocated on first use and freed in nbody_batch_destroy",
                   "its slot, n_systems, max_bodies and the other systems change no bit",
                   "ids count from counts[s] and not from max_bodies", "names the function", "max_levels outside 1 ... 16",
                   "a NaN or negative tolerance", "refused before any device work", "Out of scope", "softened elements",
                   "test particles as leaves or satellites", "re-pairing a dissolved node", "secular (Kozai) criteria",
                   "changing the state"):
        assert phrase in text, phrase
    assert "nbody_batch_hierarchy" not in open(os.path.join(INCLUDE, "nbody_batch_members.h")).read()


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert _lib.hierarchy_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.evolve_names()) | set(_lib.stop_names()) |
                             set(_lib.merge_exported_names()) | set(_lib.radii_names()) | set(_lib.massive_names()) |
                             set(_lib.fate_names()) | set(_lib.accrete_names()) | set(_lib.field_names()) | set(_lib.pairs_names()) |
                             set(_lib.structure_names()) | set(_lib.members_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchHierarchyNode) == 128 and ctypes.sizeof(_lib.BatchHierarchyBody) == 16
    assert ctypes.sizeof(_lib.BatchHierarchySystem) == 40
    assert [f[0] for f in _lib.BatchHierarchyNode._fields_] == ["child", "parent", "level", "leaves", "slot", "stable", "reserved", "mass",
                                                               "energy", "semi_major_axis", "eccentricity", "inclination",
                                                               "separation", "perturbation", "mutual_inclination", "h"]
    assert [f[0] for f in _lib.BatchHierarchyBody._fields_] == ["parent", "root", "depth", "reserved"]
    assert [f[0] for f in _lib.BatchHierarchySystem._fields_] == [*href.SYSTEM_FIELDS, "reserved"]
    assert _lib.BatchHierarchyNode.mass.offset == 32 and _lib.BatchHierarchyNode.h.offset == 104
    assert _lib.BATCH_HIERARCHY_MAX_LEVELS == href.MAX_LEVELS == 16


def test_the_abi_stays_at_version_5_and_a_null_handle_is_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchHierarchySystem * 1)()
    assert lib.nbody_batch_hierarchy(None, None, None, 1.0, 8, out, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_hierarchy: batch is NULL" in lib.nbody_batch_last_error(None)


def test_the_python_wrapper_has_the_documented_surface_and_the_dtype_sizes():
    import n_body_problem_amd as nb
    from n_body_problem_amd import batch
    sig = inspect.signature(nb.BatchedSystem.hierarchy)
    assert list(sig.parameters) == ["self", "tidal_tolerance", "max_levels", "nodes", "bodies"]
    assert [sig.parameters[p].default for p in ("tidal_tolerance", "max_levels", "nodes", "bodies")] == [np.inf, 8, True, True]
    names = {"HierarchyResult", "HIERARCHY_NODE_DTYPE", "HIERARCHY_BODY_DTYPE", "HIERARCHY_SYSTEM_DTYPE"}
    assert names <= set(batch.__all__) and names <= set(nb.__all__) and nb.HierarchyResult is batch.HierarchyResult
    assert batch.HIERARCHY_NODE_DTYPE.itemsize == 128 and batch.HIERARCHY_BODY_DTYPE.itemsize == 16
    assert batch.HIERARCHY_SYSTEM_DTYPE.itemsize == 40
    assert batch.HIERARCHY_NODE_DTYPE.fields["mass"][1] == 32 and batch.HIERARCHY_NODE_DTYPE.fields["h"][1] == 104
    assert batch.HIERARCHY_NODE_DTYPE.fields["perturbation"][1] == 80 and batch.HIERARCHY_SYSTEM_DTYPE.fields["unstable"][1] == 32


def test_the_cpp_wrapper_compiles_and_links(tmp_path):
    from n_body_problem_amd import build
    build.build_library()
    src = tmp_path / "batch_hierarchy.cpp"
    src.write_text(r'''
#include "nbody.hpp"
#include <cstdio>
static_assert(sizeof(nbody_batch_hierarchy_node) == 128 && sizeof(nbody_batch_hierarchy_body) == 16 &&
              sizeof(nbody_batch_hierarchy_system) == 40, "the records");
int main() {
    try {
        nbody::Batch b(16, 64);
        std::vector<nbody_batch_hierarchy_node> nodes;
        std::vector<nbody_batch_hierarchy_body> bodies;
        std::vector<nbody_batch_hierarchy_system> s = b.hierarchy(nullptr, nullptr);
        std::vector<nbody_batch_hierarchy_system> t = b.hierarchy(nullptr, nullptr, 0.01, 4, nodes, bodies);
        std::printf("%lld %lld %lld\n", (long long)s.size(), (long long)t.size(), (long long)nodes.size());
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
    }
    return 0;
}
''')
    exe = tmp_path / "batch_hierarchy"
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + INCLUDE, str(src), "-L" + os.path.join(ROOT, "n_body_problem_amd"),
           "-lnbody_amd", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "n_body_problem_amd"), "-Wl,-rpath,/opt/rocm/lib",
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_hierarchy_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_hierarchy.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_hierarchy_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and '#include "nbody_batch_pairs_elements.h"' in text
    assert "batch_pair_record(" in text                       # the elements are the pairs header's, not a copy
    hip = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    assert '#include "nbody_batch_hierarchy_math.h"' in hip
    kernel = hip[hip.index("void batch_hierarchy_kernel("):hip.index("hipError_t launch_batch_hierarchy(")]
    for call in ("hierarchy_elements(", "hierarchy_merged(", "hierarchy_perturbation(", "hierarchy_accepts(",
                 "hierarchy_mutual_inclination(", "hierarchy_child_passes(", "hierarchy_empty_node()", "hierarchy_empty_body()"):
        assert call in kernel, call
    assert kernel.count("#pragma unroll 1") >= 2              # the record loop and the children stay rolled


# ---- the arithmetic, through the driver ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hierarchy") / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_hierarchy_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        out = [[float(w) for w in line.split()] for line in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def words(*values):
    return " ".join(repr(float(u)) for u in np.ravel(np.concatenate([np.ravel(v) for v in values])))


def test_the_elements_of_a_known_binary(driver):
    for E in pref.KNOWN_PHASES.values():
        P, V, (a, e, inc, energy, sep) = pref.known_binary(E)
        (mass, en, sma, ecc, incl, r, hx, hy, hz), = driver(["elements " + words(P[0, 0, :3], V[0, 0, :3], P[0, 0, 3:], P[0, 2, :3],
                                                                                 V[0, 2, :3], P[0, 2, 3:])])
        assert mass == 1.0 and en == pytest.approx(energy, rel=1e-6) and sma == pytest.approx(a, rel=1e-6)
        assert ecc == pytest.approx(e, rel=1e-6) and incl == pytest.approx(inc, rel=1e-6) and r == pytest.approx(sep, rel=1e-6)
        want = np.sqrt(a * (1 - e * e)) * np.array([0.0, -np.sin(inc), np.cos(inc)])      # |h| = sqrt(mu a (1 - e^2)), mu = 1
        assert np.allclose([hx, hy, hz], want, rtol=1e-6, atol=1e-7)
        # and they are the reference's own numbers to rounding order
        ref = pref.elements(P[0, 0, :3], V[0, 0, :3], P[0, 2, :3], V[0, 2, :3], 1.0)
        assert np.allclose([en, sma, ecc, incl, r], [float(u) for u in ref], rtol=1e-13)


def test_the_merged_state_is_the_merge_references(driver):
    rng = np.random.default_rng(5)
    mi, mj = rng.uniform(0.5, 1.5, 50).astype(np.float32), rng.uniform(0.5, 1.5, 50).astype(np.float32)
    ui, uj = rng.normal(size=50).astype(np.float32), rng.normal(size=50).astype(np.float32)
    got = np.array(driver([f"merged {words([a], [b], [c], [d])}" for a, b, c, d in zip(mi, ui, mj, uj)]))[:, 0]
    want = np.array([href.merged(a, b, c, d) for a, b, c, d in zip(mi, ui, mj, uj)], dtype=np.float64)
    assert np.array_equal(got, want)
    assert driver(["merged 0 1.5 0 -0.5", "merged 1 2 3 2", "merged 1 0 3 1"]) == [[0.5], [2.0], [0.75]]   # mu == 0: the mean


def test_the_elements_at_mu_zero(driver):
    (mass, en, sma, ecc, incl, r, hx, hy, hz), = driver(["elements 0 0 0 0 0 0 0  3 4 0 0 2 0 0"])
    assert mass == 0 and en == 2.0 and sma == 0 and ecc == np.inf and r == 5.0 and [hx, hy, hz] == [0, 0, 6.0] and incl == 0


def test_the_stability_threshold_on_both_sides(driver):
    pi = np.pi
    for q, e, imut in ((0.5, 0.2, 0.0), (1.0, 0.0, 0.0), (0.1, 0.6, 1.0), (2.0, 0.4, pi)):
        want = 2.8 * ((1 + q) * (1 + e) / np.sqrt(1 - e)) ** 0.4 * (1 - 0.3 * imut / pi)
        (thr,), = driver([f"threshold {q!r} {e!r} {imut!r}"])
        assert thr == pytest.approx(want, rel=1e-14)
        a_c = 0.05
        for side, passes in ((1 + 1e-9, 1), (1 - 1e-9, 0)):
            a = thr * side * a_c / (1 - e)
            (ratio, got), = driver([f"passes {a!r} {e!r} {a_c!r} {q!r} {imut!r}"])
            assert got == passes and ratio == pytest.approx(thr * side, rel=1e-14)
    assert driver(["threshold 1 0 0"])[0][0] == pytest.approx(2.8 * 2 ** 0.4, rel=1e-15)
    # a retrograde child needs 30 % less room than a coplanar prograde one
    (pro,), (retro,) = driver(["threshold 0.5 0.2 0", f"threshold 0.5 0.2 {pi!r}"])
    assert retro / pro == pytest.approx(0.7, rel=1e-14)
    assert driver(["passes 1 1.5 0.05 1 0", "passes nan 0.5 0.05 1 0"])[0][1] == 0        # sqrt(1 - e) is NaN: no pass


def test_the_mutual_inclination_of_prograde_retrograde_and_tilted_children(driver):
    got = driver(["imut 0 0 2 0 0 0.5", "imut 0 0 2 0 0 -3", "imut 0 0 1 0 1 0", "imut 0 0 1 0 0 0", "imut 0 0 0 0 0 1",
                  f"imut 0 0 1 0 {float(np.sin(0.3))!r} {float(np.cos(0.3))!r}"])
    assert got[0] == [0.0] and got[1] == [np.pi] and got[2][0] == pytest.approx(np.pi / 2, rel=1e-15)
    assert got[3] == [0.0] and got[4] == [0.0] and got[5][0] == pytest.approx(0.3, rel=1e-14)


def test_the_perturbation_and_the_decision(driver):
    # Q = 0.5 x 1.5 = 0.75: 2 x 4 x 0.421875 / 3 = 1.125
    assert driver(["perturbation 4 0.5 0.5 3", "perturbation 0 0.5 0.5 3"]) == [[1.125], [0.0]]
    got = driver(["accepts -1 0.5 1", "accepts -1 1 1", "accepts -1 1.5 1", "accepts 0 0 1", "accepts 1 0 1", "accepts -1 1e300 inf",
                  "accepts -1 inf inf", "accepts nan 0 1", "accepts -1 nan 1", "accepts -1 0 0"])
    assert [g[0] for g in got] == [1, 1, 0, 0, 0, 1, 1, 0, 1, 1]


def test_the_record_sizes_offsets_and_the_empty_records(driver):
    assert driver(["layout", "empty"]) == [[128, 0, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 104, 16, 0, 4, 8, 40, 0, 16, 32],
                                          [-1, -1, -1, 0, 0, 0, 0, 0, -1, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 16]]


# ---- the reference on hand-worked cases -----------------------------------------------------------------------------------
def run(obj, capacity=8, **kw):
    P, V = href.place(obj, capacity, order=kw.pop("order", None))
    return href.hierarchy(P, V, kw.pop("n", len(obj[0])), **kw)


def test_an_empty_system_one_body_and_two_unbound_bodies():
    P, V = href.place(href.leaf(1.0), 4)
    empty = href.hierarchy(P, V, 0)
    assert [empty[k] for k in href.SYSTEM_FIELDS] == [0, 0, 0, 1, 0, 0, 0, 0, 0] and href.describe(empty) == ""
    assert (empty["parent"] == -1).all() and (empty["root"] == -1).all() and (empty["child"] == -1).all()
    one = href.hierarchy(P, V, 1)
    assert [one[k] for k in href.SYSTEM_FIELDS] == [0, 1, 0, 1, 1, 0, 0, 0, 0] and href.describe(one) == "0"
    assert one["root"].tolist() == [0, -1, -1, -1] and one["depth"].tolist() == [0, 0, 0, 0]
    P[1], V[1] = [3, 0, 0, 1], [0, 5, 0, 0]                     # v^2 / 2 = 12.5 against mu / r = 2 / 3
    two = href.hierarchy(P, V, 2)
    assert [two[k] for k in href.SYSTEM_FIELDS] == [0, 2, 1, 1, 2, 0, 0, 0, 0] and href.describe(two) == "0 1"


def test_coincident_bodies_are_no_pair():
    P, V = href.place(href.leaf(1.0), 4)
    P[1], V[1] = P[0], V[0]
    ref = href.hierarchy(P, V, 2)
    assert ref["nodes"] == 0 and ref["levels"] == 1 and ref["singles"] == 2 and href.describe(ref) == "0 1"


def test_a_binary_plus_a_far_single():
    P, V, (a, e, inc, energy, sep) = pref.known_binary(1.3)       # the binary is bodies 0 and 2
    assert href.describe(href.hierarchy(P[0], V[0], 3)) == "[[0 2] 1]"    # at 0.01 the single at 213 is bound: 5e-5 < 1.5 / 213
    V[0, 1, :3] = [0.0, 1.0, 0.0]
    ref = href.hierarchy(P[0], V[0], 3)
    assert href.describe(ref) == "[0 2] 1" and ref["nodes"] == 1 and ref["levels"] == 2 and ref["converged"] == 1
    assert [ref[k] for k in ("singles", "binaries", "triples", "higher", "unstable")] == [1, 1, 0, 0, 0]
    assert ref["child"][0].tolist() == [0, 2] and ref["slot"][0] == 0 and ref["leaves"][0] == 2 and ref["stable"][0] == 1
    assert ref["semi_major_axis"][0] == pytest.approx(a, rel=1e-6) and ref["eccentricity"][0] == pytest.approx(e, rel=1e-6)
    assert ref["parent"].tolist() == [3, -1, 3] and ref["root"].tolist() == [3, 1, 3] and ref["depth"].tolist() == [1, 0, 1]
    # the single at 213 with mass 0.5 against a binary of mass 1 with apocentre 1.6: 2 x (0.5 / 213^3) x 1.6^3
    d = np.linalg.norm(P[0, 1, :3].astype(np.float64) - href.merged(P[0, 0, 3], P[0, 0, :3], P[0, 2, 3], P[0, 2, :3]))
    assert ref["perturbation"][0] == pytest.approx(2 * 0.5 / d ** 3 * (a * (1 + e)) ** 3, rel=1e-5)


def test_a_designed_triple_is_stable_and_a_tight_one_is_not():
    wide, tight = run(href.designed_triple()), run(href.designed_triple(outer_a=0.1))
    for ref, stable in ((wide, 1), (tight, 0)):
        assert href.describe(ref) == "[[0 1] 2]" and ref["nodes"] == 2 and ref["levels"] == 2 and ref["converged"] == 1
        assert ref["child"][:2].tolist() == [[0, 1], [3, 2]] and ref["node_parent"][:2].tolist() == [4, -1]
        assert ref["level"][:2].tolist() == [1, 2] and ref["leaves"][:2].tolist() == [2, 3] and ref["stable"][:2].tolist() == [1, stable]
        assert [ref[k] for k in ("singles", "binaries", "triples", "higher", "unstable")] == [0, 0, 1, 0, 1 - stable]
        assert ref["parent"][:3].tolist() == [3, 3, 4] and ref["root"][:3].tolist() == [4, 4, 4] and ref["depth"][:3].tolist() == [2, 2, 1]
        assert ref["mass"][:2].tolist() == [1.5, 2.25] and ref["mutual_inclination"][1].tolist() == pytest.approx([0.2, 0.0], abs=1e-6)
    assert wide["semi_major_axis"][1] == pytest.approx(1.0, rel=1e-5) and tight["semi_major_axis"][1] == pytest.approx(0.1, rel=1e-5)
    # the threshold of the docstring: q = 0.75 / 1.5, e = 0.2
    thr = 2.8 * (1.5 * 1.2 / np.sqrt(0.8)) ** 0.4 * (1 - 0.3 * 0.2 / np.pi)
    assert 0.1 * 0.8 / 0.05 < thr < 1.0 * 0.8 / 0.05
    tilted = run(href.designed_triple(tilt=0.7))
    assert tilted["mutual_inclination"][1].tolist() == pytest.approx([0.7, 0.0], abs=1e-6)


def test_two_plus_two_numbers_its_nodes_in_creation_order():
    ref = run(href.designed_two_plus_two())
    assert href.describe(ref) == "[[0 1] [2 3]]" and ref["nodes"] == 3 and ref["levels"] == 2 and ref["higher"] == 1
    assert ref["child"][:3].tolist() == [[0, 1], [2, 3], [4, 5]] and ref["slot"][:3].tolist() == [0, 2, 0]
    assert ref["node_parent"][:3].tolist() == [6, 6, -1] and ref["leaves"][:3].tolist() == [2, 2, 4] and ref["stable"][2] == 1
    assert ref["depth"][:4].tolist() == [2, 2, 2, 2] and (ref["root"][:4] == 6).all()
    # the same bodies in another order: the slots follow, the lower slot's child first
    other = run(href.designed_two_plus_two(), order=[3, 0, 2, 1])
    assert href.describe(other) == "[[0 2] [1 3]]" and other["child"][:3].tolist() == [[0, 2], [1, 3], [4, 5]]


def test_a_tolerance_rejects_the_outer_orbit_of_a_triple_and_keeps_the_inner():
    obj = href.designed_triple()
    free = run(obj)
    # inner: 2 x (0.75 / 1^3-ish) x 0.065^3 / 1.5 is ~1e-4; outer has no perturber at all, so a fourth body far away gives it one
    P, V = href.place(obj, 8)
    P[3], V[3] = [6, 0, 0, 40.0], [0, 0, 30.0, 0]
    loose, strict = href.hierarchy(P, V, 4), href.hierarchy(P, V, 4, tidal_tolerance=0.1)
    assert href.describe(loose) == "[[0 1] 2] 3" and href.describe(strict) == "[0 1] 2 3"
    assert loose["perturbation"][1] > 0.1 > loose["perturbation"][0] > 0 and strict["nodes"] == 1 and strict["converged"] == 1
    assert strict["margins"]["d"] > 0.5 and free["perturbation"][1] == 0 and np.isinf(free["margins"]["d"])


def test_max_levels_one_on_a_triple_is_not_converged():
    ref = run(href.designed_triple(), max_levels=1)
    assert ref["nodes"] == 1 and ref["levels"] == 1 and ref["converged"] == 0 and href.describe(ref) == "[0 1] 2"
    nested = [run(href.designed_nested(), max_levels=k) for k in (1, 2, 3, 4)]
    assert [r["nodes"] for r in nested] == [1, 2, 3, 3] and [r["converged"] for r in nested] == [0, 0, 1, 1]
    assert href.describe(nested[2]) == "[[[0 1] 2] 3]" and nested[2]["depth"][:4].tolist() == [3, 3, 2, 1]


def test_tracers_bound_to_a_planet_stay_singles_and_are_counted_nowhere():
    P, V, counts, massive = href.massive_inputs()
    refs = [href.hierarchy(P[s], V[s], counts[s], massive=massive[s]) for s in range(len(counts))]
    assert [r["roots"] + r["nodes"] for r in refs] == massive
    for r, m in zip(refs, massive):
        assert (r["parent"][m:] == -1).all() and (r["depth"][m:] == 0).all()
        assert r["root"][m:counts[0]].tolist() == list(range(m, counts[0]))
        assert r["singles"] + r["binaries"] + r["triples"] + r["higher"] == r["roots"]
        assert (r["child"][:r["nodes"]] < counts[0] + r["nodes"]).all()
    assert refs[0]["levels"] == 0 and refs[1]["levels"] == 0 and refs[1]["singles"] == 1
    # a planet with a tracer bound to it: with one massive body the tracer is no leaf
    P2, V2 = href.place(href.join(href.leaf(1.0), href.leaf(1e-6), 0.05, 0.1, 1.0, href.EX, href.EY), 4)
    assert href.describe(href.hierarchy(P2, V2, 2)) == "[0 1]"
    alone = href.hierarchy(P2, V2, 2, massive=1)
    assert href.describe(alone) == "0" and alone["singles"] == 1 and alone["parent"][:2].tolist() == [-1, -1]
    assert alone["root"][:2].tolist() == [0, 1]


def test_describe_and_multiplicity_of_the_result_on_the_hand_cases():
    objs = [href.designed_triple(), href.designed_triple(outer_a=0.1), href.designed_two_plus_two(), href.designed_nested()]
    refs = [run(o) for o in objs]
    P, V, _ = pref.known_binary(1.3)
    Pk, Vk = np.full((8, 4), href.FILL, np.float32), np.full((8, 4), href.FILL, np.float32)
    Pk[:3], Vk[:3] = P[0], V[0]
    Vk[1, :3] = [0.0, 1.0, 0.0]
    refs += [href.hierarchy(Pk, Vk, 3), href.hierarchy(Pk, Vk, 0)]
    res = result_of(refs)
    want = ["[[0 1] 2]", "[[0 1] 2]", "[[0 1] [2 3]]", "[[[0 1] 2] 3]", "[0 2] 1", ""]
    assert [res.describe(s) for s in range(6)] == want == [href.describe(r) for r in refs]
    assert res.multiplicity().tolist() == [[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 0, 0]]
    assert res.roots_of(0) == [4] and res.roots_of(2) == [6] and res.roots_of(4) == [3, 1] and res.roots_of(5) == []
    assert res.unstable.tolist() == [0, 1, 0, 0, 0, 0] and res.converged.all() and res.converged.dtype == np.bool_
    assert res.stable.dtype == np.bool_ and res.child.shape == (6, 8, 2) and res.h.shape == (6, 8, 3)
    assert res.parent.shape == res.root.shape == res.depth.shape == (6, 8) and res.nodes.tolist() == [2, 2, 3, 3, 1, 0]
    assert res.node_parent[0, :2].tolist() == [4, -1] and res.levels.dtype == np.int32
    from n_body_problem_amd import batch
    none = batch.HierarchyResult(res.systems, None, None, res.counts)
    assert none.child is None and none.stable is None and none.parent is None and none.multiplicity().tolist() == res.multiplicity().tolist()
    with pytest.raises(ValueError, match="node records"):
        none.describe(0)


# ---- the inputs condition -------------------------------------------------------------------------------------------------
def test_the_inputs_condition():
    """Every input of the GPU suite keeps (a) >= 2e-5, (b) >= 1e-4, (c) >= 1e-5 and, where a tolerance is used, (d) >= 1e-4: a
    condition on the inputs, not a tolerance of the kernel.  The designed objects come back as designed, with a few chance
    pairs among them: several levels, and multiples of every kind."""
    seen, worst = 0, dict(a=np.inf, b=np.inf, c=np.inf, d=np.inf)

    def hold(tag, ref, tolerance=np.inf):
        nonlocal seen
        seen += 1
        for k, v in ref["margins"].items():
            worst[k] = min(worst[k], v)
        print(tag, {k: f"{v:.3g}" for k, v in ref["margins"].items()}, ref["levels"], "levels", ref["nodes"], "nodes")
        assert href.holds(ref, tolerance), (tag, ref["margins"])

    for capacity, tolerances in href.TOLERANCES.items():
        counts = href.CAPACITIES[capacity]
        for tolerance in tolerances:
            for s, (n, ref) in enumerate(zip(counts, href.reference(capacity, tolerance))):
                hold((capacity, tolerance, s, n), ref, tolerance)
                assert ref["converged"] == 1
                if n >= 63 and np.isinf(tolerance):
                    assert 4 <= ref["levels"] <= 8, (capacity, s, ref["levels"])
                    assert min(ref[k] for k in ("singles", "binaries", "triples", "higher", "unstable")) >= 3
    for obj in (href.designed_triple(), href.designed_triple(outer_a=0.1), href.designed_triple(tilt=0.7), href.designed_two_plus_two(),
                href.designed_nested()):
        hold(("designed",), run(obj, capacity=64, max_levels=16))
    P, V, counts, massive = href.massive_inputs()
    for s, n in enumerate(counts):
        hold(("massive", s), href.hierarchy(P[s], V[s], n, massive=massive[s]))
    P, V = href.invariance_inputs(130)
    hold(("invariance",), href.hierarchy(P, V, href.INVARIANCE_BODIES))
    print(f"{seen} systems, smallest margins {worst}")
    assert seen == 6 * 4 + 6 + 2 * 2 + 5 + 4 + 1
    assert href.MARGINS == dict(a=2e-5, b=1e-4, c=1e-5, d=1e-4)
