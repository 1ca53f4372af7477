"""CPU-only: the nearest-neighbour lists of batched ensembles (nbody_batch_neighbours, include/nbody_batch_neighbours.h).  The
header is self-contained C99, included by nbody.h after the span header, and declares its one entry point alone; it is exported,
bound and listed apart; the arithmetic without a GPU (csrc/nbody_batch_neighbours_math.h), built into a stand-alone driver with
g++ -- once more with the address and undefined-behaviour sanitizers -- gives the reference's lists, counts and means on every
input of the GPU suite exactly, and on adversarial sequences; and on every input the fp32 chain gives the integer r2, which is
the premise of all the exact comparisons."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_neighbours_ref as nref
import hermite_span_ref as sref
from conftest import ROOT

NAMES = ["nbody_batch_neighbours"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
INF_BITS = int(np.float32(np.inf).view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_span_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_neighbours.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_neighbours.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_span.h"') < nbody_h.index('#include "nbody_batch_neighbours.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_40_and_8_bytes(tmp_path):
    src = tmp_path / "neighbours.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char system_is_40_bytes[sizeof(nbody_batch_neighbour_system) == 40 ? 1 : -1];
typedef char body_is_8_bytes[sizeof(nbody_batch_neighbour_body) == 8 ? 1 : -1];
typedef char bodies_at_0[offsetof(nbody_batch_neighbour_system, bodies) == 0 ? 1 : -1];
typedef char sources_at_4[offsetof(nbody_batch_neighbour_system, sources) == 4 ? 1 : -1];
typedef char listed_at_8[offsetof(nbody_batch_neighbour_system, listed) == 8 ? 1 : -1];
typedef char complete_at_12[offsetof(nbody_batch_neighbour_system, complete) == 12 ? 1 : -1];
typedef char mutual_at_16[offsetof(nbody_batch_neighbour_system, mutual) == 16 ? 1 : -1];
typedef char reserved_at_20[offsetof(nbody_batch_neighbour_system, reserved) == 20 ? 1 : -1];
typedef char mean_nearest_at_24[offsetof(nbody_batch_neighbour_system, mean_nearest) == 24 ? 1 : -1];
typedef char mean_kth_at_32[offsetof(nbody_batch_neighbour_system, mean_kth) == 32 ? 1 : -1];
typedef char found_at_0[offsetof(nbody_batch_neighbour_body, found) == 0 ? 1 : -1];
typedef char within_at_4[offsetof(nbody_batch_neighbour_body, within) == 4 ? 1 : -1];
typedef char limit[NBODY_BATCH_NEIGHBOURS_MAX == 8 ? 1 : -1];
int main(void) {
    nbody_batch_neighbour_system s;
    return (nbody_batch_neighbours(0, 0, 6, 0, 0, &s, 0, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_neighbours.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_span.h", "The rows are all i < min(counts[s], max_bodies)",
                   "whatever the massive counts", "this is geometry", "Removed tracers and merged bodies are seen as the state holds them",
                   "every body j < count when sources is NULL", "n_systems x max_bodies bytes", "like subset of nbody_batch_span",
                   "initial of nbody_batch_members", "Rows are never restricted", "the nearest planets of every planetesimal",
                   "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))", "every fmaf one fused operation", "nothing else contracted",
                   "Column j is a candidate of row i iff j != i, j is a source, and r2 < +inf",
                   "A coincident body (r2 == 0) is a neighbour", "this differs from nbody_batch_structure",
                   "A NaN or infinite r2 is not a candidate", "ordered by r2, ties go to the lower j", "The order is total",
                   "does not depend on the schedule, the slot, n_systems or max_bodies", "1 <= k <= NBODY_BATCH_NEIGHBOURS_MAX (8)",
                   "found(i) = min(k, candidates)", "Slots from found on hold index -1 and r2 +inf", "found = 0 and within = 0",
                   "both or neither", "the number of candidates with r2 <= b2", "one fp32 product",
                   "the predicate and the product of nbody_batch_groups", "within is then 0 for every row",
                   "bodies is the number of rows", "listed the rows with found >= 1", "complete the rows with found == k",
                   "whose nearest j has found(j) >= 1 and whose own nearest is i", "reserved is 0",
                   "the fp64 sum, in ascending i, of sqrt((double)r2[0]) over the listed rows", "divided by listed in one division",
                   "0 when listed is 0", "the same over r2[k - 1] of the complete rows", "{found, within}", "NULL skips that copy",
                   "the same bits either way", "synchronous", "forgets nothing", "bit for bit", "allocated on first use",
                   "grown when a later call asks for a larger k", "freed in nbody_batch_destroy",
                   "the same bits in any slot, n_systems and max_bodies", "names the function", "a NULL handle",
                   "NULL d_positions_xyzm or systems_out", "k outside 1 ... 8", "exactly one of index_out and r2_out NULL",
                   "a radius that is negative or NaN", "refused before any device work",
                   # what the three headers before it left out, in their words
                   'the "neighbour lists" of nbody_batch_pairs.h', '"the neighbours\' indices" of nbody_batch_structure.h',
                   'the "k-nearest-neighbour lists" of nbody_batch_span.h',
                   "Out of scope", "k > 8", "neighbours in velocity or phase space", "softened distances", "lists across systems",
                   "device-side outputs", "a shorter-list instantiation for small k", "changing the state"):
        assert phrase in text, phrase
    # the three headers that name the gap are as they were
    for header, phrase in (("nbody_batch_pairs.h", "neighbour lists"), ("nbody_batch_structure.h", "k > 8, the neighbours' indices"),
                           ("nbody_batch_span.h", "k-nearest-neighbour lists")):
        other = " ".join(open(os.path.join(INCLUDE, header)).read().replace(" *", " ").split())
        assert phrase in other and "nbody_batch_neighbours" not in other, header


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.neighbours_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.span_names()) | set(_lib.groups_names()) |
                             set(_lib.gravity_names()) | set(_lib.members_names()) | set(_lib.structure_names()) |
                             set(_lib.pairs_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 9, name
    assert ctypes.sizeof(_lib.BatchNeighbourSystem) == 40 and ctypes.sizeof(_lib.BatchNeighbourBody) == 8
    assert [f[0] for f in _lib.BatchNeighbourSystem._fields_] == ["bodies", "sources", "listed", "complete", "mutual", "reserved",
                                                                  "mean_nearest", "mean_kth"]
    assert [f[0] for f in _lib.BatchNeighbourBody._fields_] == ["found", "within"]
    assert _lib.BatchNeighbourSystem.mean_nearest.offset == 24 and _lib.BatchNeighbourBody.within.offset == 4
    assert _lib.BATCH_NEIGHBOURS_MAX == nref.MAX == 8
    assert batch.NEIGHBOUR_SYSTEM_DTYPE.names == tuple(f[0] for f in _lib.BatchNeighbourSystem._fields_)
    assert {"NeighbourResult", "NEIGHBOUR_SYSTEM_DTYPE", "NEIGHBOUR_BODY_DTYPE"} <= set(batch.__all__)
    assert nb.NeighbourResult is batch.NeighbourResult and "NeighbourResult" in nb.__all__ and batch.NeighbourResult.__doc__
    assert batch.BatchedSystem.neighbours.__doc__
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_neighbours") == 1 and exports[exports.index("nbody_batch_neighbours") - 1].startswith("#")
    hpp = open(os.path.join(INCLUDE, "nbody.hpp")).read()
    assert "std::vector<nbody_batch_neighbour_system> neighbours(" in hpp and "nbody_batch_neighbours(b_, dPositions, k," in hpp


def test_the_abi_stays_at_version_5_and_the_errors_of_the_header_are_refused_without_a_device(lib):
    """The error list of the header, as far as it can be walked without a handle: a NULL handle is refused first, with the
    function's name.  (The other cases need a handle; test_batch_neighbours_gpu.py walks them.)"""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchNeighbourSystem * 1)()
    assert lib.nbody_batch_neighbours(None, None, 6, None, None, out, None, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_neighbours: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_neighbours("):]
    body = body[:body.index("\n}\n")]
    for message in ("nbody_batch_neighbours: batch is NULL", "nbody_batch_neighbours: NULL argument",
                    "nbody_batch_neighbours: k must be 1 ... 8",
                    "nbody_batch_neighbours: index_out and r2_out must be given both or neither",
                    "nbody_batch_neighbours: the radius of system "):
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
    assert "batch_analysis(b, a)" in body and body.index("must be >= 0") < body.index("batch_analysis(b, a)")


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_and_reuses_r2_and_friends():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_neighbours_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_neighbours.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_neighbours_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and '#include "nbody_batch_groups_math.h"' in text
    assert "groups_r2(" in text and "groups_friends(" in text and "fmaf" not in text       # reused, not restated
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_neighbours_kernel("):source.index("hipError_t launch_batch_neighbours(")]
    for call in ("neighbours_clear(", "neighbours_measure(", "neighbours_wanted(", "neighbours_insert(", "neighbours_found(", "neighbours_kth(", "neighbours_mutual(",
                 "neighbours_term(", "neighbours_mean(", "neighbours_empty_body(", "neighbours_no_r2(", "readfirstlane("):
        assert call in kernel, call
    assert "fmaf" not in kernel and "sqrt" not in kernel                                    # the kernel states none of them again
    step = text[text.index("inline void neighbours_step("):]
    step = step[:step.index("\n}\n")]
    for call in ("neighbours_measure(", "neighbours_wanted(", "neighbours_insert("):     # the driver's step is the kernel's three parts
        assert call in step, call
    # between the spanning trees and the diagnostics, inside the anonymous namespace: no existing pair of markers is split
    assert source.index("hipError_t launch_batch_span(") < source.index("void batch_neighbours_kernel(") \
        < source.index("hipError_t launch_batch_neighbours(") < source.index("void batch_diag_kernel(") \
        < source.index("}  // namespace\n")
    for sibling in ("pairs", "structure", "members", "gravity", "hierarchy", "groups", "span"):
        cut = source[source.index(f"void batch_{sibling}_kernel("):source.index(f"hipError_t launch_batch_{sibling}(")]
        assert "neighbours" not in cut, sibling


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_neighbours_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("neighbours"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("neighbours_checked"),
                        ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(driver, pos, n, k, radius=None, sources=None):
    sel = np.ones(n, np.uint8) if sources is None else (np.asarray(sources)[:n] != 0).astype(np.uint8)
    lines = [f"system {n} {k} {'none' if radius is None else repr(float(radius))}"]
    lines += [f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(s)}" for p, s in zip(np.asarray(pos)[:n], sel)]
    out = driver("\n".join(lines) + "\n")
    head = out[0].split()
    got = dict(zip(("bodies", "sources", "listed", "complete", "mutual", "reserved"), (int(w) for w in head[:6])))
    got["mean_nearest"], got["mean_kth"] = float(head[6]), float(head[7])
    rows = np.array([[int(w) for w in line.split()] for line in out[1:1 + n]], dtype=np.int64).reshape(n, 2 + 2 * k)
    got["found"], got["within"] = rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32)
    got["index"] = rows[:, 2:2 + k].astype(np.int32)
    got["r2"] = rows[:, 2 + k:].astype(np.uint32).view(np.float32)
    return got


def same(got, ref):
    for name in ("bodies", "sources", "listed", "complete", "mutual"):
        assert got[name] == ref[name], (name, got[name], ref[name])
    assert got["reserved"] == 0
    assert np.array_equal(got["index"], ref["index"]), np.argwhere(got["index"] != ref["index"])[:8]
    assert np.array_equal(got["r2"].view(np.uint32), ref["r2"].view(np.uint32))
    assert np.array_equal(got["found"], ref["found"]) and np.array_equal(got["within"], ref["within"])
    for name in ("mean_nearest", "mean_kth"):
        assert np.float64(got[name]).view(np.uint64) == np.float64(ref[name]).view(np.uint64), (name, got[name], ref[name])


def test_the_layout_the_empty_values_and_the_constants(driver):
    assert [int(w) for w in driver("layout\n")[0].split()] == [40, 0, 4, 8, 12, 16, 20, 24, 32, 8, 0, 4]
    assert driver("empty\n")[0].split() == ["-1", str(INF_BITS), "0", "0", "8", "-1"]


@pytest.mark.parametrize("capacity", [64, 128, 320])
def test_the_driver_gives_the_references_lists_counts_and_means_exactly(driver, capacity):
    P, counts = nref.gpu_inputs(capacity)
    radii = nref.gpu_radii(capacity)
    for k in nref.KS:
        refs = nref.gpu_reference(capacity, k)
        for s, n in enumerate(counts):
            got = drive(driver, P[s], n, k, radius=radii[s])
            print(f"capacity {capacity} k {k} system {s} (n = {n}): listed {got['listed']}, complete {got['complete']}, mutual "
                  f"{got['mutual']}, means {got['mean_nearest']!r} {got['mean_kth']!r}, within up to {got['within'].max(initial=0)}")
            same(got, refs[s])
            assert got["mutual"] % 2 == 0
    assert sum(int(nref.gpu_reference(capacity, 6)[s]["within"].sum()) for s in range(len(counts))) > 0
    # without a radius nothing is within, and nothing else moves
    s = 0
    plain = drive(driver, P[s], counts[s], 6)
    assert not plain["within"].any()
    same(dict(plain, within=nref.gpu_reference(capacity, 6)[s]["within"]), nref.gpu_reference(capacity, 6)[s])


def test_the_driver_at_4096_bodies(driver):
    P, counts = nref.gpu_inputs(4096)
    radii = nref.gpu_radii(4096)
    refs = nref.gpu_reference(4096, 8)
    for s, n in enumerate(counts):
        same(drive(driver, P[s], n, 8, radius=radii[s]), refs[s])


def test_source_masks_on_the_driver(driver):
    pos, n, masks = nref.source_inputs(320)
    for s, mask in enumerate(masks):
        for k in (1, 6):
            ref = nref.reference(pos, n, k, radius=3.0, sources=mask)
            got = drive(driver, pos, n, k, radius=3.0, sources=mask)
            same(got, ref)
            listed = got["index"][got["index"] >= 0]
            assert mask[listed].all() and not (got["index"] == np.arange(n)[:, None]).any()
    assert drive(driver, pos, n, 6, sources=masks[0])["listed"] == 0
    single = drive(driver, pos, n, 6, sources=masks[2])
    assert single["listed"] == n - 1 and single["found"][n // 2] == 0 and single["mutual"] == 0
    same(drive(driver, pos, n, 6, radius=3.0, sources=masks[1]), nref.reference(pos, n, 6, radius=3.0))


def rows_of(xyz):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def test_adversarial_sequences_on_the_driver(driver):
    """What row 0 meets, in ascending j: all distances equal, descending, ascending, fewer than k, zeros, a NaN coordinate."""
    # all equal: twelve bodies at distance 5 of row 0 (permutations and signs of (3, 4, 0)); ties go to the lower j
    ring = [(3, 4, 0), (4, 3, 0), (-3, 4, 0), (0, 3, 4), (0, -4, 3), (3, 0, -4), (-4, 0, 3), (0, 4, -3), (4, 0, 3), (-3, -4, 0),
            (0, -3, -4), (-4, -3, 0)]
    pos = rows_of([(0, 0, 0)] + ring)
    got = drive(driver, pos, 13, 8, radius=5.0)
    assert got["index"][0].tolist() == list(range(1, 9)) and (got["r2"][0] == 25.0).all() and got["within"][0] == 12
    same(got, nref.reference(pos, 13, 8, radius=5.0))
    # descending and ascending distances from row 0
    for order in (np.arange(20, 0, -1), np.arange(1, 21)):
        pos = rows_of([(0, 0, 0)] + [(int(d), 0, 0) for d in order])
        for k in (1, 3, 8):
            got = drive(driver, pos, 21, k, radius=4.0)
            want = sorted(range(1, 21), key=lambda j: order[j - 1])[:k]
            assert got["index"][0].tolist() == want and got["r2"][0].tolist() == [float(d * d) for d in range(1, k + 1)]
            assert got["within"][0] == 4
            same(got, nref.reference(pos, 21, k, radius=4.0))
    # fewer than k: the slots from found on hold -1 and +inf
    pos = rows_of([(0, 0, 0), (2, 0, 0), (1, 0, 0)])
    got = drive(driver, pos, 3, 6)
    assert got["index"][0].tolist() == [2, 1, -1, -1, -1, -1] and got["found"].tolist() == [2, 2, 2]
    assert got["r2"][0].view(np.uint32).tolist()[2:] == [INF_BITS] * 4 and got["complete"] == 0 and got["mean_kth"] == 0.0
    same(got, nref.reference(pos, 3, 6))
    # zeros: coincident bodies are neighbours, in ascending j, and never the row itself
    pos = rows_of([(7, 7, 7)] * 5 + [(8, 7, 7)])
    got = drive(driver, pos, 6, 8, radius=0.0)
    assert got["index"][2].tolist() == [0, 1, 3, 4, 5, -1, -1, -1] and got["r2"][2].tolist()[:5] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert got["within"].tolist() == [4, 4, 4, 4, 4, 0] and got["mean_nearest"] == 1.0 / 6.0
    same(got, nref.reference(pos, 6, 8, radius=0.0))
    # a NaN coordinate: that body is nobody's neighbour and has none; an infinite one the same
    for bad in (np.nan, np.inf):
        pos = rows_of([(0, 0, 0), (bad, 0, 0), (3, 0, 0), (1, 0, 0)])
        got = drive(driver, pos, 4, 2, radius=10.0)
        assert got["index"].tolist() == [[3, 2], [-1, -1], [3, 0], [0, 2]] and got["found"].tolist() == [2, 0, 2, 2]
        assert got["within"].tolist() == [2, 0, 2, 2] and got["listed"] == 3 and got["complete"] == 3 and got["mutual"] == 2
        assert got["r2"][1].view(np.uint32).tolist() == [INF_BITS] * 2
        assert got["mean_nearest"] == (1.0 + 2.0 + 1.0) / 3.0 and got["mean_kth"] == (3.0 + 3.0 + 2.0) / 3.0


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    P, counts = nref.gpu_inputs(128)
    radii = nref.gpu_radii(128)
    for k in (1, 8):
        refs = nref.gpu_reference(128, k)
        for s, n in enumerate(counts):
            same(drive(checked_driver, P[s], n, k, radius=radii[s]), refs[s])
    pos, n, masks = nref.source_inputs(64)
    for mask in masks:
        same(drive(checked_driver, pos, n, 6, radius=2.0, sources=mask), nref.reference(pos, n, 6, radius=2.0, sources=mask))
    pos = rows_of([(0, 0, 0), (np.nan, 0, 0), (3, 0, 0), (1, 0, 0)])
    assert drive(checked_driver, pos, 4, 8)["found"].tolist() == [2, 0, 2, 2]
    assert checked_driver("layout\nempty\nsystem 0 8 none\n")[2].split()[:6] == ["0"] * 6


# ---- the premise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", nref.CAPACITIES)
def test_the_fp32_chain_gives_the_integer_r2_on_every_input(driver, capacity):
    """On grid inputs every operation of the chain is exact, so the fp32 operations one by one (numpy has no fused multiply-add,
    and needs none where nothing rounds) give the r2 of the fp64 reference, whose Gram form keeps to integer numbers of squared
    grid units below 2^24; and the chain itself, with its fused operations, as the driver runs it through the math header, gives
    that r2 for every pair it lists."""
    P, counts = nref.gpu_inputs(capacity)
    pos, n, _ = nref.source_inputs(capacity)
    for p, m in [(P[s], c) for s, c in enumerate(counts)] + [(pos, n)]:
        if m == 0:
            continue
        x = np.asarray(p[:m, :3], dtype=np.float32)
        rows = np.arange(0, m, max(m // 64, 1))
        d = x[None, :, :] - x[rows][:, None, :]
        assert d.dtype == np.float32
        r2 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
        exact = sref.r2_exact(x.astype(np.float64), rows)
        assert r2.dtype == np.float32 and np.array_equal(r2.astype(np.float64), exact)
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)                  # it fits fp32's 24 bits
        assert np.array_equal(nref.r2_float(p, m, rows), r2)
        got = drive(driver, p, m, 8)
        listed = got["index"][rows] >= 0
        pairs = np.take_along_axis(exact, np.where(listed, got["index"][rows], 0), axis=1)
        assert np.array_equal(got["r2"][rows][listed].astype(np.float64), pairs[listed])
