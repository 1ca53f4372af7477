"""CPU-only: the spanning trees of batched ensembles (nbody_batch_span, include/nbody_batch_span.h).  The header is
self-contained C99, included by nbody.h after the groups header, and declares its one entry point alone; it is exported, bound
and listed apart; the arithmetic without a GPU (csrc/nbody_batch_span_math.h), built into a stand-alone driver with g++ -- once
more with the address and undefined-behaviour sanitizers -- gives Prim's tree and the reference's sums on every input of the GPU
suite exactly; the sort's network sorts adversarial key sets; and on every input the fp32 chain gives the integer r2, which is
the premise of all the exact comparisons."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_span_ref as sref
from conftest import ROOT

NAMES = ["nbody_batch_span"]
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
def test_the_header_is_included_by_nbody_h_after_groups_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_span.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_span.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_groups.h"') < nbody_h.index('#include "nbody_batch_span.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_40_16_and_8_bytes(tmp_path):
    src = tmp_path / "span.c"
    src.write_text(r'''
#include "nbody.h"
#include <stddef.h>
typedef char system_is_40_bytes[sizeof(nbody_batch_span_system) == 40 ? 1 : -1];
typedef char edge_is_16_bytes[sizeof(nbody_batch_span_edge) == 16 ? 1 : -1];
typedef char body_is_8_bytes[sizeof(nbody_batch_span_body) == 8 ? 1 : -1];
typedef char edges_at_0[offsetof(nbody_batch_span_system, edges) == 0 ? 1 : -1];
typedef char selected_at_4[offsetof(nbody_batch_span_system, selected) == 4 ? 1 : -1];
typedef char rounds_at_8[offsetof(nbody_batch_span_system, rounds) == 8 ? 1 : -1];
typedef char reserved_at_12[offsetof(nbody_batch_span_system, reserved) == 12 ? 1 : -1];
typedef char total_length_at_16[offsetof(nbody_batch_span_system, total_length) == 16 ? 1 : -1];
typedef char longest_at_24[offsetof(nbody_batch_span_system, longest) == 24 ? 1 : -1];
typedef char mean_separation_at_32[offsetof(nbody_batch_span_system, mean_separation) == 32 ? 1 : -1];
typedef char i_at_0[offsetof(nbody_batch_span_edge, i) == 0 ? 1 : -1];
typedef char j_at_4[offsetof(nbody_batch_span_edge, j) == 4 ? 1 : -1];
typedef char r2_at_8[offsetof(nbody_batch_span_edge, r2) == 8 ? 1 : -1];
typedef char edge_reserved_at_12[offsetof(nbody_batch_span_edge, reserved) == 12 ? 1 : -1];
typedef char degree_at_0[offsetof(nbody_batch_span_body, degree) == 0 ? 1 : -1];
typedef char nearest_at_4[offsetof(nbody_batch_span_body, nearest) == 4 ? 1 : -1];
typedef char limit[NBODY_BATCH_SPAN_MAX_ROUNDS == 13 ? 1 : -1];
int main(void) {
    nbody_batch_span_system s;
    return (nbody_batch_span(0, 0, 0, 0, &s, 0, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    text = " ".join(open(os.path.join(INCLUDE, "nbody_batch_span.h")).read().replace(" *", " ").split())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_groups.h", "The rows are all i < counts[s]",
                   "whatever the massive counts", "this is geometry", "A body is selected when subset is NULL or",
                   "n_systems x max_bodies bytes", "like initial of nbody_batch_members", "The tree spans the selected bodies",
                   "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))", "every fmaf one fused operation", "bit-symmetric in i and j and never -0",
                   "K = (bits(r2) << 24) | (i << 12) | j", "its bits order as its value does",
                   "ties in length go to the lower i, then to the lower j", "K is a strict total order",
                   "the minimum spanning tree is unique", "the result is that tree",
                   "does not depend on the algorithm or the schedule that found it", "A non-finite coordinate still has integer keys",
                   "the launch stays bounded and deterministic", "the tree then has no meaning", "all reads before any write",
                   "Each component takes the minimum K over the edges with exactly one end in it",
                   "records the edge and hooks under o when o's minimum is a different edge",
                   "does the same when o's minimum is the same edge and c > o",
                   "does nothing when o's minimum is the same edge and c < o", "repeated until a pass changes nothing",
                   "rounds is the number of rounds run until one component is left", "at most 12 for 4096 bodies",
                   "NBODY_BATCH_SPAN_MAX_ROUNDS (13) bounds the loop", "Every component is absorbed exactly once",
                   "edges is selected - 1, or 0 for selected <= 1", "the fp64 sum of sqrt((double)r2) over the edges in ascending K",
                   "longest is the last of those terms", "slot e holds the e-th edge in ascending K, with i < j",
                   "slots from edges on hold {-1, -1, 0, 0}", "degree is the number of tree edges at the body",
                   "the first round's row result and always a tree neighbour", "a lone selected body has {0, -1}",
                   "NULL skips that copy", "the same bits either way", "(double)sqrtf(r2_ij) over the selected j != i in ascending j",
                   "correctly rounded fp32 square root", "summed in ascending i in fp64", "selected (selected - 1), one fp64 division",
                   "0 with separations = 0 or selected < 2", "runs only when asked for", "synchronous", "forgets nothing",
                   "bit for bit", "allocated on first use and freed in nbody_batch_destroy",
                   "the same bits in any slot, n_systems and max_bodies", "names the function", "a NULL handle",
                   "NULL d_positions_xyzm or systems_out", "separations other than 0 or 1", "refused before any device work",
                   "Out of scope", "weighted or projected (2-D) trees", "trees across systems", "k-nearest-neighbour lists",
                   "changing the state"):
        assert phrase in text, phrase
    # the groups header, which this one follows, is as it was
    assert "nbody_batch_span" not in open(os.path.join(INCLUDE, "nbody_batch_groups.h")).read()


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib
    assert _lib.span_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.groups_names()) | set(_lib.gravity_names()) |
                             set(_lib.members_names()) | set(_lib.pairs_names()))
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert ctypes.sizeof(_lib.BatchSpanSystem) == 40 and ctypes.sizeof(_lib.BatchSpanEdge) == 16
    assert ctypes.sizeof(_lib.BatchSpanBody) == 8
    assert [f[0] for f in _lib.BatchSpanSystem._fields_] == ["edges", "selected", "rounds", "reserved", "total_length", "longest",
                                                             "mean_separation"]
    assert [f[0] for f in _lib.BatchSpanEdge._fields_] == ["i", "j", "r2", "reserved"]
    assert [f[0] for f in _lib.BatchSpanBody._fields_] == ["degree", "nearest"]
    assert _lib.BatchSpanSystem.total_length.offset == 16 and _lib.BatchSpanEdge.r2.offset == 8
    assert _lib.BATCH_SPAN_MAX_ROUNDS == sref.MAX_ROUNDS == 13


def test_the_abi_stays_at_version_5_and_the_errors_of_the_header_are_refused_without_a_device(lib):
    """The error list of the header, as far as it can be walked without a handle: a NULL handle is refused first, with the
    function's name.  (The other cases need a handle; test_batch_span_gpu.py walks them.)"""
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchSpanSystem * 1)()
    assert lib.nbody_batch_span(None, None, None, 0, out, None, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_span: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_span("):]
    body = body[:body.index("\n}\n")]
    for message in ("nbody_batch_span: batch is NULL", "nbody_batch_span: NULL argument",
                    "nbody_batch_span: separations must be 0 or 1"):
        assert message in body and body.index(message) < body.index("hipSetDevice"), message


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_and_reuses_r2():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_span_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_span.h" for h in build.HEADERS)
    text = open(os.path.join(CSRC, "nbody_batch_span_math.h")).read()
    assert "hip/" not in text and "NBODY_HD inline" in text and '#include "nbody_batch_groups_math.h"' in text
    assert "groups_r2(" in text and "fmaf" not in text.replace("fmaf(dz", "")       # the chain is reused, not restated
    kernel = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = kernel[kernel.index("void batch_span_kernel("):kernel.index("hipError_t launch_batch_span(")]
    for call in ("span_step(", "span_row_key(", "span_other(", "span_hooks(", "span_compress(", "span_exchange(", "span_edge(",
                 "span_length(", "span_separation(", "span_mean_separation(", "block_any(", "atomicMin(&key["):
        assert call in kernel, call


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_span_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("span"), [])


@pytest.fixture(scope="module")
def checked_driver(tmp_path_factory):
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    return build_driver(tmp_path_factory.mktemp("span_checked"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def drive(driver, pos, n, subset=None, separations=1):
    sel = np.ones(n, np.uint8) if subset is None else (np.asarray(subset)[:n] != 0).astype(np.uint8)
    lines = [f"system {n} {separations}"]
    lines += [f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(s)}" for p, s in zip(np.asarray(pos)[:n], sel)]
    out = driver("\n".join(lines) + "\n")
    head = out[0].split()
    got = {"edges": int(head[0]), "selected": int(head[1]), "rounds": int(head[2]), "reserved": int(head[3]),
           "total_length": float(head[4]), "longest": float(head[5]), "mean_separation": float(head[6])}
    E = got["edges"]
    rows = np.array([[int(w) for w in line.split()] for line in out[1:1 + E]], dtype=np.int64).reshape(E, 3)
    got["i"], got["j"] = rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32)
    got["r2"] = rows[:, 2].astype(np.uint32).view(np.float32)
    got["degree"] = np.array(out[1 + E].split(), dtype=np.int32)
    got["nearest"] = np.array(out[2 + E].split(), dtype=np.int32)
    return got


def same(got, ref, n, separations=1):
    for name in ("edges", "selected", "rounds"):
        assert got[name] == ref[name], (name, got[name], ref[name])
    assert got["reserved"] == 0
    assert np.array_equal(got["i"], ref["i"]) and np.array_equal(got["j"], ref["j"])
    assert np.array_equal(got["r2"].view(np.uint32), ref["r2"].view(np.uint32))
    for name in ("total_length", "longest"):
        assert np.float64(got[name]).view(np.uint64) == np.float64(ref[name]).view(np.uint64), (name, got[name], ref[name])
    want = ref["mean_separation"] if separations else 0.0
    assert np.float64(got["mean_separation"]).view(np.uint64) == np.float64(want).view(np.uint64)
    assert np.array_equal(got["degree"], ref["degree"][:n]) and np.array_equal(got["nearest"], ref["nearest"][:n])


def test_the_layout_the_empty_records_and_the_constants(driver):
    assert [int(w) for w in driver("layout\n")[0].split()] == [40, 0, 4, 8, 12, 16, 24, 32, 16, 0, 4, 8, 12, 8, 0, 4]
    assert driver("empty\n")[0].split() == ["-1", "-1", "0", "0", "0", "-1", "0", "0", "0", "0", "0", "13", "12",
                                            str(2 ** 64 - 1)]


@pytest.mark.parametrize("capacity", [64, 128, 320])
def test_the_driver_gives_prims_tree_and_the_references_sums_exactly(driver, capacity):
    P, counts = sref.gpu_inputs(capacity)
    refs = sref.gpu_reference(capacity)
    for s, n in enumerate(counts):
        got = drive(driver, P[s], n)
        print(f"capacity {capacity} system {s} (n = {n}): {got['edges']} edges in {got['rounds']} rounds, length "
              f"{got['total_length']!r}, mean separation {got['mean_separation']!r}")
        same(got, refs[s], n)
        assert sref.is_spanning_tree(got["i"], got["j"], range(n))
        same(drive(driver, P[s], n, separations=0), refs[s], n, separations=0)


def test_the_driver_at_4096_bodies(driver):
    P, counts = sref.gpu_inputs(4096)
    refs = sref.gpu_reference(4096)
    for s, n in enumerate(counts):
        got = drive(driver, P[s], n)
        print(f"system {s} (n = {n}): {got['edges']} edges in {got['rounds']} rounds")
        same(got, refs[s], n)
    assert max(r["rounds"] for r in refs) <= 12


def test_the_rounds_of_the_lattice_the_chain_and_the_spheres():
    """The permuted 4 x 4 x 4 lattice takes 3 rounds; every component is absorbed exactly once (reference() asserts it); the
    rounds at least halve the components, so ceil(log2 n) bounds them."""
    assert sref.reference(sref.lattice(), 64)["rounds"] == 3
    for capacity in (64, 128, 320):
        P, counts = sref.gpu_inputs(capacity)
        for ref, n in zip(sref.gpu_reference(capacity), counts):
            assert ref["rounds"] <= max(int(np.ceil(np.log2(max(n, 1)))), 0), (capacity, n, ref["rounds"])
            assert (ref["rounds"] == 0) == (n < 2)


def test_subsets_on_the_driver(driver):
    pos, n, masks = sref.subset_inputs(320)
    for s, mask in enumerate(masks):
        ref = sref.reference(pos, n, mask)
        got = drive(driver, pos, n, mask)
        same(got, ref, n)
        assert got["selected"] == int(mask[:n].sum()) and sref.is_spanning_tree(got["i"], got["j"], np.flatnonzero(mask[:n]))
        outside = np.flatnonzero(mask[:n] == 0)
        assert not got["degree"][outside].any() and (got["nearest"][outside] == -1).all()
    assert np.array_equal(drive(driver, pos, n, masks[0])["i"], drive(driver, pos, n)["i"])


def test_the_driver_is_clean_under_the_address_and_undefined_behaviour_sanitizers(checked_driver):
    P, counts = sref.gpu_inputs(128)
    refs = sref.gpu_reference(128)
    for s, n in enumerate(counts):
        same(drive(checked_driver, P[s], n), refs[s], n)
    pos, n, masks = sref.subset_inputs(64)
    for mask in masks:
        same(drive(checked_driver, pos, n, mask), sref.reference(pos, n, mask), n)
    keys = np.random.default_rng(5).integers(0, 2 ** 56, 300, dtype=np.uint64)
    out = checked_driver(f"sort {len(keys)}\n" + " ".join(str(int(k)) for k in keys) + "\n")
    assert [int(w) for w in out[0].split()] == sorted(int(k) for k in keys)


# ---- the sort ------------------------------------------------------------------------------------------------------------
def test_the_network_sorts_adversarial_key_sets(driver):
    rng = np.random.default_rng(9)
    top = 2 ** 56 - 1
    cases = [[], [5], [2, 1], list(range(64)), list(range(64, 0, -1)), list(range(1, 130)), list(range(129, 0, -1)),
             [top - k for k in range(320)], [0] + [top - k for k in range(4094)],                    # next to the padding
             list(range(0, 4096, 2)) + list(range(4095, 0, -2)),                                   # a mountain
             [int(k) for k in rng.integers(0, 2 ** 56, 4096, dtype=np.uint64)],
             [int(k) << 24 | 5 << 12 | 7 for k in rng.integers(0, 4, 1000)],                       # a few distinct values, repeated
             [(1 << 55) + (k ^ 0x2a5) for k in range(1023)]]                                       # bit-reversed neighbours
    for keys in cases:
        out = driver(f"sort {len(keys)}\n" + " ".join(str(k) for k in keys) + "\n")
        got = [int(w) for w in out[0].split()] if out and out[0].strip() else []
        assert got == sorted(keys), len(keys)


# ---- the premise -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", sref.CAPACITIES)
def test_the_fp32_chain_gives_the_integer_r2_on_every_input(capacity):
    """On grid inputs every operation of the chain is exact, so the fp32 operations one by one (numpy has no fused multiply-add,
    and needs none where nothing rounds) give the r2 of the fp64 reference, whose Gram form keeps to integer numbers of squared
    grid units below 2^24."""
    P, counts = sref.gpu_inputs(capacity)
    pos, n, _ = sref.subset_inputs(capacity)
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
