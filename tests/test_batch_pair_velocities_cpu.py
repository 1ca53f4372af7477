"""CPU-only: the pair velocity statistics of batched ensembles (nbody_batch_pair_velocities,
include/nbody_batch_pair_velocities.h).  The header is self-contained C99, included by nbody.h after the shape header, and
declares its one entry point alone; it is exported, bound and listed; the arithmetic without a GPU
(csrc/nbody_batch_pair_velocities_math.h), built into a stand-alone driver with g++ -- once more with the address and
undefined-behaviour sanitizers -- gives the reference's bytes on every case of the three smaller capacities, for four workgroup
shapes and five numbers of bins per pass; the reference itself is checked against a plain numpy pair walk and against
hermite_correlation_ref's counts; its spread under moved roots and quotients is measured again (hermite_pair_velocities_ref.BOUND
= 2.72e-14 is four times the constant it stays within); and the derived quantities of PairVelocityResult do what they say on
hand-made records."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_correlation_ref as cref
import hermite_pair_velocities_ref as pref
from conftest import ROOT

NAMES = ["nbody_batch_pair_velocities"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
SHAPES = ((64, 1), (64, 2), (128, 4), (1024, 4))
PASS_BINS = (1, 2, 4, 8, 32)


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_shape_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_pair_velocities.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_pair_velocities.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_shape.h"') < nbody_h.index('#include "nbody_batch_pair_velocities.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_96_and_56_bytes(tmp_path):
    bin_offsets = dict(zip(pref.INTEGERS + pref.TERMS, range(0, 96, 8)))
    system_offsets = dict(zip(pref.SYSTEM_WORDS, (0, 4, 8, 12, 16, 20, 24, 32, 40, 48)))
    checks = [f"typedef char bin_{w}[offsetof(nbody_batch_pair_velocities_bin, {w}) == {o} ? 1 : -1];" for w, o in bin_offsets.items()]
    checks += [f"typedef char system_{w}[offsetof(nbody_batch_pair_velocities_system, {w}) == {o} ? 1 : -1];"
               for w, o in system_offsets.items()]
    src = tmp_path / "pair_velocities.c"
    src.write_text('#include "nbody.h"\n#include <stddef.h>\n' + "\n".join(checks) + r'''
typedef char bin_is_96_bytes[sizeof(nbody_batch_pair_velocities_bin) == 96 ? 1 : -1];
typedef char system_is_56_bytes[sizeof(nbody_batch_pair_velocities_system) == 56 ? 1 : -1];
typedef char limit[NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS == 32 ? 1 : -1];
int main(void) {
    nbody_batch_pair_velocities_system s;
    float edges[2] = {0.f, 1.f};
    return (nbody_batch_pair_velocities(0, 0, 0, 1, edges, 0, 0, 0, NBODY_BATCH_WEIGHT_NUMBER, &s, 0) != NBODY_ERR_INVALID) +
           (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert [pref.BIN_DTYPE.fields[w][1] for w in pref.INTEGERS + pref.TERMS] == list(bin_offsets.values())
    assert [pref.SYSTEM_DTYPE.fields[w][1] for w in pref.SYSTEM_WORDS] == list(system_offsets.values())


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_pair_velocities.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_shape.h", "n_systems x max_bodies bytes",
                   "An ordered pair (i, j) is examined iff rows[i], sources[j] and j != i", "r2 is groups_r2",
                   "r2 = fmaf(dz, dz, fmaf(dy, dy, dx dx))", "1 <= bins <= NBODY_BATCH_PAIR_VELOCITIES_MAX_BINS (32)",
                   "strictly ascending", "e2[t] = edges[t] * edges[t] is one fp32 product on the host", "e2[t] < r2 <= e2[t + 1]",
                   "decided in fp32 by the code nbody_batch_correlation runs", "!(r2 < +inf)", "!(v2 < +inf)",
                   "below + sum of count + above + unmeasured == pairs == rows * sources - both",
                   "the same integers that nbody_batch_correlation returns", "ww = (double)m_i * (double)m_j",
                   "the fourth velocity word is not read", "s = (dx dx + dy dy) + dz dz", "rv = (dx wx + dy wy) + dz wz",
                   "v2 = (wx wx + wy wy) + wz wz", "vt2 = fmax(v2 - vr vr, 0)", "s > 0 and r > 0", "96 bytes", "56 bytes",
                   "An empty bin reads 0 everywhere", "NULL skips that copy", "the same bits either way", "in ascending j",
                   "Block k is rows 64 k ... 64 k + 63", "off = 32, 16, 8, 4, 2, 1", "total += partial_k",
                   "Adding +0.0 changes no bit and no sum can be -0",
                   "r1, vr1, vr2, vt2 and v1 pass through the device's fp64 square root and division",
                   "weight, r2, rv, v2 and the integers are made of +, -, x and comparisons alone", "synchronous", "forgets nothing",
                   "bit for bit", "freed in nbody_batch_destroy", "workgroup shape and number of passes", "names the function",
                   "a weight that is not 0 or 1", "refused before any device work", "Out of scope", "per-body (per-row) profiles",
                   "more than 32 bins in one call", "projected separations", "a triangular walk for the auto case",
                   "pairs across systems", "device-side outputs", "the external field"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.pair_velocities_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.correlation_names()) | set(_lib.shape_names()) | set(_lib.pairs_names()))
    fn = lib.nbody_batch_pair_velocities
    assert fn.argtypes is not None and len(fn.argtypes) == 11
    assert ctypes.sizeof(_lib.BatchPairVelocitiesBin) == 96 and ctypes.sizeof(_lib.BatchPairVelocitiesSystem) == 56
    assert [f[0] for f in _lib.BatchPairVelocitiesBin._fields_] == list(pref.INTEGERS + pref.TERMS)
    assert [f[0] for f in _lib.BatchPairVelocitiesSystem._fields_] == list(pref.SYSTEM_WORDS)
    for w in pref.INTEGERS + pref.TERMS:
        assert getattr(_lib.BatchPairVelocitiesBin, w).offset == pref.BIN_DTYPE.fields[w][1] == batch.PAIR_VELOCITIES_BIN_DTYPE.fields[w][1]
    for w in pref.SYSTEM_WORDS:
        assert getattr(_lib.BatchPairVelocitiesSystem, w).offset == pref.SYSTEM_DTYPE.fields[w][1] == \
            batch.PAIR_VELOCITIES_SYSTEM_DTYPE.fields[w][1]
    assert batch.PAIR_VELOCITIES_BIN_DTYPE == pref.BIN_DTYPE and batch.PAIR_VELOCITIES_SYSTEM_DTYPE == pref.SYSTEM_DTYPE
    assert _lib.BATCH_PAIR_VELOCITIES_MAX_BINS == pref.MAX_BINS == 32
    assert (_lib.BATCH_WEIGHT_MASS, _lib.BATCH_WEIGHT_NUMBER) == (pref.WEIGHT_MASS, pref.WEIGHT_NUMBER)
    assert "PairVelocityResult" in nb.__all__ and nb.PairVelocityResult is batch.PairVelocityResult
    assert batch.PairVelocityResult.__doc__ and batch.BatchedSystem.pair_velocities.__doc__
    for helper in ("mean_separation", "mean_radial_velocity", "sigma_radial", "sigma_tangential", "anisotropy", "structure_function",
                   "approaching_fraction", "expansion_rate", "unordered"):
        assert getattr(batch.PairVelocityResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_pair_velocities") == 1
    assert exports[exports.index("nbody_batch_pair_velocities") - 1].startswith("# nbody_batch_pair_velocities")
    assert sorted(e for e in exports if not e.startswith("#")) == [e for e in exports if not e.startswith("#")]
    hpp = open(os.path.join(INCLUDE, "nbody.hpp")).read()
    assert "std::vector<nbody_batch_pair_velocities_system> pairVelocities(" in hpp and "nbody_batch_pair_velocities(b_, dPositions," in hpp


def test_the_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "wrapper.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_pair_velocities_system> use(nbody::Batch &b, const float *p, const float *v)
{
    std::vector<nbody_batch_pair_velocities_bin> bins;
    return b.pairVelocities(p, v, {0.f, 1.f, 2.f}, &bins, NBODY_BATCH_WEIGHT_MASS);
}
''')
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_the_errors_of_the_header_are_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchPairVelocitiesSystem * 1)()
    edges = (ctypes.c_float * 2)(0.0, 1.0)
    assert lib.nbody_batch_pair_velocities(None, None, None, 1, edges, 0, None, None, 1, out, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_pair_velocities: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_pair_velocities("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_pair_velocities: batch is NULL", "nbody_batch_pair_velocities: NULL argument",
                "nbody_batch_pair_velocities: bins must be 1 ... 32", "nbody_batch_pair_velocities: weight must be",
                "must be finite and >= 0", "the edges must be strictly ascending")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_pair_velocities: ') == len(messages)                       # every message names the function


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip_and_reuses_correlations_functions():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_pair_velocities_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_pair_velocities.h" for h in build.HEADERS)
    assert "-ffp-contract=off" in build.FLAGS
    text = open(os.path.join(CSRC, "nbody_batch_pair_velocities_math.h")).read()
    code = re.sub(r"//.*", "", text)
    assert "hip/" not in code and "NBODY_HD inline" in code and '#include "nbody_batch_correlation_math.h"' in code
    assert "fma(" not in code and "fmaf(" not in code                                          # the r2 chain is reused, not restated
    for call in ("groups_r2(", "groups_friends(", "correlation_measured(", "correlation_pairs(", "correlation_below(",
                 "correlation_above(", "correlation_unmeasured("):
        assert call in code, call
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_pair_velocities_kernel("):source.index("hipError_t launch_batch_pair_velocities(")]
    for call in ("pair_velocities_flags(", "pair_velocities_body_measured(", "correlation_examined(", "pair_velocities_r2(",
                 "pair_velocities_system_step(", "pair_velocities_bin<G>(", "pair_velocities_member<G>(", "pair_velocities_add<G>(",
                 "pair_velocities_tree_step(", "pair_velocities_total(", "pair_velocities_store(", "pair_velocities_system(",
                 "readfirstlane(", "__shfl_down("):
        assert call in kernel, call
    assert "asm" not in kernel and "fma" not in kernel and "sqrt" not in kernel and "groups_r2" not in kernel
    launch = source[source.index("hipError_t launch_batch_pair_velocities("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "launch_analysis_kernel(" in launch and "kPairVelocitiesPassBins" in launch
    assert "pair_velocities_threads(" in launch
    assert source.index("hipError_t launch_batch_shape(") < source.index("void batch_pair_velocities_kernel(") \
        < source.index("hipError_t launch_batch_pair_velocities(") < source.index("void batch_diag_kernel(") < source.index("}  // namespace\n")
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchPairVelocitiesSystem> pair_velocities_systems", "DeviceArray<BatchPairVelocitiesBin> pair_velocities_bins",
                   "DeviceArray<unsigned char> pair_velocities_rows", "DeviceArray<unsigned char> pair_velocities_sources",
                   "DeviceArray<float> pair_velocities_edges2"):
        assert member in members, member
    entry = source[source.index("int nbody_batch_pair_velocities("):]
    entry = entry[:entry.index("\n}\n")]
    assert "hipFree" not in entry and "hipMalloc" not in entry and "correlation_edge2(" in entry and "correlation_edge_valid(" in entry


def test_the_lds_of_the_largest_launch_fits_a_gfx950_workgroup():
    """The launcher's sum, recomputed: 32 bytes per body, then G x 9 doubles per wave of the workgroup, and the static words."""
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    threads = int(re.search(r"#define NBODY_BATCH_PAIR_VELOCITIES_MAX_THREADS (\d+)", source).group(1))
    assert threads % 64 == 0 and 64 <= threads <= 1024
    dynamic = 32 * 4096 + 8 * (threads // 64) * pref.G_BUILT * 9
    static = 4 * (3 * pref.G_BUILT + 3) + 4 * 3
    assert dynamic + static <= 160 * 1024


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_pair_velocities_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("pair_velocities"), [])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("pair_velocities_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def command(pos, vel, n, edges, rows, sources, weight, shape, g):
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    lines = [f"system {n} {len(edges) - 1} {weight} {shape[0]} {shape[1]} {g}", " ".join(str(w) for w in bits(edges))]
    p, v = bits(pos[:n]), bits(vel[:n])
    for i in range(n):
        row = 1 if rows is None or rows[i] else 0
        source = 1 if sources is None or sources[i] else 0
        lines.append(" ".join(str(w) for w in (*p[i], *v[i, :3])) + f" {row} {source}")
    return "\n".join(lines) + "\n"


def parse(lines, bins):
    system = np.zeros((), pref.SYSTEM_DTYPE)
    for word, value in zip(pref.SYSTEM_WORDS, lines[0].split()):
        system[word] = int(value)
    out = np.zeros(bins, pref.BIN_DTYPE)
    for t in range(bins):
        words = lines[1 + t].split()
        for word, value in zip(pref.INTEGERS, words[:3]):
            out[word][t] = int(value)
        out.view(np.uint64).reshape(bins, 12)[t, 3:] = [int(w) for w in words[3:]]
    return system, out, lines[1 + bins:]


def run_case(run, capacity, name, shapes, pass_bins):
    _, bins, weight, kind, per_system = next(c for c in pref.cases_of(capacity) if c[0] == name)
    P, V, counts, _ = pref.gpu_inputs(capacity)
    rows, sources = pref.gpu_masks(capacity, kind)
    edges = pref.gpu_edges(capacity, bins, per_system)
    refs = pref.gpu_reference(capacity, name)
    compared = 0
    for shape in shapes:
        for g in pass_bins:
            text, which = "", []
            for s, n in enumerate(counts):
                if n <= shape[0] * shape[1]:
                    text += command(P[s], V[s], n, edges[s] if per_system else edges, None if rows is None else rows[s],
                                    None if sources is None else sources[s], weight, shape, g)
                    which.append(s)
            lines = run(text)
            for s in which:
                system, out, lines = parse(lines, bins)
                assert system.tobytes() == refs[s]["system"].tobytes(), (capacity, name, shape, g, s, system, refs[s]["system"])
                assert out.tobytes() == refs[s]["bins"].tobytes(), (capacity, name, shape, g, s)
                compared += 1
            assert not lines
    return compared


@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_driver_gives_the_references_bytes_for_every_shape_and_every_number_of_bins_per_pass(driver, capacity):
    """Every case, every system that the shape holds, (64,1), (64,2), (128,4) and (1024,4), G = 1, 2, 4, 8 and 32: byte-equal
    to the reference, so the same bytes for every G and shape."""
    compared = sum(run_case(driver, capacity, name, SHAPES, PASS_BINS) for name, *_ in pref.cases_of(capacity))
    assert compared >= len(pref.CASES) * len(PASS_BINS) * (len(SHAPES) - 1) * 4


def test_the_driver_gives_the_references_bytes_at_1024_bodies(driver):
    """Capacity 1024 (counts up to 1024: sixteen blocks), the shape of the device and one other, G as built and 32."""
    assert run_case(driver, 1024, "mass-disjoint-own-edges", ((256, 4), (1024, 1)), (pref.G_BUILT, 32)) > 0
    assert run_case(driver, 1024, "bins9", ((256, 4),), (pref.G_BUILT,)) > 0


def test_the_sanitized_driver_gives_the_references_bytes(sanitized_driver):
    """The same arithmetic as a stand-alone program under the address and undefined-behaviour sanitizers: every case of capacity
    128 at two shapes and three G."""
    for name, *_ in pref.cases_of(128):
        assert run_case(sanitized_driver, 128, name, ((64, 2), (128, 4)), (1, 2, 32)) > 0


def test_the_driver_states_the_layout_and_the_limits(driver):
    lines = driver("layout\nlimits\n")
    assert [int(w) for w in lines[0].split()] == [96] + [pref.BIN_DTYPE.fields[w][1] for w in pref.INTEGERS + pref.TERMS]
    assert [int(w) for w in lines[1].split()] == [56] + [pref.SYSTEM_DTYPE.fields[w][1] for w in pref.SYSTEM_WORDS]
    assert [int(w) for w in lines[2].split()] == [32, 64, 9, pref.G_BUILT, 3, 7]                # 5 bins at 2 per pass: 3 passes, 7 edges


# ---- independent checks of the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_reference_agrees_with_a_plain_numpy_pair_walk(capacity):
    """Counts equal; every sum within 1e-12 of the sum of its absolute addends."""
    P, V, counts, _ = pref.gpu_inputs(capacity)
    for name, bins, weight, kind, per_system in pref.cases_of(capacity):
        rows, sources = pref.gpu_masks(capacity, kind)
        edges = pref.gpu_edges(capacity, bins, per_system)
        for s, ref in enumerate(pref.gpu_reference(capacity, name)):
            count, sums, absolute = pref.plain_walk(P[s], V[s], counts[s], edges[s] if per_system else edges,
                                                    None if rows is None else rows[s], None if sources is None else sources[s], weight)
            assert (count == ref["bins"]["count"]).all(), (name, s)
            for c, word in enumerate(pref.TERMS):
                assert (np.abs(sums[:, c] - ref["bins"][word]) <= 1e-12 * absolute[:, c]).all(), (name, s, word)
                assert (np.abs(absolute[:, c] - ref["absolute"][:, c]) <= 1e-12 * absolute[:, c]).all(), (name, s, word)
            assert (ref["bins"]["approaching"] + ref["bins"]["receding"] <= ref["bins"]["count"]).all()


@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_references_counts_are_hermite_correlation_refs(capacity):
    """With the bodies of unmeasurable velocity taken out of both masks (their pairs are unmeasured here and counted there),
    every integer is hermite_correlation_ref.reference's on the coordinates scaled to its integers; with them in, the
    difference is in `unmeasured` alone... and in the bins those pairs would have fallen into."""
    P, V, counts, Q = pref.gpu_inputs(capacity)
    for name, bins, weight, kind, per_system in pref.cases_of(capacity):
        rows, sources = pref.gpu_masks(capacity, kind)
        edges = pref.gpu_edges(capacity, bins, per_system)
        for s, n in enumerate(counts):
            moving = np.isfinite(V[s, :n, :3]).all(axis=1)
            row = (np.ones(n, bool) if rows is None else rows[s, :n]) & moving
            source = (np.ones(n, bool) if sources is None else sources[s, :n]) & moving
            e = np.asarray(edges[s] if per_system else edges, np.float32)
            ours = pref.reference(P[s], V[s], n, Q[s], e, row, source, weight)
            scaled = np.array(P[s, :n], np.float64)
            scaled[:, :3] *= Q[s]
            theirs = cref.reference(scaled, n, e * np.float32(Q[s]), row, source)       # Q e: the squares scale exactly by Q^2
            cref.check_identity(theirs)
            for word in ("rows", "sources", "both", "bins", "pairs", "below", "above", "unmeasured"):
                assert int(ours["system"][word]) == theirs[word], (name, s, word)
            assert (ours["bins"]["count"] == theirs["counts"]).all(), (name, s)
            full = pref.gpu_reference(capacity, name)[s]
            total = int(full["system"]["below"]) + int(full["bins"]["count"].sum()) + int(full["system"]["above"]) + \
                int(full["system"]["unmeasured"])
            assert total == int(full["system"]["pairs"]) == int(full["system"]["rows"]) * int(full["system"]["sources"]) - \
                int(full["system"]["both"])


def test_the_inputs_hold_what_they_should():
    for capacity in pref.CAPACITIES:
        P, V, counts, Q = pref.gpu_inputs(capacity)
        assert max(counts) == capacity and (capacity == 4096 or counts[:4] == [0, 1, 2, 3])
        for s, n in enumerate(counts):
            x = P[s, :n, :3].astype(np.float64) * Q[s]
            finite = np.isfinite(x)
            assert (x[finite] == np.round(x[finite])).all() and (np.abs(x[finite]) <= cref.LIMIT).all()
            if n >= 63:
                assert np.isnan(P[s, 5, 1]) and np.isinf(V[s, 9, 0]) and (P[s, 11, :3] == P[s, 12, :3]).all()
    assert pref.BINS == (1, 7, 8, 9, 32) and pref.shared_edges(3)[0] == 0.0
    assert {c[2] for c in pref.CASES} == {0, 1} and {c[3] for c in pref.CASES} == set(pref.MASKS) and {c[4] for c in pref.CASES} == {False, True}
    # unmeasured by velocity alone is a property of the two bodies: v2 of finite words is finite
    big = np.float64(np.finfo(np.float32).max)
    assert np.isfinite(3.0 * (2.0 * big) ** 2)


def test_the_spread_of_the_reference_under_moved_roots_and_quotients_is_within_the_constant():
    """BOUND, measured again: the largest error measure of the reference against itself when every root and quotient is moved
    by up to one ulp at random, over all cases of the three smaller capacities (5.09e-15 with this seed and 6.79e-15 with three others when the constant, 6.8e-15, was set); no
    integer and no exact word moves."""
    spread, same = pref.jitter_spread()
    print(f"spread {spread:.3g}; SPREAD {pref.SPREAD:.3g}; BOUND {pref.BOUND:.3g}")
    assert same and 0.0 < spread <= pref.SPREAD and pref.BOUND == 4.0 * pref.SPREAD


# ---- the derived quantities ----------------------------------------------------------------------------------------------------
def test_the_derived_quantities_on_hand_made_records():
    from n_body_problem_amd import batch
    systems = np.zeros(2, batch.PAIR_VELOCITIES_SYSTEM_DTYPE)
    systems["rows"], systems["sources"], systems["both"] = [4, 4], [4, 3], [4, 0]
    systems["pairs"] = [12, 12]
    records = np.zeros((2, 2), batch.PAIR_VELOCITIES_BIN_DTYPE)
    records[0, 0] = (4, 2, 2, 8.0, 16.0, 40.0, 20.0, -4.0, 10.0, 16.0, 12.0, 26.0)
    records[1, 0] = (3, 1, 2, 3.0, 3.0, 3.0, 6.0, 3.0, 3.0, 0.0, 3.0, 3.0)
    res = batch.PairVelocityResult(systems, records, np.array([0.0, 1.0, 2.0], np.float32), "mass")
    assert res.bins == 2 and res.auto.tolist() == [True, False]
    assert res.mean_separation()[0, 0] == 2.0 and np.isnan(res.mean_separation()[0, 1])
    assert res.mean_radial_velocity()[0, 0] == -0.5 and res.mean_radial_velocity()[1, 0] == 1.0
    assert res.sigma_radial()[0, 0] == 1.0 and res.sigma_radial()[1, 0] == 0.0             # sqrt(10 / 8 - 0.25)
    assert res.sigma_tangential()[0, 0] == 1.0 and res.sigma_tangential()[1, 0] == 0.0     # sqrt(16 / (2 * 8))
    assert res.anisotropy()[0, 0] == 0.0 and np.isnan(res.anisotropy()[1, 0]) and np.isnan(res.anisotropy()[0, 1])
    assert res.structure_function(1)[0, 0] == 1.5 and res.structure_function(2)[0, 0] == 3.25
    assert res.approaching_fraction()[0, 0] == 0.5 and np.isnan(res.approaching_fraction()[1, 1])
    assert res.expansion_rate()[0, 0] == 0.5 and res.expansion_rate()[1, 0] == 2.0
    half = res.unordered()
    assert half["count"][0, 0] == 2 and half["weight"][0, 0] == 4.0 and half["v2"][0, 0] == 13.0
    assert half[1].tobytes() == records[1].tobytes()                                      # not auto: as they are
    with pytest.raises(ValueError):
        res.structure_function(3)
    lean = batch.PairVelocityResult(systems, None, np.array([0.0, 1.0, 2.0], np.float32))
    assert lean.count is None
    with pytest.raises(ValueError):
        lean.mean_separation()
    assert "PairVelocityResult(bins=2" in repr(res)
