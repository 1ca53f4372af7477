"""CPU-only: the mutual gravity of labelled sets of batched ensembles (nbody_batch_mutual_gravity,
include/nbody_batch_mutual_gravity.h).  The header is self-contained C99, included by nbody.h after the pair velocities header,
and declares its one entry point alone; it is exported, bound and listed; the arithmetic without a GPU
(csrc/nbody_batch_mutual_gravity_math.h), built into a stand-alone driver with g++ -- once more with the address and
undefined-behaviour sanitizers -- gives the reference's bytes on every case of the three smaller capacities for four workgroup
shapes; its counting sort is numpy's stable argsort; the reference itself is checked against a plain numpy pair walk, against
Newton's third law and against a closed form in which every operation is exact; its spread under moved roots and quotients is
measured again (hermite_mutual_gravity_ref.BOUND is four times the constant it stays within); and the derived quantities of
MutualGravityResult do what they say on hand-made records."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import hermite_mutual_gravity_ref as mref
from conftest import ROOT

NAMES = ["nbody_batch_mutual_gravity"]
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
THREADS = (64, 128, 256, 1024)


@pytest.fixture(scope="module")
def lib():
    from n_body_problem_amd import _lib, build
    build.build_library()
    return _lib.load()


def declared(text):
    return set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))


# ---- the surface --------------------------------------------------------------------------------------------------------
def test_the_header_is_included_by_nbody_h_after_pair_velocities_and_declares_its_one_entry_point_alone():
    assert declared(open(os.path.join(INCLUDE, "nbody_batch_mutual_gravity.h")).read()) == set(NAMES)
    for header in glob.glob(os.path.join(INCLUDE, "*.h")):
        if os.path.basename(header) != "nbody_batch_mutual_gravity.h":
            assert not declared(open(header).read()) & set(NAMES), header
    res = subprocess.run(["gcc", "-E", "-P", "-std=c99", os.path.join(INCLUDE, "nbody.h")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(NAMES) <= set(re.findall(r"\b(nbody_[a-z0-9_]+)\s*\(", res.stdout))
    nbody_h = open(os.path.join(INCLUDE, "nbody.h")).read()
    assert nbody_h.index('#include "nbody_batch_pair_velocities.h"') < nbody_h.index('#include "nbody_batch_mutual_gravity.h"')


def test_the_header_is_self_contained_c99_and_the_records_are_80_and_128_bytes(tmp_path):
    checks = [f"typedef char entry_{w}[offsetof(nbody_batch_mutual_gravity_entry, {w}) == {o} ? 1 : -1];" for w, o in mref.ENTRY_OFFSETS.items()]
    checks += [f"typedef char system_{w}[offsetof(nbody_batch_mutual_gravity_system, {w}) == {o} ? 1 : -1];"
               for w, o in mref.SYSTEM_OFFSETS.items()]
    src = tmp_path / "mutual_gravity.c"
    src.write_text('#include "nbody.h"\n#include <stddef.h>\n' + "\n".join(checks) + r'''
typedef char entry_is_80_bytes[sizeof(nbody_batch_mutual_gravity_entry) == 80 ? 1 : -1];
typedef char system_is_128_bytes[sizeof(nbody_batch_mutual_gravity_system) == 128 ? 1 : -1];
typedef char limit[NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS == 8 && NBODY_BATCH_MUTUAL_GRAVITY_NO_SET == 255 ? 1 : -1];
int main(void) {
    nbody_batch_mutual_gravity_system s;
    unsigned char labels[1] = {0};
    return (nbody_batch_mutual_gravity(0, 0, 0, 1, labels, 0.f, 0, 0, &s, 0) != NBODY_ERR_INVALID) + (NBODY_ABI_VERSION != 5);
}
''')
    res = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert {w: mref.ENTRY_DTYPE.fields[w][1] for w in mref.ENTRY_WORDS} == mref.ENTRY_OFFSETS
    assert {w: mref.SYSTEM_DTYPE.fields[w][1] for w in mref.SYSTEM_WORDS} == mref.SYSTEM_OFFSETS


def test_the_header_states_the_rules_and_what_is_out_of_scope():
    def plain(words):
        return " ".join(words.replace(" *", " ").split())
    text = plain(open(os.path.join(INCLUDE, "nbody_batch_mutual_gravity.h")).read())
    for phrase in ("ABI version 5", "no new status", "after nbody_batch_pair_velocities.h", "n_systems x max_bodies bytes",
                   "NBODY_BATCH_MUTUAL_GRAVITY_NO_SET (255)", "1 <= sets <= NBODY_BATCH_MUTUAL_GRAVITY_MAX_SETS (8)",
                   "whatever the massive counts are", "any of its seven words x, y, z, m, vx, vy, vz is a NaN or infinite",
                   "a property of the body, not of a pair", "A body in no set may hold anything",
                   "widened fp32 words cannot overflow fp64 through these products", "d_c = (double)x_j,c - (double)x_i,c",
                   "e2 = (double)softening * (double)softening", "s2 = ((dx dx + dy dy) + dz dz) + e2",
                   "counts in `pairs` and in `coincident` and adds nothing", "r = sqrt(s2)", "inv = 1.0 / r", "mi = (double)m_j * inv",
                   "g = (mi * inv) * inv", "in ascending j, one add per member", "P_b += mi", "A_b,c += g * d_c", "f_c = mm * A_b,c",
                   "torque_x: p_y f_z - p_z f_y", "virial: (p_x f_x + p_y f_y) + p_z f_z", "power: (q_x f_x + q_y f_y) + q_z f_z",
                   "ranked 0 ... n_a - 1 in ascending body index", "Block k of set a is its ranks 64 k ... 64 k + 63",
                   "off = 32, 16, 8, 4, 2, 1", "total += partial_k", "The potential word is 0.0 - total", "80 bytes", "128 bytes",
                   "(s * sets + a) * sets + b", "An entry with an empty set reads 0 everywhere",
                   "selected + left_out + unmeasured == min(counts[s], max_bodies)",
                   "entry.pairs == members[a] * members[b] - (a == b) * members[a]", "the sum of its entries' pairs",
                   "NULL skips that copy", "the same bits either way", "NULL for zeros", "workgroup shape and launch plan",
                   "Renaming the sets permutes the entries byte for byte", "correctly rounded", "synchronous", "forgets nothing",
                   "bit for bit", "freed in nbody_batch_destroy", "names the function", "sets outside 1 ... 8",
                   "the message names the system and the body", "NBODY_MIN_SOFTENING", "a NaN or infinite centre or velocity word",
                   "refused before any device work", "Out of scope", "tensors", "a per-body breakdown", "more than 8 sets",
                   "overlapping sets", "the external field", "pairs across systems", "device-side outputs"):
        assert plain(phrase) in text, phrase


def test_the_name_is_mirrored_in_a_list_of_its_own_exported_and_bound(lib):
    from n_body_problem_amd import _lib, batch
    import n_body_problem_amd as nb
    assert _lib.mutual_gravity_names() == NAMES
    assert not set(NAMES) & (set(_lib.exported_names()) | set(_lib.pair_velocities_names()) | set(_lib.members_names()))
    fn = lib.nbody_batch_mutual_gravity
    assert fn.argtypes is not None and len(fn.argtypes) == 10
    assert ctypes.sizeof(_lib.BatchMutualGravityEntry) == 80 and ctypes.sizeof(_lib.BatchMutualGravitySystem) == 128
    assert [f[0] for f in _lib.BatchMutualGravityEntry._fields_] == list(mref.ENTRY_WORDS)
    assert [f[0] for f in _lib.BatchMutualGravitySystem._fields_] == list(mref.SYSTEM_WORDS)
    for w in mref.ENTRY_WORDS:
        assert getattr(_lib.BatchMutualGravityEntry, w).offset == mref.ENTRY_OFFSETS[w] == batch.MUTUAL_GRAVITY_ENTRY_DTYPE.fields[w][1]
    for w in mref.SYSTEM_WORDS:
        assert getattr(_lib.BatchMutualGravitySystem, w).offset == mref.SYSTEM_OFFSETS[w] == batch.MUTUAL_GRAVITY_SYSTEM_DTYPE.fields[w][1]
    assert batch.MUTUAL_GRAVITY_ENTRY_DTYPE == mref.ENTRY_DTYPE and batch.MUTUAL_GRAVITY_SYSTEM_DTYPE == mref.SYSTEM_DTYPE
    assert _lib.BATCH_MUTUAL_GRAVITY_MAX_SETS == mref.MAX_SETS == 8 and _lib.BATCH_MUTUAL_GRAVITY_NO_SET == mref.NO_SET == 255
    assert "MutualGravityResult" in nb.__all__ and nb.MutualGravityResult is batch.MutualGravityResult
    assert batch.MutualGravityResult.__doc__ and batch.BatchedSystem.mutual_gravity.__doc__
    for helper in ("interaction_energy", "self_energy", "total_potential_energy", "force_on", "torque_on", "power_into",
                   "acceleration_of", "two_body_energy", "labels_from_masks"):
        assert getattr(batch.MutualGravityResult, helper).__doc__, helper
    exports = open(os.path.join(ROOT, "profiles", "ctx_ownership_exports.txt")).read().splitlines()
    assert exports.count("nbody_batch_mutual_gravity") == 1
    assert exports[exports.index("nbody_batch_mutual_gravity") - 1].startswith("# nbody_batch_mutual_gravity")
    assert sorted(e for e in exports if not e.startswith("#")) == [e for e in exports if not e.startswith("#")]
    hpp = open(os.path.join(INCLUDE, "nbody.hpp")).read()
    assert "std::vector<nbody_batch_mutual_gravity_system> mutualGravity(" in hpp and "nbody_batch_mutual_gravity(b_, dPositions," in hpp


def test_the_cpp_wrapper_compiles(tmp_path):
    src = tmp_path / "wrapper.cpp"
    src.write_text(r'''
#include "nbody.hpp"
std::vector<nbody_batch_mutual_gravity_system> use(nbody::Batch &b, const float *p, const float *v, const std::vector<unsigned char> &labels)
{
    std::vector<nbody_batch_mutual_gravity_entry> matrix;
    return b.mutualGravity(p, v, 2, labels, &matrix, 0.01f);
}
''')
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_the_abi_stays_at_version_5_and_the_errors_of_the_header_are_refused_without_a_device(lib):
    from n_body_problem_amd import _lib
    assert lib.nbody_abi_version() == 5
    out = (_lib.BatchMutualGravitySystem * 1)()
    labels = (ctypes.c_ubyte * 1)(0)
    assert lib.nbody_batch_mutual_gravity(None, None, None, 1, labels, 0.0, None, None, out, None) == _lib.NBODY_ERR_INVALID
    assert b"nbody_batch_mutual_gravity: batch is NULL" in lib.nbody_batch_last_error(None)
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    body = source[source.index("int nbody_batch_mutual_gravity("):]
    body = body[:body.index("\n}\n")]
    messages = ("nbody_batch_mutual_gravity: batch is NULL", "nbody_batch_mutual_gravity: NULL argument",
                "nbody_batch_mutual_gravity: sets must be 1 ... 8", "nbody_batch_mutual_gravity: softening must be finite",
                "nbody_batch_mutual_gravity: the label ", "nbody_batch_mutual_gravity: the centre of system ",
                "nbody_batch_mutual_gravity: the velocity of system ")
    for message in messages:
        assert message in body and body.index(message) < body.index("hipSetDevice"), message
        assert body.index(message) < body.index("batch_analysis(b, a)"), message
    assert body.count('"nbody_batch_mutual_gravity: ') == len(messages)                        # every message names the function
    assert " of body " in body and " of system " in body                                       # the label's message names both


def test_the_headers_are_build_dependencies_and_the_math_header_is_free_of_hip():
    from n_body_problem_amd import build
    assert os.path.join(CSRC, "nbody_batch_mutual_gravity_math.h") in build.HEADERS
    assert any(os.path.basename(h) == "nbody_batch_mutual_gravity.h" for h in build.HEADERS)
    assert "-ffp-contract=off" in build.FLAGS and not any("fast" in f for f in build.FLAGS)
    text = open(os.path.join(CSRC, "nbody_batch_mutual_gravity_math.h")).read()
    code = re.sub(r"//.*", "", text)
    assert "hip/" not in code and "NBODY_HD inline" in code and '#include "nbody_batch_pair_velocities_math.h"' in code
    assert "fma(" not in code and "fmaf(" not in code and "rsq" not in code
    source = open(os.path.join(CSRC, "nbody_batch_analysis.hip")).read()
    kernel = source[source.index("void batch_mutual_gravity_kernel("):source.index("hipError_t launch_batch_mutual_gravity(")]
    for call in ("mutual_gravity_body(", "mutual_gravity_chunk_count(", "mutual_gravity_chunk_rank(", "mutual_gravity_prefix(",
                 "mutual_gravity_starts(", "mutual_gravity_slot(", "mutual_gravity_unit_set(", "mutual_gravity_step(",
                 "mutual_gravity_addends(", "pair_velocities_tree_step(", "mutual_gravity_total(", "mutual_gravity_store(",
                 "mutual_gravity_pairs(", "mutual_gravity_mass(", "ballot_w64(", "__shfl_down("):
        assert call in kernel, call
    assert "asm" not in kernel and "fma" not in kernel and "sqrt" not in kernel
    launch = source[source.index("hipError_t launch_batch_mutual_gravity("):source.index("void batch_diag_kernel(")]
    assert "batch_shape(max_bodies)" in launch and "launch_analysis_kernel(" in launch and "mutual_gravity_threads(" in launch
    assert source.index("hipError_t launch_batch_pair_velocities(") < source.index("void batch_mutual_gravity_kernel(") \
        < source.index("hipError_t launch_batch_mutual_gravity(") < source.index("void batch_diag_kernel(") < source.index("}  // namespace\n")
    members = source[source.index("struct BatchAnalysis {"):source.index("void batch_analysis_destroy(")]
    for member in ("DeviceArray<BatchMutualGravitySystem> mutual_gravity_systems", "DeviceArray<BatchMutualGravityEntry> mutual_gravity_entries",
                   "DeviceArray<unsigned char> mutual_gravity_labels", "DeviceArray<double> mutual_gravity_frames"):
        assert member in members, member
    entry = source[source.index("int nbody_batch_mutual_gravity("):]
    entry = entry[:entry.index("\n}\n")]
    assert "hipFree" not in entry and "hipMalloc" not in entry and "batch_softening_ok(" in entry and "mutual_gravity_e2(" in entry


def test_the_lds_of_the_largest_launch_fits_a_gfx950_workgroup():
    """The launcher's sum, recomputed: 16 bytes per column, sets x 9 doubles per unit, 4 bytes per slot, and the static words."""
    for sets in range(1, 9):
        dynamic = 16 * 4096 + 8 * (4096 // 64 + sets) * sets * 9 + 4 * 4096
        static = 2 * 4 * 64 * 8 + 4 * (8 + 9 + 9 + 3 + 1)
        assert dynamic + static <= 160 * 1024


# ---- the arithmetic on the CPU -----------------------------------------------------------------------------------------------
def build_driver(path, extra):
    exe = str(path / "driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I" + CSRC,
           os.path.join(ROOT, "tests", "batch_mutual_gravity_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return res.stdout.splitlines()
    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("mutual_gravity"), [])


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("mutual_gravity_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def command(pos, vel, n, labels, sets, eps, centre, velocity, threads):
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    frame = np.concatenate([np.zeros(3) if centre is None else centre, np.zeros(3) if velocity is None else velocity]).astype(np.float64)
    lines = [f"system {n} {sets} {threads}", " ".join([str(int(bits([eps])[0]))] + [str(int(w)) for w in frame.view(np.uint64)])]
    p, v, wire = bits(pos[:n]), bits(vel[:n]), mref.wire_labels(labels)
    for i in range(n):
        lines.append(" ".join(str(w) for w in (*p[i], *v[i, :3])) + f" {wire[i]}")
    return "\n".join(lines) + "\n"


def parse(lines, sets):
    system = np.zeros((), mref.SYSTEM_DTYPE)
    words = lines[0].split()
    for word, value in zip(mref.SYSTEM_WORDS[:6], words[:6]):
        system[word] = int(value)
    system["members"] = [int(w) for w in words[6:14]]
    system["mass"] = np.array([int(w) for w in words[14:22]], np.uint64).view(np.float64)
    out = np.zeros(sets * sets, mref.ENTRY_DTYPE)
    for t in range(sets * sets):
        words = lines[1 + t].split()
        out["pairs"][t] = int(words[0])
        out.view(np.uint64).reshape(sets * sets, 10)[t, 1:] = [int(w) for w in words[1:]]
    return system, out.reshape(sets, sets), lines[1 + sets * sets:]


def run_case(run, capacity, name, shapes):
    _, sets, _, eps, frame = next(c for c in mref.cases_of(capacity) if c[0] == name)
    P, V, counts = mref.gpu_inputs(capacity)
    L = mref.gpu_labels(capacity, name)
    centre, velocity = mref.gpu_frames(capacity, frame)
    refs = mref.gpu_reference(capacity, name)
    compared = 0
    for threads in shapes:
        text = "".join(command(P[s], V[s], n, L[s], sets, eps, None if centre is None else centre[s],
                               None if velocity is None else velocity[s], threads) for s, n in enumerate(counts))
        lines = run(text)
        for s in range(len(counts)):
            system, out, lines = parse(lines, sets)
            assert system.tobytes() == refs[s]["system"].tobytes(), (capacity, name, threads, s, system, refs[s]["system"])
            assert out.tobytes() == refs[s]["entries"].tobytes(), (capacity, name, threads, s)
            compared += 1
        assert not lines
    return compared


@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_driver_gives_the_references_bytes_for_every_workgroup_shape(driver, capacity):
    """Every case and system at 64, 128, 256 and 1024 threads: byte-equal to the reference, so the same bytes for every shape."""
    compared = sum(run_case(driver, capacity, name, THREADS) for name, *_ in mref.cases_of(capacity))
    assert compared == len(mref.CASES) * len(THREADS) * len(mref.counts_of(capacity))


def test_the_driver_gives_the_references_bytes_at_1024_bodies(driver):
    """Capacity 1024 (sets of up to 1024 bodies: sixteen blocks; eight sets with ragged blocks) at two shapes."""
    assert run_case(driver, 1024, "interleaved-1", (256, 1024)) > 0
    assert run_case(driver, 1024, "ranks-8-frame", (256,)) > 0
    assert run_case(driver, 1024, "contiguous-8-soft-frame", (1024,)) > 0


def test_the_sanitized_driver_gives_the_references_bytes(sanitized_driver):
    """The same arithmetic as a stand-alone program under the address and undefined-behaviour sanitizers: every case of capacity
    128 at two shapes."""
    for name, *_ in mref.cases_of(128):
        assert run_case(sanitized_driver, 128, name, (64, 256)) > 0


def test_the_driver_states_the_layout_and_the_limits(driver):
    lines = driver("layout\nlimits\n")
    assert [int(w) for w in lines[0].split()] == [80] + [mref.ENTRY_OFFSETS[w] for w in mref.ENTRY_WORDS]
    assert [int(w) for w in lines[1].split()] == [128] + [mref.SYSTEM_OFFSETS[w] for w in mref.SYSTEM_WORDS]
    assert [int(w) for w in lines[2].split()] == [8, 255, 64, 9, 64, 72]


def test_the_counting_sort_is_a_stable_argsort(driver, sanitized_driver):
    """The rank function of the math header -- ballots per chunk of 64, the prefix over the chunks, the slot -- against
    numpy.argsort(kind="stable") on random sets with bodies in no set, at sizes around the chunk and at 4096."""
    rng = np.random.default_rng(5)
    for run in (driver, sanitized_driver):
        for n in (0, 1, 63, 64, 65, 200, 1025, 4096):
            for sets in (1, 3, 8):
                sets_of = rng.integers(-1, sets, size=n)
                if n > 70:
                    sets_of[sets_of == sets - 1] = -1 if sets > 1 else 0            # an empty set among the others
                lines = run(f"sort {n} {sets}\n" + " ".join(str(a) for a in sets_of) + "\n")
                order, start = mref.stable_ranks(sets_of, sets)
                assert [int(w) for w in lines[0].split()] == order.tolist(), (n, sets)
                assert [int(w) for w in lines[1].split()] == start.tolist(), (n, sets)
                blocks = -(-np.diff(start) // 64)
                assert [int(w) for w in lines[2].split()] == np.concatenate([[0], np.cumsum(blocks)]).tolist(), (n, sets)
                chosen = sets_of[order]
                assert (np.diff(chosen) >= 0).all() and all((np.diff(order[chosen == a]) > 0).all() for a in range(sets))


# ---- independent checks of the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_reference_agrees_with_a_plain_unordered_pair_walk(capacity):
    """Every floating word within BOUND of its companion."""
    P, V, counts = mref.gpu_inputs(capacity)
    worst = 0.0
    for name, sets, _, eps, frame in mref.cases_of(capacity):
        L = mref.gpu_labels(capacity, name)
        centre, velocity = mref.gpu_frames(capacity, frame)
        for s, ref in enumerate(mref.gpu_reference(capacity, name)):
            plain = mref.plain_walk(P[s], V[s], counts[s], L[s], sets, eps, None if centre is None else centre[s],
                                    None if velocity is None else velocity[s])
            diff, scale = np.abs(plain - mref.floats_of(ref["entries"])), ref["absolute"]
            assert (diff[scale == 0.0] == 0.0).all(), (name, s)
            if (scale > 0.0).any():
                worst = max(worst, float((diff[scale > 0.0] / scale[scale > 0.0]).max()))
            assert (diff <= mref.BOUND * scale).all(), (name, s, worst)
    print(f"capacity {capacity}: plain walk within {worst:.3g} of the companions; BOUND {mref.BOUND:.3g}")


@pytest.mark.parametrize("capacity", (64, 128, 256))
def test_the_reference_obeys_newtons_third_law_within_the_bound(capacity):
    """U_ab against U_ba, F_ab + F_ba against 0 and F_aa against 0, each within BOUND of the two companions' sum; the
    identities of the integers exactly."""
    for name, sets, *_ in mref.cases_of(capacity):
        for s, ref in enumerate(mref.gpu_reference(capacity, name)):
            e, absolute, system = ref["entries"], ref["absolute"], ref["system"]
            for a in range(sets):
                assert (np.abs(e["force"][a, a]) <= mref.BOUND * absolute[a, a, 1:4]).all(), (name, s, a)
                for b in range(sets):
                    scale = absolute[a, b] + absolute[b, a]
                    assert abs(e["potential"][a, b] - e["potential"][b, a]) <= mref.BOUND * scale[0], (name, s, a, b)
                    assert (np.abs(e["force"][a, b] + e["force"][b, a]) <= mref.BOUND * scale[1:4]).all(), (name, s, a, b)
                    assert e["pairs"][a, b] == int(system["members"][a]) * int(system["members"][b]) - (a == b) * int(system["members"][a])
            assert int(system["pairs"]) == int(e["pairs"].sum())
            assert int(system["selected"]) == int(system["members"].sum())


def test_the_closed_form_holds_bit_for_bit_in_the_reference_and_in_the_driver(driver):
    """Set 0 is one body of mass 4 at the origin, set 1 bodies of power-of-two mass at +-2^k on the axes, softening 0: every
    operation of the two cross entries is exact, so they are the rational closed form, bit for bit."""
    pos, vel, labels, centre, velocity = mref.closed_form_state()
    want = mref.closed_form()
    ref = mref.reference(pos, vel, len(pos), labels, 2, 0.0, centre, velocity)
    system, out, rest = parse(driver(command(pos, vel, len(pos), labels, 2, 0.0, centre, velocity, 128)), 2)
    assert not rest and system.tobytes() == ref["system"].tobytes() and out.tobytes() == ref["entries"].tobytes()
    for (a, b), words in want.items():
        assert mref.floats_of(ref["entries"])[a, b].tobytes() == words.tobytes(), (a, b)
        assert mref.floats_of(out)[a, b].tobytes() == words.tobytes(), (a, b)
    assert want[(0, 1)][0] == want[(1, 0)][0] and (want[(0, 1)][1:4] == -want[(1, 0)][1:4]).all()
    assert int(system["members"][0]) == 1 and int(system["members"][1]) == 36 and float(system["mass"][0]) == 4.0


def test_the_inputs_hold_what_they_should():
    for capacity in mref.CAPACITIES:
        P, V, counts = mref.gpu_inputs(capacity)
        assert max(counts) == capacity and (capacity == 4096 or counts[:4] == [0, 1, 2, 3])
        for s, n in enumerate(counts):
            if n >= 63:
                assert np.isnan(P[s, 5, 1]) and np.isinf(V[s, 9, 0]) and (P[s, 11, :3] == P[s, 12, :3]).all()
    assert mref.counts_of(4096) == [4096, 1025] and [c[1] for c in mref.LARGE_CASES] == [2, 8]
    assert (mref.gpu_labels(4096, "large-2")[1] == -1).all() and (mref.gpu_labels(4096, "large-8")[0] == -1).all()
    assert {c[1] for c in mref.CASES} >= {1, 2, 3, 8} and {c[2] for c in mref.CASES} == {"interleaved", "contiguous", "ranks", "none"}
    assert {c[3] > 0 for c in mref.CASES} == {False, True} and {c[4] for c in mref.CASES} == {False, True}
    s = mref.counts_of(256).index(256)
    ranks = mref.gpu_labels(256, "ranks-8-frame")[s]
    assert [int((ranks[:256] == a).sum()) for a in range(5)] == list(mref.RANK_SIZES)
    ref = mref.gpu_reference(256, "interleaved-2-frame")[s]
    assert int(ref["system"]["unmeasured"]) == 2 and int(ref["system"]["coincident"]) == 2      # (11, 12) and (12, 11)
    assert int(mref.gpu_reference(256, "interleaved-3-soft")[s]["system"]["coincident"]) == 0
    # widened fp32 words cannot overflow fp64 through the products of the header
    big = np.float64(np.finfo(np.float32).max)
    assert np.isfinite(4096.0 * (2.0 * big) * 4096.0 * big * 2.0 ** 575 * (2.0 * big))


def test_the_spread_of_the_reference_under_moved_roots_and_quotients_is_within_the_constant():
    """BOUND, measured again: the largest error measure of the reference against itself when every root and quotient is moved
    by up to one ulp at random, over all cases of the three smaller capacities; no integer and no system record moves."""
    spread, same = mref.jitter_spread()
    print(f"spread {spread:.3g}; SPREAD {mref.SPREAD:.3g}; BOUND {mref.BOUND:.3g}")
    assert same and 0.0 < spread <= mref.SPREAD and mref.BOUND == 4.0 * mref.SPREAD


# ---- the derived quantities ----------------------------------------------------------------------------------------------------
def test_the_derived_quantities_on_hand_made_records():
    from n_body_problem_amd import batch
    systems = np.zeros(2, batch.MUTUAL_GRAVITY_SYSTEM_DTYPE)
    systems["sets"], systems["selected"] = 3, [5, 2]
    systems["members"][:, :3] = [[2, 3, 0], [2, 0, 0]]
    systems["mass"][:, :3] = [[2.0, 4.0, 0.0], [2.0, 0.0, 0.0]]
    entries = np.zeros((2, 3, 3), batch.MUTUAL_GRAVITY_ENTRY_DTYPE)
    entries["potential"][0] = [[-6.0, -8.0, 0.0], [-8.0, -10.0, 0.0], [0.0, 0.0, 0.0]]
    entries["potential"][1, 0, 0] = -4.0
    entries["force"][0, 0, 1], entries["force"][0, 1, 0] = (1.0, 2.0, -4.0), (-1.0, -2.0, 4.0)
    entries["torque"][0, 0, 1] = (0.5, 0.0, 0.25)
    entries["power"][0, 0, 1] = 3.0
    res = batch.MutualGravityResult(systems, entries, 3)
    assert res.sets == 3 and res.members.shape == (2, 3) and res.potential.shape == (2, 3, 3) and res.force.shape == (2, 3, 3, 3)
    assert res.interaction_energy(0, 1)[0] == -8.0 and np.isnan(res.interaction_energy(0, 1)[1]) and np.isnan(res.interaction_energy(0, 2)[0])
    assert res.self_energy(0).tolist() == [-3.0, -2.0] and np.isnan(res.self_energy(2)).all()
    assert res.total_potential_energy().tolist() == [-16.0, -2.0]
    assert res.force_on(0)[0].tolist() == [1.0, 2.0, -4.0] and res.force_on(1)[0].tolist() == [-1.0, -2.0, 4.0]
    assert np.isnan(res.force_on(2)).all() and np.isnan(res.force_on(1)[1]).all()
    assert res.torque_on(0)[0].tolist() == [0.5, 0.0, 0.25] and res.power_into(0)[0] == 3.0 and res.power_into(0)[1] == 0.0
    assert res.acceleration_of(0)[0].tolist() == [0.5, 1.0, -2.0] and res.acceleration_of(1)[0].tolist() == [-0.25, -0.5, 1.0]
    centres, velocities = np.zeros((2, 3, 3)), np.zeros((2, 3, 3))
    centres[:, 1, 0], velocities[:, 1, 1] = 4.0, 3.0
    orbit = res.two_body_energy(0, 1, centres, velocities)
    assert orbit[0] == 0.5 * (8.0 / 6.0) * 9.0 - 2.0 and np.isnan(orbit[1])
    a, b = np.array([[True, False, False]]), np.array([[False, False, True]])
    assert batch.MutualGravityResult.labels_from_masks(a, b).tolist() == [[0, -1, 1]]
    with pytest.raises(ValueError):
        batch.MutualGravityResult.labels_from_masks(a, a)
    with pytest.raises(ValueError):
        res.interaction_energy(0, 0)
    with pytest.raises(ValueError):
        res.force_on(3)
    lean = batch.MutualGravityResult(systems, None, 3)
    assert lean.potential is None and lean.mass[0].tolist() == [2.0, 4.0, 0.0]
    with pytest.raises(ValueError):
        lean.total_potential_energy()
    assert "MutualGravityResult(sets=3" in repr(res)
