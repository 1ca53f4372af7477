"""CPU-only: which kernel family a batch handle runs, with what launch shape, and what nbody_batch_evolve_on refuses
(csrc/nbody_batch_choice.h), printed by tests/batch_choice_driver.cpp (g++, no HIP) over the whole domain and compared, entry
for entry, with tests/golden/batch_choice.json.  That table was recorded from the two if / else chains the header replaced (see
tests/golden/README.md): a change to it must be deliberate.  The properties are the conditions the kernels put on their launch
shape and the invariants the chains held by the order of their early returns."""
import itertools
import json
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
KICK_DRIFT, KDK, HERMITE = 0, 1, 2
STOP, MERGE = 0, 1
REFUSE, REMOVE = 0, 1
CAPACITIES = (1, 64, 65, 128, 129, 256, 257, 4096)
SOFTENINGS = ("0", "1e-9", "0.01")
FAMILIES = ("step", "step_massive", "hermite", "hermite_massive", "adaptive", "stop", "merge", "radii", "adaptive_massive", "fate")
FIELDS = ("family", "rpl", "threads", "guard", "lds", "refusal")


def settings():
    """Every combination of the settings: (integrator, massive_set, radii_set, collision radius, escape radius, collision
    action, tracer action)."""
    return list(itertools.product((KICK_DRIFT, KDK, HERMITE), (0, 1), (0, 1), ("0", "0.05"), ("0", "10"), (STOP, MERGE),
                                  (REFUSE, REMOVE)))


def domain():
    """{section: [command]}: every input the golden table lists."""
    return {call: [f"{call} {' '.join(str(v) for v in s)} {cap} {eps}" for s in settings() for cap in CAPACITIES for eps in SOFTENINGS]
            for call in ("step", "evolve")}


def parse(line):
    e = dict(zip(FIELDS, line.split("|"), strict=True))
    return {k: v if k in ("family", "refusal") else int(v) for k, v in e.items()}


def inputs(command):
    call, integrator, massive, radii, rc, re, action, tracers, cap, eps = command.split()
    return dict(call=call, integrator=int(integrator), massive=int(massive), radii=int(radii), rc=float(rc), re=float(re),
                action=int(action), tracers=int(tracers), cap=int(cap), eps=float(eps))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_choice") / "batch_choice_driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "batch_choice_driver.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == len(commands)
        return lines
    return run


@pytest.fixture(scope="module")
def golden(golden_dir):
    """{section: {command: entry}} of the file, which keeps each section's distinct output lines once ("outcomes") and, in the
    order of domain(), the number of the line each input gets ("index")."""
    with open(os.path.join(golden_dir, "batch_choice.json")) as f:
        table = json.load(f)
    d = domain()
    assert table.keys() == d.keys()
    out = {}
    for section, commands in d.items():
        index = [int(i) for row in table[section]["index"] for i in row.split()]
        assert len(index) == len(commands), section
        out[section] = {c: parse(table[section]["outcomes"][i]) for c, i in zip(commands, index)}
    return out


def test_the_domain_is_complete(golden):
    d = domain()
    for section in ("step", "evolve"):
        assert len(d[section]) == len(set(d[section])) == 3 * 2 ** 6 * 8 * 3
    ran = {e["family"] for g in golden.values() for e in g.values()} - {"none"}
    assert ran == set(FAMILIES)                                   # every family is chosen somewhere
    for fam in FAMILIES:                                          # at every <rows per lane, guard>
        assert {(e["rpl"], e["guard"]) for g in golden.values() for e in g.values() if e["family"] == fam} == \
            {(r, g) for r in (1, 2, 4) for g in (0, 1)}, fam
    assert len({e["refusal"] for e in golden["evolve"].values()}) == 5 and {e["refusal"] for e in golden["step"].values()} == {"none"}


def test_every_choice_is_the_recorded_one(driver, golden):
    for section, commands in domain().items():
        got = {c: parse(line) for c, line in zip(commands, driver(commands))}
        assert got.keys() == golden[section].keys(), section
        assert {c: (got[c], golden[section][c]) for c in got if got[c] != golden[section][c]} == {}, section


def test_launch_shapes_fit_their_kernels(golden):
    for section in golden:
        for command, e in golden[section].items():
            i = inputs(command)
            if e["refusal"] != "none":
                assert (e["family"], e["rpl"], e["threads"], e["lds"]) == ("none", 0, 0, 0), command
                continue
            assert e["rpl"] in (1, 2, 4) and e["threads"] * e["rpl"] >= i["cap"], command     # every body has a row
            assert e["threads"] % 64 == 0 and 0 < e["threads"] <= 1024, command               # whole waves, one workgroup
            per_body = 16 if e["family"] in ("step", "step_massive") else 32                  # float4: positions (and velocities)
            assert e["lds"] == per_body * i["cap"] and e["lds"] <= 160 << 10, command
            assert e["guard"] == (i["eps"] == 0.0), command


def test_families_go_with_their_settings(golden):
    for section in golden:
        for command, e in golden[section].items():
            i = inputs(command)
            fam = e["family"]
            if fam == "none":
                continue
            conditions = i["rc"] > 0 or i["re"] > 0 or i["radii"]
            assert ("massive" in fam or fam == "fate") == bool(i["massive"]), command
            assert (fam in ("step", "step_massive", "hermite", "hermite_massive")) == (section == "step"), command
            assert (fam in ("hermite", "hermite_massive")) == (section == "step" and i["integrator"] == HERMITE), command
            if section == "evolve":
                assert i["integrator"] == HERMITE, command
                assert (fam == "fate") == bool(i["massive"] and conditions and i["tracers"] == REMOVE), command
                assert (fam == "adaptive_massive") == bool(i["massive"] and not conditions), command   # never with conditions
                assert (fam == "adaptive") == (not i["massive"] and not conditions), command
                assert (fam == "radii") == bool(i["radii"] and not i["massive"]), command
                assert (fam == "merge") == bool(i["rc"] > 0 and i["action"] == MERGE and not i["massive"]), command
                assert not (i["radii"] and i["rc"] > 0), command


def test_refusals_say_what_the_gpu_tests_look_for(golden):
    """The substrings tests/test_batch_*_gpu.py match, each on the combinations it belongs to, in the order the library looks."""
    seen = set()
    for command, e in golden["evolve"].items():
        i = inputs(command)
        conditions = i["rc"] > 0 or i["re"] > 0 or i["radii"]
        collisions = i["rc"] > 0 or i["radii"]
        if i["integrator"] != HERMITE:
            want = "NBODY_INTEGRATOR_HERMITE"
        elif i["radii"] and i["rc"] > 0:
            want = "radii and collision_radius are both set"
        elif i["massive"] and conditions and i["tracers"] == REMOVE and i["action"] == MERGE and collisions:
            want = "MERGE together with massive counts"
        elif i["massive"] and conditions and i["tracers"] == REFUSE:
            want = "massive counts are set together with a stopping condition"
        else:
            want = None
        if want is None:
            assert e["refusal"] == "none", command
        else:
            status, message = e["refusal"].split(":", 1)
            assert int(status) == -1 and want in message and message.startswith("nbody_batch_evolve: "), command   # NBODY_ERR_INVALID
            seen.add(want)
    assert len(seen) == 4


def test_modes(driver):
    """BatchMode, which the calls that read stops, mergers and fates share with nbody_batch_evolve_on."""
    cfgs = [s[1:] for s in settings() if s[0] == HERMITE]
    lines = driver(["mode " + " ".join(str(v) for v in c) for c in cfgs])
    for (massive, radii, rc, re, action, tracers), line in zip(cfgs, lines):
        collisions = float(rc) > 0 or bool(radii)
        stopping = collisions or float(re) > 0
        want = (collisions, stopping, action == MERGE and collisions, bool(massive) and tracers == REMOVE and stopping)
        assert tuple(bool(int(v)) for v in line.split("|")) == want, (massive, radii, rc, re, action, tracers)


def test_numeric_arguments(driver):
    """args levels n_intervals dt_max eta eta_start softening: the message of the first bad one, in the library's order."""
    levels = "nbody_batch_evolve: levels outside [0, NBODY_BATCH_EVOLVE_MAX_LEVELS = 20]"
    intervals = "nbody_batch_evolve: n_intervals < 0 or n_intervals x 2^levels >= 2^62"
    dt_max = "nbody_batch_evolve: dt_max must be finite and positive"
    eta = "nbody_batch_evolve: eta and eta_start must be finite and positive"
    softening = ("nbody_batch_evolve: softening must be finite, 0 or >= NBODY_MIN_SOFTENING (1e-9): "
                 "0 < softening < 1e-9 would overflow fp32 (eps^-3 x mass of the self pair)")
    cases = [("12 4 0.01 0.01 0.01 0.01", "none"), ("0 0 1 1 1 0", "none"), ("20 %d 0.01 0.01 0.01 1e-9" % ((1 << 42) - 1), "none"),
             ("-1 4 0.01 0.01 0.01 0.01", levels), ("21 4 0.01 0.01 0.01 0.01", levels),
             ("12 -1 0.01 0.01 0.01 0.01", intervals), ("20 %d 0.01 0.01 0.01 0.01" % (1 << 42), intervals),
             ("0 %d 0.01 0.01 0.01 0.01" % ((1 << 62) - 1), "none"),
             ("12 4 0 0.01 0.01 0.01", dt_max), ("12 4 -1 0.01 0.01 0.01", dt_max), ("12 4 inf 0.01 0.01 0.01", dt_max),
             ("12 4 nan 0.01 0.01 0.01", dt_max),
             ("12 4 0.01 0 0.01 0.01", eta), ("12 4 0.01 nan 0.01 0.01", eta), ("12 4 0.01 0.01 0 0.01", eta),
             ("12 4 0.01 0.01 inf 0.01", eta),
             ("12 4 0.01 0.01 0.01 1e-10", softening), ("12 4 0.01 0.01 0.01 -1", softening), ("12 4 0.01 0.01 0.01 inf", softening),
             ("12 4 0.01 0.01 0.01 nan", softening),
             # the first bad argument speaks
             ("21 -1 0 0 0 -1", levels), ("12 -1 0 0 0 -1", intervals), ("12 4 0 0 0 -1", dt_max), ("12 4 0.01 0 0 -1", eta)]
    lines = driver(["args " + c for c, _ in cases])
    assert {c: (got, want) for (c, want), got in zip(cases, lines) if got != want} == {}


def test_the_header_needs_no_hip():
    """g++ reads the driver, and through it the header, with no HIP include path."""
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + CSRC,
                          os.path.join(ROOT, "tests", "batch_choice_driver.cpp")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    with open(os.path.join(CSRC, "nbody_batch_choice.h")) as f:
        includes = [line.split()[1] for line in f if line.startswith("#include")]
    assert includes == ['"../../include/nbody.h"', "<cmath>", "<cstddef>", "<cstdint>"]
