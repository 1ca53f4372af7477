"""CPU-only: which force kernel a configuration runs and with what launch shape (csrc/nbody_launch_choice.h), printed by
tests/launch_choice_driver.cpp (g++) over the whole domain and compared, entry for entry, with tests/golden/launch_choice.json.
That table was recorded from the dispatch code the header replaced (see tests/golden/README.md): a change to it must be
deliberate.  The anchors are the kernel names the profiles in the tree recorded on hardware; the properties are the conditions
the kernels put on their launch shape.  The finish choice (which kernel turns the partial sums into velocities and positions)
is compared over its whole domain with the rule its call sites held before the header did; tests/test_finish_bits_cpu.py ties
the GPU cases of the finish tests to it."""
import itertools
import json
import os
import random
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")


def domain():
    """{section: [command]}: every input the golden table lists."""
    d = {}
    sym = [(L, 1) for L in range(256, 4097, 256)] + [(2048, K) for K in (2, 4, 8)]   # strips exist with 2048-body splits only
    d["sym"] = [f"sym {L} {eps} {pps} {packed} {K}" for L, K in sym for eps in (0, 1) for pps in (0, 1) for packed in range(4)]
    d["force"] = [f"force {b} {L} {eps} {pps}" for b in (1, 2, 4, 8, -4, 40, 41)
                  for L in list(range(64, 577, 64)) + [1024, 8192] for eps in (0, 1) for pps in (0, 1)]
    # blocks of 1024 rows x splits around 10 x 256 (splits of up to 512 columns) and 4 x 256 (longer ones)
    grid = [(rows, splits) for rows in (1024, 20225, 32768, 1 << 20) for splits in (1, 32, 64, 79, 80, 128)]
    d["pick"] = [f"pick {s} {L} {rows} {splits} 256 {em}" for s in (0, 1, 41) for L in (256, 320, 512, 576, 8192)
                 for em in (0, 1) for rows, splits in grid]
    d["packed"] = [f"packed {rpl} {em}" for rpl in (0, 1, 2, 4, 8, -4, 40, 41) for em in (0, 1)]
    rng = random.Random(20225)
    sizes = [1, 255, 256, 257, 4096, 20000, 20225, 32767, 32768, 65535, 65536, 131071, 131072, (1 << 20) - 1, 1 << 20, 1 << 21,
             1 << 22, 1 << 23, 1 << 30] + [int(2 ** rng.uniform(0, 24)) for _ in range(200)]
    d["split"] = [f"split {n}" for n in sizes]
    d["graph"] = [f"graph {g} {mode} {parts} {n} {L} {eps} {pps} {rpl} 1" for g in (-1, 0, 1) for mode in (0, 1)
                  for parts in (0, 1, 2) for n in (20225, 32768, 32769) for L in (256, 512, 1024) for eps in (0, 1)
                  for pps in (0, 1) for rpl in (0, 4)]
    return d


FIELDS = {"sym": ("tiles", "threads", "lds", "serves_diag", "reads_flags", "diag", "diag_threads", "diag_lds"),
          "force": ("kernel", "threads", "rows_per_block"), "pick": ("blocking", "own_split_mass"), "packed": ("packed",),
          "split": ("one_sided", "pair_once"), "graph": ("replay",)}


def parse(section, line):
    return {k: v if k in ("tiles", "diag", "kernel") else int(v) for k, v in zip(FIELDS[section], line.split("|"), strict=True)}


def run_domain(run):
    """{section: {command: entry}} of the program `run` (commands -> stdout)."""
    d = domain()
    out = {}
    for section, commands in d.items():
        lines = run(commands).splitlines()
        assert len(lines) == len(commands), section
        out[section] = {c: parse(section, line) for c, line in zip(commands, lines)}
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_choice") / "launch_choice_driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "launch_choice_driver.cpp"),
           "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout
    return run


@pytest.fixture(scope="module")
def golden(golden_dir):
    """{section: {command: entry}} of the file, which keeps each section's distinct output lines once ("outcomes") and, in the
    order of domain(), the number of the line each input gets ("index")."""
    with open(os.path.join(golden_dir, "launch_choice.json")) as f:
        table = json.load(f)
    d = domain()
    assert table.keys() == d.keys()
    out = {}
    for section, commands in d.items():
        index = [int(i) for row in table[section]["index"] for i in row.split()]
        assert len(index) == len(commands), section
        out[section] = {c: parse(section, table[section]["outcomes"][i]) for c, i in zip(commands, index)}
    return out


def test_the_domain_is_complete():
    d = domain()
    assert len(d["sym"]) == 304 and len(set(d["sym"])) == 304
    assert len(d["force"]) == 7 * 11 * 4
    picks = [[int(v) for v in c.split()[1:]] for c in d["pick"]]
    blocks4 = lambda rows, splits: -(-rows // 1024) * splits  # noqa: E731
    for short, want in ((True, 10 * 256), (False, 4 * 256)):    # both sides of each threshold, and the threshold itself
        seen = {(blocks4(rows, splits) > want) - (blocks4(rows, splits) < want)
                for s, L, rows, splits, cu, em in picks if s == 0 and (L <= 512) == short}
        assert seen == {-1, 0, 1}, (short, seen)


def test_every_choice_is_the_recorded_one(driver, golden):
    got = run_domain(driver)
    assert got.keys() == golden.keys()
    for section in got:
        assert got[section].keys() == golden[section].keys(), section
        assert {c: (got[section][c], golden[section][c]) for c in got[section] if got[section][c] != golden[section][c]} == {}, section


def test_anchors_from_measured_runs(golden):
    sym, force, pick, split = golden["sym"], golden["force"], golden["pick"], golden["split"]
    for K in (2, 4):   # profiles/r04_kernel_stats_pair_once.csv, r04_diagonal_tiles.txt
        e = sym[f"sym 2048 1 0 3 {K}"]
        assert (e["tiles"], e["diag"]) == ("force_sym_kernel<4, false, 2, 1>", "force_sym_general_kernel<4, true, false, false>")
    e = sym["sym 1024 1 0 3 1"]   # r04_diagonal_tiles.txt
    assert (e["tiles"], e["diag"]) == ("force_sym_kernel<2, false, 2, 1>", "force_sym_general_kernel<2, true, false, false>")
    for L, name in ((256, "force_sym_quarter_kernel<0, 1>"), (512, "force_sym_quarter_kernel<0, 2>")):
        e = sym[f"sym {L} 1 0 3 1"]   # r04_kernel_stats_reference_size.csv
        assert (e["tiles"], e["diag"], e["serves_diag"], e["reads_flags"]) == (name, "none", 1, 0)
    # one-sided, r04_kernel_stats_one_sided.csv: N = 2^20
    n = 1 << 20
    L = split[f"split {n}"]["one_sided"]
    assert L == 8192 and pick[f"pick 0 {L} {n} {n // L} 256 1"] == dict(blocking=4, own_split_mass=0)
    assert force[f"force 4 {L} 1 0"]["kernel"] == "force_kernel_r4pk<false, false>"
    # r04_pmc_small_n_one_sided.txt: N = 20 225
    L = split["split 20225"]["one_sided"]
    assert L == 320 and pick[f"pick 0 {L} 20225 {-(-20225 // L)} 256 1"] == dict(blocking=41, own_split_mass=1)
    assert force[f"force 41 {L} 1 0"]["kernel"] == "force_kernel_r4pk_w1<false, 5, false>"


def template_args(name):
    kernel, args = re.fullmatch(r"(\w+)<(.*)>", name).groups()
    return kernel, [{"true": 1, "false": 0}.get(a, a) for a in args.split(", ")]


def test_launch_shapes_fit_their_kernels(golden):
    for command, e in golden["sym"].items():
        L, eps, pps, packed, strip_len = (int(v) for v in command.split()[1:])
        assert (e["diag"] == "none") == bool(e["serves_diag"]), command
        for name, threads, lds in ((e["tiles"], e["threads"], e["lds"]), (e["diag"], e["diag_threads"], e["diag_lds"])):
            if name == "none":
                continue
            kernel, t = template_args(name)
            t = [int(v) for v in t]
            waves = 4 * t[1] if kernel == "force_sym_quarter_kernel" else t[0]   # <LOOP, NH>: four waves per 256 bodies
            assert threads == 64 * waves and lds <= 160 << 10, (command, name)
            if kernel == "force_sym_quarter_kernel":
                assert 256 * t[1] == L and lds == 0 and (eps or t[0] == 2), (command, name)   # LOOP 2: the guarded loop
            elif kernel == "force_sym_kernel":   # <W, GUARD, ROWS8, MODE>
                eight_rows = t[2] in (1, 2, 3)
                assert waves * (512 if eight_rows else 256) <= L, (command, name)
                assert strip_len == 1 or t[3] != 0, (command, name)
                assert eps or t[1], (command, name)
            else:                                # force_sym_general_kernel<W, DIAG, GUARD, PPS>
                assert eps or t[2], (command, name)
    for command, e in golden["force"].items():
        blocking, L, eps, pps = (int(v) for v in command.split()[1:])
        kernel, t = template_args(e["kernel"])
        guard = t[1] if kernel == "force_kernel" else t[0]
        assert eps or guard, (command, e)
        assert e["threads"] in (64, 256) and e["rows_per_block"] % e["threads"] == 0, (command, e)


def test_every_choice_has_a_table_entry(golden):
    """Each instantiation is named once, as ROW(kernel, template arguments), in the launchers' tables."""
    tables = ""
    for source in ("nbody_symmetric.hip", "nbody_kernels.hip"):
        with open(os.path.join(CSRC, source)) as f:
            text = f.read()
        # x_ROWS_y(W): the rows that differ in one argument only, spelled out for each W the table asks for
        for macro, arg, body in re.findall(r"^#define (\w+_ROWS_\w+)\((\w+)\) \\\n((?:.*\\\n)*.*)\n", text, re.M):
            for w in re.findall(macro + r"\((\d)\)", text):
                tables += re.sub(r"\b" + arg + r"\b", w, body)
        tables += text
    names = {e[k] for e in golden["sym"].values() for k in ("tiles", "diag")} | {e["kernel"] for e in golden["force"].values()}
    names.discard("none")
    assert len(names) > 40
    for name in sorted(names):
        kernel, args = re.fullmatch(r"(\w+)<(.*)>", name).groups()
        assert f"ROW({kernel}, {args})" in tables, name


def finish_rule(op, pair_once, whole, one_part_unsummed, n_splits, strip_len, row_count):
    """The decisions nbody_update, nbody_kdk_prepare, nbody_kdk_kick and the update launchers made, each at its own place."""
    if pair_once and whole and one_part_unsummed and n_splits <= 320 and strip_len == 1:      # one finishing kernel
        return f"sym_finish_update_kernel<{dict(update=0, kick=1, prepare=2)[op]}>|256|0"
    if op == "update":
        block = 64 if row_count < 256 * 256 else 256
        return f"{'update_sym_kernel' if pair_once else 'update_kernel'}<{block}>|{block}|0"
    return f"kdk_kick_kernel<{1 if op == 'kick' else 0}>|256|{int(bool(pair_once))}"


def test_the_finish_choice_is_the_rule_its_call_sites_held(driver):
    domain = list(itertools.product(("update", "prepare", "kick"), (0, 1), (0, 1), (0, 1), (1, 20, 319, 320, 321, 4096), (1, 2, 4, 8),
                                    (1, 64, 1000, 65535, 65536, 65537, 1 << 20)))
    lines = driver(["choice " + " ".join(str(v) for v in d) for d in domain]).splitlines()
    assert len(lines) == len(domain)
    assert {d: (got, finish_rule(*d)) for d, got in zip(domain, lines) if got != finish_rule(*d)} == {}
    assert len(set(lines)) == 11          # two block sizes of two update kernels, three modes fused, two kicks with and without the combination
