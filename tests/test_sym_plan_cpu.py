"""CPU-only: the launch plan of the pair-once mode (csrc/nbody_sym_plan.h) -- which strips and diagonal tiles a force call
launches, in which order, in which summation parts -- built by tests/sym_plan_driver.cpp with g++ and checked here: every
tile exactly once, the row-side slots, the parts' split ranges and partial-sum regions, column ranges and their complements,
and the launch order against tests/golden/sym_plan_digests.json."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
BUDGET = 5 << 30   # NBODY_PARTIAL_SUM_BUDGET_BYTES


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sym_plan") / "sym_plan_driver")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "sym_plan_driver.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout
    return run


class Case:
    """A context's geometry as nbody_set_force_mode sets it up, and the column range of one force call."""

    def __init__(self, n_total, split_len, strip_len, row_lo=0, row_count=None, first=0, count=None, complement=False,
                 sum_parts=0):
        self.n, self.L, self.SL = n_total, split_len, strip_len
        self.S = S = -(-n_total // split_len)
        self.row_lo, self.row_count = row_lo, n_total - row_lo if row_count is None else row_count
        self.gs = max(1, -(-S // 8))
        self.own_lo, self.own_hi = row_lo // split_len, -(-(row_lo + self.row_count) // split_len)
        self.group_lo = self.own_lo // self.gs
        self.group_count = -(-self.own_hi // self.gs) - self.group_lo
        self.first, self.count = first, S if count is None else count
        self.complement, self.sum_parts = complement, sum_parts

    def command(self):
        return " ".join(str(v) for v in ("plan", self.n, self.L, self.S, self.SL, self.row_lo, self.row_count, self.gs,
                                         self.group_lo, self.group_count, self.first, self.count, int(self.complement),
                                         self.sum_parts))

    def with_columns(self, first, count, complement=False):
        return Case(self.n, self.L, self.SL, self.row_lo, self.row_count, first, count, complement, self.sum_parts)

    def selected(self, C):
        return ((C >= self.first) & (C < self.first + self.count)) != self.complement


def parse_plans(text):
    """[(text of the plan, {"K", "row_entries", "col_entries", "slots", "parts": [...]})] in the order of the commands."""
    lines = text.splitlines()
    plans, i = [], 0
    while i < len(lines):
        head = lines[i].split()
        assert head[0] == "plan", lines[i]
        K = int(head[1])
        plan = dict(K=K, row_entries=int(head[2]), col_entries=int(head[3]), slots=int(head[4]), parts=[])
        for p in range(K):
            f = [int(v) for v in lines[i + 1 + 3 * p].split()[1:]]
            strips = np.array(lines[i + 2 + 3 * p].split()[1:], dtype=np.int64).reshape(-1, 4)
            diag = np.array(lines[i + 3 + 3 * p].split()[1:], dtype=np.int64).reshape(-1, 2)
            plan["parts"].append(dict(g0=f[0], g1=f[1], split_lo=f[2], split_hi=f[3], b0=f[4], rows=f[5], row_off=f[6],
                                      col_off=f[7], strips=strips, diag=diag))
        plans.append(("\n".join(lines[i:i + 1 + 3 * K]), plan))
        i += 1 + 3 * K
    return plans


def rows_side(R, C, S):
    """sharded_harness.sym_rows_side over arrays."""
    d = (C - R) % S
    lo = np.minimum(R, C)
    return np.where(2 * d == S, ((lo & 1) == 0) == (R == lo), (d != 0) & (2 * d < S))


def row_slot(R, C, S, K):
    j = C // K - ((R + 1) % S) // K
    return np.where(j < 0, j + S // K, j) + 1


def tile_sets(case, plan):
    """(sorted keys R * S + C of the off-diagonal tiles the strips cover, sorted diagonal splits)"""
    S, SL = case.S, case.SL
    strips = np.concatenate([p["strips"] for p in plan["parts"]])
    diag_strip = strips[:, 0] == strips[:, 1]
    if SL == 1:
        assert not diag_strip.any()
        diags = np.concatenate([p["diag"] for p in plan["parts"]])
        assert (diags[:, 0] == diags[:, 1]).all()
        diags = diags[:, 0]
    else:
        assert all(len(p["diag"]) == 0 for p in plan["parts"])
        assert (strips[diag_strip, 2:] == [1, 0]).all()   # {R, R, 1, 0}
        diags = strips[diag_strip, 0]
    strips = strips[~diag_strip]
    R, C0, n = strips[:, 0], strips[:, 1], strips[:, 2]
    assert (n >= 1).all() and (n <= SL).all()
    assert (C0 // SL == (C0 + n - 1) // SL).all()                # one absolute block per strip
    rr = np.repeat(R, n)
    cc = np.repeat(C0, n) + (np.arange(len(rr)) - np.repeat(np.cumsum(n) - n, n))
    keys = np.sort(rr * S + cc)
    assert (np.diff(keys) > 0).all(), "a tile listed twice"
    diags = np.sort(diags)
    assert (np.diff(diags) > 0).all(), "a diagonal tile listed twice"
    return keys, diags


def check_plan(case, plan):
    S, L, SL = case.S, case.L, case.SL
    assert plan["slots"] == (S // 2 + 1 if SL == 1 else S // (2 * SL) + 3)
    # exactly the pairs (R owned, C selected, R the row side), and every owned, selected diagonal
    keys, diags = tile_sets(case, plan)
    R, C = np.meshgrid(np.arange(case.own_lo, case.own_hi), np.arange(S), indexing="ij")
    want = np.sort((R * S + C)[case.selected(C) & rows_side(R, C, S)])
    assert np.array_equal(keys, want)
    own = np.arange(case.own_lo, case.own_hi)
    assert np.array_equal(diags, own[case.selected(own)])
    # parts: the owned splits in order, their rows, their slots and their partial-sum regions
    parts = plan["parts"]
    assert parts[0]["split_lo"] == case.own_lo and parts[-1]["split_hi"] == case.own_hi
    regions = []
    for p, q in zip(parts, parts[1:]):
        assert p["split_hi"] == q["split_lo"] and p["g1"] == q["g0"]
    for p in parts:
        assert p["split_lo"] == max(case.own_lo, p["g0"] * case.gs) and p["split_hi"] == min(case.own_hi, p["g1"] * case.gs)
        assert p["b0"] == p["split_lo"] * L - case.row_lo
        assert p["rows"] == min(p["split_hi"] * L, case.row_lo + case.row_count) - p["split_lo"] * L
        s = p["strips"]
        if len(s):
            assert ((s[:, 0] >= p["split_lo"]) & (s[:, 0] < p["split_hi"])).all()
            off = s[:, 0] != s[:, 1]
            assert (s[off, 3] == row_slot(s[off, 0], s[off, 1], S, SL)).all()
            assert ((s[:, 3] >= 0) & (s[:, 3] < plan["slots"])).all()
            assert len(np.unique(s[:, 0] * plan["slots"] + s[:, 3])) == len(s)    # one strip per (row split, slot)
        if len(p["diag"]):
            assert ((p["diag"][:, 0] >= p["split_lo"]) & (p["diag"][:, 0] < p["split_hi"])).all()
        rows = (p["row_off"], p["row_off"] + plan["slots"] * p["rows"])
        cols = (p["col_off"], p["col_off"] + (p["split_hi"] - p["split_lo"]) * (S // 2) * L)
        assert rows[1] <= plan["row_entries"] and cols[1] <= plan["col_entries"]
        regions.append((rows, cols))
    K = plan["K"]
    disjoint = lambda a, b: a[1] <= b[0] or b[1] <= a[0] or a[0] == a[1] or b[0] == b[1]  # noqa: E731
    for i in range(K):
        for j in range(i + 1, K):
            if K <= 2 or j == i + 1:   # more than two parts: two slots used in turn
                assert disjoint(regions[i][0], regions[j][0]) and disjoint(regions[i][1], regions[j][1]), (i, j)
    if K > 2:
        assert all(parts[i]["row_off"] == (i & 1) * (plan["row_entries"] // 2) for i in range(K))


def expected_parts(case):
    """The number of summation parts nbody_set_summation_parts documents."""
    whole = case.row_lo == 0 and case.row_count == case.n and not case.complement and case.first == 0 and case.count == case.S
    n_groups = -(-case.S // case.gs)
    K = case.sum_parts
    if K == 0:
        pass_bytes = 6.0 * case.n * case.n / case.L * (1.0 + 1.0 / case.SL)
        K = 1 if pass_bytes <= BUDGET else 4 if 0.75 * pass_bytes <= BUDGET else 8
    if not whole or case.S * case.S // 2 < (32768 if case.sum_parts == 0 else 0) or n_groups < 2:
        return 1
    return 2 if K > 2 and n_groups % K else K


def whole_cases():
    """{name: Case}: contexts that own every row, all columns in one call."""
    cases = {}
    for S in range(1, 81):                                    # single tiles, ragged last splits among them
        cases[f"S{S}"] = Case(S * 256 - (S % 3) * 37, 256, 1)
    for S in (8, 16, 24, 40, 64, 80):
        for K in (1, 2, 4, 8):
            cases[f"S{S}_K{K}"] = Case(S * 256, 256, 1, sum_parts=K)
    for SL, Ss in ((2, (16, 32, 48, 80, 128, 512, 1024)), (4, (32, 64, 96, 160, 1024)), (8, (64, 128, 192, 1024))):
        for S in Ss:
            cases[f"S{S}_SL{SL}"] = Case(S * 2048, 2048, SL)
    for S, SL in ((512, 2), (1024, 4)):                       # N = 2^20 and 2^21 as the library runs them
        for K in (1, 2, 4, 8):
            cases[f"S{S}_SL{SL}_K{K}"] = Case(S * 2048, 2048, SL, sum_parts=K)
    cases["S512_L2048"] = Case(1 << 20, 2048, 1)              # automatic: 4 parts
    cases["S1024_L4096"] = Case(1 << 22, 4096, 1)             # automatic: 8 parts
    cases["S300"] = Case(300 * 256, 256, 1)
    return cases


def shard_cases():
    """{name: [Case]}: a shard's (or one context's) rows, with all columns, a chunk of them, its complement, and the next chunk."""
    out = {}
    for S, L, SL in ((16, 256, 1), (80, 256, 1), (64, 2048, 2), (128, 2048, 4), (128, 2048, 8), (512, 2048, 2)):
        for world in (1, 2, 4, 8):
            chunks = max(world, 2)
            width = S // chunks
            ranks = sorted({0, world - 1})
            group = []
            for r in ranks:
                rows = S * L // world
                base = Case(S * L, L, SL, r * rows, rows)
                mine, nxt = (r * width) % S, ((r + 1) * width) % S
                group += [base, base.with_columns(mine, width), base.with_columns(mine, width, True), base.with_columns(nxt, width)]
            out[f"S{S}_SL{SL}_world{world}"] = group
    return out


def digest(texts):
    return hashlib.sha256("\n".join(texts).encode()).hexdigest()[:16]


def run_all(driver):
    whole = whole_cases()
    shards = shard_cases()
    order = [(k, c) for k, c in whole.items()] + [(k, c) for k, g in shards.items() for c in g]
    plans = parse_plans(driver([c.command() for _, c in order]))
    assert len(plans) == len(order)
    return whole, shards, order, plans


@pytest.fixture(scope="module")
def plans(driver):
    return run_all(driver)


def test_every_tile_once_and_the_parts_consistent(plans):
    whole, shards, order, results = plans
    for (name, case), (_, plan) in zip(order, results):
        try:
            assert plan["K"] == expected_parts(case)
            check_plan(case, plan)
        except AssertionError as e:
            raise AssertionError(f"{name}: {case.command()}: {e}") from e


def test_a_column_range_and_its_complement_are_the_whole_pass(driver):
    for group in shard_cases().values():
        for base in group[::4]:
            for first, count in ((base.first, base.count), (0, base.S // 2), (base.S // 4, base.S // 2)):
                if base.SL > 1 and (first % base.SL or count % base.SL):
                    continue
                a, b, w = (base.with_columns(first, count), base.with_columns(first, count, True), base.with_columns(0, base.S))
                pa, pb, pw = (p for _, p in parse_plans(driver([a.command(), b.command(), w.command()])))
                ka, da = tile_sets(a, pa)
                kb, db = tile_sets(b, pb)
                kw, dw = tile_sets(w, pw)
                assert np.array_equal(np.sort(np.concatenate([ka, kb])), kw)
                assert np.array_equal(np.sort(np.concatenate([da, db])), dw)


def test_the_automatic_parts_at_scale(plans):
    whole, _, order, results = plans
    got = {name: plan["K"] for (name, _), (_, plan) in zip(order, results)}
    assert got["S512_SL2"] == 1 and got["S1024_SL4"] == 8         # strips: N = 2^20 in one launch, 2^21 in 8 parts
    assert got["S512_L2048"] == 4 and got["S1024_L4096"] == 8      # single tiles: 3 + 3 + 1 + 1 groups, 8 equal parts
    assert got["S300"] == 1 and got["S80_K4"] == 4 and got["S80_K8"] == 8 and got["S40_K4"] == 4


def test_strip_length_rule(driver):
    n_splits = lambda n, L: -(-n // L)  # noqa: E731
    queries = [(n_splits(1 << 20, 2048), 2048, 0), (n_splits(1 << 21, 2048), 2048, 0), (n_splits(1 << 22, 2048), 2048, 0),
               (n_splits(1 << 20, 1024), 1024, 0), (n_splits(1 << 23, 4096), 4096, 0), (n_splits(20225, 256), 256, 0),
               (n_splits((1 << 20) - 2048, 2048), 2048, 0), (511, 2048, 2), (512, 2048, 8), (80, 2048, 4), (512, 1024, 4),
               (1024, 2048, 8), (64, 2048, 2), (1, 256, 0)]
    got = [int(v) for v in driver([f"strip {s} {L} {k}" for s, L, k in queries]).split()]
    assert got == [2, 4, 4, 1, 1, 1, 1, 1, 8, 1, 1, 8, 2, 1]


def test_rows_side_agrees_with_the_python_harness(driver):
    from sharded_harness import sym_rows_side
    out = driver([f"sides {S}" for S in range(1, 81)]).split()
    for S, row in zip(range(1, 81), out):
        assert row == "".join("1" if sym_rows_side(R, C, S) else "0" for R in range(S) for C in range(S)), S
        R, C = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
        assert row == "".join("1" if v else "0" for v in rows_side(R, C, S).ravel()), S


def test_launch_order_is_frozen(plans, golden_dir):
    """The order of the strips is a speed property (profiles/r04_strips_ab.txt): a change to it must be deliberate."""
    whole, shards, order, results = plans
    texts = {}
    for (name, _), (text, _) in zip(order, results):
        texts.setdefault(name, []).append(text)
    got = {name: digest(t) for name, t in texts.items()}
    with open(os.path.join(golden_dir, "sym_plan_digests.json")) as f:
        want = json.load(f)
    assert got.keys() == want.keys()
    assert {k for k in got if got[k] != want[k]} == set()
