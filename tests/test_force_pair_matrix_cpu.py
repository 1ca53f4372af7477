"""CPU: the single-system pair tests' own parts (tests/force_pair_ref.py) -- the reference summed over its sources against
the fp64 oracle, a numpy fp32 restatement of every term form held under the derived tolerance, the checker on emulated
subtly wrong kernels, the conditions of the row-level diagonal checks, and the table of GPU cases against the kernels
csrc/nbody_launch_choice.h chooses for them (tests/launch_choice_driver.cpp, as test_launch_choice_cpu.py builds it).

Worst |fp32 restatement - ref| / tol, over n = 805 and 549, eps = 1e-2 and 0, the rsq exact, moved up, down and at random:
general one-sided 0.735, general pair-once 0.744, equal-mass 0.750 (K 18.5); with softening lengths 0.679, 0.673, 0.697
(K 20).  Lowest |term| / row tolerance of the diagonal checks: 18 (805 bodies), 21 (549), 4.5 (1573), 9.0 (the 496 windows)."""
import os
import subprocess

import numpy as np
import pytest

import force_pair_ref as fp
from conftest import ROOT

CSRC = os.path.join(ROOT, "n_body_problem_amd", "csrc")
SIZES = (805, 549)
EPS32 = float(np.float32(fp.EPS))      # the softening the kernels receive


def state(n, mass=fp.MASS):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = fp.configuration(n)
    p[:, 3] = mass
    return p


@pytest.mark.parametrize("n", SIZES)
def test_reference_summed_over_all_sources_is_the_oracle(oracle_mod, n):
    x, e = fp.configuration(n), fp.softening_lengths(n)
    assert np.array_equal(x[fp.coincident_row(n)], x[fp.COINCIDENT])
    mine = fp.terms(x, np.arange(n), fp.EPS).sum(0)
    want = oracle_mod.accel_f64(state(n), eps=EPS32)
    assert np.abs(mine - want).max() <= 1e-13 * np.abs(want).max()
    mine = fp.terms(x, np.arange(n), fp.EPS, e).sum(0)
    want = oracle_mod.accel_f64_pps(state(n), e, eps=EPS32)
    assert np.abs(mine - want).max() <= 1e-13 * np.abs(want).max()
    # the coincident pair and the self pair with nothing to soften them: exactly nothing, and nothing that is not finite
    for eps_pp in (None, e):
        a = fp.terms(x, np.arange(n), 0.0, eps_pp)
        assert np.isfinite(a).all()
        assert not a[fp.COINCIDENT, fp.coincident_row(n)].any() and not a[fp.coincident_row(n), fp.COINCIDENT].any()
        assert not a[np.arange(n), np.arange(n)].any()
        assert np.count_nonzero((a == 0.0).all(-1)) == n + 2


def test_configuration_and_far_slots():
    for n in sorted({c["n"] for c in fp.CASES}):
        x, e = fp.configuration(n), fp.softening_lengths(n)
        assert x.dtype == np.float32 and x.shape == (n, 3) and 0.7 < x.min() and x.max() < 4.3
        assert e.dtype == np.float32 and e[fp.COINCIDENT] == 0.0 and e[fp.coincident_row(n)] == 0.0 and (e[1:5] >= 0.004).all()
    f = fp.far_slots(2048).astype(np.float64)
    assert np.array_equal(f, fp.FAR + fp.FAR_STEP * np.round((f - fp.FAR) / fp.FAR_STEP)) and len(np.unique(f, axis=0)) == 2048
    assert f.min() >= fp.FAR and (3 * f.max() ** 2) < 1e19                       # r^2 far below fp32 overflow
    d = np.abs(f[:, None, :] - f[None, :, :]).max(-1)
    assert d[~np.eye(2048, dtype=bool)].min() >= fp.FAR_STEP
    # a far companion's term on any near row, |a_c| <= m / r^2 with r^2 >= 3 (FAR - 4.3)^2, is below FAR_TERM
    assert fp.MASS / (3.0 * (fp.FAR - 4.3) ** 2) <= fp.FAR_TERM


@pytest.mark.parametrize("pps", [False, True], ids=["eps", "pps"])
@pytest.mark.parametrize("form", fp.FORMS)
def test_fp32_restatement_stays_under_the_tolerance(form, pps):
    worst = 0.0
    rng = np.random.default_rng(5)
    for n in SIZES:
        x = fp.configuration(n)
        e = fp.softening_lengths(n) if pps else None
        for eps in (fp.EPS, 0.0):
            ref = fp.terms(x, np.arange(n), eps, e)
            tol = fp.tolerance(ref, fp.k_of(pps))
            for wobble in (0, 1, -1, rng.integers(-1, 2, size=(n, n))):
                got = fp.numpy_term(form, x, np.arange(n), eps, e, wobble)
                w, fails = fp.check(got, ref, tol, f"{form} n {n} eps {eps}", np.arange(n))
                assert not fails, fp.describe(fails)
                worst = max(worst, w)
    print(f"force pair matrix: fp32 restatement {form}{' with softening lengths' if pps else ''}: worst ratio {worst:.3f}")
    assert 0.05 < worst < 1.0


def test_the_two_forms_differ_in_bits():
    x = fp.configuration(549)
    a = fp.numpy_term("general_pair_once", x, np.arange(549), fp.EPS)
    b = fp.numpy_term("equal_mass", x, np.arange(549), fp.EPS)
    assert (a.view(np.uint32) != b.view(np.uint32)).mean() > 0.2


# ---- fault classes on a correct fp32 matrix: each reported at its own (source, row), all of them, and nothing else ----------

N_FAULT, PAD = 805, 832       # rows 805 .. 831: the padding of the last 64-row block


@pytest.fixture(scope="module")
def matrix():
    x = fp.configuration(N_FAULT)
    ref = np.zeros((N_FAULT, PAD, 3))
    ref[:, :N_FAULT] = fp.terms(x, np.arange(N_FAULT), fp.EPS)
    good = np.zeros((N_FAULT, PAD, 3), np.float32)
    good[:, :N_FAULT] = fp.numpy_term("general_pair_once", x, np.arange(N_FAULT), fp.EPS,
                                      wobble=np.random.default_rng(3).integers(-1, 2, size=(N_FAULT, N_FAULT)))
    for a in (ref, good):
        a.setflags(write=False)
    return ref, fp.tolerance(ref, fp.K_GENERAL), good


def _group_partner(c):
    return (c & ~63) | ((c + 32) & 63)


FAULTS = {
    "dropped": lambda g, c, i: 0.0 * g[c, i],
    "doubled": lambda g, c, i: 2.0 * g[c, i],
    "column c + 1": lambda g, c, i: g[c + 1, i],
    "column c - 1": lambda g, c, i: g[c - 1, i],
    "row i + 64": lambda g, c, i: g[c, i + 64],
    "row i - 64": lambda g, c, i: g[c, i - 64],
    "column (c + 32) mod 64 of its group": lambda g, c, i: g[_group_partner(c), i],
    "sign flipped": lambda g, c, i: -g[c, i],
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_every_injected_fault_is_reported_at_its_entry(matrix, fault):
    ref, tol, good = matrix
    n = N_FAULT
    rng = np.random.default_rng(11)
    cs, rows = rng.integers(64, n - 64, size=4000), rng.integers(64, n - 64, size=4000)
    special = (fp.COINCIDENT, fp.coincident_row(n))
    keep = (cs != rows) & (np.abs(cs - rows) != 1) & (np.abs(cs - rows) != 64) & (_group_partner(cs) != rows) & \
        ~np.isin(cs, special) & ~np.isin(rows, special) & (_group_partner(cs) < n)
    entries = sorted(set(zip(cs[keep].tolist(), rows[keep].tolist())))
    assert len(entries) > 3000
    got = good.copy()
    for c, i in entries:
        got[c, i] = FAULTS[fault](good, c, i)
    worst, fails = fp.check(got, ref, tol, fault, np.arange(n), limit=None)
    assert {(f["source"], f["row"]) for f in fails} == set(entries)           # 100 % of them, and no other entry
    assert all(f["case"] == fault and f["component"] in fp.COMPONENTS for f in fails) and worst == fails[0]["ratio"] > 1.0


def test_self_terms_and_terms_beyond_the_last_row_are_reported(matrix):
    ref, tol, good = matrix
    n = N_FAULT
    assert fp.check(good, ref, tol, "good", np.arange(n))[1] == []
    got = good.copy()
    selfs = [0, 7, 63, 64, 500, n - 3, n - 1]
    for c in selfs:
        got[c, c] = good[c, (c + 1) % n]                                       # what the neighbouring row gets
    got[fp.COINCIDENT, fp.coincident_row(n)] = good[fp.COINCIDENT, 8]            # the row on top of its source
    beyond = [(0, n), (n - 1, PAD - 1), (300, n + 5)]
    for c, i in beyond:
        got[c, i] = good[c, i - 64]
    _, fails = fp.check(got, ref, tol, "self", np.arange(n), limit=None)
    assert {(f["source"], f["row"]) for f in fails} == {(c, c) for c in selfs} | {(fp.COINCIDENT, fp.coincident_row(n))} | set(beyond)
    assert all(f["ratio"] == np.inf for f in fails)
    got = good.copy()
    got[5, 9, 1] = np.nan
    _, fails = fp.check(got, ref, tol, "nan", np.arange(n))
    assert [(f["source"], f["row"], f["component"]) for f in fails] == [(5, 9, "vy")]


# ---- the diagonal checks' conditions, from the reference alone ---------------------------------------------------------------

def test_single_terms_stand_out_of_the_row_tolerance_of_the_diagonal_checks():
    lowest = {}
    for case in fp.CASES:
        if case["diag"] is None:
            continue
        x = fp.configuration(case["n"])
        e = fp.softening_lengths(case["n"]) if case["pps"] else None
        sets = fp.lit_sets(case)
        assert len(sets) == (496 if case["diag"] == "windows" else -(-case["n"] // case["split_len"]))
        for lo, cnt, near in sets:
            assert lo <= near.min() and near.max() < lo + cnt and len(set(near.tolist())) == len(near)
            assert not {fp.COINCIDENT, fp.coincident_row(case["n"])} <= set(near.tolist())
            c = fp.diag_clearance(x, near, case["eps"], e)
            lowest[case["name"]] = min(lowest.get(case["name"], np.inf), c)
            assert c >= fp.DIAG_CLEARANCE, (case["name"], lo, c)
    print("force pair matrix: lowest |term| / row tolerance of the diagonal checks: " +
          ", ".join(f"{k} {v:.1f}" for k, v in lowest.items()))
    # why windows: over a whole 2048-body split a single term drowns in its row's tolerance
    x = fp.configuration(32768)
    assert fp.diag_clearance(x, np.arange(2048, 4096), fp.EPS) < 1.0


# ---- the sources ------------------------------------------------------------------------------------------------------------

def test_sources_cover_what_they_claim():
    for case in fp.CASES:
        n, L = case["n"], case["split_len"]
        src = fp.sources_of(case)
        assert len(set(src.tolist())) == len(src) and src.min() >= 0 and src.max() < n
        assert {fp.COINCIDENT, fp.coincident_row(n)} <= set(src.tolist())
        if case["sources"] == "all":
            assert len(src) == n
        if case["sources"] == "thin":
            for lo, cnt in fp.splits(n, L):
                mine = src[(src >= lo) & (src < lo + cnt)]
                assert {lo, lo + cnt - 1} <= set(mine.tolist())
                assert len(set(((mine - lo) % 64).tolist())) == min(cnt, 64), (case["name"], lo)
                assert len(set(((mine - lo) // 64).tolist())) == -(-cnt // 64) or cnt > 64 * 64, (case["name"], lo)
        if case["sources"] == "strips":
            for s in (0, 1, 7, 8, 15):
                mine = src[(src >= s * L) & (src < (s + 1) * L)]
                assert len(set((mine % 64).tolist())) == 64 and {s * L, (s + 1) * L - 1} <= set(mine.tolist())


# ---- the case table lands where it claims -----------------------------------------------------------------------------------

#: every kernel instantiation the GPU cases must reach, spelled out
EXPECTED_KERNELS = [
    "force_kernel<1, false, false>", "force_kernel<2, false, false>", "force_kernel<4, false, false>", "force_kernel<8, false, false>",
    "force_kernel_r4<false>",
    "force_kernel_r4pk<false, false>", "force_kernel_r4pk<false, true>", "force_kernel_r4pk<true, false>",
    "force_kernel_r4pk_w1<false, 0, false>", "force_kernel_r4pk_w1<false, 4, false>", "force_kernel_r4pk_w1<false, 5, false>",
    "force_kernel_r4pk_w1<false, 8, false>", "force_kernel_r4pk_w1<true, 0, false>", "force_kernel_r4pk_w1<true, 4, false>",
    "force_kernel_r4pk_w1<true, 5, false>", "force_kernel_r4pk_w1<true, 8, false>",
    "force_sym_quarter_kernel<0, 1>", "force_sym_quarter_kernel<1, 1>", "force_sym_quarter_kernel<2, 1>",
    "force_sym_quarter_kernel<0, 2>", "force_sym_quarter_kernel<2, 2>",
    "force_sym_kernel<2, false, 2, 1>", "force_sym_kernel<4, false, 2, 1>",             # S9 / S8
    "force_sym_kernel<4, true, 0, 0>", "force_sym_kernel<4, true, 0, 2>",               # SY, guarded; in-memory strips
    "force_sym_kernel<2, false, 3, 1>", "force_sym_kernel<4, false, 3, 1>",             # S10 / S12
    "force_sym_kernel<4, false, 0, 0>", "force_sym_kernel<2, false, 0, 0>",             # S3 / S2, one column per step
    "force_sym_kernel<2, false, 4, 0>",                                                 # S11
    "force_sym_general_kernel<4, false, false, true>", "force_sym_general_kernel<4, false, true, true>",
    "force_sym_general_kernel<2, true, false, false>", "force_sym_general_kernel<2, true, true, false>",
    "force_sym_general_kernel<2, true, false, true>", "force_sym_general_kernel<2, true, true, true>",
    "force_sym_general_kernel<4, true, false, false>", "force_sym_general_kernel<4, true, true, false>",
    "force_sym_general_kernel<4, true, false, true>", "force_sym_general_kernel<4, true, true, true>",
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("force_pair") / "launch_choice_driver")
    res = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC,
                          os.path.join(ROOT, "tests", "launch_choice_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    def run(commands):
        res = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert len(lines) == len(commands)
        return lines
    return run


def chosen(driver, case):
    """The kernels of a case, equal-mass path on and off: the same ones (the switch changes flags, not kernels)."""
    cmds = fp.driver_commands(case)
    if case["mode"] == "one_sided":
        return [driver(cmds)[0].split("|")[0]]
    packed = driver(cmds[:2])
    names = []
    for p in packed:
        line = driver([cmds[2].format(packed=p)])[0].split("|")
        names.append([k for k in (line[0], line[5]) if k != "none"])
    assert names[0] == names[1], case["name"]
    return names[0]


def has_equal_mass_loop(case):
    """Whether the tiles of a lit split can take an equal-mass loop, as the kernels state it: none with eps = 0 (GUARD, LOOP 2:
    the flag is NaN), in force_sym_general_kernel, in the quarter kernel's LOOP 1 and in S11 (ROWS8 = 4: masses in the loop),
    and none in force_sym_kernel where a pass of W waves is partial."""
    kernel, args = case["kernels"][0].rstrip(">").split("<")
    t = args.split(", ")
    if case["eps"] == 0.0 or kernel == "force_sym_general_kernel":
        return False
    if kernel == "force_sym_quarter_kernel":
        return t[0] == "0"
    if kernel == "force_sym_kernel":
        rows8 = int(t[2])
        return rows8 <= 3 and case["split_len"] % (int(t[0]) * 64 * (8 if rows8 else 4)) == 0
    return True


def test_every_case_lands_on_the_kernels_it_names(driver):
    union = set()
    for case in fp.CASES:
        got = chosen(driver, case)
        assert got == list(case["kernels"]), (case["name"], got)
        union |= set(got)
        assert case["equal_mass_loop"] == has_equal_mass_loop(case), case["name"]
    assert union == set(EXPECTED_KERNELS) == set(fp.KERNELS) and len(EXPECTED_KERNELS) == len(set(EXPECTED_KERNELS))
    names = [c["name"] for c in fp.CASES]
    assert len(names) == len(set(names))
    # the shapes: ragged by 37 bodies, more than one row block, strips only where strips exist
    for case in fp.CASES:
        n, L = case["n"], case["split_len"]
        if case["sources"] != "strips":
            assert (n % L) % 64 == 37 and n % 256 == 37, case["name"]
        else:
            assert n == 16 * L and case["strip"] in (1, 2)
