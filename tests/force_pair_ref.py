"""Inputs, the fp64 reference, the tolerance and the checker of the single-system pair tests (no HIP, no GPU).

The idea.  One NBodySystem, every velocity zero, dt = 1: the kick `(float)fma((double)a, 1.0, 0.0)` returns the fp32
acceleration itself, so a step's new velocities ARE the force pass' sums.  Three ways of lighting the bodies:

  (A) one source.  Body c carries the only non-zero mass word MASS.  Every other term of every chain is an exact +-0 (a
      split whose masses are all 0 takes the equal-mass loop with scale 0, and finite x 0 = 0), the additions across waves,
      splits and groups add exact zeros, and row i's new velocity is the fp32 pair term (i, c) alone.  In the pair-once
      mode the same launch applies the pair to c with m_i = 0.  The split of c is not of one mass: its tiles run the general
      loops, with the equal-mass path on as with it off.
  (B) a lit split.  Every body of c's split carries MASS and every other body 0, so the split's tiles run the equal-mass
      loops (the flags are per side of a tile and per column split).  Source c stands in place and its companions stand
      far away, `far_slots`: coordinates from 2^30 up, 2^20 apart, so r^2 ~ 1e18, inv^3 ~ 1e-27 (normal numbers, far from
      overflow) and a companion's term on a near row is at most MASS 2^-60: FAR_TERM.
  (C) a lit near set (the equal-mass diagonal squares, where rows and columns are the same bodies and single terms cannot
      be isolated): all q bodies of a split, or of a 128-body window of it, stand in place with MASS, the check is per row.

Configuration.  `configuration(n)`: the near positions of pair_matrix_ref.configuration(n), body n - 3 moved exactly onto
body 7 (the coincident pair: with eps = 0 the guard gives 0, with eps > 0 d = 0 gives 0).  `softening_lengths(n)`: the
per-particle softening lengths, hashed in [0.004, 0.02), every fifth one and the coincident pair's 0.  MASS = 1.7 is no
power of two, so that (d inv^3) m and d (m inv^3) differ in bits.

Reference, fp64 from the fp32 inputs: a_ic = m d / (r^2 + E)^1.5, d = x_c - x_i, E = eps^2 from the fp32 softening, with
per-particle softening E = eps^2 + eps_i^2 + eps_c^2 from the fp32 values; r^2 + E = 0 gives 0.

Tolerance per entry and component:    tol = K u |a_ic,comp| + 2 (far companions) FAR_TERM,    u = 2^-24.
K from the loops' operations, counted as pair_matrix_ref counts K_A (v_rsq_f32 is documented to 1 ulp = 2 u):
  * d_c = x_c - x_i: 1 u.  r2 = fma(dz, dz, fma(dy, dy, fma(dx, dx, E))): each square carries 2 u, E = eps * eps carries
    1 u, a sum of positive parts carries the largest of them, and three roundings: 2 + 3 = 5 u.  inv = rsq(r2): 2.5 + 2 = 4.5 u.
  * general, one-sided (PK_POST, force_kernel): fma(d_c, (m inv)(inv inv), acc): m inv 5.5 u, inv inv 10 u, their product
    16.5 u; the fma 1 + 16.5 + 1 = 18.5 u.                                                               K_GENERAL = 18.5
  * general, pair-once (SY_POST, S3, S9, force_sym_general_kernel): fma(d_c, m (inv (inv inv)), acc): inv inv 10 u,
    inv^3 15.5 u, with the mass 16.5 u; the fma 18.5 u.  The column side is the same product with the row's mass and is
    subtracted exactly.                                                                                  K_GENERAL = 18.5
  * equal-mass (PK_POSTU, SY_POSTU, S2, S8, S12): fma(d_c, inv (inv inv), acc) 1 + 15.5 + 1 = 17.5 u, times the other
    side's mass when the sum is written out: 18.5 u.                                                       K_EQUAL = 18.5
  * per-particle softening (the _E loops, S10, S11, S12, PPS kernels): E = fl(fma(e_i, e_i, eps2) + fl(e_c e_c)); eps2
    carries 1 u, the fma one more on its sum (2 u), e_c^2 1 u, the addition 1 u: 3 u instead of 1 u in the first addend,
    so r2 carries 3 + 3 = 6 u, inv 5 u, inv^3 17 u, with the mass 18 u, the fma 20 u; equal-mass the same.      K_PPS = 20
  * guarded (eps = 0: GUARD, LOOP 2): a compare and a select on r2, no rounding; E = 0 is exact.  The same K.
Every addition of a far companion's term f to a partial sum s errs by at most |f| (s is representable) and leaves f itself
in the sum: 2 |f| per companion.  No margin, nothing fitted to a kernel's output.

Row-level tolerance of (C), vector lengths: |got_i - sum_j a_ij| <= (K + 1 + q) u sum_j |a_ij| (+ the far companions' share),
q the number of lit near bodies: K u per term, q - 1 additions of at most u times the sum each, the write-out's product.

Checker.  `check(...)` returns the worst |got - ref| / tol and the entries beyond tolerance, worst first, each naming case,
source, row and component.  `numpy_term` restates each term form in numpy fp32 with the rsq moved by up to 1 ulp, for the
CPU test of the tolerance.  `CASES` is the table of GPU cases with the kernels each must land on; `sources_of` the sources
a case probes: every body up to 1573 bodies; `thin` from 2341 bodies on (with every body a source the 3109-body cases took
8 s each on an MI355X, the 2341-body ones 4.7 s): every residue mod 64 of every split spread over its 64-body blocks, both
ends of every split and the coincident pair; `strips`: 64 consecutive sources across a block boundary plus both ends, in
five splits.  Rows are never thinned."""
import math

import numpy as np

import pair_matrix_ref as pm

U = pm.U
W_WORD = pm.W_WORD
MASS = float(np.float32(1.7))      # the mass word itself
EPS = 1e-2
K_GENERAL = 18.5
K_EQUAL = 18.5
K_PPS = 20.0
FAR = 2.0 ** 30
FAR_STEP = 2.0 ** 20
FAR_TERM = MASS * 2.0 ** -60       # a far companion's term on a near row: its distance exceeds 2^30 on every axis
COINCIDENT = 7                     # body n - 3 lies on body 7
COMPONENTS = ("vx", "vy", "vz")
DIAG_CLEARANCE = 4.0               # (C): every off-diagonal term of the lit near set is at least this many row tolerances


def coincident_row(n):
    return n - 3


def configuration(n):
    """(n, 3) float32 near positions; body n - 3 lies exactly on body 7."""
    x = pm.configuration(n)[0].copy()
    x[coincident_row(n)] = x[COINCIDENT]
    return x


def softening_lengths(n):
    e = (0.004 + 0.016 * pm._hash01(np.arange(n), 91)).astype(np.float32)
    e[::5] = 0.0
    e[COINCIDENT] = e[coincident_row(n)] = 0.0
    return e


def far_slots(count):
    """(count, 3) float32: slot k at FAR + FAR_STEP (k mod 16, (k / 16) mod 16, k / 256), exactly representable."""
    k = np.arange(count)
    g = np.stack([k % 16, (k // 16) % 16, k // 256], axis=1).astype(np.float64)
    return (FAR + FAR_STEP * g).astype(np.float32)


def k_of(pps):
    return K_PPS if pps else K_GENERAL


def softening2(eps, eps_pp, rows, cols):
    """E (len(cols), len(rows)) or a scalar, fp64 from the fp32 values."""
    e2 = float(np.float32(eps)) ** 2
    if eps_pp is None:
        return e2
    e = np.asarray(eps_pp, np.float32).astype(np.float64)
    return e2 + e[rows][None, :] ** 2 + e[cols][:, None] ** 2


def terms(x, sources, eps, eps_pp=None, mass=MASS, rows=None):
    """a[k, i] (S, R, 3) fp64: the acceleration of row rows[i] (default: every body) from source sources[k] alone."""
    x = np.asarray(x, np.float32).astype(np.float64)
    cols = np.asarray(sources, np.int64).reshape(-1)
    rows = np.arange(len(x)) if rows is None else np.asarray(rows, np.int64)
    d = x[cols][:, None, :] - x[rows][None, :, :]
    r2 = np.einsum("ijk,ijk->ij", d, d) + softening2(eps, eps_pp, rows, cols)
    ok = r2 > 0.0
    s = np.where(ok, mass / np.where(ok, r2, 1.0) ** 1.5, 0.0)
    return s[..., None] * d


def tolerance(ref, K, far=0):
    return K * U * np.abs(ref) + 2.0 * far * FAR_TERM


def row_tolerance(term_lengths_sum, K, q, far=0):
    """(C): tol_i of the summed row, from sum_j |a_ij| (vector lengths)."""
    return (K + 1.0 + q) * U * term_lengths_sum + 2.0 * far * FAR_TERM * math.sqrt(3.0)


def check(got, ref, tol, case, sources, rows=None, limit=8):
    """got, ref, tol (S, R, 3).  (worst |got - ref| / tol, failures): failures name case, source, row and component, worst
    first, at most `limit` (None: all)."""
    got = np.asarray(got)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.abs(got - ref)
        ratio /= tol
    ratio[np.isnan(ratio)] = 0.0                  # 0 / 0: an entry with no tolerance that is its reference, bit for bit up to the sign of zero
    ratio[~np.isfinite(got)] = np.inf
    worst = float(ratio.max()) if ratio.size else 0.0
    bad = np.argwhere(ratio > 1.0)
    if not len(bad):
        return worst, []
    order = np.argsort(-ratio[tuple(bad.T)], kind="stable")
    out = []
    for s, i, c in bad[order if limit is None else order[:limit]]:
        out.append({"case": case, "source": int(sources[s]), "row": int(i if rows is None else rows[i]),
                    "component": COMPONENTS[c], "got": float(got[s, i, c]), "ref": float(ref[s, i, c]),
                    "tol": float(tol[s, i, c]), "ratio": float(ratio[s, i, c])})
    return worst, out


def describe(failures):
    return "; ".join(f"{f['case']}: source {f['source']} row {f['row']} {f['component']}: got {f['got']!r} ref {f['ref']!r} "
                     f"tol {f['tol']:.3g} (x{f['ratio']:.3g})" for f in failures)


def near_set_sums(x, near, rows, eps, eps_pp=None):
    """(C): (sum_j a_ij (R, 3), sum_j |a_ij| (R,)) over the lit near bodies j for the rows `rows`."""
    a = terms(x, near, eps, eps_pp, rows=rows)
    return a.sum(0), np.linalg.norm(a, axis=-1).sum(0)


def diag_clearance(x, near, eps, eps_pp=None):
    """(C): the smallest |a_ij| / tol_i over the off-diagonal pairs of the lit near set: a single term of a diagonal square
    stands out of its row's tolerance by this factor."""
    near = np.asarray(near, np.int64)
    length = np.linalg.norm(terms(x, near, eps, eps_pp, rows=near), axis=-1)          # [j, i]
    tol = row_tolerance(length.sum(0), k_of(eps_pp is not None), len(near))
    ratio = length / tol[None, :]
    ratio[np.arange(len(near)), np.arange(len(near))] = np.inf
    return float(ratio.min())


def lit_sets(case):
    """(C): [(first body of the lit split, its count, near bodies)] of a case."""
    n, L = case["n"], case["split_len"]
    if case["diag"] == "splits":
        return [(lo, cnt, np.arange(lo, lo + cnt)) for lo, cnt in splits(n, L)]
    if case["diag"] == "windows":
        lo = WINDOW_SPLIT * L
        return [(lo, L, np.concatenate([np.arange(lo + 64 * i, lo + 64 * i + 64), np.arange(lo + 64 * j, lo + 64 * j + 64)]))
                for i, j in window_pairs(L)]
    return []


# ---- the term forms in numpy fp32 ------------------------------------------------------------------------------------------

FORMS = ("general_one_sided", "general_pair_once", "equal_mass")


def numpy_term(form, x, sources, eps, eps_pp=None, wobble=0, mass=MASS, rows=None):
    """What a correct fp32 loop returns for (rows[i], sources[k]) alone: (S, R, 3) float32.  wobble: (S, R) in {-1, 0, 1}."""
    f, fma, rsq = pm._f, pm._fma, pm._rsq
    x = f(x)
    cols = np.asarray(sources, np.int64).reshape(-1)
    rows = np.arange(len(x)) if rows is None else np.asarray(rows, np.int64)
    d = x[cols][:, None, :] - x[rows][None, :, :]
    eps2 = np.float32(eps) * np.float32(eps)
    if eps_pp is None:
        E = eps2
    else:
        e = f(eps_pp)
        E = fma(e[rows], e[rows], eps2)[None, :] + (e[cols] * e[cols])[:, None]
    r2 = fma(d[..., 2], d[..., 2], fma(d[..., 1], d[..., 1], fma(d[..., 0], d[..., 0], E)))
    if float(eps) == 0.0:
        r2 = np.where(r2 >= np.float32(2.0 ** -84), r2, np.float32(np.inf)).astype(np.float32)
    inv = rsq(r2, np.broadcast_to(np.asarray(wobble), r2.shape))
    m = np.float32(mass)
    zero = np.float32(0.0)
    if form == "general_one_sided":
        s = (m * inv) * (inv * inv)
        return np.stack([fma(d[..., k], s, zero) for k in range(3)], axis=-1)
    if form == "general_pair_once":
        s = m * (inv * (inv * inv))
        return np.stack([fma(d[..., k], s, zero) for k in range(3)], axis=-1)
    if form == "equal_mass":
        s = inv * (inv * inv)
        return np.stack([fma(d[..., k], s, zero) * m for k in range(3)], axis=-1)
    raise ValueError(form)


# ---- splits and sources ---------------------------------------------------------------------------------------------------

def splits(n, L):
    """[(first body, count)] of the splits."""
    return [(lo, min(L, n - lo)) for lo in range(0, n, L)]


def sources_of(case):
    n, L = case["n"], case["split_len"]
    how = case["sources"]
    special = {COINCIDENT, coincident_row(n)}
    if how == "all":
        return np.arange(n)
    if how == "thin":
        out = set(special)
        for s, (lo, cnt) in enumerate(splits(n, L)):
            blocks = -(-cnt // 64)
            for k in range(64):
                c = 64 * ((5 * k + s) % blocks) + k
                out.add(lo + (c if c < cnt else k % cnt))
            out |= {lo, lo + cnt - 1}
        return np.array(sorted(out))
    if how == "strips":
        out = set(special)
        for s in (0, 1, 7, 8, 15):
            lo = s * L
            out |= set(range(lo + 64 * 3 + 17, lo + 64 * 4 + 17)) | {lo, lo + L - 1}
        return np.array(sorted(out))
    if how == "sixteen":
        return np.array(sorted(special | {0, 1, 63, 64, 255, 256, 257, 511, 700, 1023, 1024, 1279, 1280, n - 1}))
    raise ValueError(how)


def lit_state(case, x, lo, cnt, near=None):
    """(B), (C): positions and mass words (n, 4) float32 with the split [lo, lo + cnt) lit: its bodies carry MASS and stand
    at `far_slots` except those in `near` (indices; (B) restores its source itself), every other body in place with mass 0."""
    p = np.zeros((len(x), 4), np.float32)
    p[:, :3] = x
    p[lo:lo + cnt, :3] = far_slots(cnt)
    p[lo:lo + cnt, 3] = MASS
    if near is not None:
        p[near, :3] = x[near]
    return p


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------

def _case(name, mode, n, L, rpl, eps, pps, sources, kernels, strip=0, equal_mass_loop=True, diag=None, parts="AB"):
    return {"name": name, "mode": mode, "n": n, "split_len": L, "rows_per_lane": rpl, "eps": eps, "pps": pps, "strip": strip,
            "sources": sources, "kernels": tuple(kernels), "equal_mass_loop": equal_mass_loop, "diag": diag, "parts": parts}


def _cases():
    c = []
    G, S, Q = "force_sym_general_kernel", "force_sym_kernel", "force_sym_quarter_kernel"
    # one-sided, packed: two row blocks of 1024, the second ragged
    for tag, eps, pps, t in (("soft", EPS, False, "false, false"), ("guard", 0.0, False, "true, false"), ("pps", EPS, True, "false, true")):
        c.append(_case(f"one_sided_packed_{tag}", "one_sided", 1317, 256, 4, eps, pps, "all", [f"force_kernel_r4pk<{t}>"],
                       equal_mass_loop=eps > 0))
    # one-sided, one wave per workgroup: QT 4 (a padded tile), 5, 8 and 0
    for L, qt in ((64, 4), (320, 5), (512, 8), (768, 0)):
        for tag, eps in (("soft", EPS), ("guard", 0.0)):
            g = "true" if eps == 0.0 else "false"
            c.append(_case(f"one_sided_one_wave_{L}_{tag}", "one_sided", 1317, L, 41, eps, False, "all",
                           [f"force_kernel_r4pk_w1<{g}, {qt}, false>"], equal_mass_loop=eps > 0))
    # one-sided, the other blockings: bit-equal to blocking 4 on sixteen sources
    for rpl, k in ((40, "force_kernel_r4<false>"), (1, "force_kernel<1, false, false>"), (2, "force_kernel<2, false, false>"),
                   (8, "force_kernel<8, false, false>"), (-4, "force_kernel<4, false, false>")):
        c.append(_case(f"one_sided_blocking_{rpl}", "one_sided", 1317, 256, rpl, EPS, False, "sixteen", [k], parts="E"))
    # quarter tiles, 256-body splits: tiles and diagonal squares in one launch
    for n in (805, 549):
        for tag, eps, pps, loop in (("soft", EPS, False, 0), ("pps", EPS, True, 1), ("guard", 0.0, False, 2)):
            c.append(_case(f"quarter_256_{n}_{tag}", "pair_once", n, 256, 0, eps, pps, "all", [f"{Q}<{loop}, 1>"],
                           equal_mass_loop=loop == 0, diag="splits"))                      # LOOP 0 alone has an equal-mass loop
    for tag, eps, loop in (("soft", EPS, 0), ("guard", 0.0, 2)):
        c.append(_case(f"quarter_512_1573_{tag}", "pair_once", 1573, 512, 0, eps, False, "all", [f"{Q}<{loop}, 2>"],
                       equal_mass_loop=eps > 0, diag="splits"))
    # eight rows per lane; the diagonal tiles are the general kernel's
    for n, L, w, src in ((3109, 1024, 2, "thin"), (6181, 2048, 4, "thin")):
        c.append(_case(f"eight_rows_{L}_soft", "pair_once", n, L, 0, EPS, False, src,
                       [f"{S}<{w}, false, 2, 1>", f"{G}<{w}, true, false, false>"]))
        c.append(_case(f"eight_rows_{L}_guard", "pair_once", n, L, 0, 0.0, False, src,
                       [f"{S}<4, true, 0, 0>", f"{G}<{w}, true, true, false>"], equal_mass_loop=False))
        c.append(_case(f"eight_rows_{L}_pps", "pair_once", n, L, 0, EPS, True, src,
                       [f"{S}<{w}, false, 3, 1>", f"{G}<{w}, true, false, true>"]))
        c.append(_case(f"eight_rows_{L}_pps_guard", "pair_once", n, L, 0, 0.0, True, src,
                       [f"{G}<4, false, true, true>", f"{G}<{w}, true, true, true>"], equal_mass_loop=False))
    # four rows per lane: packed (4), one column per step (1), and 768-body splits (no multiple of 512: S11 with softening lengths)
    for rpl in (4, 1):
        c.append(_case(f"four_rows_1024_rpl{rpl}_soft", "pair_once", 3109, 1024, rpl, EPS, False, "thin",
                       [f"{S}<4, false, 0, 0>", f"{G}<2, true, false, false>"]))
        c.append(_case(f"four_rows_1024_rpl{rpl}_pps", "pair_once", 3109, 1024, rpl, EPS, True, "thin",
                       [f"{G}<4, false, false, true>", f"{G}<2, true, false, true>"], equal_mass_loop=False))
    c.append(_case("four_rows_768_soft", "pair_once", 2341, 768, 0, EPS, False, "thin",
                   [f"{S}<2, false, 0, 0>", f"{G}<2, true, false, false>"], equal_mass_loop=False))   # a pass is partial
    c.append(_case("four_rows_768_pps", "pair_once", 2341, 768, 0, EPS, True, "thin",
                   [f"{S}<2, false, 4, 0>", f"{G}<2, true, false, true>"], equal_mass_loop=False))    # S11: masses in the loop
    # strips of two tiles and single tiles, 2048-body splits
    for strip in (2, 1):
        c.append(_case(f"strips_{strip}_soft", "pair_once", 32768, 2048, 0, EPS, False, "strips",
                       [f"{S}<4, false, 2, 1>", f"{G}<4, true, false, false>"], strip=strip, diag="windows"))
        c.append(_case(f"strips_{strip}_guard_rpl4", "pair_once", 32768, 2048, 4, 0.0, False, "strips",
                       [f"{S}<4, true, 0, {2 if strip == 2 else 0}>", f"{G}<4, true, true, false>"], strip=strip,
                       equal_mass_loop=False, diag="windows"))
    return c


CASES = _cases()

#: the union of kernel instantiations the cases reach
KERNELS = sorted({k for case in CASES for k in case["kernels"]})

WINDOW_SPLIT = 1           # (C) at 32 768 bodies: the lit split whose 64-body blocks form the windows
WINDOW_ROWS_ELSEWHERE = (0, 2)   # ... and the splits whose first 256 rows are checked beside the window's own


def window_pairs(L=2048):
    b = L // 64
    return [(i, j) for i in range(b) for j in range(i + 1, b)]


def driver_commands(case):
    """The commands of tests/launch_choice_driver.cpp that name the kernels of `case`, with the equal-mass path on."""
    eps, pps = int(case["eps"] > 0), int(case["pps"])
    if case["mode"] == "one_sided":
        return [f"force {case['rows_per_lane']} {case['split_len']} {eps} {pps}"]
    return [f"packed {case['rows_per_lane']} 1", f"packed {case['rows_per_lane']} 0",
            "sym {L} {eps} {pps} {{packed}} {strip}".format(L=case["split_len"], eps=eps, pps=pps, strip=max(case["strip"], 1))]
