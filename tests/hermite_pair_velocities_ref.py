"""Numpy reference of nbody_batch_pair_velocities (include/nbody_batch_pair_velocities.h) in IEEE doubles in the pinned order, and
the inputs of its tests.

The bin decision.  Every finite coordinate lies on a lattice 1 / Q (Q = 4 in the lattice states, 64 in the Gaussian states) with
|Q x| <= 512, so Q x is an integer hermite_correlation_ref.r2_codes takes: its exact integer r2 of Q x is Q^2 times the r2 of x,
every step of the fp32 chain is exact, and code / Q^2 is the fp32 r2 the library forms, as a number.  The squared edges are
hermite_correlation_ref.squared_edges (one fp32 product, the library's), and a pair is within an edge iff r2 <= e2: neither is
written again here.  The CPU driver, which runs the library's own fp32 chain, is byte-equal to this on every input, which checks
the premise.  Velocities are on no lattice in the Gaussian states: no velocity word enters a decision.

The sums.  Row sums are sequential accumulations over ascending j (one vector add per column, over all rows at once: never
np.sum); blocks of 64 rows by the halving tree; blocks in ascending order.  numpy's fp64 +, -, x, / and sqrt are IEEE.

The error measure of the five words that pass through a square root or a division (r1, vr1, vr2, vt2, v1): |got - ref| over the
sum of the absolute addends of that word and bin.  BOUND is four times the spread the reference itself shows when every root
and quotient is moved by up to one ulp at random (jitter_spread, measured by test_batch_pair_velocities_cpu.py)."""
import functools

import numpy as np

import hermite_correlation_ref as cref

MAX_BINS = 32
BLOCK = 64
G_BUILT = 8                                  # kPairVelocitiesPassBins of the kernel built
WEIGHT_MASS, WEIGHT_NUMBER = 0, 1
INTEGERS = ("count", "approaching", "receding")
TERMS = ("weight", "r1", "r2", "rv", "vr1", "vr2", "vt2", "v1", "v2")
EXACT_WORDS = ("weight", "r2", "rv", "v2")   # +, -, x and comparisons alone
ROOTED_WORDS = ("r1", "vr1", "vr2", "vt2", "v1")
SYSTEM_WORDS = ("rows", "sources", "both", "bins", "weight", "reserved", "pairs", "below", "above", "unmeasured")
BIN_DTYPE = np.dtype([(w, np.int64) for w in INTEGERS] + [(w, np.float64) for w in TERMS])
SYSTEM_DTYPE = np.dtype([(w, np.int32) for w in SYSTEM_WORDS[:6]] + [(w, np.int64) for w in SYSTEM_WORDS[6:]])
assert BIN_DTYPE.itemsize == 96 and SYSTEM_DTYPE.itemsize == 56

#: Measured by jitter_spread() over every case of the capacities 64, 128 and 256: 5.09e-15 with its seed, 6.79e-15 with three
#: others; the largest, rounded up.  It is vt2's, in bins of one or two nearly radial pairs, where v2 - vr vr cancels and the
#: moved quotient shows in what is left (the other four words stay below 9e-16).  No integer and no exact word moved.
SPREAD = 6.8e-15
BOUND = 4.0 * SPREAD  # 2.72e-14


# ---- the reference -----------------------------------------------------------------------------------------------------------
def decisions(pos, vel, n, q, edges, rows=None, sources=None):
    """(t, examined, measured, e2): t (n, n) int16, the number of edges an ordered pair is not within, minus 1 (-1 below,
    0 ... bins - 1 a bin, bins above; meaningless where not measured); examined and measured (n, n) bool."""
    pos, vel = np.asarray(pos)[:n], np.asarray(vel)[:n]
    codes = cref.r2_codes(pos[:, :3].astype(np.float64) * q, n)
    row = np.ones(n, bool) if rows is None else np.asarray(rows)[:n] != 0
    source = np.ones(n, bool) if sources is None else np.asarray(sources)[:n] != 0
    examined = row[:, None] & source[None, :] & ~np.eye(n, dtype=bool)
    moving = np.isfinite(vel[:, :3].astype(np.float64)).all(axis=1)
    measured = (codes < cref.TOP) & moving[:, None] & moving[None, :]
    r2 = (codes.astype(np.float32) / np.float32(q * q)).astype(np.float32)     # exact: the code is below 2^24
    assert (codes[codes < cref.TOP] < 2 ** 24).all()
    e2 = cref.squared_edges(edges)
    t = np.full((n, n), -1, np.int16)
    for edge in e2:
        t += ~(r2 <= edge)                                                        # groups_friends, per edge
    return t, examined, measured, e2, row, source


def move(x, rng):
    """x moved by -1, 0 or +1 ulp at random."""
    k = rng.integers(-1, 2, size=x.shape)
    return np.where(k < 0, np.nextafter(x, -np.inf), np.where(k > 0, np.nextafter(x, np.inf), x))


def terms_of(xi, vi, mi, xj, vj, mj, weight, rng=None):
    """The nine addends and rv of rows (arrays) against one column, in the header's order of operations."""
    d = xj[None, :] - xi
    w = vj[None, :] - vi
    dx, dy, dz, wx, wy, wz = d[:, 0], d[:, 1], d[:, 2], w[:, 0], w[:, 1], w[:, 2]
    s = (dx * dx + dy * dy) + dz * dz
    rv = (dx * wx + dy * wy) + dz * wz
    v2 = (wx * wx + wy * wy) + wz * wz
    r = np.sqrt(s)
    if rng is not None:
        r = move(r, rng)
    vr = rv / r
    if rng is not None:
        vr = move(vr, rng)
    vrvr = vr * vr
    vt2 = np.maximum(v2 - vrvr, 0.0)
    v = np.sqrt(v2)
    if rng is not None:
        v = move(v, rng)
    ww = np.ones_like(s) if weight == WEIGHT_NUMBER else mi * mj
    return np.stack([ww, ww * r, ww * s, ww * rv, ww * vr, ww * vrvr, ww * vt2, ww * v, ww * v2], axis=1), rv


def reference(pos, vel, n, q, edges, rows=None, sources=None, weight=WEIGHT_NUMBER, rng=None):
    """Every word of one system: {"system": SYSTEM_DTYPE scalar, "bins": (bins,) BIN_DTYPE, "absolute": (bins, 9) the sums of
    the absolute addends}."""
    pos, vel = np.asarray(pos), np.asarray(vel)
    t, examined, measured, e2, row, source = decisions(pos, vel, n, q, edges, rows, sources)
    bins = len(e2) - 1
    seen = examined & measured
    member = seen & (t >= 0) & (t < bins)
    x, v, m = pos[:n, :3].astype(np.float64), vel[:n, :3].astype(np.float64), pos[:n, 3].astype(np.float64)
    padded = -(-max(n, 1) // BLOCK) * BLOCK
    sums = np.zeros((padded, bins, len(TERMS)))                                # row sums, +0.0 beyond the count
    absolute = np.zeros((bins, len(TERMS)))
    out = np.zeros(bins, BIN_DTYPE)
    with np.errstate(all="ignore"):
        for j in range(n):                                                      # ascending j: one add per member and term
            i = np.nonzero(member[:, j])[0]
            if not len(i):
                continue
            addends, rv = terms_of(x[i], v[i], m[i], x[j], v[j], m[j], weight, rng)
            b = t[i, j].astype(np.int64)
            sums[i, b] = sums[i, b] + addends                                   # every i once: no two addends meet
            np.add.at(absolute, b, np.abs(addends))
            np.add.at(out["count"], b, 1)
            np.add.at(out["approaching"], b, rv < 0.0)
            np.add.at(out["receding"], b, rv > 0.0)
        p = sums.reshape(padded // BLOCK, BLOCK, bins, len(TERMS)).copy()
        off = BLOCK // 2
        while off:                                                              # the halving tree of every block
            p[:, :off] = p[:, :off] + p[:, off:2 * off]
            off //= 2
        total = np.zeros((bins, len(TERMS)))
        for k in range(p.shape[0]):                                             # the blocks in ascending order
            total = total + p[k, 0]
    for c, word in enumerate(TERMS):
        out[word] = total[:, c]
    system = np.zeros((), SYSTEM_DTYPE)
    n_rows, n_sources, both = int(row.sum()), int(source.sum()), int((row & source).sum())
    pairs, n_seen = n_rows * n_sources - both, int(seen.sum())
    for word, value in (("rows", n_rows), ("sources", n_sources), ("both", both), ("bins", bins), ("weight", weight), ("pairs", pairs),
                        ("below", int((seen & (t < 0)).sum())), ("above", int((seen & (t >= bins)).sum())),
                        ("unmeasured", pairs - n_seen)):
        system[word] = value
    assert int(examined.sum()) == pairs
    return {"system": system, "bins": out, "absolute": absolute}


def error_of(got_bins, ref):
    """The largest |got - ref| over the sum of the absolute addends, over the bins and the five rooted words."""
    worst = 0.0
    for word in ROOTED_WORDS:
        scale = ref["absolute"][:, TERMS.index(word)]
        diff = np.abs(np.asarray(got_bins[word], np.float64) - ref["bins"][word])
        assert (diff[scale == 0.0] == 0.0).all(), word
        if (scale > 0.0).any():
            worst = max(worst, float(np.max(diff[scale > 0.0] / scale[scale > 0.0])))
    return worst


def exact_equal(got_bins, ref_bins):
    return all(np.asarray(got_bins[w]).tobytes() == ref_bins[w].tobytes() for w in INTEGERS + EXACT_WORDS)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
CAPACITIES = (64, 128, 256, 1024, 4096)
COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 257, 1025)
BINS = tuple(sorted({1, G_BUILT - 1, G_BUILT, G_BUILT + 1, 32}))
LATTICE_Q, GAUSSIAN_Q = 4, 64


def lattice_state(n, seed):
    """(pos, vel): positions, velocities and masses on quarter-integers, so s, rv, v2 and ww are exact; a cube narrow enough
    for coincident bodies and for many pairs at a distance exactly on an edge."""
    rng = np.random.default_rng(seed)
    side = 3 if n <= 130 else 6
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.integers(-4 * side, 4 * side + 1, size=(n, 3)) / 4.0
    pos[:, 3] = rng.integers(1, 9, size=n) / 4.0
    vel[:, :3] = rng.integers(-32, 33, size=(n, 3)) / 4.0
    vel[:, 3] = np.nan                                                          # the fourth velocity word is not read
    return pos, vel


def gaussian_state(n, seed):
    """(pos, vel): Gaussian positions rounded to 1 / 64 within +-8 (see the module's docstring), Gaussian velocities and
    uniform masses as fp32 draws them."""
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = np.clip(np.round(rng.normal(0.0, 2.0, size=(n, 3)) * 64.0), -512, 512) / 64.0
    pos[:, 3] = rng.uniform(0.5, 1.5, size=n)
    vel[:, :3] = rng.normal(0.0, 1.0, size=(n, 3))
    vel[:, 3] = -7.0
    return pos, vel


def counts_of(capacity):
    if capacity == 4096:
        return [4096, 1025]
    return [c for c in COUNTS if c <= capacity] + [capacity]


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, V, counts, Q): one system per count; even systems lattice states, odd ones Gaussian states.  From 63 bodies on a
    system holds a body with a NaN coordinate (5), one with an infinite velocity word (9) and two coincident bodies (11, 12)."""
    counts = counts_of(capacity)
    B = len(counts)
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    Q = []
    for s, n in enumerate(counts):
        q = LATTICE_Q if s % 2 == 0 else GAUSSIAN_Q
        Q.append(q)
        p, v = (lattice_state if q == LATTICE_Q else gaussian_state)(n, 100 * capacity + s)
        if n >= 63:
            p[5, 1] = np.nan
            v[9, 0] = np.inf
            p[12, :3] = p[11, :3]
        P[s, :n], V[s, :n] = p, v
    P[:, :, 3] = np.where(np.arange(capacity)[None, :] < np.array(counts)[:, None], P[:, :, 3], 3.0)   # words beyond the count
    P.flags.writeable = V.flags.writeable = False
    return P, V, counts, tuple(Q)


def shared_edges(bins):
    """Edge 0 = 0 (the coincident pairs are `below`), then equal steps: 2 up to three bins, 1.5 up to eight, 0.5 beyond; integer
    distances of the lattice meet an edge exactly."""
    step = 2.0 if bins <= 3 else (1.5 if bins <= 8 else 0.5)
    return (step * np.arange(bins + 1)).astype(np.float32)


def system_edges(bins, B):
    """(B, bins + 1): system s starts at 0 (even s) or 0.25 (odd s) and steps by (s % 5 + 2) / (bins <= 3 ? 2 : 8)."""
    s = np.arange(B)[:, None]
    return (0.25 * (s % 2) + (s % 5 + 2) / (2.0 if bins <= 3 else 8.0) * np.arange(bins + 1)[None, :]).astype(np.float32)


MASKS = ("none", "sparse", "disjoint")


@functools.lru_cache(maxsize=None)
def gpu_masks(capacity, kind):
    """(rows, sources): (B, capacity) bool arrays or None.  Bytes beyond a system's count are set too, and change nothing."""
    B = len(counts_of(capacity))
    rng = np.random.default_rng(2000 + capacity)
    a, b = rng.random((B, capacity)) < 0.5, rng.random((B, capacity)) < 0.1
    a[:, :16] = True
    b[:, :16] = rng.random((B, 16)) < 0.5
    masks = {"none": (None, None), "sparse": (a, b), "disjoint": (a, ~a)}[kind]
    for m in masks:
        if m is not None:
            m.flags.writeable = False
    return masks


#: (name, bins, weight, masks, per-system edges): every number of bins around the passes of the kernel built, both weights,
#: the masks, per-system edges.
CASES = tuple([(f"bins{b}", b, WEIGHT_NUMBER, "none", False) for b in BINS] +
              [("mass-sparse", G_BUILT + 1, WEIGHT_MASS, "sparse", False), ("mass-disjoint-own-edges", 32, WEIGHT_MASS, "disjoint", True),
               ("number-sparse-own-edges", G_BUILT + 1, WEIGHT_NUMBER, "sparse", True), ("mass", 8, WEIGHT_MASS, "none", False)])
LARGE_CASES = (("mass", 8, WEIGHT_MASS, "none", False),)                        # capacity 4096: 8 bins only


def cases_of(capacity):
    return LARGE_CASES if capacity == 4096 else CASES


def gpu_edges(capacity, bins, per_system):
    return system_edges(bins, len(counts_of(capacity))) if per_system else shared_edges(bins)


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity, name, jitter_seed=None):
    """The references of gpu_inputs(capacity) in case `name`, one dict per system; computed once per session."""
    _, bins, weight, kind, per_system = next(c for c in cases_of(capacity) if c[0] == name)
    P, V, counts, Q = gpu_inputs(capacity)
    rows, sources = gpu_masks(capacity, kind)
    edges = gpu_edges(capacity, bins, per_system)
    rng = None if jitter_seed is None else np.random.default_rng(jitter_seed)
    return [reference(P[s], V[s], counts[s], Q[s], edges[s] if per_system else edges, None if rows is None else rows[s],
                      None if sources is None else sources[s], weight, rng) for s in range(len(counts))]


def jitter_spread(capacities=(64, 128, 256), seed=77):
    """(spread, same): the largest error measure of the reference with every root and quotient moved by up to one ulp at
    random, against itself unmoved; and whether every integer and every exact word stayed the same bits."""
    spread, same = 0.0, True
    for capacity in capacities:
        for name, *_ in cases_of(capacity):
            for ref, moved in zip(gpu_reference(capacity, name), gpu_reference(capacity, name, seed)):
                spread = max(spread, error_of(moved["bins"], ref))
                same = same and exact_equal(moved["bins"], ref["bins"]) and moved["system"].tobytes() == ref["system"].tobytes()
    return spread, same


# ---- a plain pair walk: the independent check of the reference -------------------------------------------------------------------
def plain_walk(pos, vel, n, edges, rows=None, sources=None, weight=WEIGHT_NUMBER):
    """(count (bins,), sums (bins, 9), absolute (bins, 9)) by vectorised numpy over all pairs at once, in any order: float64
    separations against float64 edges (the inputs keep every pair away from an edge's rounding: lattices), np.sum."""
    pos, vel = np.asarray(pos)[:n].astype(np.float64), np.asarray(vel)[:n].astype(np.float64)
    row = np.ones(n, bool) if rows is None else np.asarray(rows)[:n] != 0
    source = np.ones(n, bool) if sources is None else np.asarray(sources)[:n] != 0
    e = np.asarray(edges, np.float64)
    bins = len(e) - 1
    with np.errstate(all="ignore"):
        d = pos[None, :, :3] - pos[:, None, :3]
        w = vel[None, :, :3] - vel[:, None, :3]
        s, rv, v2 = (d * d).sum(-1), (d * w).sum(-1), (w * w).sum(-1)
        ok = row[:, None] & source[None, :] & ~np.eye(n, dtype=bool) & np.isfinite(s) & np.isfinite(v2)
        r = np.sqrt(s)
        vr = rv / r
        ww = np.ones_like(s) if weight == WEIGHT_NUMBER else pos[:, None, 3] * pos[None, :, 3]
        words = np.stack([ww, ww * r, ww * s, ww * rv, ww * vr, ww * vr * vr, ww * np.maximum(v2 - vr * vr, 0), ww * np.sqrt(v2), ww * v2], -1)
    count, sums, absolute = np.zeros(bins, np.int64), np.zeros((bins, 9)), np.zeros((bins, 9))
    for t in range(bins):
        inside = ok & (s > e[t] * e[t]) & (s <= e[t + 1] * e[t + 1])
        count[t] = inside.sum()
        sums[t] = words[inside].sum(axis=0)
        absolute[t] = np.abs(words[inside]).sum(axis=0)
    return count, sums, absolute
