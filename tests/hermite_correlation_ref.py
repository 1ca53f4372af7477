"""Numpy reference of nbody_batch_correlation (include/nbody_batch_correlation.h) over exact integer arithmetic, and the inputs of
its tests.

Every finite coordinate is an integer in [-512, 512], so every difference, square and sum of the fp32 chain is exact and r2 is
an integer below 2^24, the same number in fp32, in fp64 and in int32; edges are halves or integers, so their fp32 squares are
exact too (test_batch_correlation_cpu.py checks the premise on every input).  A pair is then within an edge iff its integer r2
is <= floor(e2), and the cumulative counts are sums over a histogram of the integers, taken once per system and pair of masks.
A body with a NaN or an infinite coordinate has no measured pair: its r2 is NaN or +inf with every other body."""
import functools

import numpy as np

MAX_BINS = 32
CAPACITIES = (64, 128, 320, 4096)
BINS = (1, 8, 9, 32)                 # the GPU suite: every instantiation boundary
DRIVER_BINS = (1, 8, 9, 16, 17, 32)  # the CPU driver
MASKS = ("none", "rows", "sources", "disjoint", "overlapping")
LIMIT = 512                          # |coordinate| <=
TOP = 3 * (2 * LIMIT) ** 2 + 1       # above every measured r2: the code of an unmeasured pair
FLT_MAX = np.finfo(np.float32).max


# ---- the reference -----------------------------------------------------------------------------------------------------------
def r2_codes(pos, n):
    """int32 (n, n): the exact r2 of every ordered pair, TOP where it is not measured (a NaN or infinite coordinate)."""
    x = np.asarray(pos)[:n, :3].astype(np.float64)
    finite = np.isfinite(x).all(axis=1)
    xi = np.where(finite[:, None], x, 0.0).astype(np.int32)
    r2 = np.zeros((n, n), np.int32)
    for c in range(3):
        d = xi[:, c][:, None] - xi[:, c][None, :]
        r2 += d * d
    r2[~finite, :] = TOP
    r2[:, ~finite] = TOP
    return r2


def cumulative_histogram(codes, row, source):
    """(H, pairs...): H[k] = examined ordered pairs with r2 <= k for k < TOP (int64), so H[-1] is the measured pairs."""
    n = len(codes)
    row, source = np.asarray(row[:n], bool), np.asarray(source[:n], bool)
    hist = np.bincount(codes[row][:, source].ravel(), minlength=TOP + 1).astype(np.int64)
    both = row & source
    np.subtract.at(hist, codes[both, both], 1)                  # a body is never paired with itself
    return np.cumsum(hist[:TOP]), int(row.sum()), int(source.sum()), int(both.sum())


def squared_edges(edges):
    """e2 as the library forms it: one fp32 product per edge; a product that overflows is the largest finite value."""
    e = np.asarray(edges, np.float32)
    with np.errstate(over="ignore"):
        e2 = e * e
    return np.where(np.isfinite(e2), e2, FLT_MAX).astype(np.float32)


def from_histogram(hist, edges):
    """Every word nbody_batch_correlation returns for one system, as a dict, from cumulative_histogram's tuple."""
    H, rows, sources, both = hist
    e2 = squared_edges(edges).astype(np.float64)
    within = H[np.minimum(np.floor(e2), TOP - 1).astype(np.int64)]
    pairs, measured = rows * sources - both, int(H[-1])
    return {"rows": rows, "sources": sources, "both": both, "bins": len(e2) - 1, "pairs": pairs, "below": int(within[0]),
            "above": measured - int(within[-1]), "unmeasured": pairs - measured, "counts": np.diff(within).astype(np.int64)}


def reference(pos, n, edges, rows=None, sources=None):
    row = np.ones(n, bool) if rows is None else np.asarray(rows)[:n] != 0
    source = np.ones(n, bool) if sources is None else np.asarray(sources)[:n] != 0
    return from_histogram(cumulative_histogram(r2_codes(pos, n), row, source), edges)


def check_identity(ref):
    assert ref["below"] + int(np.sum(ref["counts"])) + ref["above"] + ref["unmeasured"] == ref["pairs"] \
        == ref["rows"] * ref["sources"] - ref["both"]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def cube(n, seed, side):
    """n bodies at random integer positions of a cube of half-width ``side``: (n, 4) float32, mass 1."""
    out = np.ones((n, 4), np.float32)
    out[:, :3] = np.random.default_rng(seed).integers(-side, side + 1, size=(n, 3))
    return out


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, counts): five systems of 0, 1, 2, min(65, capacity) and capacity bodies.  The two large ones are cubes narrow enough
    for coincident bodies and for many pairs at integer distances (3, 6, 9, ...: exactly on an edge); the fourth holds a body with
    a NaN coordinate and one at +inf, the last a body at the limit of the grid."""
    counts = [0, 1, 2, min(65, capacity), capacity]
    P = np.zeros((5, capacity, 4), np.float32)
    P[1, :1] = cube(1, 11, 5)
    P[2, :2] = [[3, -2, 7, 1], [3, 1, 3, 1]]                    # at distance 5 exactly
    P[3, :counts[3]] = cube(counts[3], 13, 6)
    P[3, 5, 1] = np.nan
    P[3, 9, 0] = np.inf
    P[4, :capacity] = cube(capacity, 14 + capacity, 4 if capacity <= 128 else (6 if capacity <= 320 else 14))
    P[4, capacity - 1, :3] = [LIMIT, -LIMIT, LIMIT]
    P[4, 0, :3] = [-LIMIT, LIMIT, -LIMIT]
    P.flags.writeable = False
    return P, counts


def shared_edges(bins):
    """bins + 1 multiples of 1.5 from 0: r = 3, 6, 9, ... meet an edge exactly, and edge 0 = 0 counts the coincident pairs."""
    return (1.5 * np.arange(bins + 1)).astype(np.float32)


def system_edges(bins, B):
    """(B, bins + 1): system s steps by (s + 2) / 2 from 0 (even s) or from 0.5 (odd s: coincident pairs are `below`)."""
    s = np.arange(B)[:, None]
    return (0.5 * (s % 2) + 0.5 * (s + 2) * np.arange(bins + 1)[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gpu_masks(capacity, kind):
    """(rows, sources): (5, capacity) bool arrays or None.  Bytes beyond a system's count are set too, and change nothing."""
    rng = np.random.default_rng(1000 + capacity)
    a, b = rng.random((5, capacity)) < 0.5, rng.random((5, capacity)) < 0.4
    masks = {"none": (None, None), "rows": (a, None), "sources": (None, b), "disjoint": (a, ~a), "overlapping": (a, b)}[kind]
    for m in masks:
        if m is not None:
            m.flags.writeable = False
    return masks


@functools.lru_cache(maxsize=None)
def gpu_codes(capacity, s):
    P, counts = gpu_inputs(capacity)
    codes = r2_codes(P[s], counts[s])
    codes.flags.writeable = False
    return codes


@functools.lru_cache(maxsize=None)
def gpu_histogram(capacity, s, kind):
    n = gpu_inputs(capacity)[1][s]
    rows, sources = gpu_masks(capacity, kind)
    return cumulative_histogram(gpu_codes(capacity, s), np.ones(n, bool) if rows is None else rows[s],
                                np.ones(n, bool) if sources is None else sources[s])


def gpu_edges(bins, per_system):
    return system_edges(bins, 5) if per_system else shared_edges(bins)


def gpu_reference(capacity, bins, per_system, kind):
    """The references of gpu_inputs(capacity), one dict per system: the histograms are taken once per system and masks."""
    edges = gpu_edges(bins, per_system)
    return [from_histogram(gpu_histogram(capacity, s, kind), edges[s] if per_system else edges) for s in range(5)]


# ---- adversarial inputs --------------------------------------------------------------------------------------------------------
def rows_of(xyz):
    out = np.ones((len(xyz), 4), np.float32)
    out[:, :3] = xyz
    return out


def tied_edges():
    """Two adjacent edges of sub-normal scale whose fp32 squares coincide (both products underflow to 0), then 1 and 2."""
    a = np.float32(1e-23)
    b = np.nextafter(a, np.float32(1))
    assert b > a and np.float32(a * a) == np.float32(b * b) == 0
    return np.array([a, b, 1.0, 2.0], np.float32)
