"""Numpy reference of nbody_batch_neighbours (include/nbody_batch_neighbours.h) over exact integer arithmetic, and the inputs of
its tests.

Every input lies on hermite_span_ref's grid: integer coordinates in [0, 1024), optionally scaled by a power of two, so every
difference, square and sum of the fp32 chain is exact and r2 is the same number in fp32 and in fp64, whose bits as int64 order
as it does (test_batch_neighbours_cpu.py checks the premise on every input).  A row's list is then a stable argsort of int64 r2 with the
row's own column and the columns that are no sources removed: stable, so ties go to the lower index, which is the header's
order.  ``within`` is a comparison of the fp32 values, ``mutual`` a look at the nearest's nearest, and the two means are
sequential fp64 sums in ascending row."""
import functools

import numpy as np

import hermite_span_ref as sref

MAX = 8
KS = (1, 6, 8)
CAPACITIES = sref.CAPACITIES
BLOCK = 512


def r2_float(pos, n, rows):
    """float32 (len(rows), n): the squared distances of the bodies ``rows`` to all bodies, exact on grid inputs."""
    return sref.r2_exact(sref.positions64(pos, n), rows).astype(np.float32)


def nearest_eight(pos, n, radius=None, sources=None):
    """(index, r2, within): every row's eight nearest candidates, (n, 8) with -1 and +inf where there are fewer, and the
    candidates within the radius.  The lists of every k are the first k columns."""
    sel = np.ones(n, bool) if sources is None else (np.asarray(sources)[:n] != 0)
    index = np.full((n, MAX), -1, np.int32)
    r2 = np.full((n, MAX), np.inf, np.float32)
    within = np.zeros(n, np.int32)
    b2 = None if radius is None else np.float32(radius) * np.float32(radius)       # one fp32 product
    cols = np.flatnonzero(sel)
    for lo in range(0, n, BLOCK):
        rows = np.arange(lo, min(lo + BLOCK, n))
        d = r2_float(pos, n, rows)
        whole = sref.r2_bits(d)        # int64: r2 is never negative, so its bits order as its value does (the grid may be scaled)
        for a, i in enumerate(rows):
            cand = cols[cols != i]
            order = cand[np.argsort(whole[a, cand], kind="stable")][:MAX]
            index[i, :len(order)], r2[i, :len(order)] = order, d[a, order]
            if b2 is not None:
                within[i] = int((d[a, cand] <= b2).sum())
    return index, r2, within


def reference(pos, n, k, radius=None, sources=None, eight=None):
    """Every word nbody_batch_neighbours returns for one system of n bodies, as a dict: index and r2 (n, k), found and within
    (n,), and the system's words.  ``eight``: what nearest_eight gave for the same arguments, to share it among the k."""
    index8, r28, within = eight if eight is not None else nearest_eight(pos, n, radius, sources)
    index, r2 = np.ascontiguousarray(index8[:, :k]), np.ascontiguousarray(r28[:, :k])
    found = (index >= 0).sum(axis=1).astype(np.int32)
    selected = n if sources is None else int((np.asarray(sources)[:n] != 0).sum())
    nearest = index[:, 0]
    listed = found >= 1
    complete = found == k
    mutual = np.array([listed[i] and nearest[nearest[i]] == i for i in range(n)], bool)
    near_terms = np.sqrt(r2[listed, 0].astype(np.float64))
    kth_terms = np.sqrt(r2[complete, k - 1].astype(np.float64))
    return {"index": index, "r2": r2, "found": found, "within": within, "bodies": n, "sources": selected,
            "listed": int(listed.sum()), "complete": int(complete.sum()), "mutual": int(mutual.sum()),
            "mean_nearest": sref.sequential_sum(near_terms) / float(listed.sum()) if listed.any() else 0.0,
            "mean_kth": sref.sequential_sum(kth_terms) / float(complete.sum()) if complete.any() else 0.0}


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, counts): hermite_span_ref's systems of this capacity (ragged counts, 0, 1 and 2 among them) and behind them systems
    of 6, 7, 8 and 9 bodies: k and k + 1 for the lists of 6 and 8."""
    P0, counts0 = sref.gpu_inputs(capacity)
    extra = [sref.cube(m, seed=20 + m, side=3) for m in (6, 7, 8, 9)]
    P = np.zeros((len(counts0) + len(extra), capacity, 4), np.float32)
    P[:len(counts0)] = P0
    for s, rows in enumerate(extra):
        P[len(counts0) + s, :len(rows)] = rows
    P.flags.writeable = False
    return P, list(counts0) + [len(rows) for rows in extra]


def radius_of(pos, n):
    """A radius that is some pair's distance exactly (so that <= is met with equality), about the tenth of the sorted pair
    distances of the first rows; 1 for a system without a pair."""
    if n < 2:
        return np.float32(1.0)
    d = r2_float(pos, n, np.arange(min(n, 16)))
    d = np.sort(d[d > 0])
    r = np.sqrt(np.float64(d[len(d) // 10]))
    return np.float32(r) if np.float32(r) * np.float32(r) == d[len(d) // 10] else np.float32(r * 1.0001)


@functools.lru_cache(maxsize=None)
def gpu_radii(capacity):
    P, counts = gpu_inputs(capacity)
    return np.array([radius_of(P[s], n) for s, n in enumerate(counts)], np.float32)


@functools.lru_cache(maxsize=None)
def gpu_eights(capacity):
    P, counts = gpu_inputs(capacity)
    radii = gpu_radii(capacity)
    return [nearest_eight(P[s], n, radius=radii[s]) for s, n in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity, k):
    """The references of gpu_inputs(capacity) with gpu_radii(capacity): the search is done once per capacity."""
    P, counts = gpu_inputs(capacity)
    radii = gpu_radii(capacity)
    return [reference(P[s], n, k, radius=radii[s], eight=e) for (s, n), e in zip(enumerate(counts), gpu_eights(capacity))]


def has_zero_distance(pos, n):
    """Whether two bodies of the system coincide (the random cubes and the spheres' cores do; the lattice and the chain do
    not): there nbody_batch_structure, which counts no pair at distance 0, and the lists differ."""
    x = sref.positions64(pos, n)
    return len(np.unique(x, axis=0)) < n


@functools.lru_cache(maxsize=None)
def source_inputs(capacity):
    """(pos, n, masks): hermite_span_ref's cluster of ``capacity - 3`` bodies and five masks over the capacity: none, all, a
    single body, a random 20, and the first 8."""
    pos, n, _ = sref.subset_inputs(capacity)
    masks = np.zeros((5, capacity), np.uint8)
    masks[1, :] = 1
    masks[2, n // 2] = 1
    masks[3, np.random.default_rng(31).choice(n, size=20, replace=False)] = 1
    masks[4, :8] = 1
    masks.flags.writeable = False
    return pos, n, masks
