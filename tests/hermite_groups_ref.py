"""Numpy reference of nbody_batch_groups (include/nbody_batch_groups.h), in two independent parts.

``union_find`` links the pairs whose fp64 distance is within the linking length and joins them with a union-find: the truth
for ``group`` and ``size``, which knows nothing of sweeps.  ``schedule`` mirrors the header's schedule -- Link, Hook, Compress,
all reads of a step before its writes -- and gives ``sweeps``, ``converged`` and the labels a bounded run ends with;
``records`` forms the fp64 sums of a labelling member by member in ascending index, and the system summary.

The fp32 predicate of the library and the fp64 one of the truth agree wherever no pair sits on the linking length: ``margin``
is the smallest ``|r2 / b2 - 1|`` over all pairs of a system, and test_batch_groups_cpu.py holds every input of the GPU suite to
``MARGIN`` = 1e-4, a thousand times the few 1e-7 that three fp32 roundings can move r2 by.  Those inputs, not a tolerance,
carry the GPU test."""
import functools

import numpy as np

MAX_SWEEPS = 64
MARGIN = 1e-4
WEIGHT_MASS, WEIGHT_NUMBER = "mass", "number"
BLOCK = 512  # rows per block of the n x n distance work


def _r2(x, lo, hi):
    """fp64 squared distances of the rows lo ... hi - 1 to all bodies, from the fp32 coordinates."""
    d = x[None, :, :] - x[lo:hi, None, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def edges(pos, n, b):
    """(i, j, margin): the friend pairs i != j, both orders, row-major, by the fp64 distances of the fp32 coordinates against
    b2 = (double)b (double)b with b as fp32; and the smallest |r2 / b2 - 1| over all pairs (inf for b = 0 or n < 2).  NaN
    links to nothing."""
    x = np.asarray(pos, dtype=np.float32)[:n, :3].astype(np.float64)
    b2 = float(np.float32(b)) ** 2
    ii, jj, margin = [], [], np.inf
    for lo in range(0, n, BLOCK):
        hi = min(lo + BLOCK, n)
        r2 = _r2(x, lo, hi)
        rows = np.arange(lo, hi)
        with np.errstate(invalid="ignore"):
            f = r2 <= b2
        f[rows - lo, rows] = False
        i, j = np.nonzero(f)
        ii.append(i + lo)
        jj.append(j)
        if b2 > 0 and n > 1:
            with np.errstate(invalid="ignore"):
                rel = np.abs(r2 / b2 - 1.0)
            rel[rows - lo, rows] = np.inf
            rel[np.isnan(rel)] = np.inf
            margin = min(margin, float(rel.min()))
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), margin
    return np.concatenate(ii), np.concatenate(jj), margin


def union_find(pos, n, b):
    """(group, size): every body's group as the lowest index connected to it, and the members of that group.  A union-find
    with path halving over the friend pairs i < j; the lower root always wins, so a root is its group's lowest index."""
    i, j, _ = edges(pos, n, b)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, c in zip(i.tolist(), j.tolist()):
        if a < c:
            ra, rc = find(a), find(c)
            if ra != rc:
                parent[max(ra, rc)] = min(ra, rc)
    group = np.array([find(a) for a in range(n)], dtype=np.int32).reshape(n)
    size = np.bincount(group, minlength=n)[group].astype(np.int32) if n else np.zeros(0, np.int32)
    return group, size


def schedule(pos, n, b, max_sweeps=MAX_SWEEPS, hook=True, pairs=None):
    """(labels, sweeps, converged) of the header's schedule.  hook=False leaves the root alone (plain min-label sweeps with
    compression): what the hook is measured against.  pairs: edges(pos, n, b), where the caller has them already."""
    i, j, _ = edges(pos, n, b) if pairs is None else pairs
    L = np.arange(n, dtype=np.int64)
    sweeps, converged = 0, 1
    if n == 0:
        return L.astype(np.int32), sweeps, converged
    for t in range(1, max_sweeps + 1):
        # Link: all reads
        c = L.copy()
        np.minimum.at(c, i, L[j])
        lowered = c < L
        sweeps = t
        if not lowered.any():
            converged = 1
            break
        converged = 0
        # Hook: the roots take the minimum of what their rows found, the rows take what they found
        new = L.copy()
        if hook:
            np.minimum.at(new, L[lowered], c[lowered])
        np.minimum.at(new, np.flatnonzero(lowered), c[lowered])
        L = new
        # Compress: all rows at once until a pass changes nothing
        while True:
            nxt = L[L]
            if np.array_equal(nxt, L):
                break
            L = nxt
    return L.astype(np.int32), sweeps, converged


def records(pos, vel, n, labels, m=None, weight=WEIGHT_MASS, min_members=2, sweeps=0, converged=1):
    """The records of a labelling: per body (group, size), per slot the group records at the roots (zero elsewhere), and the
    system summary.  The sums run over the members in ascending index, one fp64 addition each, as the header says."""
    m = n if m is None else min(m, n)
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int32)[:n]
    out = {"group": labels.copy(), "size": np.zeros(n, np.int32), "weight": np.zeros(n), "centre": np.zeros((n, 3)),
           "velocity": np.zeros((n, 3)), "count": np.zeros(n, np.int32), "sources": np.zeros(n, np.int32)}
    if weight == WEIGHT_NUMBER:
        w = np.ones(n, dtype=np.float64)
    else:
        w = np.where(np.arange(n) < m, pos[:n, 3].astype(np.float64), 0.0)     # a tracer's mass word is not read into anything
    x, v = pos[:n, :3].astype(np.float64), vel[:n, :3].astype(np.float64)
    groups = grouped = singles = 0
    largest, largest_count = -1, 0
    for r in np.flatnonzero(labels == np.arange(n)).tolist():
        members = np.flatnonzero(labels == r)
        sw, sx, sv = 0.0, np.zeros(3), np.zeros(3)
        for k in members.tolist():                   # ascending, sequential
            sw += w[k]
            sx += w[k] * x[k]
            sv += w[k] * v[k]
        count = len(members)
        out["size"][members] = count
        out["weight"][r], out["count"][r], out["sources"][r] = sw, count, int((members < m).sum())
        if sw != 0.0:
            with np.errstate(invalid="ignore", over="ignore"):
                out["centre"][r], out["velocity"][r] = sx / sw, sv / sw
        if count >= min_members:
            groups, grouped = groups + 1, grouped + count
        singles += count == 1
        if count > largest_count:                    # ascending roots: ties stay with the lower root
            largest, largest_count = r, count
    out.update({"groups": groups, "grouped": grouped, "singles": int(singles), "largest": largest, "largest_count": largest_count,
                "sweeps": sweeps, "converged": converged})
    return out


def groups(pos, vel, n, b, m=None, weight=WEIGHT_MASS, min_members=2, max_sweeps=MAX_SWEEPS):
    """The whole reference of one system: the schedule's labels, sweeps and converged, their records, and beside them the
    union-find's truth as ``true_group`` and ``true_size``."""
    labels, sweeps, converged = schedule(pos, n, b, max_sweeps)
    out = records(pos, vel, n, labels, m, weight, min_members, sweeps, converged)
    out["true_group"], out["true_size"] = union_find(pos, n, b)
    return out


def margin(pos, n, b):
    return edges(pos, n, b)[2]


# ---- the inputs -----------------------------------------------------------------------------------------------------------
FILL = 0.5                       # what the slots beyond a system's count hold: numbers that nothing may read
#: the capacities of the GPU suite: one wave with one row per lane, two rows per lane, four rows per lane in two waves, and
#: sixteen waves with the raised LDS limit
CAPACITIES = (64, 128, 320, 4096)
CHAIN_B = 1.25                   # unit spacing: neighbours at r2 = 1, next neighbours at r2 = 4, b2 = 1.5625
CUBE_SPACINGS = 0.87
HALF_MASS_RADIUS = 1.3048        # of a Plummer sphere of scale radius 1


def _dress(x, seed):
    """(pos, vel) (n, 4) float32 from coordinates: masses 0.5 ... 1.5 over n, velocities normal."""
    n = x.shape[0]
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = x
    pos[:, 3] = rng.uniform(0.5, 1.5, n) / max(n, 1)
    vel[:, :3] = rng.normal(0.0, 0.5, (n, 3)) + np.array([0.3, -0.2, 0.1])
    return pos, vel


def chain(n, seed=0):
    """A chain of n bodies at unit spacing along (2, 3, 6) / 7 in a random index order: one group at b = 1.25, and the worst
    case for label propagation, which the hook is there for."""
    rng = np.random.default_rng(1000 + seed)
    place = rng.permutation(n).astype(np.float64)
    return _dress(place[:, None] * (np.array([2.0, 3.0, 6.0]) / 7.0), seed)


def plummer_spacing(n):
    """The mean interparticle spacing within the half-mass radius of a Plummer sphere of n bodies."""
    return (4.0 / 3.0 * np.pi * HALF_MASS_RADIUS ** 3 / max(n / 2.0, 1.0)) ** (1.0 / 3.0)


CLUMP_RADIUS, CLUMP_OFFSET = 3.0, 3.5   # the clumps are cut at radius 3 and centred at x = -+ 3.5 or further: they do not touch


def bridge(n, seed=0, middle=True):
    """(pos, vel, b): two Plummer clumps, cut at CLUMP_RADIUS, whose centres are joined by a straight bridge of k bodies 0.8 b
    apart (k odd, so that the bridge has a middle body), in a random index order: n bodies with the bridge's middle body and
    n - 1 without it (the others keep their order).  b is one mean spacing of a clump.  With the middle body the two cores are
    one group; without it the bridge has a gap of 1.6 b."""
    from n_body_problem_amd import plummer
    b = float(np.float32(plummer_spacing((n - 7) // 2)))
    k = 2 * int(np.ceil(CLUMP_OFFSET / (0.8 * b))) - 1           # 0.8 b (k + 1) >= 2 CLUMP_OFFSET
    half = 0.4 * b * (k + 1)
    n1 = (n - k) // 2
    n2 = n - k - n1
    a, _ = plummer(n1, seed=300 + seed, r_max=CLUMP_RADIUS)
    c, _ = plummer(n2, seed=400 + seed, r_max=CLUMP_RADIUS)
    x = np.zeros((n, 3))
    x[:n1] = a[:, :3].astype(np.float64) - [half, 0, 0]
    x[n1:n1 + n2] = c[:, :3].astype(np.float64) + [half, 0, 0]
    x[n1 + n2:, 0] = -half + 0.8 * b * (np.arange(k) + 1)
    order = np.random.default_rng(2000 + seed).permutation(n)
    keep = order if middle else order[order != n1 + n2 + k // 2]
    pos, vel = _dress(x[keep], 50 + seed)
    return pos, vel, b


def cube(n, seed=0):
    """(pos, vel, b): n bodies uniform in the unit cube, b = 0.87 mean spacings: many groups of many sizes."""
    rng = np.random.default_rng(3000 + seed)
    pos, vel = _dress(rng.random((n, 3)), 80 + seed)
    return pos, vel, float(np.float32(CUBE_SPACINGS * n ** (-1.0 / 3.0)))


#: the seeds of the clumps and of the cube at each capacity.  At 4096 bodies a few of the sixteen million pairs come within 1e-4
#: of the linking length under most seeds; these keep MARGIN (test_batch_groups_cpu.py asserts it)
BRIDGE_SEED = {64: 64, 128: 128, 320: 320, 4096: 4118}
CUBE_SEED = {64: 64, 128: 128, 320: 320, 4096: 4099}


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity, which):
    """(P, V, counts, b) of the GPU suite's two batches at a capacity; both hold systems of 0, 1, 2 and capacity bodies.
    "a": the permuted chain at the capacity, an empty system, the two clumps with their bridge (capacity - 1 bodies), a lone
    body, the same clumps without the bridge's middle body (capacity - 2) and two friends.
    "b": two bodies that are no friends, the uniform cube at the capacity, an empty system, a lone body and a permuted chain of
    capacity - 3 bodies.  Cached and read-only."""
    if which == "a":
        with_middle = bridge(capacity - 1, BRIDGE_SEED[capacity])
        without = bridge(capacity - 1, BRIDGE_SEED[capacity], middle=False)
        systems = [chain(capacity, capacity) + (CHAIN_B,), _dress(np.zeros((0, 3)), 1) + (1.0,), with_middle,
                   chain(1, 3) + (CHAIN_B,), without, chain(2, 5) + (CHAIN_B,)]
    else:
        far = _dress(np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), 7)
        systems = [far + (CHAIN_B,), cube(capacity, CUBE_SEED[capacity]), _dress(np.zeros((0, 3)), 2) + (0.0,), chain(1, 4) + (0.0,),
                   chain(capacity - 3, capacity + 1) + (CHAIN_B,)]
    counts = [s[0].shape[0] for s in systems]
    P = np.full((len(systems), capacity, 4), FILL, dtype=np.float32)
    V = np.full((len(systems), capacity, 4), FILL, dtype=np.float32)
    for slot, (pos, vel, _) in enumerate(systems):
        P[slot, :counts[slot]], V[slot, :counts[slot]] = pos, vel
    b = np.array([s[2] for s in systems], dtype=np.float32)
    for a in (P, V, b):
        a.setflags(write=False)
    return P, V, counts, b


@functools.lru_cache(maxsize=None)
def reference(capacity, which):
    """The references of the systems of gpu_inputs(capacity, which), computed once and shared."""
    P, V, counts, b = gpu_inputs(capacity, which)
    return [groups(P[s], V[s], n, b[s]) for s, n in enumerate(counts)]


MASSIVE_CAPACITY = 128


@functools.lru_cache(maxsize=None)
def massive_inputs():
    """(P, V, counts, massive, b): cubes and clumps at capacity 128 whose first bodies are massive; one massive count is 0 and
    one is above its system's count."""
    systems = [cube(128, 11), bridge(97, 12), cube(64, 13), cube(50, 14)]
    counts, massive = [128, 97, 64, 50], [40, 128, 9, 0]
    P = np.full((4, MASSIVE_CAPACITY, 4), FILL, dtype=np.float32)
    V = np.full_like(P, FILL)
    for s, (pos, vel, _) in enumerate(systems):
        P[s, :counts[s]], V[s, :counts[s]] = pos, vel
    b = np.array([s[2] for s in systems], dtype=np.float32)
    for a in (P, V, b):
        a.setflags(write=False)
    return P, V, counts, massive, b


INVARIANCE_BODIES = 60


@functools.lru_cache(maxsize=None)
def invariance_inputs():
    """(pos, vel, b), (pos, vel, b): the 60-body system that moves between slots, batches and capacities, and its neighbour."""
    return cube(INVARIANCE_BODIES, 71), bridge(INVARIANCE_BODIES, 72)


LADDER_BODIES, LADDER_SLOTS = 64, 6


@functools.lru_cache(maxsize=None)
def ladder_inputs():
    """(pos, vel, b): one 64-body cube and six linking lengths from 0.5 to 1.6 mean spacings, for the same state in every slot."""
    pos, vel, _ = cube(LADDER_BODIES, 91)
    b = (np.array([0.5, 0.7, 0.87, 1.0, 1.25, 1.6]) * LADDER_BODIES ** (-1.0 / 3.0)).astype(np.float32)
    b.setflags(write=False)
    return pos, vel, b
