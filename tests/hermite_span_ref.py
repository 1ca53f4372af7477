"""Numpy reference of nbody_batch_span (include/nbody_batch_span.h), in two independent parts, and the inputs of its tests.

``prim`` is Prim's algorithm over the exact 64-bit keys: the truth for the edges, which knows nothing of rounds.  ``rounds``
mirrors the header's rounds literally -- every component's minimum, the decision of every component, Hook, Compress, all reads
of a step before its writes -- and gives ``rounds``, ``nearest`` and, once more, the edges.  ``reference`` adds the fp64 sums.

Every input lies on a grid: integer coordinates in [0, 1024), optionally scaled by a power of two.  Every difference, square
and sum of the fp32 chain is then exact (r2 stays below 2^22 grid units), so r2 is the same number in fp32 and in the fp64
arithmetic used here, and int64 arithmetic gives every key exactly.  Equal lengths are plentiful, which is what the tie rule
has to survive.  test_batch_span_cpu.py checks the premise on every input."""
import functools

import numpy as np

MAX_ROUNDS = 13
INDEX_BITS = 12
NO_KEY = np.int64(-1)                      # the all-ones word
BIG = np.int64(np.iinfo(np.int64).max)     # above every key (keys stay below 2^56)
GRID = 1024
CAPACITIES = (64, 128, 320, 4096)
BLOCK = 512


# ---- keys ------------------------------------------------------------------------------------------------------------------
def r2_exact(x64, rows):
    """fp64 squared distances of the bodies ``rows`` to all bodies, exact on grid inputs (the Gram form keeps to integers)."""
    sq = (x64 * x64).sum(axis=1)
    return sq[rows][:, None] + sq[None, :] - 2.0 * (x64[rows] @ x64.T)


def r2_bits(r2):
    """The bits of the fp32 r2 as int64; the cast is exact on grid inputs."""
    return r2.astype(np.float32).view(np.uint32).astype(np.int64)


def keys(x64, rows):
    """int64 (len(rows), n): K = (bits(r2) << 24) | (min << 12) | max of the edges from the bodies ``rows`` to all bodies."""
    n = x64.shape[0]
    cols = np.arange(n, dtype=np.int64)[None, :]
    r = np.asarray(rows, dtype=np.int64)[:, None]
    return (r2_bits(r2_exact(x64, rows)) << (2 * INDEX_BITS)) | (np.minimum(r, cols) << INDEX_BITS) | np.maximum(r, cols)


def key_fields(k):
    k = np.asarray(k, dtype=np.int64)
    mask = (1 << INDEX_BITS) - 1
    bits = (k >> (2 * INDEX_BITS)).astype(np.uint32)
    return ((k >> INDEX_BITS) & mask).astype(np.int32), (k & mask).astype(np.int32), bits.view(np.float32)


def positions64(pos, n):
    return np.asarray(pos, dtype=np.float32)[:n, :3].astype(np.float64)


def selection(n, subset):
    """The selected bodies in ascending order."""
    if subset is None:
        return np.arange(n, dtype=np.int64)
    return np.flatnonzero(np.asarray(subset)[:n] != 0).astype(np.int64)


# ---- Prim -------------------------------------------------------------------------------------------------------------------
def prim(pos, n, subset=None):
    """The sorted keys of the minimum spanning tree of the selected bodies under the strict order of the keys."""
    x = positions64(pos, n)
    sel = selection(n, subset)
    m = len(sel)
    if m < 2:
        return np.zeros(0, np.int64)
    best = keys(x, sel[:1])[0][sel]
    outside = np.ones(m, bool)
    outside[0] = False
    best[0] = BIG
    out = []
    for _ in range(m - 1):
        u = int(np.argmin(best))
        out.append(best[u])
        outside[u] = False
        best = np.minimum(best, keys(x, sel[u:u + 1])[0][sel])
        best[~outside] = BIG
    return np.sort(np.array(out, dtype=np.int64))


# ---- the header's rounds ---------------------------------------------------------------------------------------------------
def rounds(pos, n, subset=None):
    """(sorted keys, rounds, nearest, absorbed): the header's rounds, literally.  nearest is per body (n,), -1 where there is
    none; absorbed the number of times each component was absorbed (every one exactly once, but the last root)."""
    x = positions64(pos, n)
    sel = selection(n, subset)
    m = len(sel)
    nearest = np.full(n, -1, np.int32)
    label = np.full(n, -1, np.int64)
    label[sel] = sel
    absorbed = np.zeros(n, np.int64)
    recorded = []
    t = 0
    while len(np.unique(label[sel])) > 1 and t < MAX_ROUNDS:
        t += 1
        # every row's minimum over the columns of another component, then every component's minimum: reads alone
        row_min = np.empty(m, np.int64)
        for lo in range(0, m, BLOCK):
            rows = sel[lo:lo + BLOCK]
            k = keys(x, rows)[:, sel]
            k[label[rows][:, None] == label[sel][None, :]] = BIG
            row_min[lo:lo + BLOCK] = k.min(axis=1)
        if t == 1:
            i, j, _ = key_fields(row_min)
            nearest[sel] = np.where(i == sel, j, i)
        comp_min = np.full(n, BIG, np.int64)
        np.minimum.at(comp_min, label[sel], row_min)
        # every component decides: reads alone
        hooks = {}
        for c in np.unique(label[sel]).tolist():
            mine = comp_min[c]
            i, j, _ = key_fields(mine)
            o = int(label[j]) if label[i] == c else int(label[i])
            assert o != c
            other = comp_min[o]
            if other != mine or c > o:
                hooks[c] = o
                recorded.append(mine)
                absorbed[c] += 1
        # Hook, then Compress until every label is a root
        parent = label.copy()
        for c, o in hooks.items():
            parent[c] = o
        label[sel] = parent[label[sel]]
        while True:
            nxt = label.copy()
            nxt[sel] = label[label[sel]]
            if np.array_equal(nxt, label):
                break
            label = nxt
    return np.sort(np.array(recorded, dtype=np.int64)), t, nearest, absorbed


# ---- the records -------------------------------------------------------------------------------------------------------------
def sequential_sum(terms):
    """The fp64 sum of the terms in order (numpy's cumulative sum adds one term at a time; its plain sum does not)."""
    terms = np.asarray(terms, dtype=np.float64)
    return float(np.cumsum(terms)[-1]) if terms.size else 0.0


def mean_separation(pos, n, subset=None):
    """Row i sums (double)sqrtf(r2_ij) over the selected j != i in ascending j; the rows are summed in ascending i; one division
    by selected (selected - 1)."""
    x = positions64(pos, n)
    sel = selection(n, subset)
    m = len(sel)
    if m < 2:
        return 0.0
    row_sums = np.empty(m, np.float64)
    for lo in range(0, m, BLOCK):
        rows = sel[lo:lo + BLOCK]
        d = np.sqrt(r2_exact(x, rows)[:, sel].astype(np.float32)).astype(np.float64)   # the row's own column adds sqrtf(0) = +0
        row_sums[lo:lo + BLOCK] = np.cumsum(d, axis=1)[:, -1]
    return sequential_sum(row_sums) / (float(m) * float(m - 1))


def reference(pos, n, subset=None):
    """Every word nbody_batch_span returns for one system, as a dict; mean_separation is the value of separations = 1."""
    sel = selection(n, subset)
    tree = prim(pos, n, subset)
    mirrored, t, nearest, absorbed = rounds(pos, n, subset)
    assert np.array_equal(tree, mirrored), "the header's rounds and Prim's algorithm disagree"
    roots_left = 1 if len(sel) else 0
    assert absorbed.sum() == len(sel) - roots_left and absorbed.max(initial=0) <= 1
    i, j, r2 = key_fields(tree)
    lengths = np.sqrt(r2.astype(np.float64))
    degree = (np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.int32)
    return {"keys": tree, "i": i, "j": j, "r2": r2, "edges": len(tree), "selected": len(sel), "rounds": t,
            "total_length": sequential_sum(lengths), "longest": float(lengths[-1]) if len(tree) else 0.0,
            "mean_separation": mean_separation(pos, n, subset), "degree": degree[:n], "nearest": nearest}


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _rows(xyz, scale=1.0):
    out = np.zeros((len(xyz), 4), np.float32)
    out[:, :3] = np.asarray(xyz, dtype=np.float64) * scale
    out[:, 3] = 1.0
    return out


def lattice(seed=1, spacing=3, scale=1.0):
    """A 4 x 4 x 4 lattice in permuted index order: every tie is decided by indices alone."""
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) * spacing + 100
    return _rows(g[np.random.default_rng(seed).permutation(64)], scale)


def chain(n, seed=2, scale=1.0):
    """n <= 1024 bodies one grid unit apart on a line, in permuted index order: the tree is forced, and there are many rounds
    and long Compress chains."""
    assert n <= GRID
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.random.default_rng(seed).permutation(n)
    xyz[:, 1:] = 7
    return _rows(xyz, scale)


def plummer(n, seed=3, radius=60.0, scale=1.0):
    """A Plummer sphere of scale radius ``radius`` grid units about the grid's centre, rounded to the grid: the core holds a
    few coincident bodies (r2 = 0)."""
    rng = np.random.default_rng(seed)
    r = radius / np.sqrt(rng.uniform(1e-3, 1.0, n) ** (-2.0 / 3.0) - 1.0 + 1e-12)
    u = rng.normal(size=(n, 3))
    xyz = GRID / 2 + r[:, None] * u / np.linalg.norm(u, axis=1)[:, None]
    return _rows(np.clip(np.rint(xyz), 0, GRID - 1), scale)


def cube(n, seed=4, side=64, scale=1.0):
    """A uniform cube of ``side`` grid units, rounded to the grid."""
    return _rows(np.random.default_rng(seed).integers(0, side, (n, 3)) + 200, scale)


def _pack(capacity, systems):
    P = np.zeros((len(systems), capacity, 4), np.float32)
    counts = []
    for s, rows in enumerate(systems):
        P[s, :len(rows)] = rows
        counts.append(len(rows))
    P.flags.writeable = False
    return P, counts


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, counts) of one capacity: ragged counts with 0, 1, 2 and the full capacity among them."""
    c = capacity
    if capacity == 64:
        systems = [lattice(), chain(0), chain(1), chain(2), chain(64, scale=2.0 ** -7), plummer(37, radius=6.0), cube(64, side=4)]
    elif capacity == 4096:   # two full systems: the reference stays within seconds
        systems = [plummer(c, radius=40.0), chain(0), chain(1), chain(2), chain(1000), cube(c, side=24, scale=2.0 ** -9)]
    else:
        systems = [chain(c), chain(0), chain(1), chain(2), plummer(c - 29, seed=5, radius=8.0, scale=4.0), cube(c, side=8),
                   lattice(seed=6, spacing=1), plummer(c, seed=7, radius=30.0, scale=2.0 ** -10)]
    return _pack(capacity, systems)


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity):
    P, counts = gpu_inputs(capacity)
    return [reference(P[s], n) for s, n in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def subset_inputs(capacity, slots=8, members=20):
    """(pos, n, masks): one cluster of ``capacity - 3`` bodies and ``slots`` masks over the capacity: all bodies, none, one body,
    two bodies, the first ``members``, and random sets (the last with marks beyond the count, which select nothing)."""
    n = capacity - 3
    pos = np.zeros((capacity, 4), np.float32)
    pos[:n] = plummer(n, seed=11, radius=12.0 if capacity < 1024 else 40.0)
    rng = np.random.default_rng(12)
    masks = np.zeros((slots, capacity), np.uint8)
    masks[0, :] = 1
    masks[2, n // 2] = 1
    masks[3, [1, n - 1]] = 1
    masks[4, :members] = 1
    for s in range(5, slots):
        masks[s, rng.choice(n, size=min(members + 7 * (s - 5), n), replace=False)] = 1
    masks[slots - 1, n:] = 1
    pos.flags.writeable = False
    masks.flags.writeable = False
    return pos, n, masks


def is_spanning_tree(i, j, vertices):
    """Whether the edges (i, j) form a spanning tree of the bodies ``vertices`` (indices): a union-find."""
    vertices = [int(v) for v in vertices]
    if len(i) != max(len(vertices) - 1, 0):
        return False
    parent = {v: v for v in vertices}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, c in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        if a not in parent or c not in parent:
            return False
        ra, rc = find(a), find(c)
        if ra == rc:
            return False
        parent[ra] = rc
    return len({find(v) for v in vertices}) <= 1
