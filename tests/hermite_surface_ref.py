"""The reference of the surface maps of batched ensembles (include/nbody_batch_surface.h), operation by operation in Python
floats -- IEEE doubles whose +, - and * are correctly rounded -- with no numpy sum and no dot product anywhere, because the
order of the additions is what the header pins.  It bins with `bisect` and keeps one accumulator per cell that the bodies join
in ascending index: no sort, no rank, nothing of csrc/nbody_batch_surface_math.h.  Every word of every record is made of +, -
and x alone, so the device is compared with it bit for bit on any input.  Also the inputs that
tests/test_batch_surface_cpu.py and tests/test_batch_surface_gpu.py share; besides random bodies they hold the shapes at which
a sort by cell can go wrong (SPECIAL below)."""
import bisect
import functools
import math

import numpy as np

SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("outside", np.int32), ("unmeasured", np.int32), ("columns", np.int32),
                         ("rows", np.int32), ("occupied", np.int32), ("peak", np.int32), ("peak_count", np.int32),
                         ("total_weight", np.float64), ("centre", np.float64, 3), ("velocity", np.float64, 3)])
CELL_DTYPE = np.dtype([("count", np.int64), ("weight", np.float64), ("v1", np.float64), ("v2", np.float64),
                       ("pa", np.float64), ("pb", np.float64), ("z1", np.float64), ("z2", np.float64)])
BODY_DTYPE = np.dtype([("cell", np.int32), ("reserved", np.int32), ("a", np.float64), ("b", np.float64)])
MAX_SIDE = 64
OUTSIDE, UNMEASURED, NOT_TAKING = -1, -2, -3
SUMS = ("weight", "v1", "v2", "pa", "pb", "z1", "z2")
#: (T, RPL) of the workgroups the CPU driver is run at; batch_shape's for 64, 128, 320 and 4096 bodies
SHAPES = ((64, 1), (64, 2), (128, 4), (1024, 4))
CAPACITIES = (64, 128, 320, 4096)


def shape_of(capacity):
    """batch_shape (csrc/nbody_batch_choice.h): (T, RPL)."""
    if capacity <= 64:
        return 64, 1
    if capacity <= 128:
        return 64, 2
    return (capacity + 255) // 256 * 64, 4


def along(axis, x, y, z):
    return (float(axis[0]) * x + float(axis[1]) * y) + float(axis[2]) * z


def words(p, v, centre, velocity, axes):
    """a, b, q, ua, ub, uq of one body: p and v its float32 words, widened."""
    d = [float(p[k]) - float(centre[k]) for k in range(3)]
    u = [float(v[k]) - float(velocity[k]) for k in range(3)]
    return tuple(along(axes[r], *d) for r in range(3)) + tuple(along(axes[r], *u) for r in range(3))


def bin_of(v, edges):
    """t with edges[t] <= v < edges[t + 1], or -1."""
    passed = bisect.bisect_right(edges, v)  # the edges <= v
    return -1 if passed == 0 or passed == len(edges) else passed - 1


def surface(pos, vel, count, edges_a, edges_b, centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), axes=None, weight="mass", subset=None):
    """One system: pos and vel are (slots, 4) float32, count its bodies.  Returns the system record, the cell records
    (rows, columns) and the body records (slots of them)."""
    slots = pos.shape[0]
    n = min(int(count), slots)
    ea, eb = [float(e) for e in edges_a], [float(e) for e in edges_b]
    columns, rows = len(ea) - 1, len(eb) - 1
    axes = np.eye(3) if axes is None else axes
    system = np.zeros((), dtype=SYSTEM_DTYPE)
    body = np.zeros(slots, dtype=BODY_DTYPE)
    body["cell"] = NOT_TAKING
    acc = [[0] + [0.0] * 7 for _ in range(columns * rows)]
    selected = outside = unmeasured = 0
    total = 0.0
    for i in range(n):  # ascending body index: the pinned order
        if subset is not None and not subset[i]:
            continue
        selected += 1
        a, b, q, ua, ub, uq = words(pos[i], vel[i], centre, velocity, axes)
        if not all(math.isfinite(x) for x in (a, b, q, ua, ub, uq)):
            body["cell"][i] = UNMEASURED
            unmeasured += 1
            continue
        w = 1.0 if weight == "number" else float(pos[i][3])
        total += w
        body["a"][i], body["b"][i] = a, b
        col, row = bin_of(a, ea), bin_of(b, eb)
        if col < 0 or row < 0:
            body["cell"][i] = OUTSIDE
            outside += 1
            continue
        c = row * columns + col
        body["cell"][i] = c
        s = acc[c]
        s[0] += 1
        s[1] += w
        s[2] += w * uq
        s[3] += w * (uq * uq)
        s[4] += w * ua
        s[5] += w * ub
        s[6] += w * q
        s[7] += w * (q * q)
    rec = np.zeros(columns * rows, dtype=CELL_DTYPE)
    for k, name in enumerate(CELL_DTYPE.names):
        rec[name] = [s[k] for s in acc]
    counts = [s[0] for s in acc]
    best = max(counts)
    system["selected"], system["outside"], system["unmeasured"] = selected, outside, unmeasured
    system["columns"], system["rows"] = columns, rows
    system["occupied"] = sum(1 for c in counts if c > 0)
    system["peak"], system["peak_count"] = (counts.index(best), best) if best > 0 else (-1, 0)
    system["total_weight"] = total
    system["centre"], system["velocity"] = [float(c) for c in centre], [float(c) for c in velocity]
    return system, rec.reshape(rows, columns), body


def surface_batch(pos, vel, counts, edges_a, edges_b, centre=None, velocity=None, axes=None, weight="mass", subset=None):
    """Every system of a batch: pos, vel (B, slots, 4); edges (bins + 1,) or (B, bins + 1); centre and velocity (B, 3) or None;
    axes (3, 3), (B, 3, 3) or None.  Returns systems (B,), cells (B, rows, columns) and bodies (B, slots)."""
    B = pos.shape[0]
    ea, eb = np.asarray(edges_a, dtype=np.float64), np.asarray(edges_b, dtype=np.float64)
    view = None if axes is None else np.broadcast_to(np.asarray(axes, dtype=np.float64), (B, 3, 3))
    out = []
    for s in range(B):
        out.append(surface(pos[s], vel[s], counts[s], ea[s] if ea.ndim == 2 else ea, eb[s] if eb.ndim == 2 else eb,
                           (0.0, 0.0, 0.0) if centre is None else centre[s], (0.0, 0.0, 0.0) if velocity is None else velocity[s],
                           None if view is None else view[s], weight, None if subset is None else subset[s]))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------
CENTRE = (0.5, -1.0, 2.0)
VELOCITY = (1.0, -0.5, 0.0)
HALF = 8.0                    # the grids span -8 ... 8 on both axes; at 64 bins the edges are the multiples of 1/4
COUNTS = (0, 1, 2, 65)        # and the capacity
#: the systems after those: every body in one cell; body i in cell i; body i in cell n - 1 - i; one mass of 2^53 among ones
SPECIAL = ("one-cell", "own-cell", "reversed", "order")
BIG = 2.0 ** 53               # 2^53 + 1 + 1 = 2^53 in ascending index, and 2^53 + 2 where the ones are added first


def rotation(alpha, beta, gamma):
    """A proper rotation, the rows A, B, Q: about z by alpha, then about x by beta, then about z by gamma."""
    def rz(t):
        return np.array([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(beta), -math.sin(beta)], [0.0, math.sin(beta), math.cos(beta)]])
    return rz(gamma) @ rx @ rz(alpha)


def projection(p):
    """The view of projected = p: the unit vectors of the two axes that are not p, ascending, then p."""
    kept = [k for k in range(3) if k != p]
    return np.eye(3)[[kept[0], kept[1], p]]


def generic_system(slots, count, seed):
    """`count` bodies, every other one on the lattice of quarters within -9 ... 9 about CENTRE (on an edge of the 64-bin grid,
    some beyond it) and the rest normal with spread 3; masses 1 ... 3 and velocities of quarters.  With at least 9 bodies: body 3
    has a NaN coordinate, body 4 infinite ones, body 5 an infinite velocity (all unmeasured); body 6 sits exactly on the first
    edge of both axes in every projection (inside, cell 0), body 7 exactly on the last (outside) and body 8 on interior edges of
    the 64-bin grid.  The slots from the count on hold values no result may depend on."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((slots, 4), dtype=np.float32)
    vel = np.zeros((slots, 4), dtype=np.float32)
    lattice = rng.integers(-36, 37, size=(slots, 3)) / 4.0
    cloud = rng.normal(size=(slots, 3)) * 3.0
    pos[:, :3] = np.where((np.arange(slots) % 2 == 0)[:, None], lattice, cloud) + np.array(CENTRE)
    pos[:, 3] = rng.integers(1, 4, size=slots)
    vel[:, :3] = rng.integers(-12, 13, size=(slots, 3)) / 4.0
    if count >= 9:
        pos[3, 1] = np.nan
        pos[4, :3] = (np.inf, -np.inf, np.inf)
        vel[5, :3] = (np.inf, 0.0, 0.0)
        pos[6, :3] = np.array(CENTRE) - HALF
        pos[7, :3] = np.array(CENTRE) + HALF
        pos[8, :3] = np.array(CENTRE) + np.array([0.0, 0.25, 0.5])
    pos[count:, :3] = 1.0e30  # beyond the count: never read
    vel[count:, :3] = -7.0
    return pos, vel


def special_system(slots, kind, seed):
    """A full system (count = slots) of SPECIAL.  In the plane z of the 64 x 64 grid about CENTRE: `one-cell` has every body
    within the cell that starts at the origin; `own-cell` has body i in the middle of cell i and `reversed` in the middle of
    cell n - 1 - i (cells 0 ... n - 1 of the 4096).  `order` is a generic system whose body 0 weighs 2^53 and every other body 1."""
    rng = np.random.default_rng(seed)
    pos, vel = generic_system(slots, 0 if kind != "order" else slots, seed)
    vel[:, :3] = rng.integers(-12, 13, size=(slots, 3)) / 4.0
    index = np.arange(slots)
    if kind == "one-cell":
        pos[:, :3] = np.array(CENTRE) + rng.integers(1, 8, size=(slots, 3)) / 32.0
        pos[:, 3] = rng.integers(1, 4, size=slots)
    elif kind in ("own-cell", "reversed"):
        cell = index if kind == "own-cell" else slots - 1 - index
        pos[:, 0] = CENTRE[0] - HALF + 0.25 * (cell % MAX_SIDE) + 0.125
        pos[:, 1] = CENTRE[1] - HALF + 0.25 * (cell // MAX_SIDE) + 0.125
        pos[:, 2] = CENTRE[2] + rng.integers(-8, 9, size=slots) / 4.0
        pos[:, 3] = rng.integers(1, 4, size=slots)
    else:
        pos[:, 3] = 1.0
        pos[0, 3] = BIG
        pos[0, :3] = np.array(CENTRE) + 0.125   # measured, inside every grid here
        vel[0, :3] = 0.25
    return pos, vel


def batch_counts(capacity):
    return [min(c, capacity) for c in COUNTS] + [capacity] * (1 + len(SPECIAL))


def shared_batch(capacity, seed=23):
    """One system per count of COUNTS, one at the capacity, and the SPECIAL ones."""
    counts = batch_counts(capacity)
    systems = [generic_system(capacity, c, seed + 17 * k) for k, c in enumerate(counts[:len(COUNTS) + 1])]
    systems += [special_system(capacity, kind, seed + 101 * k) for k, kind in enumerate(SPECIAL)]
    return np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems]), np.array(counts, dtype=np.int32)


def grid(bins, scale=1.0):
    return np.linspace(-HALF * scale, HALF * scale, bins + 1)


def edges_for(bins, own, B):
    """Shared: -8 ... 8.  Per system: system s spans (1 - s / 16) of that, so bodies fall on other sides of other edges."""
    return np.stack([grid(bins, 1.0 - s / 16.0) for s in range(B)]) if own else grid(bins)


def masks(capacity, B, kind, seed=5):
    if kind == "none":
        return None
    if kind == "all-false":
        return np.zeros((B, capacity), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    return (rng.random((B, capacity)) < 0.3).astype(np.uint8)  # sparse


def views(kind, B):
    """(B, 3, 3): the projection p for kind p, one general rotation for "rotated", one rotation per system for "each"."""
    if kind in (0, 1, 2):
        return np.tile(projection(kind), (B, 1, 1))
    if kind == "rotated":
        return np.tile(rotation(0.4, 1.1, -0.7), (B, 1, 1))
    return np.stack([rotation(0.3 * s, 0.2 + 0.25 * s, 1.0 - 0.1 * s) for s in range(B)])


#: what is run at every capacity: (name, columns, rows, per-system edges, weight, view, mask)
CASES = (("1x1-mass", 1, 1, False, "mass", 2, "none"),
         ("1x64-number-x-sparse", 1, 64, False, "number", 0, "sparse"),
         ("64x1-own-y", 64, 1, True, "mass", 1, "none"),
         ("3x5-own-number-rotated-sparse", 3, 5, True, "number", "rotated", "sparse"),
         ("64x64-mass", 64, 64, False, "mass", 2, "none"),
         ("64x64-each-view", 64, 64, False, "mass", "each", "none"),
         ("3x5-all-false", 3, 5, False, "mass", 2, "all-false"))


def case_inputs(capacity, case):
    """pos, vel, counts and the keyword arguments of one case."""
    _, columns, rows, own, weight, view, mask = case
    pos, vel, counts = shared_batch(capacity)
    B = len(counts)
    centre = np.tile(np.array(CENTRE, dtype=np.float64), (B, 1))
    velocity = np.tile(np.array(VELOCITY, dtype=np.float64), (B, 1))
    return pos, vel, counts, dict(edges_a=edges_for(columns, own, B), edges_b=edges_for(rows, own, B), centre=centre, velocity=velocity,
                                  axes=views(view, B), weight=weight, subset=masks(capacity, B, mask))


@functools.lru_cache(maxsize=None)
def reference(capacity, name):
    """The inputs and the reference's records of one case at one capacity, computed once and shared: pos, vel, counts, the
    keyword arguments, and surface_batch's (systems, cells, bodies).  Nobody changes them."""
    case = next(c for c in CASES if c[0] == name)
    pos, vel, counts, kw = case_inputs(capacity, case)
    out = surface_batch(pos, vel, counts, **kw)
    for a in (pos, vel, counts, *out):
        a.setflags(write=False)
    return pos, vel, counts, kw, out
