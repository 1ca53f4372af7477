"""The reference of the radial profiles of batched ensembles (include/nbody_batch_radial.h), operation by operation in Python
floats -- IEEE doubles whose +, -, *, / and math.sqrt are correctly rounded -- with no numpy sum and no dot product anywhere,
because the order of the additions is what the header pins.  Also the inputs that tests/test_batch_radial_cpu.py and
tests/test_batch_radial_gpu.py share: bodies on an integer lattice with small integer velocities and masses, centres and
frame velocities whose components are integers or half-integers -- so that s, rv and v2 of every body are exact -- and edges
sqrt(k + 0.5) for integers k, whose squares lie strictly between two attainable values of s whatever the rounding of the
square root and of the product.  `premises` states both and the CPU test asserts them for every input set."""
import functools
import math
from fractions import Fraction

import numpy as np

SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("below", np.int32), ("above", np.int32), ("unmeasured", np.int32),
                         ("shells", np.int32), ("projected", np.int32), ("total_weight", np.float64),
                         ("centre", np.float64, 3), ("velocity", np.float64, 3)])
SHELL_DTYPE = np.dtype([("count", np.int64), ("weight", np.float64), ("radius", np.float64), ("vr1", np.float64),
                        ("vr2", np.float64), ("vt2", np.float64), ("L", np.float64, 3), ("U", np.float64, 3),
                        ("M", np.float64, 6), ("V", np.float64, 6)])
BODY_DTYPE = np.dtype([("shell", np.int32), ("reserved", np.int32), ("radius", np.float64), ("radial_velocity", np.float64)])
MAX_SHELLS = 32
BELOW, UNMEASURED, NOT_TAKING = -1, -2, -3
LARGEST = float(np.finfo(np.float64).max)
INF = float("inf")
#: the words of a shell that +, - and x alone make, and those that pass through a square root and a division
EXACT_WORDS = ("count", "weight", "L", "U", "M", "V")
ROOTED_WORDS = ("radius", "vr1", "vr2", "vt2")
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


def edge2(e):
    """One product; an overflow becomes the largest finite double."""
    e2 = float(e) * float(e)
    return e2 if e2 <= LARGEST else LARGEST


def words(p, v, centre, velocity, projected):
    """d[3], u[3], s, rv, v2 of one body: p and v its float32 words, widened."""
    d = [float(p[a]) - float(centre[a]) for a in range(3)]
    u = [float(v[a]) - float(velocity[a]) for a in range(3)]
    dd = [d[a] * d[a] for a in range(3)]
    du = [d[a] * u[a] for a in range(3)]
    if projected is None or projected < 0:
        s = (dd[0] + dd[1]) + dd[2]
        rv = (du[0] + du[1]) + du[2]
    else:
        a, b = [axis for axis in range(3) if axis != projected]
        s = dd[a] + dd[b]
        rv = du[a] + du[b]
    v2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
    return d, u, s, rv, v2


def shell_of(s, v2, e2):
    """-2 unmeasured, -1 below, t in shell t, len(e2) - 1 above."""
    if not (s < INF) or not (v2 < INF):
        return UNMEASURED
    if s <= e2[0]:
        return BELOW
    for t in range(len(e2) - 1):
        if e2[t] < s <= e2[t + 1]:
            return t
    assert s > e2[-1]
    return len(e2) - 1


PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # xx, yy, zz, xy, xz, yz


def profile(pos, vel, count, edges, centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), weight="mass", projected=None, subset=None):
    """One system: pos and vel are (slots, 4) float32, count its bodies, edges its shells + 1 edges.  Returns the system
    record, the shell records, the body records (slots of them) and `scale` (shells, 4): per shell the sums of w r, w |u|,
    w v2 and w v2 over its members, what the error bound of radius, vr1, vr2 and vt2 is stated in."""
    slots = pos.shape[0]
    n = min(int(count), slots)
    shells = len(edges) - 1
    e2 = [edge2(e) for e in edges]
    system = np.zeros((), dtype=SYSTEM_DTYPE)
    rec = np.zeros(shells, dtype=SHELL_DTYPE)
    body = np.zeros(slots, dtype=BODY_DTYPE)
    body["shell"] = NOT_TAKING
    scale = np.zeros((shells, 4))
    acc = [dict(count=0, weight=0.0, radius=0.0, vr1=0.0, vr2=0.0, vt2=0.0, L=[0.0] * 3, U=[0.0] * 3, M=[0.0] * 6, V=[0.0] * 6)
           for _ in range(shells)]
    bound = [[0.0] * 4 for _ in range(shells)]
    selected = below = above = unmeasured = 0
    total = 0.0
    for i in range(n):  # ascending body index: the pinned order
        if subset is not None and not subset[i]:
            continue
        selected += 1
        d, u, s, rv, v2 = words(pos[i], vel[i], centre, velocity, projected)
        t = shell_of(s, v2, e2)
        body["shell"][i] = t
        if t == UNMEASURED:
            unmeasured += 1
            continue
        w = 1.0 if weight == "number" else float(pos[i][3])
        total += w
        r = math.sqrt(s)
        body["radius"][i] = r
        body["radial_velocity"][i] = rv / r if r > 0.0 else 0.0
        if t == BELOW:
            below += 1
            continue
        if t == shells:
            above += 1
            continue
        a = acc[t]
        vr = rv / r
        vrvr = vr * vr
        vt2 = max(v2 - vrvr, 0.0)
        a["count"] += 1
        a["weight"] += w
        a["radius"] += w * r
        a["vr1"] += w * vr
        a["vr2"] += w * vrvr
        a["vt2"] += w * vt2
        cross = (d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0])
        for c in range(3):
            a["L"][c] += w * cross[c]
            a["U"][c] += w * u[c]
        for c, (p, q) in enumerate(PAIRS):
            a["M"][c] += w * (d[p] * d[q])
            a["V"][c] += w * (u[p] * u[q])
        bound[t][0] += w * r
        bound[t][1] += w * math.sqrt(v2)
        bound[t][2] += w * v2
        bound[t][3] += w * v2
    for t in range(shells):
        for name in SHELL_DTYPE.names:
            rec[name][t] = acc[t][name]
        scale[t] = bound[t]
    system["selected"], system["below"], system["above"], system["unmeasured"] = selected, below, above, unmeasured
    system["shells"], system["projected"] = shells, -1 if projected is None else projected
    system["total_weight"] = total
    system["centre"], system["velocity"] = [float(c) for c in centre], [float(c) for c in velocity]
    return system, rec, body, scale


def profile_batch(pos, vel, counts, edges, centre=None, velocity=None, weight="mass", projected=None, subset=None):
    """Every system of a batch: pos, vel (B, slots, 4), edges (shells + 1,) or (B, shells + 1), centre and velocity (B, 3) or
    None.  Returns systems (B,), shells (B, shells), bodies (B, slots) and scale (B, shells, 4)."""
    B = pos.shape[0]
    edges = np.asarray(edges, dtype=np.float64)
    out = []
    for s in range(B):
        out.append(profile(pos[s], vel[s], counts[s], edges[s] if edges.ndim == 2 else edges,
                           (0.0, 0.0, 0.0) if centre is None else centre[s], (0.0, 0.0, 0.0) if velocity is None else velocity[s],
                           weight, projected, None if subset is None else subset[s]))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


# ---- the shared inputs ---------------------------------------------------------------------------------------------------------
CENTRE = (0.5, -1.0, 2.0)     # one half-integer component: s is k + 1/4 in space and an integer or k + 1/4 in a plane
VELOCITY = (1.0, -0.5, 0.0)
SPAN, SPEED = 6, 3            # lattice coordinates in -6 ... 6 and velocity components in -3 ... 3
COUNTS = (0, 1, 2, 65)        # and the capacity
INTEGER_CENTRE = (1.0, 0.0, -2.0)
ON_EDGE = (3.0, 0.0, -2.0)


def lattice_system(slots, count, seed, specials=True):
    """(slots, 4) float32 positions with masses 1 ... 3 and velocities, `count` bodies on the integer lattice; the slots from
    the count on hold values no result may depend on.  With `specials` and at least 8 bodies: body 3 has NaN coordinates,
    body 4 infinite ones, body 5 an infinite velocity (all unmeasured), body 6 sits exactly at CENTRE (below) and body 7 at ON_EDGE, two lattice steps from INTEGER_CENTRE: exactly on
    the edge 2 of integer_edges."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((slots, 4), dtype=np.float32)
    vel = np.zeros((slots, 4), dtype=np.float32)
    pos[:, :3] = rng.integers(-SPAN, SPAN + 1, size=(slots, 3))
    pos[:, 3] = rng.integers(1, 4, size=slots)
    vel[:, :3] = rng.integers(-SPEED, SPEED + 1, size=(slots, 3))
    if specials and count >= 8:
        pos[3, :3] = np.nan
        pos[4, :3] = (np.inf, -np.inf, np.inf)
        vel[5, :3] = (np.inf, 0.0, 0.0)
        pos[6, :3] = CENTRE
        pos[7, :3] = ON_EDGE
    pos[count:, :3] = 1.0e30  # beyond the count: never read
    vel[count:, :3] = -7.0
    return pos, vel


def batch_counts(capacity):
    return [min(c, capacity) for c in COUNTS] + [capacity]


def lattice_batch(capacity, seed=11):
    """One system per count of COUNTS and one at the capacity."""
    counts = batch_counts(capacity)
    systems = [lattice_system(capacity, c, seed + 17 * k) for k, c in enumerate(counts)]
    return np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems]), np.array(counts, dtype=np.int32)


def half_edges(shells, first=0, step=None):
    """sqrt(k + 0.5) for shells + 1 ascending integers k from `first`: the last below the largest s of the lattice, so that
    there are bodies above."""
    if step is None:
        step = max(1, 48 // shells)
    return np.array([math.sqrt(first + step * t + 0.5) for t in range(shells + 1)], dtype=np.float64)


def edges_for(shells, per_system, B):
    return np.stack([half_edges(shells, first=s) for s in range(B)]) if per_system else half_edges(shells)


def integer_edges(shells):
    """0, 1, 2, ...: with an integer centre bodies sit exactly on them -- the shells are closed on the right."""
    return np.arange(shells + 1, dtype=np.float64)


def masks(capacity, B, kind, seed=5):
    if kind == "none":
        return None
    if kind == "all-false":
        return np.zeros((B, capacity), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    return (rng.random((B, capacity)) < 0.3).astype(np.uint8)  # sparse


#: what is run at every capacity: (name, shells, per-system edges, weight, projected, mask, integer edges)
CASES = (("8-mass", 8, False, "mass", None, "none", False),
         ("1-number-sparse", 1, False, "number", None, "sparse", False),
         ("9-own-x", 9, True, "mass", 0, "none", False),
         ("32-own-number-y-sparse", 32, True, "number", 1, "sparse", False),
         ("32-mass-z", 32, False, "mass", 2, "none", False),
         ("8-all-false", 8, False, "mass", None, "all-false", False),
         ("9-integer-edges", 9, False, "number", None, "none", True))


def case_inputs(capacity, case):
    """pos, vel, counts and the keyword arguments of one case: edges, centre, velocity, weight, projected, subset."""
    _, shells, own, weight, projected, mask, integer = case
    pos, vel, counts = lattice_batch(capacity)
    B = len(counts)
    centre = np.tile(np.array(INTEGER_CENTRE if integer else CENTRE, dtype=np.float64), (B, 1))
    velocity = np.tile(np.array(VELOCITY, dtype=np.float64), (B, 1))
    edges = integer_edges(shells) if integer else edges_for(shells, own, B)
    return pos, vel, counts, dict(edges=edges, centre=centre, velocity=velocity, weight=weight, projected=projected,
                                  subset=masks(capacity, B, mask))


@functools.lru_cache(maxsize=None)
def reference(capacity, name):
    """The inputs and the reference's records of one case at one capacity, computed once and shared: pos, vel, counts, the
    keyword arguments, and profile_batch's (systems, shells, bodies, scale).  Nobody changes them."""
    case = next(c for c in CASES if c[0] == name)
    pos, vel, counts, kw = case_inputs(capacity, case)
    out = profile_batch(pos, vel, counts, **kw)
    for a in (pos, vel, counts, *out):
        a.setflags(write=False)
    return pos, vel, counts, kw, out


def premises(pos, vel, counts, edges, centre, velocity, projected, integer=False, **_):
    """The two premises of the exact comparison, in rational arithmetic.  (1) s, rv and v2 of every finite body are exact:
    the doubles equal the fractions.  (2) Unless the edges are integers on purpose, no attainable s is nearer to a squared
    edge than 1/8: every s is a multiple of 1/4 and every squared edge is k + 1/2 up to rounding, so no rounding of the
    square root or of the product moves a body across an edge.  Returns the number of bodies checked."""
    checked = 0
    edges = np.asarray(edges, dtype=np.float64)
    for s in range(pos.shape[0]):
        e2 = [edge2(e) for e in (edges[s] if edges.ndim == 2 else edges)]
        for i in range(min(int(counts[s]), pos.shape[1])):
            if not (np.isfinite(pos[s, i, :3]).all() and np.isfinite(vel[s, i, :3]).all()):
                continue
            d = [Fraction(float(pos[s, i, a])) - Fraction(float(centre[s][a])) for a in range(3)]
            u = [Fraction(float(vel[s, i, a])) - Fraction(float(velocity[s][a])) for a in range(3)]
            keep = [a for a in range(3) if a != projected]
            exact = (sum(d[a] * d[a] for a in keep), sum(d[a] * u[a] for a in keep), sum(c * c for c in u))
            got = words(pos[s, i], vel[s, i], centre[s], velocity[s], projected)[2:]
            assert all(Fraction(g) == x for g, x in zip(got, exact)), (s, i, got, exact)
            assert (exact[0] * 4).denominator == 1, (s, i, exact[0])
            if not integer:
                assert all(abs(exact[0] - Fraction(e)) > Fraction(1, 8) for e in e2), (s, i, exact[0])
            checked += 1
    return checked
