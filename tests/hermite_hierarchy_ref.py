"""The fp64 numpy reference of nbody_batch_hierarchy (include/nbody_batch_hierarchy.h): the nested bound pairs of one system,
level by level -- every live root's partner by the smallest two-body energy, the mutual bound pairs, the worst perturber of
each, the new nodes with the merged body's state, the stability of nested pairs -- and the inputs the GPU suite runs (objects
of six kinds built by nesting Kepler orbits, one per site of a jittered lattice), which the CPU suite checks too.

The reference takes the state as float32 and does everything else in float64; a node's state is hermite_merge_ref's merged
body rounded to float32, and only the rule "a pair whose fp32 squared distance is 0 is no candidate" looks at a float32
number, as in hermite_pairs_ref.  Besides the records it reports four margins per system, which the inputs must keep:
    a  over every live root at every level, the gap between its best and second-best candidate energy over the larger
       v^2/2 + mu/r of the two
    b  over every mutual pair, |energy| / (v^2/2 + mu/r)
    c  over every stability comparison, |ratio / threshold - 1|
    d  with a finite tolerance, |perturbation / tolerance - 1| over every candidate pair"""
import numpy as np

import hermite_pairs_ref as pref

MAX_LEVELS = 16
#: what every generated system must keep: ten times test_batch_pairs_gpu's ENERGY_TIE for the fp32 search; the fp64
#: comparisons differ from the kernel's by rounding order alone; the fp32 g is a maximum of m inv^3, under ten ulps off
MARGINS = dict(a=2e-5, b=1e-4, c=1e-5, d=1e-4)
SYSTEM_FIELDS = ("nodes", "roots", "levels", "converged", "singles", "binaries", "triples", "higher", "unstable")


def merged(mi, ui, mj, uj):
    """hermite_merge_ref's merged body: the mass-weighted mean in fp64 of float32 operands (the arithmetic mean for a zero
    mass), rounded once to float32."""
    mi, mj = np.float64(mi), np.float64(mj)
    ui, uj = np.asarray(ui, np.float64), np.asarray(uj, np.float64)
    M = mi + mj
    if M == 0.0:
        return (0.5 * (ui + uj)).astype(np.float32)
    return ((mj * uj + mi * ui) / M).astype(np.float32)


def mutual_inclination(h, hc):
    n, nc = np.sqrt((h * h).sum()), np.sqrt((hc * hc).sum())
    if not n > 0 or not nc > 0:
        return 0.0
    return float(np.arccos(np.clip((h * hc).sum() / (n * nc), -1.0, 1.0)))


def threshold(q, e, imut):
    """Mardling & Aarseth (2001)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.8 * ((1.0 + q) * (1.0 + e) / np.sqrt(1.0 - e)) ** 0.4 * (1.0 - 0.3 * imut / np.pi)


def _search(x, v, ms, chunk=256):
    """Among L live roots: (partner, margin a).  partner is -1 without a candidate; ties go to the lower index."""
    L = len(ms)
    partner = np.full(L, -1)
    worst = np.inf
    x64, v64, m64 = x.astype(np.float64), v.astype(np.float64), ms.astype(np.float64)
    for lo in range(0, L, chunk):
        rows = np.arange(lo, min(lo + chunk, L))
        d32 = x[None, :, :] - x[rows, None, :]
        r2_32 = (d32[..., 0] * d32[..., 0] + d32[..., 1] * d32[..., 1]) + d32[..., 2] * d32[..., 2]
        d = x64[None, :, :] - x64[rows, None, :]
        w = v64[None, :, :] - v64[rows, None, :]
        r = np.sqrt((d * d).sum(-1))
        valid = (np.arange(L)[None, :] != rows[:, None]) & (r2_32 > 0) & (r > 0)
        mu = m64[None, :] + m64[rows, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            kin, pot = 0.5 * (w * w).sum(-1), mu / r
        eps = np.where(valid, kin - pot, np.inf)
        eps = np.where(np.isnan(eps), np.inf, eps)
        scale = kin + pot
        k = np.arange(len(rows))
        j1 = np.argmin(eps, axis=1)
        e1 = eps[k, j1]
        partner[rows] = np.where(e1 < np.inf, j1, -1)
        rest = eps.copy()
        rest[k, j1] = np.inf
        j2 = np.argmin(rest, axis=1)
        e2 = rest[k, j2]
        both = e2 < np.inf
        if both.any():
            gap = (e2 - e1)[both] / np.maximum(scale[k, j1], scale[k, j2])[both]
            worst = min(worst, float(gap.min()))
    return partner, worst


def hierarchy(pos, vel, n, massive=None, tidal_tolerance=np.inf, max_levels=8):
    """The reference of one system from its (capacity, 4) float32 state, its count n and its massive count (None: off): a dict
    of the system fields, the node fields as (capacity,) arrays (entry k is node k), parent, root and depth as (capacity,)
    arrays, and ``margins``, a dict of the four."""
    assert 1 <= max_levels <= MAX_LEVELS and tidal_tolerance >= 0
    pos, vel = np.asarray(pos, dtype=np.float32), np.asarray(vel, dtype=np.float32)
    cap = pos.shape[0]
    n = min(int(n), cap)
    m = n if massive is None else min(int(massive), n)
    X, V, Ms = pos[:m, :3].copy(), vel[:m, :3].copy(), pos[:m, 3].copy()
    live, nid = np.ones(m, dtype=bool), np.arange(m)
    nodes = []
    margins = dict(a=np.inf, b=np.inf, c=np.inf, d=np.inf)
    levels, converged = 0, 1
    while live.sum() >= 2:
        levels += 1
        idx = np.nonzero(live)[0]
        x, v, ms = X[idx], V[idx], Ms[idx]
        partner, gap = _search(x, v, ms)
        margins["a"] = min(margins["a"], gap)
        new = []
        for a in np.nonzero((partner > np.arange(len(idx))) & (partner >= 0))[0]:
            b = partner[a]
            if partner[b] != a:
                continue
            i, j = idx[a], idx[b]
            mu = np.float64(Ms[j]) + np.float64(Ms[i])
            energy, sma, ecc, inc, sep = (float(u) for u in pref.elements(X[i], V[i], X[j], V[j], mu))
            with np.errstate(divide="ignore", invalid="ignore"):
                margins["b"] = min(margins["b"], abs(energy) / (energy + 2.0 * mu / sep))
            if not energy < 0:
                continue
            xn, vn = merged(Ms[i], X[i], Ms[j], X[j]), merged(Ms[i], V[i], Ms[j], V[j])
            others = idx[(idx != i) & (idx != j)]
            g = 0.0
            if len(others):
                d = X[others].astype(np.float64) - xn.astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    s = Ms[others].astype(np.float64) / np.sqrt((d * d).sum(-1)) ** 3
                s = s[~np.isnan(s)]
                g = max(0.0, float(s.max())) if len(s) else 0.0
            Q = sma * (1.0 + ecc)
            pert = 2.0 * g * Q ** 3 / mu
            if np.isfinite(tidal_tolerance) and tidal_tolerance > 0:
                margins["d"] = min(margins["d"], abs(pert / tidal_tolerance - 1.0))
            if pert > tidal_tolerance:
                continue
            r64, w64 = X[j].astype(np.float64) - X[i].astype(np.float64), V[j].astype(np.float64) - V[i].astype(np.float64)
            h = np.cross(r64, w64)
            node = dict(child=(int(nid[i]), int(nid[j])), parent=-1, level=levels, leaves=0, slot=int(i), stable=1,
                        mass=float(np.float32(Ms[i] + Ms[j])), energy=energy, semi_major_axis=sma, eccentricity=ecc,
                        inclination=inc, separation=sep, perturbation=pert, mutual_inclination=[0.0, 0.0], h=h)
            for c, (cid, mc, mo) in enumerate(((nid[i], Ms[i], Ms[j]), (nid[j], Ms[j], Ms[i]))):
                if cid < n:
                    node["leaves"] += 1
                    continue
                child = nodes[cid - n]
                imut = mutual_inclination(h, child["h"])
                ratio = sma * (1.0 - ecc) / child["semi_major_axis"]
                thr = threshold(np.float64(mo) / np.float64(mc), ecc, imut)
                with np.errstate(invalid="ignore"):
                    margins["c"] = min(margins["c"], abs(ratio / thr - 1.0))
                if not (ratio > thr and child["stable"]):
                    node["stable"] = 0
                node["leaves"] += child["leaves"]
                node["mutual_inclination"][c] = imut
            new.append((i, j, node, xn, vn))
        for i, j, node, xn, vn in new:                      # all at once, in ascending lower slot
            node_id = n + len(nodes)
            for cid in node["child"]:
                if cid >= n:
                    nodes[cid - n]["parent"] = node_id
            nodes.append(node)
            X[i], V[i], Ms[i] = xn, vn, np.float32(Ms[i] + Ms[j])
            live[j] = False
            nid[i], nid[j] = node_id, -1
        if not new or live.sum() < 2:
            converged = 1
            break
        if levels == max_levels:
            converged = 0
            break
    out = dict(nodes=len(nodes), roots=int(live.sum()), levels=levels, converged=converged, margins=margins, count=n)
    out["child"] = np.full((cap, 2), -1, dtype=np.int32)
    out["node_parent"] = np.full(cap, -1, dtype=np.int32)
    for name in ("level", "leaves", "slot", "stable"):
        out[name] = np.zeros(cap, dtype=np.int32)
    for name in ("mass", "energy", "semi_major_axis", "eccentricity", "inclination", "separation", "perturbation"):
        out[name] = np.zeros(cap)
    out["mutual_inclination"], out["h"] = np.zeros((cap, 2)), np.zeros((cap, 3))
    for k, node in enumerate(nodes):
        for name, value in node.items():
            out["node_parent" if name == "parent" else name][k] = value
    out["parent"] = np.full(cap, -1, dtype=np.int32)
    out["root"] = np.full(cap, -1, dtype=np.int32)
    out["depth"] = np.zeros(cap, dtype=np.int32)
    out["root"][:n] = np.arange(n)
    for k, node in enumerate(nodes):
        for cid in node["child"]:
            if cid < n:
                out["parent"][cid] = n + k
    for i in range(n):
        p = out["parent"][i]
        while p >= 0:
            out["root"][i], out["depth"][i] = p, out["depth"][i] + 1
            p = nodes[p - n]["parent"]
    sizes = [1] * int((nid[live] < n).sum()) + [nodes[c - n]["leaves"] for c in nid[live] if c >= n]
    out["singles"], out["binaries"], out["triples"] = (sizes.count(k) for k in (1, 2, 3))
    out["higher"] = sum(1 for k in sizes if k >= 4)
    out["unstable"] = sum(1 for c in nid[live] if c >= n and not nodes[c - n]["stable"])
    return out


def describe(ref):
    """The reference's roots in ascending slot, Fewbody style."""
    n, made = ref["count"], ref["nodes"]

    def text(i):
        return str(i) if i < n else "[" + " ".join(text(int(c)) for c in ref["child"][i - n]) + "]"
    leaves = made + ref["roots"]
    child = set(ref["child"][:made].ravel().tolist())
    roots = [(i, i) for i in range(leaves) if i not in child]
    roots += [(int(ref["slot"][k]), n + k) for k in range(made) if ref["node_parent"][k] < 0]
    return " ".join(text(i) for _, i in sorted(roots))


# ---- the inputs -------------------------------------------------------------------------------------------------------------
SPACING, JITTER, DRIFT = 2.0, 0.3, 20.0
KINDS = ("single", "binary", "triple", "unstable_triple", "two_plus_two", "two_plus_one_plus_one")
SIZES = dict(single=1, binary=2, triple=3, unstable_triple=3, two_plus_two=4, two_plus_one_plus_one=4)


def _leaf(rng):
    return np.array([rng.uniform(0.5, 1.5)]), np.zeros((1, 3)), np.zeros((1, 3))


def kepler(mu, a, e, E, p, q):
    """(r, v) of the relative orbit at eccentric anomaly E in the plane of the orthonormal p (to pericentre) and q."""
    b = a * np.sqrt(1 - e * e)
    Edot = np.sqrt(mu / a ** 3) / (1 - e * np.cos(E))
    return a * (np.cos(E) - e) * p + b * np.sin(E) * q, -a * np.sin(E) * Edot * p + b * np.cos(E) * Edot * q


def join(A, B, a, e, E, p, q):
    """Two objects (masses, positions and velocities about their centres of mass) on a Kepler orbit about each other."""
    MA, MB = A[0].sum(), B[0].sum()
    r, v = kepler(MA + MB, a, e, E, p, q)
    fa, fb = MB / (MA + MB), MA / (MA + MB)
    return (np.concatenate([A[0], B[0]]), np.concatenate([A[1] - fa * r, B[1] + fb * r]),
            np.concatenate([A[2] - fa * v, B[2] + fb * v]))


def _random_join(rng, A, B, a, e):
    p = pref._unit(rng, 1)[0]
    q = np.cross(p, pref._unit(rng, 1)[0])
    q /= np.linalg.norm(q)
    return join(A, B, rng.uniform(*a), rng.uniform(*e), rng.uniform(0, 2 * np.pi), p, q)


def make_object(rng, kind):
    """(masses, positions, velocities) of one object about its centre of mass."""
    inner, wide, e = (0.01, 0.02), (0.2, 0.4), (0.1, 0.5)
    if kind == "single":
        return _leaf(rng)
    if kind == "binary":
        return _random_join(rng, _leaf(rng), _leaf(rng), (0.01, 0.05), (0.1, 0.8))
    if kind == "triple":
        return _random_join(rng, _random_join(rng, _leaf(rng), _leaf(rng), inner, e), _leaf(rng), wide, e)
    if kind == "unstable_triple":
        return _random_join(rng, _random_join(rng, _leaf(rng), _leaf(rng), inner, e), _leaf(rng), (0.05, 0.08), (0.3, 0.6))
    if kind == "two_plus_two":
        return _random_join(rng, _random_join(rng, _leaf(rng), _leaf(rng), inner, e),
                            _random_join(rng, _leaf(rng), _leaf(rng), inner, e), wide, e)
    if kind == "two_plus_one_plus_one":
        core = _random_join(rng, _random_join(rng, _leaf(rng), _leaf(rng), (0.002, 0.004), e), _leaf(rng), (0.03, 0.05), e)
        return _random_join(rng, core, _leaf(rng), (0.4, 0.5), e)
    raise ValueError(kind)


def objects(n, seed):
    """(pos, vel): (n, 4) float32.  The six kinds in rotation until the count is filled (a kind that no longer fits is passed
    over), one object per site of a cubic lattice of spacing 2 with a jitter of +-0.3 and a drift of up to 20 per component,
    so that objects bind to each other only by a rare chance; the bodies in a random order."""
    rng = np.random.default_rng(seed)
    made, left, k = [], n, 0
    while left:
        kind = KINDS[k % len(KINDS)]
        k += 1
        if SIZES[kind] <= left:
            made.append(make_object(rng, kind))
            left -= SIZES[kind]
    K = len(made)
    side = max(1, int(np.ceil(K ** (1.0 / 3.0))))
    sites = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(side ** 3)[:K]]
    centre = (sites - 0.5 * (side - 1)) * SPACING + rng.uniform(-JITTER, JITTER, size=(K, 3))
    drift = rng.uniform(-DRIFT, DRIFT, size=(K, 3))
    pos, vel = np.zeros((n, 4)), np.zeros((n, 4))
    at = 0
    for (ms, x, v), c, d in zip(made, centre, drift):
        pos[at:at + len(ms), :3], pos[at:at + len(ms), 3], vel[at:at + len(ms), :3] = x + c, ms, v + d
        at += len(ms)
    order = rng.permutation(n)
    return pos[order].astype(np.float32), vel[order].astype(np.float32)


CAPACITIES = pref.CAPACITIES
FILL = pref.FILL
SEED0 = 7100  # 7000 left the 4096-body system 3.6e-5 from the tolerance 0.01 (margin d)
#: capacity -> the tolerances the GPU suite runs at it
TOLERANCES = {64: (np.inf,), 128: (np.inf,), 130: (np.inf,), 257: (np.inf, 0.01), 4096: (np.inf, 0.01)}


def gpu_inputs(capacity):
    """(P, V, counts) of the GPU suite's batch at a capacity."""
    counts = CAPACITIES[capacity]
    P = np.full((len(counts), capacity, 4), FILL, dtype=np.float32)
    V = np.full((len(counts), capacity, 4), FILL, dtype=np.float32)
    for s, n in enumerate(counts):
        if n:
            P[s, :n], V[s, :n] = objects(n, SEED0 + capacity + s)
    return P, V, counts


_cache = {}


def reference(capacity, tolerance=np.inf):
    """The references of gpu_inputs(capacity) at a tolerance and max_levels = 16, computed once."""
    key = (capacity, float(tolerance))
    if key not in _cache:
        P, V, counts = gpu_inputs(capacity)
        _cache[key] = [hierarchy(P[s], V[s], n, tidal_tolerance=tolerance, max_levels=MAX_LEVELS) for s, n in enumerate(counts)]
    return _cache[key]


def holds(ref, tolerance=np.inf):
    """The inputs condition of one reference."""
    mg = ref["margins"]
    return mg["a"] >= MARGINS["a"] and mg["b"] >= MARGINS["b"] and mg["c"] >= MARGINS["c"] and \
        (not np.isfinite(tolerance) or mg["d"] >= MARGINS["d"])


# ---- hand-worked cases ------------------------------------------------------------------------------------------------------
EX, EY, EZ = np.eye(3)


def place(obj, capacity, centre=(0.0, 0.0, 0.0), order=None):
    """(pos, vel): (capacity, 4) float32 with the object's bodies first (in `order`), the rest FILL."""
    ms, x, v = obj
    order = np.arange(len(ms)) if order is None else np.asarray(order)
    pos, vel = np.full((capacity, 4), FILL, np.float32), np.full((capacity, 4), FILL, np.float32)
    pos[:len(ms), :3], pos[:len(ms), 3], vel[:len(ms), :3] = (x + np.asarray(centre))[order], ms[order], v[order]
    vel[:len(ms), 3] = 0
    return pos, vel


def leaf(mass):
    return np.array([float(mass)]), np.zeros((1, 3)), np.zeros((1, 3))


def _turned(obj):
    """The object turned by 0.9 about (1, 2, 3): no orbit lies in a coordinate plane, where the inclination's acos loses digits."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.9) * K + (1 - np.cos(0.9)) * (K @ K)
    return obj[0], obj[1] @ R.T, obj[2] @ R.T


def designed_triple(outer_a=1.0, outer_e=0.2, tilt=0.2, inner_a=0.05):
    """Bodies 0 and 1: masses 1 and 0.5 on a = inner_a, e = 0.3; body 2: mass 0.75 on an outer orbit whose plane is tilted by
    `tilt` against the inner one.  M&A threshold at tilt 0.2: 2.8 (1.5 x 1.2 / sqrt(0.8))^0.4 (1 - 0.06 / pi) = 3.63, against
    outer_a (1 - 0.2) / 0.05 = 16 for outer_a = 1 and 1.6 for outer_a = 0.1."""
    inner = join(leaf(1.0), leaf(0.5), inner_a, 0.3, 1.0, EX, EY)
    return _turned(join(inner, leaf(0.75), outer_a, outer_e, 2.0, EX, np.cos(tilt) * EY + np.sin(tilt) * EZ))


def designed_two_plus_two():
    """Bodies (0, 1) and (2, 3): inner binaries of a = 0.02 and 0.03 on an outer orbit of a = 1 tilted by 0.5 and pi / 2
    against them."""
    A = join(leaf(1.0), leaf(0.5), 0.02, 0.2, 1.0, EX, EY)
    B = join(leaf(0.75), leaf(1.25), 0.03, 0.4, 2.5, EY, EZ)
    return _turned(join(A, B, 1.0, 0.3, 1.5, EX, np.cos(0.5) * EY + np.sin(0.5) * EZ))


def designed_nested():
    """(2 + 1) + 1: bodies 0, 1 on a = 0.003 inside a = 0.04 (body 2) inside a = 0.45 (body 3)."""
    core = join(join(leaf(1.0), leaf(0.8), 0.003, 0.2, 1.0, EX, EY), leaf(0.6), 0.04, 0.2, 2.0, EY, EZ)
    return _turned(join(core, leaf(1.2), 0.45, 0.3, 3.0, EX, EY))

MASSIVE_BODIES, MASSIVE_CAPACITY, MASSIVE = 96, 128, [0, 1, 3, 96]


def massive_inputs():
    """(P, V, counts, massive): one 96-body system four times, with 0, 1, 3 and 96 of its bodies massive."""
    pos, vel = objects(MASSIVE_BODIES, SEED0 + 1)
    P = np.full((len(MASSIVE), MASSIVE_CAPACITY, 4), FILL, dtype=np.float32)
    V = np.full((len(MASSIVE), MASSIVE_CAPACITY, 4), FILL, dtype=np.float32)
    P[:, :MASSIVE_BODIES], V[:, :MASSIVE_BODIES] = pos, vel
    return P, V, [MASSIVE_BODIES] * len(MASSIVE), list(MASSIVE)


INVARIANCE_BODIES = 120


def invariance_inputs(capacity):
    """(pos, vel): one 120-body system at a capacity, the rest FILL."""
    pos, vel = np.full((capacity, 4), FILL, dtype=np.float32), np.full((capacity, 4), FILL, dtype=np.float32)
    pos[:INVARIANCE_BODIES], vel[:INVARIANCE_BODIES] = objects(INVARIANCE_BODIES, SEED0 + 2)
    return pos, vel
