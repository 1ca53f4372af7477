"""Numpy reference of nbody_batch_mutual_gravity (include/nbody_batch_mutual_gravity.h) in IEEE doubles in the pinned order, and
the inputs of its tests.

The sums.  Row sums are sequential accumulations over the sources in ascending j (one vector add per column, over all rows at
once: never np.sum); the rows of a set in ascending body index, blocks of 64 ranks by the halving tree; blocks in ascending
order.  numpy's fp64 +, -, x, / and sqrt are IEEE.

The error measure.  Beside every floating word the reference forms its absolute companion: the same formation with every
subtraction or signed addition of products replaced by a sum of absolute values (|p_y f_z| + |p_z f_y|, |mm| sum_j |g d_c|, ...).
Addends cancel -- the force of a set on itself is zero -- so an error is |got - ref| over the companion, not over the word.
Every floating word passes through a square root and a division, so a device may differ in the last place: BOUND is four times
the spread the reference itself shows when every root and quotient is moved by up to one ulp at random (jitter_spread, measured
again by test_batch_mutual_gravity_cpu.py).  Correctly rounded operations sit at zero error.  Integers and the system record
are always compared exactly."""
import functools
from fractions import Fraction

import numpy as np

MAX_SETS = 8
NO_SET = 255
BLOCK = 64
TERMS = ("potential", "force_x", "force_y", "force_z", "torque_x", "torque_y", "torque_z", "virial", "power")
ENTRY_WORDS = ("pairs", "potential", "force", "torque", "virial", "power")
SYSTEM_WORDS = ("sets", "selected", "left_out", "unmeasured", "pairs", "coincident", "members", "mass")
ENTRY_DTYPE = np.dtype([("pairs", np.int64), ("potential", np.float64), ("force", np.float64, 3), ("torque", np.float64, 3),
                        ("virial", np.float64), ("power", np.float64)])
SYSTEM_DTYPE = np.dtype([("sets", np.int32), ("selected", np.int32), ("left_out", np.int32), ("unmeasured", np.int32),
                         ("pairs", np.int64), ("coincident", np.int64), ("members", np.int32, 8), ("mass", np.float64, 8)])
ENTRY_OFFSETS = {"pairs": 0, "potential": 8, "force": 16, "torque": 40, "virial": 64, "power": 72}
SYSTEM_OFFSETS = {"sets": 0, "selected": 4, "left_out": 8, "unmeasured": 12, "pairs": 16, "coincident": 24, "members": 32, "mass": 64}
assert ENTRY_DTYPE.itemsize == 80 and SYSTEM_DTYPE.itemsize == 128

#: Measured by jitter_spread() over every case of the capacities 64, 128 and 256: 1.41e-15 with its seed and 1.39e-15, 1.42e-15
#: and 1.53e-15 with three others; the largest, rounded up.  It is the force's, in sets of one or two bodies, where one pair is
#: the whole sum and g carries the moved quotient three times.  No integer and no word of a system record moved.
SPREAD = 1.6e-15
BOUND = 4.0 * SPREAD  # 6.4e-15


# ---- the reference -----------------------------------------------------------------------------------------------------------
def wire_labels(labels):
    """Labels as the ABI takes them: uint8, 255 for every negative value."""
    labels = np.asarray(labels)
    return np.where(labels < 0, NO_SET, labels).astype(np.uint8)


def stable_ranks(sets_of, sets):
    """(order, start): the bodies with sets_of >= 0 sorted by set, ascending index within a set (numpy's stable argsort), and
    where each set starts in that order."""
    sets_of = np.asarray(sets_of)
    chosen = np.nonzero(sets_of >= 0)[0]
    order = chosen[np.argsort(sets_of[chosen], kind="stable")]
    members = np.bincount(sets_of[chosen], minlength=sets)[:sets]
    return order, np.concatenate([[0], np.cumsum(members)]).astype(np.int64)


def move(x, rng):
    """x moved by -1, 0 or +1 ulp at random."""
    k = rng.integers(-1, 2, size=x.shape)
    return np.where(k < 0, np.nextafter(x, -np.inf), np.where(k > 0, np.nextafter(x, np.inf), x))


def tree(p):
    """The halving tree over axis 1 (64 long) of p, which it overwrites; the partials p[:, 0]."""
    off = BLOCK // 2
    while off:
        p[:, :off] = p[:, :off] + p[:, off:2 * off]
        off //= 2
    return p[:, 0]


def reference(pos, vel, n, labels, sets, eps=0.0, centre=None, velocity=None, rng=None):
    """Every word of one system: {"system": SYSTEM_DTYPE scalar, "entries": (K, K) ENTRY_DTYPE, "absolute": (K, K, 9) the
    companions in the order of TERMS}.  labels: n or more integers, negative or 255 for no set."""
    pos, vel = np.asarray(pos, np.float32), np.asarray(vel, np.float32)
    lab = np.asarray(labels)[:n].astype(np.int64)
    lab = np.where((lab < 0) | (lab == NO_SET), -1, lab)
    assert (lab < sets).all()
    words = np.concatenate([pos[:n, :4], vel[:n, :3]], axis=1)
    measured = np.isfinite(words).all(axis=1)
    sets_of = np.where(measured, lab, -1)
    order, start = stable_ranks(sets_of, sets)
    members = np.diff(start)
    centre = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    velocity = np.zeros(3) if velocity is None else np.asarray(velocity, np.float64)
    e2 = np.float64(np.float32(eps)) * np.float64(np.float32(eps))
    x, m, v = pos[order, :3].astype(np.float64), pos[order, 3].astype(np.float64), vel[order, :3].astype(np.float64)
    S = len(order)
    P, A = np.zeros((S, sets)), np.zeros((S, sets, 3))                            # row sums per source set
    Pabs, Aabs = np.zeros((S, sets)), np.zeros((S, sets, 3))
    coincident = 0
    with np.errstate(all="ignore"):
        for b in range(sets):
            for j in range(start[b], start[b + 1]):                              # ascending j within the set: one add each
                d = x[j][None, :] - x
                s2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + e2
                examined = np.arange(S) != j
                apart = s2 != 0.0
                coincident += int((examined & ~apart).sum())
                adds = examined & apart
                r = np.sqrt(np.where(apart, s2, 1.0))
                if rng is not None:
                    r = move(r, rng)
                inv = 1.0 / r
                if rng is not None:
                    inv = move(inv, rng)
                mi = m[j] * inv
                g = (mi * inv) * inv
                P[:, b] = P[:, b] + np.where(adds, mi, 0.0)
                A[:, b] = A[:, b] + np.where(adds[:, None], g[:, None] * d, 0.0)
                Pabs[:, b] += np.where(adds, np.abs(mi), 0.0)
                Aabs[:, b] += np.where(adds[:, None], np.abs(g[:, None] * d), 0.0)
        p, q = x - centre[None, :], v - velocity[None, :]
        entries = np.zeros((sets, sets), ENTRY_DTYPE)
        absolute = np.zeros((sets, sets, len(TERMS)))
        for a in range(sets):
            rows = slice(start[a], start[a + 1])
            na = int(members[a])
            padded = -(-max(na, 1) // BLOCK) * BLOCK
            mm, pa, qa = m[rows], p[rows], q[rows]
            for b in range(sets):
                f = mm[:, None] * A[rows, b]
                fabs = np.abs(mm)[:, None] * Aabs[rows, b]
                w = np.zeros((padded, len(TERMS)))                                # +0.0 at the missing ranks
                w[:na, 0] = mm * P[rows, b]
                w[:na, 1:4] = f
                w[:na, 4] = pa[:, 1] * f[:, 2] - pa[:, 2] * f[:, 1]
                w[:na, 5] = pa[:, 2] * f[:, 0] - pa[:, 0] * f[:, 2]
                w[:na, 6] = pa[:, 0] * f[:, 1] - pa[:, 1] * f[:, 0]
                w[:na, 7] = (pa[:, 0] * f[:, 0] + pa[:, 1] * f[:, 1]) + pa[:, 2] * f[:, 2]
                w[:na, 8] = (qa[:, 0] * f[:, 0] + qa[:, 1] * f[:, 1]) + qa[:, 2] * f[:, 2]
                partials = tree(w.reshape(padded // BLOCK, BLOCK, len(TERMS)).copy())
                total = np.zeros(len(TERMS))
                for k in range(partials.shape[0]):                                # the blocks in ascending order
                    total = total + partials[k]
                e = entries[a, b]
                e["pairs"] = na * int(members[b]) - (na if a == b else 0)
                e["potential"] = 0.0 - total[0]
                e["force"], e["torque"], e["virial"], e["power"] = total[1:4], total[4:7], total[7], total[8]
                ap, aq = np.abs(pa), np.abs(qa)
                absolute[a, b, 0] = (np.abs(mm) * Pabs[rows, b]).sum()
                absolute[a, b, 1:4] = fabs.sum(axis=0)
                absolute[a, b, 4] = (ap[:, 1] * fabs[:, 2] + ap[:, 2] * fabs[:, 1]).sum()
                absolute[a, b, 5] = (ap[:, 2] * fabs[:, 0] + ap[:, 0] * fabs[:, 2]).sum()
                absolute[a, b, 6] = (ap[:, 0] * fabs[:, 1] + ap[:, 1] * fabs[:, 0]).sum()
                absolute[a, b, 7] = (ap * fabs).sum()
                absolute[a, b, 8] = (aq * fabs).sum()
    system = np.zeros((), SYSTEM_DTYPE)
    system["sets"] = sets
    system["selected"] = S
    system["left_out"] = int((lab < 0).sum())
    system["unmeasured"] = int(((lab >= 0) & ~measured).sum())
    system["pairs"] = int(entries["pairs"].sum())
    system["coincident"] = coincident
    system["members"][:sets] = members
    for a in range(sets):
        mass = np.float64(0.0)
        for value in m[start[a]:start[a + 1]]:                                    # ascending body index, one add each
            mass = mass + value
        system["mass"][a] = mass
    assert int(system["selected"]) + int(system["left_out"]) + int(system["unmeasured"]) == n
    return {"system": system, "entries": entries, "absolute": absolute}


def floats_of(entries):
    """(..., 9) float64: the nine floating words of entries in the order of TERMS."""
    e = np.asarray(entries)
    return np.concatenate([e["potential"][..., None], e["force"], e["torque"], e["virial"][..., None], e["power"][..., None]], axis=-1)


def error_of(got_entries, ref):
    """The largest |got - ref| over the companion, over the entries and the nine floating words."""
    got, want, scale = floats_of(got_entries), floats_of(ref["entries"]), ref["absolute"]
    diff = np.abs(got - want)
    assert (diff[scale == 0.0] == 0.0).all()
    return float(np.max(diff[scale > 0.0] / scale[scale > 0.0])) if (scale > 0.0).any() else 0.0


# ---- inputs ----------------------------------------------------------------------------------------------------------------
CAPACITIES = (64, 128, 256, 1024, 4096)
COUNTS = (0, 1, 2, 3, 63, 64, 65, 129, 257)
RANK_SIZES = (0, 1, 63, 64, 65)
CENTRE = np.array([0.75, -1.5, 0.375])
VELOCITY = np.array([-0.25, 0.5, 1.125])


def state(n, seed):
    """(pos, vel): Gaussian positions and velocities and uniform masses as fp32 draws them."""
    rng = np.random.default_rng(seed)
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.normal(0.0, 2.0, size=(n, 3))
    pos[:, 3] = rng.uniform(0.5, 1.5, size=n)
    vel[:, :3] = rng.normal(0.0, 1.0, size=(n, 3))
    vel[:, 3] = np.nan                                                          # the fourth velocity word is not read
    return pos, vel


def counts_of(capacity):
    if capacity == 4096:
        return [4096, 1025]
    return [c for c in COUNTS if c <= capacity] + [capacity]


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, V, counts): one system per count.  From 63 bodies on a system holds a body with a NaN coordinate (5), one with an
    infinite velocity word (9) and two coincident bodies (11, 12): unmeasured where they are labelled, a coincident pair
    where the softening is 0.  Words beyond the count are garbage that nothing reads."""
    counts = counts_of(capacity)
    B = len(counts)
    P, V = np.full((B, capacity, 4), np.nan, np.float32), np.full((B, capacity, 4), np.inf, np.float32)
    for s, n in enumerate(counts):
        p, v = state(n, 100 * capacity + s)
        if n >= 63:
            p[5, 1] = np.nan
            v[9, 0] = np.inf
            p[12, :3] = p[11, :3]
        P[s, :n], V[s, :n] = p, v
    P.flags.writeable = V.flags.writeable = False
    return P, V, counts


def labelling(kind, n, capacity, sets, seed):
    """(capacity,) int64 labels of a system of n bodies, -1 for no set; the words from n on are labelled too and read by
    nothing."""
    i = np.arange(capacity)
    if kind == "interleaved":
        return i % sets
    if kind == "contiguous":                                                    # runs of n / sets bodies
        return np.minimum(i * sets // max(n, 1), sets - 1)
    if kind == "none":
        return np.full(capacity, -1, np.int64)
    if kind == "ranks":                                                         # sets of 0, 1, 63, 64 and 65 bodies, scattered
        rng = np.random.default_rng(seed)
        labels = np.full(capacity, -1, np.int64)
        shuffled = rng.permutation(n)
        at = 0
        for a, size in enumerate(RANK_SIZES[:sets]):
            take = shuffled[at:at + size]
            labels[take] = a
            at += len(take)
        rest = shuffled[at:]
        if sets > len(RANK_SIZES):                                              # every other body over the sets that are left
            labels[rest[::2]] = len(RANK_SIZES) + np.arange(len(rest[::2])) % (sets - len(RANK_SIZES))
        return labels
    raise ValueError(kind)


#: (name, sets, labelling, softening, frame): K = 1, 2, 3 and 8, every labelling, the softening 0 and above, a frame or none.
CASES = (("interleaved-1", 1, "interleaved", 0.0, False), ("interleaved-2-frame", 2, "interleaved", 0.0, True),
         ("interleaved-3-soft", 3, "interleaved", 0.0625, False), ("interleaved-8-frame", 8, "interleaved", 0.0, True),
         ("contiguous-3", 3, "contiguous", 0.0, False), ("contiguous-8-soft-frame", 8, "contiguous", 0.05, True),
         ("ranks-8-frame", 8, "ranks", 0.0, True), ("ranks-5-soft", 5, "ranks", 0.01, False), ("none-2", 2, "none", 0.0, True))
#: capacity 4096: the system of 4096 bodies in 2 sets and the one of 1025 in 8, the other system unlabelled.
LARGE_CASES = (("large-2", 2, "interleaved", 0.0, True), ("large-8", 8, "interleaved", 0.0, True))


def cases_of(capacity):
    return LARGE_CASES if capacity == 4096 else CASES


@functools.lru_cache(maxsize=None)
def gpu_labels(capacity, name):
    """(B, capacity) int64 labels of gpu_inputs(capacity) in case `name`."""
    _, sets, kind, _, _ = next(c for c in cases_of(capacity) if c[0] == name)
    counts = counts_of(capacity)
    L = np.stack([labelling(kind, n, capacity, sets, 7000 + capacity + s) for s, n in enumerate(counts)])
    if capacity == 4096:
        L[1 if name == "large-2" else 0] = -1
    L.flags.writeable = False
    return L


def gpu_frames(capacity, frame):
    """(centre, velocity): (B, 3) each, a different one per system, or (None, None)."""
    if not frame:
        return None, None
    B = len(counts_of(capacity))
    shift = 0.125 * np.arange(B)[:, None]
    return CENTRE[None, :] + shift, VELOCITY[None, :] - shift


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity, name, jitter_seed=None):
    """The references of gpu_inputs(capacity) in case `name`, one dict per system; computed once per session."""
    _, sets, _, eps, frame = next(c for c in cases_of(capacity) if c[0] == name)
    P, V, counts = gpu_inputs(capacity)
    L = gpu_labels(capacity, name)
    centre, velocity = gpu_frames(capacity, frame)
    rng = None if jitter_seed is None else np.random.default_rng(jitter_seed)
    return [reference(P[s], V[s], counts[s], L[s], sets, eps, None if centre is None else centre[s],
                      None if velocity is None else velocity[s], rng) for s in range(len(counts))]


def jitter_spread(capacities=(64, 128, 256), seed=77):
    """(spread, same): the largest error measure of the reference with every root and quotient moved by up to one ulp at
    random, against itself unmoved; and whether every integer and every system record stayed the same bytes."""
    spread, same = 0.0, True
    for capacity in capacities:
        for name, *_ in cases_of(capacity):
            for ref, moved in zip(gpu_reference(capacity, name), gpu_reference(capacity, name, seed)):
                spread = max(spread, error_of(moved["entries"], ref))
                same = same and moved["system"].tobytes() == ref["system"].tobytes() and \
                    (moved["entries"]["pairs"] == ref["entries"]["pairs"]).all()
    return spread, same


# ---- a plain pair walk: the independent check of the reference -------------------------------------------------------------------
def plain_walk(pos, vel, n, labels, sets, eps=0.0, centre=None, velocity=None):
    """(K, K, 9) sums by vectorised numpy over all pairs at once in no particular order (np.sum), with g = m_j / (s2 r): every
    body's words as float64, no ranks, no trees."""
    pos, vel = np.asarray(pos)[:n].astype(np.float64), np.asarray(vel)[:n].astype(np.float64)
    lab = np.asarray(labels)[:n].astype(np.int64)
    lab = np.where((lab < 0) | (lab == NO_SET), -1, lab)
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(vel[:, :3]).all(axis=1)
    lab = np.where(ok, lab, -1)
    centre = np.zeros(3) if centre is None else np.asarray(centre, np.float64)
    velocity = np.zeros(3) if velocity is None else np.asarray(velocity, np.float64)
    out = np.zeros((sets, sets, len(TERMS)))
    e2 = float(np.float32(eps)) ** 2
    with np.errstate(all="ignore"):
        for a in range(sets):
            ia = np.nonzero(lab == a)[0]
            for b in range(sets):
                ib = np.nonzero(lab == b)[0]
                if not len(ia) or not len(ib):
                    continue
                d = pos[ib][None, :, :3] - pos[ia][:, None, :3]
                s2 = (d * d).sum(-1) + e2
                take = (ia[:, None] != ib[None, :]) & (s2 != 0.0)
                r = np.sqrt(np.where(take, s2, 1.0))
                mimj = pos[ia, 3][:, None] * pos[ib, 3][None, :]
                u = np.where(take, mimj / r, 0.0)
                f = np.where(take[..., None], (mimj / (s2 * r))[..., None] * d, 0.0)
                p = (pos[ia, :3] - centre)[:, None, :]
                q = (vel[ia, :3] - velocity)[:, None, :]
                out[a, b, 0] = -u.sum()
                out[a, b, 1:4] = f.sum(axis=(0, 1))
                out[a, b, 4:7] = np.cross(p, f).sum(axis=(0, 1))
                out[a, b, 7] = (p * f).sum()
                out[a, b, 8] = (q * f).sum()
    return out


# ---- the closed form: every operation exact ----------------------------------------------------------------------------------
def closed_form_state():
    """(pos, vel, labels, centre, velocity): set 0 is one body of mass 4 at the origin; set 1 is 36 bodies of power-of-two mass
    at +-2^k (k = -2 ... 3) on the axes.  With softening 0 every operation of the two cross entries is exact: s2 = 4^k,
    r = 2^k, and every product and sum is a dyadic number of few bits."""
    n = 37
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[0, 3] = 4.0
    vel[0, :3] = (0.5, -0.25, 2.0)
    i = 1
    for k in range(-2, 4):
        for axis in range(3):
            for sign in (1.0, -1.0):
                pos[i, axis] = sign * 2.0 ** k
                pos[i, 3] = 2.0 ** ((i % 3) - 1)
                vel[i, :3] = (0.25 * (i % 5), -0.5 * (i % 3), 0.125 * (i % 7))
                i += 1
    labels = np.ones(n, np.int64)
    labels[0] = 0
    return pos, vel, labels, np.array([0.5, -2.0, 0.25]), np.array([1.0, 0.5, -0.75])


def closed_form():
    """{(0, 1): nine floats, (1, 0): nine floats} in the order of TERMS, from exact rational arithmetic."""
    pos, vel, labels, centre, velocity = closed_form_state()
    F = Fraction
    x = [[F(float(c)) for c in row[:3]] for row in pos]
    m = [F(float(row[3])) for row in pos]
    v = [[F(float(c)) for c in row[:3]] for row in vel]
    c0, v0 = [F(float(c)) for c in centre], [F(float(c)) for c in velocity]

    def entry(rows, sources):
        total = [F(0)] * 9
        for i in rows:
            P, A = F(0), [F(0)] * 3
            for j in sources:
                d = [x[j][c] - x[i][c] for c in range(3)]
                r = max(abs(c) for c in d)                                        # on an axis: the distance is the one coordinate
                assert sum(c * c for c in d) == r * r
                P += m[j] / r
                A = [A[c] + m[j] * d[c] / r ** 3 for c in range(3)]
            f = [m[i] * A[c] for c in range(3)]
            p = [x[i][c] - c0[c] for c in range(3)]
            q = [v[i][c] - v0[c] for c in range(3)]
            add = [m[i] * P, f[0], f[1], f[2], p[1] * f[2] - p[2] * f[1], p[2] * f[0] - p[0] * f[2], p[0] * f[1] - p[1] * f[0],
                   sum(p[c] * f[c] for c in range(3)), sum(q[c] * f[c] for c in range(3))]
            total = [t + w for t, w in zip(total, add)]
        total[0] = -total[0]
        out = [float(t) for t in total]
        assert all(Fraction(o) == t for o, t in zip(out, total))                    # every word is a double
        return np.array(out) + 0.0                                                 # no -0
    ones = list(range(1, len(pos)))
    return {(0, 1): entry([0], ones), (1, 0): entry(ones, [0])}
