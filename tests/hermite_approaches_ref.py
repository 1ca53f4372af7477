"""Numpy reference of nbody_batch_approaches (include/nbody_batch_approaches.h) over exact integer arithmetic, and the inputs of
its tests.

Every finite coordinate is an integer in [-32, 32], every finite velocity component an integer in [-2, 2], every horizon an
integer <= 8 and every radius a small integer, so every word of the three chains (r2, v2, rv), of the separation at the horizon
(e, m2) and of the predicate (vh, g, lhs, rhs) is an integer below 2^24: the same number in fp32 and in int64
(test_batch_approaches_cpu.py checks the premise on every input).  The phase of a pair is then decided on integers in the
header's order.  Only the sign of a zero rv is not an integer's: the reference gives the list's rv the sign the fp32 chain
gives it (a sum of zero products is -0 iff every one of them is).  A body with a NaN or an infinite coordinate or velocity
component has no measured pair."""
import functools

import numpy as np

from hermite_contacts_ref import B, CAPACITIES, MODES, SHAPES, SIDE, check_identity, cube, truncating_capacity  # noqa: F401

LIMIT = 32                            # |coordinate| <=
SPEED = 2                             # |velocity component| <=
MAX_HORIZON = 8
RADIUS = (3.0, 3.0, 3.0, 2.0, 3.0)    # radius mode: one per system
HORIZON = (6.0, 0.0, 8.0, 4.0, 6.0)   # one per system
NOW, PASSAGE, END = 0, 1, 2
SYSTEM_DTYPE = np.dtype([("bodies", np.int32), ("approaching", np.int32), ("max_degree", np.int32), ("reserved", np.int32),
                         ("pairs", np.int64), ("stored", np.int64), ("now", np.int32), ("passing", np.int32), ("ending", np.int32),
                         ("reserved2", np.int32)])
BODY_DTYPE = np.dtype([("degree", np.int32), ("upper", np.int32), ("first", np.int32), ("now", np.int32)])
ENTRY_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("r2", np.float32), ("rv", np.float32), ("v2", np.float32),
                        ("phase", np.int32)])
assert SYSTEM_DTYPE.itemsize == 48 and BODY_DTYPE.itemsize == 16 and ENTRY_DTYPE.itemsize == 24
BLOCK = 512                           # rows of the pair matrix at a time


# ---- the reference -----------------------------------------------------------------------------------------------------------
def integers(pos, vel, n):
    """(x, v, finite): int64 (n, 3) positions and velocities, zero where the body is not finite, and which bodies are."""
    x, v = np.asarray(pos)[:n, :3].astype(np.float64), np.asarray(vel)[:n, :3].astype(np.float64)
    finite = np.isfinite(x).all(axis=1) & np.isfinite(v).all(axis=1)
    return np.where(finite[:, None], x, 0.0).astype(np.int64), np.where(finite[:, None], v, 0.0).astype(np.int64), finite


def thresholds(n, rows, radius=None, radii=None):
    """int64: t2 of every pair of `rows` with all columns, a scalar (radius mode) or (len(rows), n) (radii mode)."""
    if radius is not None:
        assert float(radius) == int(radius)
        return np.int64(int(radius) * int(radius))
    R = np.asarray(radii[:n], np.float64)
    assert np.array_equal(R, np.round(R))
    S = R.astype(np.int64)[rows][:, None] + R.astype(np.int64)[None, :]
    return S * S


def pair_words(x, v, rows, H):
    """The integer words of the pairs (row, column), d and w from the row to the column: r2, v2, rv, m2 and the mask of the
    pairs whose rv is a zero that the fp32 chain gives a minus sign."""
    shape = (len(rows), len(x))
    r2, v2, rv, m2 = (np.zeros(shape, np.int64) for _ in range(4))
    minus = np.ones(shape, bool)
    for c in range(3):
        d = x[None, :, c] - x[rows][:, None, c]
        w = v[None, :, c] - v[rows][:, None, c]
        e = d + w * H
        r2 += d * d
        v2 += w * w
        rv += d * w
        m2 += e * e
        minus &= (d * w == 0) & ((d < 0) | (w < 0))   # a zero factor is +0 (a - a), so the product's sign is the other factor's
    return r2, v2, rv, m2, minus


def phases(r2, v2, rv, m2, t2, H):
    """int8: the phase of every pair of measured, examined bodies in the header's order; -1 where it is no approach."""
    now = r2 <= t2
    closing = rv < 0
    end = -rv >= v2 * H
    ending = closing & end & (m2 <= t2)
    passing = closing & ~end & ((r2 - t2) * v2 <= rv * rv)
    out = np.full(r2.shape, -1, np.int8)
    out[passing] = PASSAGE
    out[ending] = END
    out[now] = NOW
    return out


def reference(pos, vel, n, slots, H, radius=None, radii=None, subset=None):
    """Everything nbody_batch_approaches returns for one system of n bodies in `slots` slots, whatever the capacity:
    {"bodies": (slots,) BODY_DTYPE, "list": (pairs,) ENTRY_DTYPE, "system": the record as a dict without `stored`, "largest":
    the largest integer met}."""
    assert float(H) == int(H) and 0 <= H <= MAX_HORIZON
    H = int(H)
    take = np.ones(n, bool) if subset is None else np.asarray(subset)[:n] != 0
    x, v, finite = integers(pos, vel, n)
    ok = take & finite
    bodies = np.zeros(slots, BODY_DTYPE)
    parts, largest = [], 0
    for start in range(0, n, BLOCK):
        rows = np.arange(start, min(start + BLOCK, n))
        r2, v2, rv, m2, minus = pair_words(x, v, rows, H)
        t2 = thresholds(n, rows, radius, radii)
        phase = phases(r2, v2, rv, m2, t2, H)
        phase[~ok[rows], :] = -1
        phase[:, ~ok] = -1
        phase[np.arange(len(rows)), rows] = -1
        largest = max(largest, *(int(np.abs(a).max()) for a in (r2, v2, rv, m2, v2 * H, (r2 - t2) * v2, rv * rv)))
        approach = phase >= 0
        above = approach & (np.arange(n)[None, :] > rows[:, None])
        bodies["degree"][rows] = approach.sum(axis=1)
        bodies["upper"][rows] = above.sum(axis=1)
        bodies["now"][rows] = (phase == NOW).sum(axis=1)
        i, j = np.nonzero(above)                                   # row-major: ascending in i, then in j
        part = np.zeros(len(i), ENTRY_DTYPE)
        part["i"], part["j"], part["r2"], part["rv"], part["v2"], part["phase"] = rows[i], j, r2[i, j], rv[i, j], v2[i, j], phase[i, j]
        part["rv"][minus[i, j]] = -0.0
        parts.append(part)
    entries = np.concatenate(parts) if parts else np.zeros(0, ENTRY_DTYPE)
    bodies["first"] = np.concatenate([[0], np.cumsum(bodies["upper"].astype(np.int64))[:-1]])
    system = {"bodies": int(take.sum()), "approaching": int((bodies["degree"] > 0).sum()),
              "max_degree": int(bodies["degree"].max()) if slots else 0, "reserved": 0, "pairs": len(entries),
              "now": int((entries["phase"] == NOW).sum()), "passing": int((entries["phase"] == PASSAGE).sum()),
              "ending": int((entries["phase"] == END).sum()), "reserved2": 0}
    return {"bodies": bodies, "list": entries, "system": system, "largest": largest}


def system_record(ref, capacity):
    out = np.zeros((), SYSTEM_DTYPE)
    for name, value in ref["system"].items():
        out[name] = value
    out["stored"] = min(ref["system"]["pairs"], capacity)
    return out


def pad(count):
    out = np.zeros(count, ENTRY_DTYPE)
    out["i"], out["j"], out["r2"], out["phase"] = -1, -1, np.inf, -1
    return out


def listed(ref, capacity):
    """(capacity,) ENTRY_DTYPE: the first min(pairs, capacity) entries, then the pads."""
    out = pad(capacity)
    m = min(len(ref["list"]), capacity)
    out[:m] = ref["list"][:m]
    return out


def check_phases(system):
    assert int(system["now"]) + int(system["passing"]) + int(system["ending"]) == int(system["pairs"])


# ---- inputs ----------------------------------------------------------------------------------------------------------------
#: the hand-placed pairs of the full system, as (d; w) from the lower row to the higher, with their phase at t2 = 9 and H = 6
HAND = {"threshold": ((-4, 3, 0), (1, 0, 0), PASSAGE),     # lhs == rhs == 16
        "boundary": ((-6, 3, 0), (1, 0, 0), END),          # -rv == vh == 6, and m2 == t2
        "inside_at_end": ((-8, 0, 0), (1, 0, 0), END),     # still closing at the horizon, 2 away
        "outside_at_end": ((-10, 0, 0), (1, 0, 0), None),  # its line passes through, after the horizon
        "receding": ((4, 3, 0), (1, 0, 0), None),          # passed within reach before now
        "sideways": ((0, -5, 0), (1, 0, 0), None),         # rv == 0 outside the threshold
        "same": ((0, 0, 0), (0, 0, 0), NOW)}               # coincident, equal velocities, zero radii
BEYOND = ((-4, 3, 1), (1, 0, 0))                           # from the threshold pair's lower body: one beyond, no approach
CORNERS = [(28, 28, 28), (28, 28, -28), (28, -28, 28), (28, -28, -28), (-28, 28, 28), (-28, 28, -28), (-28, -28, 28)]
DRIFT = (-1, 1, 0)                                         # the velocity of every hand-placed pair's lower body


def marks(capacity):
    """Where the hand-placed bodies of the full system sit: name -> (lower row, higher row); "beyond" shares its lower row with
    "threshold"; "last" is the last two rows and "wave" the highest two rows of a last wave (hermite_contacts_ref.marks)."""
    T = SHAPES[capacity][0]
    top = max(r for r in range(capacity) if (r % T) // 64 == T // 64 - 1)
    out = {name: (10 + 2 * k, capacity // 2 + 2 * k + 1) for k, name in enumerate(HAND)}   # the two rows far apart
    out["beyond"] = (out["threshold"][0], capacity // 2 + 20)
    out["last"], out["wave"] = (capacity - 2, capacity - 1), (top - 1, top)
    return out


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, V, counts, R): five systems of 0, 1, 2, min(65, capacity) and capacity bodies, and one integer radius per slot.
    System 1 has H = 0.  System 2 is one pair on its way to a passage inside its horizon.  System 3 is a cube with a coincident
    pair of zero radii and equal velocities, a body with a NaN velocity component and one at +inf.  System 4 is a cube with the
    hand-placed pairs of HAND at its corners, and closing pairs in its last two rows and in the highest rows of a last wave."""
    counts = [0, 1, 2, min(65, capacity), capacity]
    rng = np.random.default_rng(177 + capacity)
    P, V = np.zeros((B, capacity, 4), np.float32), np.zeros((B, capacity, 4), np.float32)
    R = rng.integers(0, 3, size=(B, capacity)).astype(np.float32)   # 0, 1 or 2: S <= 4
    for s in (1, 3, 4):
        side = 5 if s != 4 else SIDE[capacity]
        P[s, :counts[s]] = cube(counts[s], 100 * s + capacity, side)
        V[s, :counts[s], :3] = rng.integers(-SPEED, SPEED + 1, size=(counts[s], 3))
    P[2, :2], V[2, :2, :3] = [[-5, 0, 0, 1], [5, 1, 0, 1]], [[1, 0, 0], [-1, 0, 0]]
    R[2, :2] = 1
    V[3, 5, 1] = np.nan
    P[3, 9, 0] = np.inf
    P[3, 20, :3], V[3, 20, :3] = P[3, 2, :3], V[3, 2, :3]           # coincident, zero radii: phase 0 in radii mode too
    R[3, 20] = R[3, 2] = 0
    m = marks(capacity)
    for (name, (d, w, _)), corner in zip(HAND.items(), CORNERS):
        i, j = m[name]
        P[4, i, :3], V[4, i, :3] = corner, DRIFT
        P[4, j, :3], V[4, j, :3] = np.array(corner) + np.array(d), np.array(DRIFT) + np.array(w)
        R[4, i], R[4, j] = (0, 0) if name == "same" else (1, 2)
    i, j = m["beyond"]
    P[4, j, :3], V[4, j, :3] = P[4, i, :3] + np.array(BEYOND[0], np.float32), V[4, i, :3] + np.array(BEYOND[1], np.float32)
    R[4, j] = 2
    for (i, j), at in ((m["wave"], (-28, -28, -20)), (m["last"], (-28, -28, -28))):   # the same two rows but at 320
        P[4, i, :3], V[4, i, :3] = at, (0, 0, 1)
        P[4, j, :3], V[4, j, :3] = np.array(at) + [0, 0, 5], (0, 0, -1)             # closing from 5 apart: a passage
        R[4, i] = R[4, j] = 1
    for a in (P, V, R):
        a.flags.writeable = False
    return P, V, counts, R


@functools.lru_cache(maxsize=None)
def gpu_subset(capacity):
    """(5, capacity) bool: about two thirds of the slots, the hand-placed bodies among them."""
    keep = np.random.default_rng(3000 + capacity).random((B, capacity)) < 0.67
    for pair in marks(capacity).values():
        keep[4, list(pair)] = True
    keep[3, [2, 20, 5, 9]] = True
    keep[2, :2] = True
    keep.flags.writeable = False
    return keep


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity, mode, with_subset):
    """The references of gpu_inputs(capacity), one per system.  The 4096-body one takes seconds: cached."""
    P, V, counts, R = gpu_inputs(capacity)
    subset = gpu_subset(capacity) if with_subset else None
    return [reference(P[s], V[s], counts[s], capacity, HORIZON[s], radius=RADIUS[s] if mode == "radius" else None,
                      radii=R[s] if mode == "radii" else None, subset=None if subset is None else subset[s]) for s in range(B)]


def gpu_arguments(capacity, mode, with_subset):
    """The arguments of BatchedSystem.approaches for one case: (horizon, keywords)."""
    kw = {"radius": np.array(RADIUS, np.float32)} if mode == "radius" else {"radii": gpu_inputs(capacity)[3]}
    if with_subset:
        kw["subset"] = gpu_subset(capacity)
    return np.array(HORIZON, np.float32), kw
