"""Numpy reference of nbody_batch_contacts (include/nbody_batch_contacts.h) over exact integer arithmetic, and the inputs of its
tests.

Every finite coordinate is an integer in [-128, 128], so every difference, square and sum of the fp32 chain is exact and r2 is
an integer below 2^24, the same number in fp32, in fp64 and in int32; radii are small integers, so b2 = b * b, S = R_i + R_j
and S * S are exact too (test_batch_contacts_cpu.py checks the premise on every input).  A pair is then a contact iff its
integer r2 is <= its integer threshold.  From the full matrix of r2 the reference takes the sorted list, degree, upper, first,
nearest, the closest contact and the records.  A body with a NaN or an infinite coordinate has no measured pair."""
import functools

import numpy as np

CAPACITIES = (64, 128, 320, 4096)     # one row per lane, two, four with two waves, sixteen waves with the raised LDS limit
MODES = ("radius", "radii")
B = 5
LIMIT = 128                           # |coordinate| <=
TOP = 3 * (2 * LIMIT) ** 2 + 1        # above every measured r2: the code of an unmeasured pair
RADIUS = (3.0, 3.0, 3.0, 2.0, 3.0)    # radius mode: one per system
SHAPES = {64: (64, 1), 128: (64, 2), 320: (128, 4), 4096: (1024, 4)}  # batch_shape's (threads, rows per lane)
SIDE = {64: 5, 128: 7, 320: 9, 4096: 21}  # the cubes' half-widths: about 6 bodies within 3 of a body
SYSTEM_DTYPE = np.dtype([("bodies", np.int32), ("touching", np.int32), ("max_degree", np.int32), ("reserved", np.int32),
                         ("pairs", np.int64), ("stored", np.int64), ("closest_i", np.int32), ("closest_j", np.int32),
                         ("closest_r2", np.float32), ("reserved2", np.int32)])
BODY_DTYPE = np.dtype([("degree", np.int32), ("upper", np.int32), ("first", np.int32), ("nearest", np.int32)])
ENTRY_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("r2", np.float32)])
assert SYSTEM_DTYPE.itemsize == 48 and BODY_DTYPE.itemsize == 16 and ENTRY_DTYPE.itemsize == 12


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


def thresholds(n, radius=None, radii=None):
    """int32: t2 of every pair, a scalar (radius mode) or (n, n) (radii mode).  The radii are integers."""
    if radius is not None:
        assert float(radius) == int(radius)
        return np.int32(int(radius) * int(radius))
    R = np.asarray(radii[:n], np.float64)
    assert np.array_equal(R, np.round(R))
    S = R.astype(np.int32)[:, None] + R.astype(np.int32)[None, :]
    return S * S


def reference(pos, n, slots, radius=None, radii=None, subset=None):
    """Everything nbody_batch_contacts returns for one system of n bodies in `slots` slots, whatever the capacity:
    {"bodies": (slots,) BODY_DTYPE, "list": (pairs,) ENTRY_DTYPE, "system": the record as a dict without `stored`}."""
    take = np.ones(n, bool) if subset is None else np.asarray(subset)[:n] != 0
    codes = r2_codes(pos, n)
    contact = (codes < TOP) & (codes <= thresholds(n, radius, radii)) & take[:, None] & take[None, :]
    contact[np.arange(n), np.arange(n)] = False
    above = np.triu(contact, 1)
    bodies = np.zeros(slots, BODY_DTYPE)
    bodies["degree"][:n] = contact.sum(axis=1)
    bodies["upper"][:n] = above.sum(axis=1)
    bodies["first"] = np.concatenate([[0], np.cumsum(bodies["upper"].astype(np.int64))[:-1]])
    nearest = np.where(contact, codes, TOP + 1).argmin(axis=1) if n else np.zeros(0, np.int64)  # the first minimum: the lowest index
    bodies["nearest"] = -1
    bodies["nearest"][:n] = np.where(bodies["degree"][:n] > 0, nearest, -1)
    i, j = np.nonzero(above)                                       # row-major: ascending in i, then in j
    entries = np.zeros(len(i), ENTRY_DTYPE)
    entries["i"], entries["j"], entries["r2"] = i, j, codes[i, j]
    system = {"bodies": int(take.sum()), "touching": int((bodies["degree"] > 0).sum()),
              "max_degree": int(bodies["degree"].max()) if slots else 0, "reserved": 0, "pairs": len(i), "closest_i": -1,
              "closest_j": -1, "closest_r2": np.float32(np.inf), "reserved2": 0}
    if len(i):
        k = int(np.argmin(entries["r2"]))                          # the first minimum of a list sorted by (i, j)
        system.update(closest_i=int(i[k]), closest_j=int(j[k]), closest_r2=entries["r2"][k])
    return {"bodies": bodies, "list": entries, "system": system}


def system_record(ref, capacity):
    out = np.zeros((), SYSTEM_DTYPE)
    for name, value in ref["system"].items():
        out[name] = value
    out["stored"] = min(ref["system"]["pairs"], capacity)
    return out


def listed(ref, capacity):
    """(capacity,) ENTRY_DTYPE: the first min(pairs, capacity) entries, then the pads."""
    out = np.zeros(capacity, ENTRY_DTYPE)
    out["i"], out["j"], out["r2"] = -1, -1, np.inf
    m = min(len(ref["list"]), capacity)
    out[:m] = ref["list"][:m]
    return out


def check_identity(bodies, pairs):
    assert int(bodies["degree"].astype(np.int64).sum()) == 2 * pairs == 2 * int(bodies["upper"].astype(np.int64).sum())


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def cube(n, seed, side):
    """n bodies at random integer positions of a cube of half-width ``side``: (n, 4) float32, mass 1."""
    out = np.ones((n, 4), np.float32)
    out[:, :3] = np.random.default_rng(seed).integers(-side, side + 1, size=(n, 3))
    return out


def marks(capacity):
    """Where the hand-placed bodies of the full system sit: the threshold triple (a, b, c), a coincident pair, the pair of the
    last two rows (the last q that holds rows) and the pair of the highest two rows of a last wave (at 320 bodies in 128 lanes
    the rows from 256 on belong to the first wave: the last wave's highest rows are 254 and 255)."""
    T = SHAPES[capacity][0]
    top = max(r for r in range(capacity) if (r % T) // 64 == T // 64 - 1)
    return {"a": 5, "b": 7, "c": capacity // 2, "same": (9, capacity // 2 + 3), "last": (capacity - 2, capacity - 1),
            "wave": (top - 1, top)}


@functools.lru_cache(maxsize=None)
def gpu_inputs(capacity):
    """(P, counts, R): five systems of 0, 1, 2, min(65, capacity) and capacity bodies, and one integer radius per slot.
    System 2 has no contact in either mode.  System 3 is a cube with a coincident pair of zero radii, a body with a NaN
    coordinate and one at +inf.  System 4 is a cube with, far from it, three bodies a, b, c -- (a, b) exactly on the threshold
    of both modes (r2 == t2 == 9), (a, c) one beyond it (r2 == t2 + 1) -- a coincident pair inside the cube, and its last two
    rows beside each other: rows of the last wave and the last q with upper > 0."""
    counts = [0, 1, 2, min(65, capacity), capacity]
    side = SIDE[capacity]
    P = np.zeros((B, capacity, 4), np.float32)
    rng = np.random.default_rng(77 + capacity)
    R = rng.integers(0, 3, size=(B, capacity)).astype(np.float32)   # 0, 1 or 2: S <= 4
    P[1, :1] = cube(1, 11, 5)
    P[2, :2] = [[30, -20, 7, 1], [-30, 10, 3, 1]]
    P[3, :counts[3]] = cube(counts[3], 13, 5)
    P[3, 5, 1] = np.nan
    P[3, 9, 0] = np.inf
    P[3, 20, :3] = P[3, 2, :3]                                       # coincident, zero radii: a contact in radii mode
    R[3, 20] = R[3, 2] = 0
    P[4, :capacity] = cube(capacity, 14 + capacity, side)
    m = marks(capacity)
    P[4, m["a"], :3], P[4, m["b"], :3], P[4, m["c"], :3] = [100, 100, 100], [103, 100, 100], [100, 103, 101]
    R[4, m["a"]], R[4, m["b"]], R[4, m["c"]] = 1, 2, 2               # S(a, b) = S(a, c) = 3, S(b, c) = 4 < sqrt(19)
    P[4, m["same"][1], :3] = P[4, m["same"][0], :3]
    P[4, m["wave"][0], :3], P[4, m["wave"][1], :3] = [-100, -100, 100], [-100, -100, 101]   # the same two rows but at 320
    P[4, m["last"][0], :3], P[4, m["last"][1], :3] = [-100, -100, -100], [-100, -100, -99]
    R[4, m["last"][0]] = R[4, m["last"][1]] = R[4, m["wave"][0]] = R[4, m["wave"][1]] = 1
    P[4, 0, :3] = [LIMIT, -LIMIT, LIMIT]                             # the limit of the grid: alone
    for a in (P, R):
        a.flags.writeable = False
    return P, counts, R


@functools.lru_cache(maxsize=None)
def gpu_subset(capacity):
    """(5, capacity) bool: about two thirds of the slots, the hand-placed bodies among them.  Bytes beyond a system's count are
    set too, and change nothing."""
    keep = np.random.default_rng(2000 + capacity).random((B, capacity)) < 0.67
    m = marks(capacity)
    for slot in (m["a"], m["b"], m["c"], *m["same"], *m["last"], *m["wave"]):
        keep[4, slot] = True
    keep[3, [2, 20, 5, 9]] = True
    keep.flags.writeable = False
    return keep


@functools.lru_cache(maxsize=None)
def gpu_reference(capacity, mode, with_subset):
    """The references of gpu_inputs(capacity), one per system."""
    P, counts, R = gpu_inputs(capacity)
    subset = gpu_subset(capacity) if with_subset else None
    return [reference(P[s], counts[s], capacity, radius=RADIUS[s] if mode == "radius" else None,
                      radii=R[s] if mode == "radii" else None, subset=None if subset is None else subset[s]) for s in range(B)]


def gpu_arguments(capacity, mode, with_subset):
    """The keyword arguments of BatchedSystem.contacts for one case."""
    kw = {"radius": np.array(RADIUS, np.float32)} if mode == "radius" else {"radii": gpu_inputs(capacity)[2]}
    if with_subset:
        kw["subset"] = gpu_subset(capacity)
    return kw


def truncating_capacity(refs):
    """A list capacity that cuts the fullest system in the middle of a row: inside the entries of a row with upper >= 2, or
    failing that one short of all."""
    full = max(refs, key=lambda r: r["system"]["pairs"])
    rows = np.nonzero(full["bodies"]["upper"] >= 2)[0]
    if len(rows):
        row = rows[len(rows) // 2]
        return int(full["bodies"]["first"][row]) + 1
    return full["system"]["pairs"] - 1
