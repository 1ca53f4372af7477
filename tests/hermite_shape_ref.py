"""The reference of the shapes of batched ensembles (include/nbody_batch_shape.h), operation by operation in IEEE doubles whose
+, -, *, / and sqrt are correctly rounded: Python floats for everything a pass does once (the level-2 sums, the Jacobi
iteration, the sort, the signs, the update) and numpy's element-wise float64 operations -- the same roundings, one body per
element -- for what a pass does per body.  There is no numpy sum and no dot product anywhere, because the order of the additions
is what the header pins: level 1 adds the 64 bodies of a block in ascending index (a non-member adds +0.0, which the header
states is the same bits as skipping it), level 2 the blocks in ascending order.  Every case also reports its *margin*: the
smallest |r2e - out2| / out2, and the same against in2 where in2 > 0, over all measured bodies taking part, all passes (the
final walk included) and all apertures -- how far the nearest body was from changing sides.  With `jitter`, a numpy Generator,
every quotient and every root is moved by up to one ulp at random: what IEEE would still permit of a device whose division and
square root were not correctly rounded.  Also the inputs that tests/test_batch_shape_cpu.py and tests/test_batch_shape_gpu.py
share: rotated triaxial Gaussians."""
import functools
import math

import numpy as np

APERTURE_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("count", np.int64), ("radius", np.float64),
                           ("inner", np.float64), ("q", np.float64), ("s", np.float64), ("change", np.float64),
                           ("eigenvalues", np.float64, 3), ("axes", np.float64, 9), ("weight", np.float64), ("D", np.float64, 3),
                           ("M", np.float64, 6), ("L", np.float64, 3)])
SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("unmeasured", np.int32), ("apertures", np.int32), ("reduced", np.int32),
                         ("converged", np.int32), ("reserved", np.int32), ("total_weight", np.float64), ("centre", np.float64, 3),
                         ("velocity", np.float64, 3)])
BODY_DTYPE = np.dtype([("inside", np.uint32), ("reserved", np.int32)])
MAX_APERTURES, MAX_ITERATIONS, BLOCK, SWEEPS = 8, 64, 64, 16
CONVERGED, MAX, FEW, DEGENERATE = 0, 1, 2, 3
LARGEST = float(np.finfo(np.float64).max)
INF = float("inf")
#: the words of an aperture that +, - and x alone make given the members, and those that pass through / and sqrt
EXACT_WORDS = ("weight", "D", "M", "L")
ROOTED_WORDS = ("q", "s", "change", "eigenvalues", "axes")
INTEGER_WORDS = ("status", "iterations", "count")
#: (T, RPL) of the workgroups the CPU driver is run at: batch_shape's for these capacities
CAPACITIES = (64, 128, 256, 1024, 4096)
SHAPES = ((64, 1), (64, 2), (64, 4), (256, 4), (512, 8))


def shape_of(capacity):
    """batch_shape (csrc/nbody_batch_choice.h) kept at eight waves (shape_threads, shape_rows): (T, rows per lane)."""
    if capacity <= 64:
        return 64, 1
    if capacity <= 128:
        return 64, 2
    T = min((capacity + 255) // 256 * 64, 512)
    return T, 4 * ((capacity + 4 * T - 1) // (4 * T))


def square(r):
    """One product; an overflow becomes the largest finite double."""
    r2 = float(r) * float(r)
    return r2 if r2 <= LARGEST else LARGEST


class Ops:
    """Division and square root: correctly rounded, or with `jitter` moved by up to one ulp at random."""

    def __init__(self, jitter=None):
        self.jitter = jitter

    def _move(self, v):
        if self.jitter is None:
            return v
        if isinstance(v, np.ndarray):
            k = np.where(np.isfinite(v), self.jitter.integers(-1, 2, size=v.shape), 0)   # an infinity or a NaN stays
            return np.where(k > 0, np.nextafter(v, np.inf), np.where(k < 0, np.nextafter(v, -np.inf), v))
        k = int(self.jitter.integers(-1, 2))
        return v if k == 0 or not math.isfinite(v) else math.nextafter(v, INF if k > 0 else -INF)

    def div(self, a, b):
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            with np.errstate(all="ignore"):
                return self._move(a / b)
        if b == 0.0:                                       # IEEE's infinity or NaN, where Python would raise
            return np_div(a, b)
        return self._move(a / b)

    def sqrt(self, a):
        if a != a or a < 0.0:
            return float("nan")
        return self._move(math.sqrt(a)) if a < INF else INF


def np_div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def rotate(a, v, ip, iq, ops):
    """One Jacobi rotation of the pair (ip, iq): a = (a_pp, a_qq, a_pq, a_rp, a_rq), v the eigenvector matrix by rows; see the
    header.  Returns the five words after it."""
    app, aqq, apq, arp, arq = a
    if apq == 0.0:
        return a
    g = 100.0 * abs(apq)
    if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
        return app, aqq, 0.0, arp, arq
    theta = ops.div(aqq - app, 2.0 * apq)
    root = ops.sqrt(theta * theta + 1.0)
    t = ops.div(-1.0, root - theta) if theta < 0.0 else ops.div(1.0, theta + root)
    c = ops.div(1.0, ops.sqrt(t * t + 1.0))
    s = t * c
    h = t * apq
    for k in range(3):
        vp, vq = v[3 * k + ip], v[3 * k + iq]
        v[3 * k + ip] = c * vp - s * vq
        v[3 * k + iq] = s * vp + c * vq
    return app - h, aqq + h, 0.0, c * arp - s * arq, s * arp + c * arq


def jacobi(T, ops=Ops()):
    """lambda[3] sorted descending and e[9] = e1, e2, e3 as rows, of T = xx, yy, zz, xy, xz, yz."""
    d0, d1, d2, o01, o02, o12 = (float(t) for t in T)
    v = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(SWEEPS):
        if o01 == 0.0 and o02 == 0.0 and o12 == 0.0:
            break
        d0, d1, o01, o02, o12 = rotate((d0, d1, o01, o02, o12), v, 0, 1, ops)
        d0, d2, o02, o01, o12 = rotate((d0, d2, o02, o01, o12), v, 0, 2, ops)
        d1, d2, o12, o01, o02 = rotate((d1, d2, o12, o01, o02), v, 1, 2, ops)
    d = (d0, d1, d2)
    at = [sum(1 for o in range(3) if d[o] > d[c] or (d[o] == d[c] and o < c)) for c in range(3)]
    if len(set(at)) != 3:
        at = [0, 1, 2]
    lam, e = [0.0] * 3, [0.0] * 9
    for c in range(3):
        lam[at[c]] = d[c]
        if at[c] < 2:
            for k in range(3):
                e[3 * at[c] + k] = v[3 * k + c]
    for r in range(2):
        row = e[3 * r:3 * r + 3]
        big = 0
        if abs(row[1]) > abs(row[big]):
            big = 1
        if abs(row[2]) > abs(row[big]):
            big = 2
        if row[big] < 0.0:
            e[3 * r:3 * r + 3] = [-x for x in row]
    a, b = e[0:3], e[3:6]
    e[6] = a[1] * b[2] - a[2] * b[1]
    e[7] = a[2] * b[0] - a[0] * b[2]
    e[8] = a[0] * b[1] - a[1] * b[0]
    return lam, e


def two_level(addends):
    """addends: (n, words) float64, one row per body, +0.0 rows for non-members.  Level 1 per block of 64 in ascending index
    from +0.0, level 2 over the blocks in ascending order from +0.0, in Python floats."""
    n, words = addends.shape
    blocks = (n + BLOCK - 1) // BLOCK
    padded = np.zeros((blocks * BLOCK, words))
    padded[:n] = addends
    padded = padded.reshape(blocks, BLOCK, words)
    partial = np.zeros((blocks, words))
    with np.errstate(all="ignore"):
        for j in range(BLOCK):
            partial = partial + padded[:, j, :]
    total = [0.0] * words
    for k in range(blocks):
        for c in range(words):
            total[c] = total[c] + float(partial[k, c])
    return total


PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))  # xx, yy, zz, xy, xz, yz


class Margin:
    def __init__(self):
        self.value = INF

    def see(self, r2e, eligible, in2, out2):
        r = r2e[eligible]
        r = r[np.isfinite(r)]
        if len(r):
            self.value = min(self.value, float(np.min(np.abs(r - out2)) / out2))
            if in2 > 0.0:
                self.value = min(self.value, float(np.min(np.abs(r - in2)) / in2))


def r2e_of(state, d):
    e, w2, w3 = state
    with np.errstate(all="ignore"):
        a = (e[0] * d[0] + e[1] * d[1]) + e[2] * d[2]
        b = (e[3] * d[0] + e[4] * d[1]) + e[5] * d[2]
        c = (e[6] * d[0] + e[7] * d[1]) + e[8] * d[2]
        return (a * a + w2 * (b * b)) + w3 * (c * c)


def shape(pos, vel, count, radii, inner=None, centre=(0.0, 0.0, 0.0), velocity=(0.0, 0.0, 0.0), weight="mass", reduced=True,
          tol=1e-3, max_iterations=64, min_members=10, subset=None, jitter=None, start=None):
    """One system: pos and vel are (slots, 4) float32, count its bodies.  Returns the system record, the aperture records,
    the body records (slots of them), the margin and, per aperture, the tensors T of every pass (for independent checks).
    `start` replaces the identity as the first state's axes (a test's device for rotating the state)."""
    ops = Ops(jitter)
    slots = pos.shape[0]
    n = min(int(count), slots)
    A = len(radii)
    system = np.zeros((), dtype=SYSTEM_DTYPE)
    rec = np.zeros(A, dtype=APERTURE_DTYPE)
    body = np.zeros(slots, dtype=BODY_DTYPE)
    takes = np.ones(n, dtype=bool) if subset is None else np.asarray(subset[:n]) != 0
    p64, v64 = pos[:n, :3].astype(np.float64), vel[:n, :3].astype(np.float64)
    measured = np.isfinite(pos[:n, :3]).all(axis=1) & np.isfinite(vel[:n, :3]).all(axis=1)
    eligible = takes & measured
    with np.errstate(all="ignore"):
        d = [p64[:, k] - float(centre[k]) for k in range(3)]
        u = [v64[:, k] - float(velocity[k]) for k in range(3)]
        w = np.ones(n) if weight == "number" else pos[:n, 3].astype(np.float64)
        dd = [w * (d[p] * d[q]) for p, q in PAIRS]
    margin = Margin()
    tensors = []
    converged = 0
    for a in range(A):
        R, Rin = float(radii[a]), 0.0 if inner is None else float(inner[a])
        out2, in2 = square(R), square(Rin)
        state = ([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] if start is None else [float(x) for x in start], 1.0, 1.0)
        q_prev = s_prev = 1.0
        change, lam, status, iterations = 0.0, [0.0] * 3, MAX, 0
        passes = []
        while True:
            r2e = r2e_of(state, d)
            margin.see(r2e, eligible, in2, out2)
            with np.errstate(all="ignore"):
                member = eligible & (in2 < r2e) & (r2e <= out2)
                terms = [ops.div(t, r2e) if reduced else t for t in dd]
            add = np.zeros((n, 7))
            for c in range(6):
                add[:, c] = np.where(member, terms[c], 0.0)
            add[:, 6] = np.where(member, w, 0.0)
            total = two_level(add) if n else [0.0] * 7
            members = int(member.sum())
            iterations += 1
            if members < min_members:
                status = FEW
                break
            lam_new, e_new = jacobi(total[:6], ops)
            passes.append((list(total[:6]), lam_new, e_new))
            lam = lam_new
            l1, l2, l3 = lam
            w2, w3 = np_div(l1, l2), np_div(l1, l3)
            if jitter is not None:
                w2, w3 = ops._move(w2), ops._move(w3)
            if l3 <= 0.0 or not abs(w3) <= LARGEST or not abs(w2) <= LARGEST or not total[6] > 0.0:
                status = DEGENERATE
                break
            q, s = ops.sqrt(ops.div(l2, l1)), ops.sqrt(ops.div(l3, l1))
            dq, ds = abs(q - q_prev), abs(s - s_prev)
            done = dq <= tol * q_prev and ds <= tol * s_prev
            cq, cs = ops.div(dq, q_prev), ops.div(ds, s_prev)
            change = cs if cs > cq else cq
            state = (e_new, w2, w3)
            q_prev, s_prev = q, s
            if done:
                status = CONVERGED
                break
            if iterations >= max_iterations:
                status = MAX
                break
        tensors.append(passes)
        r2e = r2e_of(state, d)
        margin.see(r2e, eligible, in2, out2)
        with np.errstate(all="ignore"):
            member = eligible & (in2 < r2e) & (r2e <= out2)
            cross = (d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0])
            columns = [w, w * d[0], w * d[1], w * d[2], *dd, w * cross[0], w * cross[1], w * cross[2]]
        add = np.zeros((n, 13))
        for c in range(13):
            add[:, c] = np.where(member, columns[c], 0.0)
        total = two_level(add) if n else [0.0] * 13
        body["inside"][:n] |= np.where(member, np.uint32(1 << a), np.uint32(0)).astype(np.uint32)
        r = rec[a]
        r["status"], r["iterations"], r["count"], r["radius"], r["inner"] = status, iterations, int(member.sum()), R, Rin
        r["q"], r["s"], r["change"], r["eigenvalues"], r["axes"] = q_prev, s_prev, change, lam, state[0]
        r["weight"], r["D"], r["M"], r["L"] = total[0], total[1:4], total[4:10], total[10:13]
        converged += status == CONVERGED
    system["selected"], system["unmeasured"] = int(takes.sum()), int((takes & ~measured).sum())
    system["apertures"], system["reduced"], system["converged"] = A, 1 if reduced else 0, converged
    system["total_weight"] = two_level(np.where(eligible, w, 0.0).reshape(n, 1))[0] if n else 0.0
    system["centre"], system["velocity"] = [float(c) for c in centre], [float(c) for c in velocity]
    return system, rec, body, margin.value, tensors


def shape_batch(pos, vel, counts, radii, inner=None, centre=None, velocity=None, subset=None, jitter=None, **kw):
    """Every system of a batch: radii and inner (apertures,) or (B, apertures), centre and velocity (B, 3) or None.  Returns
    systems (B,), apertures (B, apertures), bodies (B, slots) and the batch's margin."""
    B = pos.shape[0]
    radii = np.asarray(radii, dtype=np.float64)
    inner = None if inner is None else np.asarray(inner, dtype=np.float64)
    out = []
    for s in range(B):
        out.append(shape(pos[s], vel[s], counts[s], radii[s] if radii.ndim == 2 else radii,
                         None if inner is None else (inner[s] if inner.ndim == 2 else inner),
                         (0.0, 0.0, 0.0) if centre is None else centre[s], (0.0, 0.0, 0.0) if velocity is None else velocity[s],
                         subset=None if subset is None else subset[s], jitter=jitter, **kw))
    return (*(np.stack([o[k] for o in out]) for k in range(3)), min(o[3] for o in out))


def rooted_error(got, ref):
    """The largest difference of the words that pass through / and sqrt between two sets of aperture records: q, s, change
    and the components of the axes absolutely (all are at most 1 in magnitude), the eigenvalues relative to the largest."""
    worst = 0.0
    for word in ("q", "s", "change", "axes"):
        worst = max(worst, float(np.max(np.abs(got[word] - ref[word]), initial=0.0)))
    scale = np.abs(ref["eigenvalues"][..., :1])
    diff = np.abs(got["eigenvalues"] - ref["eigenvalues"])
    worst = max(worst, float(np.max(np.where(scale > 0.0, diff / np.where(scale > 0.0, scale, 1.0), diff), initial=0.0)))
    return worst


def jitter_spread(capacities=CAPACITIES, seed=99):
    """The largest rooted_error between the reference and the reference run again with every quotient and root moved by up to
    one ulp at random, over all cases of `capacities`; also whether every integer and every word of +, - and x alone stayed."""
    rng = np.random.default_rng(seed)
    worst, same = 0.0, True
    for capacity in capacities:
        for case in CASES:
            pos, vel, counts, kw, (systems, apertures, bodies, _) = reference(capacity, case[0])
            s2, a2, b2, _ = shape_batch(pos, vel, counts, jitter=rng, **kw)
            worst = max(worst, rooted_error(a2, apertures))
            same = same and b2.tobytes() == bodies.tobytes() and s2.tobytes() == systems.tobytes()
            same = same and all(a2[w].tobytes() == apertures[w].tobytes() for w in INTEGER_WORDS + EXACT_WORDS)
    return worst, same


#: jitter_spread() over all capacities, as test_batch_shape_cpu.py measures it again, and the bound of the GPU test: four times
#: that -- one ulp per quotient and root is what IEEE permits, four allows for accumulation over 64 passes.
#: Measured: 5.63e-12 with the seed above (3.0e-12 to 4.2e-12 with three others), in the cases that never converge and carry
#: the moved roundings through all 64 passes; rounded up.  No integer and no word of +, - and x alone moved.
SPREAD = 5.7e-12
BOUND = 4.0 * SPREAD  # 2.28e-11
#: a case is compared on the GPU only if the nearest body stayed this far, relatively, from changing sides in every pass
LEAST_MARGIN = 1.0e-9

# ---- the shared inputs ---------------------------------------------------------------------------------------------------------
COUNTS =(0, 1, 3, 9, 63, 64, 65, 129, 257, 1025, 4096)
SIGMAS = (1.0, 0.7, 0.4)
CENTRE = (0.015625, -0.03125, 0.0625)
VELOCITY = (0.125, 0.0, -0.25)


def rotation(rng):
    """A proper rotation, uniformly random: the Q of a Gaussian matrix with its signs fixed."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0.0:
        q[:, 0] = -q[:, 0]
    return q


def gaussian_system(slots, count, seed, sigmas=SIGMAS, rot=None, nan_body=None):
    """(slots, 4) float32 positions with masses in 0.5 ... 1.5 and velocities: `count` bodies of a triaxial Gaussian with the
    dispersions `sigmas` along the rows of `rot` (a random rotation without it), turning about the minor axis, about CENTRE in
    the frame VELOCITY.  The slots from the count on hold values no result may depend on."""
    rng = np.random.default_rng(seed)
    rot = rotation(rng) if rot is None else np.asarray(rot)
    pos = np.zeros((slots, 4), dtype=np.float32)
    vel = np.zeros((slots, 4), dtype=np.float32)
    own = rng.normal(size=(slots, 3)) * np.asarray(sigmas)
    spin = np.cross(np.array([0.0, 0.0, 0.3]), own) + 0.1 * rng.normal(size=(slots, 3))
    pos[:, :3] = own @ rot + np.asarray(CENTRE)
    vel[:, :3] = spin @ rot + np.asarray(VELOCITY)
    pos[:, 3] = rng.uniform(0.5, 1.5, size=slots)
    if nan_body is not None and count > nan_body:
        pos[nan_body, 1] = np.nan
    pos[count:, :3] = 1.0e30  # beyond the count: never read
    vel[count:, :3] = -7.0
    return pos, vel


def batch_counts(capacity):
    return sorted({min(c, capacity) for c in COUNTS})


def gaussian_batch(capacity, seed=3):
    counts = batch_counts(capacity)
    systems = [gaussian_system(capacity, c, seed + 17 * k, nan_body=5 if c == capacity else None) for k, c in enumerate(counts)]
    return np.stack([s[0] for s in systems]), np.stack([s[1] for s in systems]), np.array(counts, dtype=np.int32)


#: what is run at every capacity: (name, radii, inner, per-system, reduced, weight, mask)
CASES = (("1-reduced-mass", (2.0,), None, False, True, "mass", "none"),
         ("3-shell-unreduced-number-sparse", (1.5, 2.5, 3.0), (0.0, 1.0, 0.0), False, False, "number", "sparse"),
         ("8-shell-reduced-mass-own", (1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0, 4.0), (0.0, 0.0, 0.75, 0.0, 0.0, 0.0, 0.0, 0.0), True, True,
          "mass", "none"))


def masks(capacity, B, kind, seed=5):
    if kind == "none":
        return None
    rng = np.random.default_rng(seed)
    return (rng.random((B, capacity)) < 0.7).astype(np.uint8)


def case_inputs(capacity, case):
    """pos, vel, counts and the keyword arguments of one case."""
    _, radii, inner, own, reduced, weight, mask = case
    pos, vel, counts = gaussian_batch(capacity)
    B = len(counts)
    radii = np.asarray(radii, dtype=np.float64)
    inner = None if inner is None else np.asarray(inner, dtype=np.float64)
    if own:
        scale = 1.0 + 0.03125 * np.arange(B)[:, None]
        radii, inner = radii[None, :] * scale, inner[None, :] * scale
    centre = np.tile(np.array(CENTRE, dtype=np.float64), (B, 1))
    velocity = np.tile(np.array(VELOCITY, dtype=np.float64), (B, 1))
    return pos, vel, counts, dict(radii=radii, inner=inner, centre=centre, velocity=velocity, weight=weight, reduced=reduced,
                                  subset=masks(capacity, B, mask))


@functools.lru_cache(maxsize=None)
def reference(capacity, name):
    """The inputs and the reference's records of one case at one capacity, computed once and shared: pos, vel, counts, the
    keyword arguments, and shape_batch's (systems, apertures, bodies, margin).  Nobody changes them."""
    case = next(c for c in CASES if c[0] == name)
    pos, vel, counts, kw = case_inputs(capacity, case)
    out = shape_batch(pos, vel, counts, **kw)
    for a in (pos, vel, counts, *out[:3]):
        a.setflags(write=False)
    return pos, vel, counts, kw, out
