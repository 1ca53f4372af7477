"""The fp64 numpy reference of nbody_batch_gravity (include/nbody_batch_gravity.h): the acceleration, the potential and the tidal
tensor that the sources j < m of one system exert at its own bodies (each skipping itself) or at given points, with
zero-distance sources dropped at eps = 0.  Beside every output it returns the sum of the absolute values of its terms, the scale
the bands of the GPU and CPU suites are taken of.  The inputs are hermite_members_ref's (boosted Plummer spheres with ragged
counts), by import; the massive counts and the point sets of the GPU suite are made here.

The reference takes the state and the points as float32 and does everything else in float64, the true 1 / sqrt included.

What a term is.  For the potential and the acceleration a term is one source's contribution, m_j / r and m_j d_a / r^3.  For the
tidal tensor the header sums p_a d_b = 3 m_j d_a d_b / r^5 per source in one chain and, for the diagonal, m_j / r^3 in a chain
of its own that is subtracted at the end: both are terms, so a diagonal component's scale is sum 3 m_j d_a^2 / r^5 + sum m_j / r^3
(r^2 including eps^2 throughout)."""
import functools

import numpy as np

from hermite_members_ref import CAPACITIES, FILL, GUARD_MIN, TERM_BAND, gpu_inputs  # noqa: F401

#: the rounding of an fp32 chain of m FMAs, per source, relative to the sum of the absolute values of its terms
CHAIN_ULP = 2.0 ** -24
SOFTENINGS = (0.0, 1e-2)


def band(m):
    """The relative band of an fp32-chained output with m sources: m 2^-24 for the chain, TERM_BAND for the term itself."""
    return m * CHAIN_ULP + TERM_BAND


def gravity(pos, n, m=None, points=None, softening=0.0):
    """The reference of one system.  pos: (>= n, 4) float32; m: the number of sources (None: n); points: (R, >= 3) float32, or
    None for the system's own bodies i < n (R = n, source j == i skipped).  A dict of acceleration (R, 3), potential (R,),
    tidal (R, 3, 3) and their scales acceleration_scale, potential_scale, tidal_scale, and sources (= m)."""
    p32 = np.asarray(pos, dtype=np.float32)
    m = n if m is None else max(0, min(int(m), n))
    own = points is None
    x = (p32[:n, :3] if own else np.asarray(points, dtype=np.float32)[:, :3]).astype(np.float64)
    src, mass = p32[:m, :3].astype(np.float64), p32[:m, 3].astype(np.float64)
    eps2 = float(np.float32(softening)) ** 2
    R = x.shape[0]
    out = dict(acceleration=np.zeros((R, 3)), acceleration_scale=np.zeros((R, 3)), potential=np.zeros(R), potential_scale=np.zeros(R),
               tidal=np.zeros((R, 3, 3)), tidal_scale=np.zeros((R, 3, 3)), sources=m)
    if R == 0 or m == 0:
        return out
    eye = np.eye(3)
    for lo in range(0, R, 256):
        hi = min(lo + 256, R)
        d = src[None, :, :] - x[lo:hi, None, :]                     # (r, m, 3)
        r2 = (d * d).sum(-1) + eps2
        with np.errstate(divide="ignore"):
            inv = 1.0 / np.sqrt(r2)
        if eps2 == 0.0:
            inv = np.where(r2 < GUARD_MIN, 0.0, inv)
        if own:
            rows = np.arange(lo, min(hi, m))
            inv[rows - lo, rows] = 0.0                              # j != i
        w1 = mass[None, :] * inv
        w3 = w1 * inv * inv
        w5 = 3.0 * w3 * inv * inv
        with np.errstate(invalid="ignore"):
            dd = np.where(inv[..., None] > 0.0, d, 0.0)             # a dropped source adds nothing, whatever its d
        out["potential"][lo:hi] = -w1.sum(1)
        out["potential_scale"][lo:hi] = w1.sum(1)
        out["acceleration"][lo:hi] = (dd * w3[..., None]).sum(1)
        out["acceleration_scale"][lo:hi] = (np.abs(dd) * w3[..., None]).sum(1)
        tr = w3.sum(1)
        out["tidal"][lo:hi] = np.einsum("rma,rmb,rm->rab", dd, dd, w5) - tr[:, None, None] * eye
        out["tidal_scale"][lo:hi] = np.einsum("rma,rmb,rm->rab", np.abs(dd), np.abs(dd), w5) + tr[:, None, None] * eye
    return out


def deviations(got_a, got_phi, got_t, ref):
    """The largest deviation of each output from the reference, in units of the sum of the absolute values of its terms (an
    output whose scale is 0 must be 0: its deviation is its absolute value)."""
    def rel(got, want, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.max(np.where(scale > 0, np.abs(got - want) / scale, np.abs(got)), initial=0.0))
    out = dict(acceleration=rel(np.asarray(got_a, np.float64), ref["acceleration"], ref["acceleration_scale"]),
               potential=rel(np.asarray(got_phi, np.float64), ref["potential"], ref["potential_scale"]))
    if got_t is not None:
        out["tidal"] = rel(np.asarray(got_t, np.float64), ref["tidal"], ref["tidal_scale"])
    return out


# ---- the inputs ---------------------------------------------------------------------------------------------------------------
def massive_of(capacity):
    """Ragged massive counts for the systems of gpu_inputs(capacity): 0 among them, and one above its system's count."""
    return [1000, 400] if capacity == 4096 else [0, 5, 1, 0, capacity // 2, 7]


@functools.lru_cache(maxsize=None)
def reference(capacity, softening, massive=False):
    """The own-bodies references of the systems of gpu_inputs(capacity), computed once and shared."""
    P, _, counts = gpu_inputs(capacity)
    ms = massive_of(capacity) if massive else [None] * len(counts)
    return [gravity(P[s], n, m=ms[s], softening=softening) for s, n in enumerate(counts)]


TRACER_SOURCES, TRACER_BODIES = 40, 105     # the invariance system: 40 massive bodies, 65 test particles


@functools.lru_cache(maxsize=None)
def tracer_inputs():
    """(pos, other): a 105-body system whose first 40 bodies are the sources and whose other 65 are test particles (mass words
    that nothing may read), and a neighbour of the same size."""
    from n_body_problem_amd import plummer
    pos = np.array(plummer(TRACER_BODIES, seed=311)[0], dtype=np.float32)
    other = np.array(plummer(TRACER_BODIES, seed=312)[0], dtype=np.float32)
    pos[TRACER_SOURCES:, 3] = 7.0
    pos.setflags(write=False)
    other.setflags(write=False)
    return pos, other
