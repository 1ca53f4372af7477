"""Shared inputs of the one-sided split tests (test_one_sided_splits_cpu.py, test_one_sided_splits_gpu.py): plain numpy.

One body set, nine split lengths, three mass patterns, one softening array.  The one-sided force kernels change their code
path with the split length (nbody_launch_choice.h, force_choice): the one-wave kernel stages 64 QT columns, and

    64, 128, 192     shorter than the 256-column tile it stages (QT = 4): the staged tile holds padding beyond the split
    256              the tile, no padding
    320, 448, 512    staged whole (QT = 5, 7, 8)
    576, 1024        double-buffered (QT = 0), the equal-mass flags come from the launch in front

2085 bodies make every last split ragged with an odd length and leave the last 256-row block (one wave of the one-wave kernel)
and the last 1024-row block (one workgroup of the four-wave kernels) partial.  The arrays handed out are read-only: every test
sees the same inputs, and the references are computed from them once (reference(), pps_reference())."""
import functools

import numpy as np

from n_body_problem_amd.initial_conditions import plummer

N = 2085
SEED = 2085
SPLIT_LENGTHS = (64, 128, 192, 256, 320, 448, 512, 576, 1024)
RAGGED_LAST = dict(zip(SPLIT_LENGTHS, (37, 37, 165, 37, 165, 293, 37, 357, 37)))   # columns of the last split
PATTERNS = ("equal", "species", "random")
SPECIES_CUTS = (768, 1536)          # rows 768 .. 1535 three times as heavy, rows 1536 .. a quarter
SPECIES_FACTORS = (3.0, 0.25)
ON_GRID = {768: (64, 128, 192, 256), 1536: (64, 128, 192, 256, 512)}   # the split lengths whose grid each cut lies on
TOL = 1e-5                          # relative L2 error of accelerations against the fp64 truth (tests/test_parity_gpu.py)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def bodies(pattern):
    """(pos, vel) of the pattern, float32 (N, 4), read-only.  vel is zero in x, y, z (one step of dt = 1 then leaves the
    accelerations in the velocities) and carries a value in w that no kernel may touch."""
    pos, vel = plummer(N, seed=SEED)
    m = pos[:, 3].view(np.uint32)
    assert np.all(m == m[0]), "plummer() is expected to give every body the same mass bits"
    if pattern == "species":
        (c0, c1), (f0, f1) = SPECIES_CUTS, SPECIES_FACTORS
        pos[c0:c1, 3] *= np.float32(f0)
        pos[c1:, 3] *= np.float32(f1)
    elif pattern == "random":
        pos[:, 3] = (np.random.default_rng(7).uniform(0.5, 2.0, N) / N).astype(np.float32)
    elif pattern != "equal":
        raise ValueError(pattern)
    vel[:, :3] = 0.0
    vel[:, 3] = (0.25 + np.arange(N) % 17).astype(np.float32)
    return _frozen(pos), _frozen(vel)


@functools.lru_cache(maxsize=None)
def particle_softening():
    """Per-particle softening lengths, float32 (N,), read-only: uniform in [0, 0.03), every seventh exactly 0."""
    e = np.random.default_rng(3).uniform(0.0, 0.03, N).astype(np.float32)
    e[::7] = 0.0
    return _frozen(e)


def last_split_len(split_len, n=N):
    return n - (n - 1) // split_len * split_len


def uniform_splits(pos, split_len):
    """Per split, whether it qualifies for the equal-mass loop as split_mass_kernel defines it: all split_len columns carry the
    same mass bits, a column at or beyond the body count counting as mass 0 (so a ragged last split never qualifies unless
    every mass is +0)."""
    n = pos.shape[0]
    count = -(-n // split_len)
    m = np.zeros(count * split_len, np.uint32)
    m[:n] = np.ascontiguousarray(pos[:, 3]).view(np.uint32)
    m = m.reshape(count, split_len)
    return np.all(m == m[:, :1], axis=1)


def min_pair_distance(pos):
    x = pos[:, :3].astype(np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d2[np.diag_indices_from(d2)] = np.inf
    return float(np.sqrt(d2.min()))


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


_REFERENCE = {}


def reference(oracle_mod, pattern, eps):
    """The fp64 truth, the oracle's reference-order fp32 accelerations and the latter's relative L2 error: once per
    (pattern, eps), read-only."""
    key = (pattern, float(eps))
    if key not in _REFERENCE:
        pos, _ = bodies(pattern)
        a64 = oracle_mod.accel_f64(pos, eps=eps)
        a32 = oracle_mod.accel_f32(pos, eps=eps)
        _REFERENCE[key] = dict(a64=_frozen(a64), a32=_frozen(a32), e_ref=rel_l2(a32, a64))
    return _REFERENCE[key]


_PPS_REFERENCE = {}


def pps_reference(oracle_mod, pattern, eps):
    """The fp64 truth under per-particle softening (eps_ij^2 = eps^2 + eps_i^2 + eps_j^2): once per (pattern, eps)."""
    key = (pattern, float(eps))
    if key not in _PPS_REFERENCE:
        _PPS_REFERENCE[key] = _frozen(oracle_mod.accel_f64_pps(bodies(pattern)[0], particle_softening(), eps))
    return _PPS_REFERENCE[key]
