"""The inputs and references of the one-sided split tests (one_sided_split_cases.py), checked without a GPU: the builder's own
claims -- equal mass bits, odd ragged last splits, which species boundary lies on which split grid, no coincident bodies -- and
the room the references leave inside the tolerance the GPU tests assert."""
import numpy as np
import pytest

import one_sided_split_cases as cases
from one_sided_split_cases import N, SPLIT_LENGTHS, TOL


def test_body_count_leaves_every_last_split_ragged_and_odd():
    assert SPLIT_LENGTHS == (64, 128, 192, 256, 320, 448, 512, 576, 1024)
    assert [cases.last_split_len(L) for L in SPLIT_LENGTHS] == [37, 37, 165, 37, 165, 293, 37, 357, 37]
    for L in SPLIT_LENGTHS:
        assert L % 64 == 0 and cases.RAGGED_LAST[L] == cases.last_split_len(L) == N % L
        assert cases.last_split_len(L) % 2 == 1 and cases.last_split_len(L) % 4 != 0       # a partial four-column iteration
    assert N % 256 != 0 and N % 1024 != 0      # the last 256-row block and the last 1024-row block are partial


def test_mass_patterns_are_what_the_builder_says():
    pos, vel = cases.bodies("equal")
    assert pos.shape == vel.shape == (N, 4) and pos.dtype == vel.dtype == np.float32
    m = pos[:, 3].view(np.uint32)
    assert np.all(m == m[0]) and pos[0, 3] == np.float32(1.0 / N)                # identical bits
    assert np.all(vel[:, :3] == 0) and np.all(vel[:, 3] > 0)
    species = cases.bodies("species")[0]
    assert np.array_equal(species[:, :3], pos[:, :3])
    assert len(np.unique(species[:, 3])) == 3
    assert np.all(species[:768, 3] == pos[0, 3]) and np.all(species[768:1536, 3] == np.float32(3.0) * pos[0, 3])
    assert np.all(species[1536:, 3] == np.float32(0.25) * pos[0, 3])
    random = cases.bodies("random")[0]
    assert np.array_equal(random[:, :3], pos[:, :3]) and len(np.unique(random[:, 3])) > N // 2
    assert random[:, 3].min() >= np.float32(0.5 / N) and random[:, 3].max() <= np.float32(2.0 / N)
    for p in (pos, species, random):
        assert not p.flags.writeable
    e = cases.particle_softening()
    assert e.dtype == np.float32 and e.shape == (N,) and np.all(e[::7] == 0) and 0 < e[e > 0].min() and e.max() < 0.03
    assert (e == 0).sum() == -(-N // 7)


def test_species_boundaries_on_and_off_the_split_grids():
    for cut, on in cases.ON_GRID.items():
        assert tuple(L for L in SPLIT_LENGTHS if cut % L == 0) == on
    species, equal, random = (cases.bodies(p)[0] for p in ("species", "equal", "random"))
    for L in SPLIT_LENGTHS:
        count = -(-N // L)
        # equal masses: every whole split qualifies for the equal-mass loop, the ragged last one never does
        assert cases.uniform_splits(equal, L).tolist() == [True] * (count - 1) + [False]
        assert not cases.uniform_splits(random, L).any()
        u = cases.uniform_splits(species, L)
        mixed = sorted({c // L for c in cases.SPECIES_CUTS if c % L})            # the splits a boundary cuts
        assert [s for s in range(count - 1) if not u[s]] == mixed and not u[-1]
        assert u.any() == (L != 1024)                         # some splits qualify (at 1024 both whole splits hold a boundary)
        assert (not u[:-1].all()) == (L not in (64, 128, 192, 256))              # ... and some whole ones do not, off the grid


def test_no_coincident_bodies():
    d = cases.min_pair_distance(cases.bodies("equal")[0])
    print(f"smallest pair distance {d:.3e}")
    assert d > 1e-3            # measured 5.6e-3: eps = 0 is a fair case for a tolerance test


@pytest.mark.parametrize("eps", [1e-2, 0.0])
@pytest.mark.parametrize("pattern", cases.PATTERNS)
def test_reference_order_fp32_stays_well_inside_the_tolerance(oracle_mod, pattern, eps):
    """The oracle's reference-order fp32 accelerations against its fp64 truth: the GPU tests allow TOL = 1e-5 and four times this
    error + 1e-7.  Measured 4.0e-7 ... 8.2e-7 at these inputs: the reference alone stays 12 x inside TOL."""
    ref = cases.reference(oracle_mod, pattern, eps)
    print(f"{pattern} eps={eps:g}: accel_f32 against accel_f64 {ref['e_ref']:.3e}")
    assert ref["a64"].shape == ref["a32"].shape == (N, 3) and np.all(np.isfinite(ref["a64"]))
    assert 0 < ref["e_ref"] < TOL / 4
    assert cases.reference(oracle_mod, pattern, eps) is ref and not ref["a64"].flags.writeable      # computed once, unchanged


@pytest.mark.parametrize("eps", [1e-3, 0.0])
@pytest.mark.parametrize("pattern", cases.PATTERNS)
def test_per_particle_softening_truth_is_finite(oracle_mod, pattern, eps):
    a = cases.pps_reference(oracle_mod, pattern, eps)
    assert a.shape == (N, 3) and np.all(np.isfinite(a)) and np.linalg.norm(a) > 0
    assert cases.pps_reference(oracle_mod, pattern, eps) is a and not a.flags.writeable
