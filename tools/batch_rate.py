"""Batched ensembles against the status quo: B independent systems of n bodies stepped by one BatchedSystem, and the same
systems stepped one NBodySystem each (timed on a subset, scaled to B).  One JSON line per (n, B, integrator):
python tools/batch_rate.py [--cases 1024x1024 ...] [--integrators kick_drift kdk hermite] [--repeats 5] [--subset 8]

Rates use the one-sided convention: n^2 ordered interactions per system and step, against the 157.3 TFLOP/s fp32 vector
peak at 20 flop per interaction for kick_drift and kdk (a force) and 60 flop per interaction for hermite (a force and a
jerk, the convention of the Hermite GPU literature); the line names its convention.  Times are HIP events around
step_n(k) after a warm-up, the median of repeats that alternate the batched and the status-quo measurement.  Hermite
exists for batches only, so its lines have no status-quo figures.

--adaptive: instead, per case, one line with Hermite step_n(k, dt) against evolve(k, dt, levels=0) -- the same k steps of
the same arithmetic through the adaptive kernel, so the difference is the cost of the step criterion, the workgroup minimum
and the per-launch counter read -- alternated, medians; then one scattering-style line: 1024 Kepler pairs with
eccentricities spread over 0 .. 0.99 in one batch, evolved one period (dt_max = period / 64, levels = 12, eta = 0.01,
no softening): wall time, the distribution of the systems' step counts and the worst relative energy error.

--stops: instead, per case, one line with evolve(k, dt, levels=0) without stopping conditions against the same call with
conditions that cannot trigger (set_stop_conditions(1e-6, 1e6)): the same k steps, so the ratio is the cost of watching
the conditions -- alternated, medians; then the scattering case above run to completion against the same batch stopped
at collision radius 0.05 a: how many pairs stop, at what step counts, and the two wall times.

--merges: instead, per case, one line with evolve(k, dt, levels=0) under the collision action "stop" against the same call
under "merge", both with conditions that cannot trigger (the stop kernel against the merge kernel on the same k steps) --
alternated, medians; then the scattering case with collision radius 0.05 a stopped against merged and run to completion: how
many pairs merge, at what step counts, and the two wall times.

--radii: instead, per case, one line with evolve(k, dt, levels=0) under set_stop_conditions(1e-6, 1e6) (the stop kernel) against
the same call with per-body radii of 5e-7 everywhere and no collision radius (the radii kernel); neither can trigger --
alternated, medians; then the scattering case with unequal radii (0.03 a and 0.02 a, the reach of collision radius 0.05 a)
stopped against merged: how many pairs collide, at what step counts, the merged radii and the two wall times.

--fates: instead, tracer fates (set_tracer_action("remove")).  For n x B = 4096 x 256 and 1024 x 1024 (or --cases) and m in
1, 8, 64, one line per evolve(k, dt, levels=0): the call with massive counts m, the tracer action "remove" and a collision and
an escape radius that never trigger, against the same call with massive counts alone, alternated, medians and spreads, and
whether the two states are equal bit for bit.

--accrete: instead, accreting tracers (set_hit_action("accrete")).  For the same cases and m, one line per evolve(k, dt,
levels=0): massive counts m, the tracer action "remove", a collision and an escape radius that never trigger and the hit
action "accrete", against the same call on the same state with the hit action "remove" (the fate kernel) -- nothing hits, so
the difference is the sibling kernel's own -- alternated, medians and spreads, and whether the two states are equal bit for bit.
Then one line for a state where about 1 % of the tracers accrete over the run (n = 1024, B = 256, m = 8, a collision radius
found by bisection on the run that removes): both actions from the same fresh state in every repeat, the accretions and the
two times.

--massive: instead, test particles (set_massive_counts).  For n x B = 4096 x 256 and 1024 x 1024 (or --cases) and m in
1, 8, 64, 512, n, one line per Hermite step_n(k, dt) and one per evolve(k, dt, levels=0): the call with massive counts m
set against the same call with the feature off, both on the same state with the mass words of the bodies from m on zeroed
(the two compute the same bits; the second walks all n columns through the kernels that exist without the feature) --
alternated, medians, both times, their ratio and the spread (max - min over the median) of each side's repeats.

--field: instead, external fields (set_external_field).  For n x B = 4096 x 256 and 1024 x 1024 (or --cases) and m in
1, 8, 64, n, one line per evolve(k, dt, levels=0): the call with a three-component field (bulge + disc + halo) against the
same call with the field off, both with massive counts m and from the same state -- alternated, medians, both times, their
ratio and the spread of each side's repeats.  The two runs differ (the field moves the bodies); the work per step does not
depend on the state.

--pairs: instead, bound pairs (BatchedSystem.pairs).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one line per case:
pairs() against energy(0) on the same state -- both synchronous calls, wall clock, alternated, medians and spreads.  pairs()
evaluates n x n pairs with positions and velocities and returns 48 bytes per body; energy() evaluates the same pairs with
positions alone and returns three numbers per system.

--structure: instead, the cluster structure (BatchedSystem.structure).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one
line per case: structure() with the per-body records and with bodies=False against energy(0) and pairs() on the same state --
all synchronous calls, wall clock, alternated, medians and spreads.  structure() walks the n x n pairs three times (the
eight-smallest lists, the neighbours inside the k-th distance, the enclosed weights in fp64) and returns 120 bytes per system
and, with the records, 40 bytes per body.  The kernel's time alone comes from a traced run of this mode.

--members: instead, the bound members (BatchedSystem.members).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one line
per case on boosted Plummer spheres (a third of the velocities multiplied by 1.5 ... 4, so that unbinding takes several
iterations): members(0) with the per-body records, with bodies=False, and with bodies=False and one iteration, against energy(0)
and pairs() on the same state -- all synchronous calls, wall clock, alternated, medians and spreads.  An iteration is one
n x n walk of fp32 pair terms summed in fp64, energy()'s own terms: the one-iteration call is one iteration of every system,
and the difference of the two lean calls is given over the further iterations of the slowest system and of the mean.  The
kernel's time alone comes from a traced run of this mode.

--hierarchy: instead, the hierarchies (BatchedSystem.hierarchy).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one line per
case on the state of tests/hermite_hierarchy_ref.py (singles, binaries, triples, 2 + 2 and (2 + 1) + 1 objects on a jittered
lattice; 64 distinct systems, the rest copies): hierarchy(max_levels=16) with the node and body records, with neither, and with
neither at tidal_tolerance = 0.01, against pairs() on the same state -- all synchronous calls, wall clock, alternated, medians
and spreads -- and the levels evaluated.  A level is one pairs search and one shorter walk over the live roots.  The kernels'
times alone come from a traced run of this mode.

--gravity: instead, gravity at points (BatchedSystem.gravity_at).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one line
per case on the boosted Plummer spheres of --members: gravity_at() in own-bodies mode with the tidal tensor and without it,
against members(max_iterations=1, bodies=False) and energy() at the same softening on the same state; then one line for a
65536-point grid per system at n x B = 1024 x 64, with and without the tensor.  All synchronous calls, wall clock, alternated,
medians and spreads.  A call is one n x n (or points x n) walk and returns 24 bytes per row, 48 with the tensor: the copy to the
host is part of the wall time, so the kernel's time alone comes from a traced run of this mode.

--groups: instead, the friends-of-friends groups (BatchedSystem.groups).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases), one
line per case on Plummer spheres, at linking lengths of 0.2 and 1.0 mean interparticle spacings within the half-mass radius:
groups() without the per-slot and per-body records (32 bytes per system come back: the kernel, its launch and the wait for it),
with the per-body records, and with both, against pairs() on the same state -- all synchronous calls, wall clock, alternated,
medians and spreads -- and the sweeps run.  A sweep is one n x n walk of nine fp32 and integer operations per pair; the records
take two more walks with fp64 sums, the second only where the per-slot records are asked for.  The kernel's time alone comes
from a traced run of this mode.

--span: instead, the minimum spanning trees (BatchedSystem.spanning_tree).  For n x B = 1024 x 1024 and 4096 x 256 (or --cases),
one line per case on Plummer spheres: spanning_tree() without the per-slot and per-body records (40 bytes per system come back:
the kernel, its launch and the wait for it), the same with separations, the whole call with both records, and a call with
subsets of 20 random bodies per system, against groups() without its records at one mean spacing and pairs() on the same
state -- all synchronous calls, wall clock, alternated, medians and spreads -- and the rounds run.  A round is one n x n walk of
about a dozen fp32 and integer operations per pair; the separations take one more walk with an fp32 square root and an fp64
add per pair.  The kernel's time alone comes from a traced run of this mode.

--neighbours: instead, the nearest-neighbour lists (BatchedSystem.neighbours).  For n x B = 1024 x 1024 and 4096 x 256 (or
--cases), one line per case on Plummer spheres: neighbours() without the lists and the per-body records (40 bytes per system come
back: the kernel, its launch and the wait for it) at k = 1, 6 and 8, the same at k = 6 with a radius of one mean spacing and with
the first 8 bodies of every system as the only sources, and the whole call at k = 6 with the lists and the records, against
structure(k=6) without its records and pairs() on the same state -- all synchronous calls, wall clock, alternated, medians and
spreads.  The kernel always keeps eight (r2, index) pairs per row, so k changes only what is stored; a column costs a row about
6 + 2 + 8 x 5 vector operations against 6 + 8 x 2 in the first of structure()'s three walks.

--correlation: instead, the pair-separation counts (BatchedSystem.correlation).  For n x B = 1024 x 1024 and 4096 x 256 (or
--cases), one line per case on Plummer spheres: correlation() without the bins (48 bytes per system come back: the kernel, its
launch and the wait for it) at 8, 16 and 32 bins between 0.02 and 5 length units, logarithmically spaced, the same at 32 bins
with the first 8 bodies of every system as the only sources, and the whole call at 32 bins with the bins, against pairs() and
neighbours(k=6) without its lists and records on the same state -- all synchronous calls, wall clock, alternated, medians and
spreads.  The kernel has two loops behind NBODY_BATCH_CORRELATION_LANE_COUNTERS: the line names the library it timed
(NBODY_AMD_LIBRARY, tools/build_variant.sh), so one run per build gives both.  By instruction count a column costs a row
about 7 + bins vector operations.

--contacts: instead, the contact lists (BatchedSystem.contacts).  For n x B = 1024 x 1024 and 256 x 4096 (or --cases), one
line per case on Plummer spheres, at radii of 0.2 and 1.0 mean interparticle spacings within the half-mass radius (few contacts
and many): the counting call (capacity 0, without the per-body records: 48 bytes per system come back), the listing call with
room for the fullest system without and with the per-body records, and the same listing call under per-body radii of half the
radius, against neighbours(k=1, radius, lists=False) without its records -- the nearest existing work, the yardstick -- and
pairs() on the same state: all synchronous calls, wall clock, alternated, medians and spreads.  The kernel has two fills behind
NBODY_BATCH_CONTACTS_FILL_ALWAYS: the line names the library it timed (NBODY_AMD_LIBRARY, tools/build_variant.sh), so one run
per build gives both, and the line carries a checksum of the list so that the two can be seen to agree.

--approaches: instead, the approach lists (BatchedSystem.approaches).  For n x B = 1024 x 1024, 4096 x 256 and 256 x 4096 (or
--cases), one line per case on Plummer spheres at a radius of 0.2 mean interparticle spacings within the half-mass radius: the
counting call (capacity 0, without the per-body records) and the listing call with room for the fullest system, at a horizon
of one crossing of that radius at the velocity dispersion (H = radius / rms speed) and at H = 0, next to the same two calls of
contacts() at the same radius in the same run: all synchronous calls, wall clock, alternated, medians and spreads, and the ratio
of every approaches() call to its contacts() call.  The H = 0 list is asserted to be contacts()' list.  The kernel computes the
separation at the horizon two ways behind NBODY_BATCH_APPROACHES_END_ALWAYS: the line names the library it timed
(NBODY_AMD_LIBRARY, tools/build_variant.sh), so one run per build gives both, and carries a checksum of the list so that the
two can be seen to agree.  By instruction count a pair costs about three r2 chains plus the compares, against one in contacts().

--radial: instead, the radial profiles (BatchedSystem.radial_profile).  For n x B = 1024 x 1024, 4096 x 256 and 256 x 4096 (or
--cases), one line per case on Plummer spheres about the origin with logarithmic edges from 0.05 to 10: the call with the shell
records alone (32 and 8 shells), with the per-body records too, and with the per-system words alone, against
structure(bodies=False) and against what the call replaces -- positions.cpu() plus velocities.cpu() plus a numpy binning of one
quantity (the mass per shell) -- in the same run: all synchronous calls, wall clock, alternated after a warm-up of every call,
medians and spreads.  The kernel walks the shells two ways behind NBODY_BATCH_RADIAL_SPLIT_WALK: the line names the library it
timed (NBODY_AMD_LIBRARY, tools/build_variant.sh), so one run per build gives both, and carries a checksum of the shell records
so that the two can be seen to agree.

--surface: instead, the surface maps (BatchedSystem.surface_map).  For n x B = 1024 x 1024, 4096 x 256 and 256 x 4096 (or
--cases), one line per case on Plummer spheres seen along z on a grid from -2 to 2 on both axes: the call at 16 x 16, 32 x 32 and
64 x 64 cells with the cell records and without them (the per-system words alone: the kernel, its launch and the wait for it),
against what the call replaces -- positions.cpu() plus velocities.cpu() plus one numpy.histogram2d per system at 64 x 64 --
against radial_profile() at 32 shells and against pairs() in the same run: all synchronous calls, wall clock, alternated after a
warm-up of every call, medians and spreads.  The counts of the 64 x 64 map are asserted to be numpy's before a line is printed.

--shape: instead, the shapes (BatchedSystem.shape).  For n x B = 1024 x 1024, 4096 x 256 and 256 x 4096 (or --cases), one line
per case on Plummer spheres flattened to 1 : 0.7 : 0.4 about the origin, four apertures of 0.5, 1, 2 and 4, the reduced tensor:
the call with the aperture records, with the per-body masks too and with the per-system words alone, against radial_profile() at
32 shells and against what the call replaces in the same run -- positions.cpu() plus velocities.cpu(), measured on the whole
batch, plus the same iteration in numpy (einsum and numpy.linalg.eigh), measured on the first --subset systems and extrapolated
to B, which the line says: all synchronous calls, wall clock, alternated after a warm-up of every call, medians of at least 15
and spreads.  The line gives the passes of the slowest system, which sets the launch's time, and the converged q and s of the
timed systems are asserted to be numpy's to 1e-2 (another order of summation, another eigensolver) before a line is printed.

--pair-velocities: instead, the pair velocity statistics (BatchedSystem.pair_velocities).  For n x B = 1024 x 1024, 4096 x 256 and
256 x 4096 (or --cases), one line per case and number of bins (8 and 32 logarithmic bins from 0.05 to 10) on Plummer spheres: the
lean call (bins=False), the call with the bin records, correlation() at the same bins in the same run, and what the call
replaces -- positions.cpu() plus velocities.cpu(), measured on the whole batch, plus a numpy walk of all ordered pairs
(numpy.histogram with weights per sum), measured once on the first --subset systems and extrapolated to B, which the line says:
all synchronous calls, wall clock, alternated after a warm-up of every device call, medians and spreads.  The counts are asserted to be
correlation()'s, and on the timed systems the sums to be numpy's to 1e-9 of their absolute addends, before a line is printed.

--mutual-gravity: instead, the mutual gravity of labelled sets (BatchedSystem.mutual_gravity).  For n x B = 1024 x 1024, 4096 x 256
and 256 x 4096 (or --cases), one line per case and number of sets (K = 2 and 8, body i in set i mod K, softening --eps) on Plummer
spheres: the call with the matrix and without it (matrix=False), pair_velocities() at 8 bins on the same state in the same run, and
what the call replaces -- positions.cpu() plus velocities.cpu(), measured on the whole batch, plus a numpy walk of all ordered
pairs resolved by set, measured once on the first --subset systems and extrapolated to B, which the line says: all synchronous
calls, wall clock, alternated after a warm-up of every device call, medians and spreads.  On the timed systems every word is
asserted to be numpy's to 1e-9 of the potential's size before a line is printed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import n_body_problem_amd as nb  # noqa: E402

PEAK_FP32 = 157.3e12
FLOP_PER_INTERACTION = {"kick_drift": 20, "kdk": 20, "hermite": 60}
CASES = [(64, 16384), (256, 4096), (1024, 1024), (4096, 256), (4096, 512)]

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="*", default=[f"{n}x{b}" for n, b in CASES], help="n x B")
ap.add_argument("--integrators", nargs="*", default=["kick_drift", "kdk"])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--subset", type=int, default=8, help="systems the status quo is timed on")
ap.add_argument("--dt", type=float, default=1e-3)
ap.add_argument("--eps", type=float, default=1e-2)
ap.add_argument("--adaptive", action="store_true", help="Hermite step_n against evolve(levels=0), and a scattering case")
ap.add_argument("--stops", action="store_true", help="evolve(levels=0) with conditions that cannot trigger against without, "
                "and the scattering case stopped at a collision radius")
ap.add_argument("--merges", action="store_true", help="evolve(levels=0) under the collision action merge against stop, with "
                "conditions that cannot trigger, and the scattering case merged at a collision radius")
ap.add_argument("--radii", action="store_true", help="evolve(levels=0) with per-body radii against a collision radius, neither "
                "of which can trigger, and the scattering case with unequal radii stopped and merged")
ap.add_argument("--fates", action="store_true", help="evolve(levels=0) with massive counts m and the tracer action 'remove' under "
                "conditions that never trigger against the same state with the feature off")
ap.add_argument("--accrete", action="store_true", help="evolve(levels=0) under the hit action 'accrete' against 'remove' on a state "
                "where nothing hits, and a state where about 1 %% of the tracers accrete")
ap.add_argument("--massive", action="store_true", help="Hermite step_n and evolve(levels=0) with massive counts m against the "
                "feature off on the same state with the other bodies' mass words zero")
ap.add_argument("--field", action="store_true", help="evolve(levels=0) with a three-component external field against the "
                "field off, with massive counts m, on the same state")
ap.add_argument("--pairs", action="store_true", help="pairs() against energy() on the same state, wall clock")
ap.add_argument("--structure", action="store_true", help="structure() with and without the per-body records against energy() "
                "and pairs() on the same state, wall clock")
ap.add_argument("--members", action="store_true", help="members() with and without the per-body records and with one iteration "
                "against energy() and pairs() on the same boosted state, wall clock, and the time per iteration")
ap.add_argument("--hierarchy", action="store_true", help="hierarchy() with and without the node and body records against "
                "pairs() on the same state of nested objects, wall clock, and the levels evaluated")
ap.add_argument("--gravity", action="store_true", help="gravity_at() at the systems' own bodies with and without the tidal tensor "
                "against members(max_iterations=1) and energy() on the same state, and a 65536-point grid per system, wall clock")
ap.add_argument("--groups", action="store_true", help="groups() at 0.2 and 1.0 mean spacings with and without the per-slot and "
                "per-body records against pairs() on the same Plummer spheres, wall clock, and the sweeps run")
ap.add_argument("--span", action="store_true", help="spanning_tree() with and without the separations, the records and subsets "
                "of 20 bodies against groups() and pairs() on the same Plummer spheres, wall clock, and the rounds run")
ap.add_argument("--neighbours", action="store_true", help="neighbours() at k = 1, 6 and 8, with a radius, with 8 sources and with "
                "the lists against structure(k=6) and pairs() on the same Plummer spheres, wall clock")
ap.add_argument("--contacts", action="store_true", help="contacts() at 0.2 and 1.0 mean spacings, counting and listing, with radii, "
                "against neighbours(k=1, radius, lists=False) and pairs() on the same Plummer spheres, wall clock")
ap.add_argument("--approaches", action="store_true", help="approaches() at 0.2 mean spacings, counting and listing, at a horizon of "
                "one crossing and at 0, against contacts() at the same radius on the same Plummer spheres, wall clock")
ap.add_argument("--correlation", action="store_true", help="correlation() at 8, 16 and 32 bins, with 8 sources and with the bins "
                "against pairs() and neighbours(k=6) on the same Plummer spheres, wall clock")
ap.add_argument("--radial", action="store_true", help="radial_profile() at 32 and 8 logarithmic shells, with and without the shell "
                "and body records, against structure(bodies=False) and the download plus a numpy binning, wall clock")
ap.add_argument("--surface", action="store_true", help="surface_map() at 16 x 16, 32 x 32 and 64 x 64 cells, with and without the cell "
                "records, against the download plus one numpy.histogram2d per system, radial_profile() and pairs(), wall clock")
ap.add_argument("--shape", action="store_true", help="shape() at four apertures, reduced, with and without the aperture and body "
                "records, against the download plus the iteration in numpy (timed on --subset systems) and radial_profile(), wall clock")
ap.add_argument("--pair-velocities", action="store_true", help="pair_velocities() at 8 and 32 bins, lean and with the bin records, "
                "against correlation() at the same bins and the download plus a numpy pair walk (timed on --subset systems), wall clock")
ap.add_argument("--mutual-gravity", action="store_true", help="mutual_gravity() at 2 and 8 sets, with and without the matrix, against "
                "pair_velocities() at 8 bins and the download plus a numpy pair walk by set (timed on --subset systems), wall clock")
args = ap.parse_args()


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1])


def ensemble(n, B):
    """B Plummer spheres of n bodies: one sphere per seed for the first 64 systems, then copies jittered by 1e-4."""
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    rng = np.random.default_rng(n * 7 + B)
    for s in range(B):
        if s < 64:
            P[s], V[s] = nb.plummer(n, seed=1000 + s)
        else:
            P[s], V[s] = P[s % 64], V[s % 64]
            P[s, :, :3] += rng.normal(0, 1e-4, (n, 3)).astype(np.float32)
    return P, V


def adaptive_lines():
    import time
    for case in args.cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        inter = B * n * n
        k = int(min(400, max(10, 2e11 // inter)))
        dt = float(np.float32(args.dt))
        with nb.BatchedSystem(B, n, integrator="hermite") as batch:
            batch.set_state(P, V)

            def fixed():
                batch.step_n(k, dt, args.eps)

            def adaptive():
                batch.evolve(k, dt, levels=0, softening=args.eps)

            fixed()
            adaptive()
            torch.cuda.synchronize()
            tf, ta = [], []
            for _ in range(args.repeats):      # alternated
                tf.append(timed(fixed) / k)
                ta.append(timed(adaptive) / k)
            mf, ma = statistics.median(tf), statistics.median(ta)
        print(json.dumps({"n": n, "B": B, "k": k, "step_n_ms_per_step": round(mf, 5), "evolve_levels0_ms_per_step": round(ma, 5),
                          "overhead": round(ma / mf - 1.0, 4), "step_n_repeats": [round(x, 5) for x in tf],
                          "evolve_repeats": [round(x, 5) for x in ta]}), flush=True)
    B = 1024
    ecc = np.linspace(0.0, 0.99, B)
    P = np.zeros((B, 2, 4), np.float32)
    V = np.zeros((B, 2, 4), np.float32)
    for s, e in enumerate(ecc):                 # two half masses, semi-major axis 1, at apocentre (G = 1): period 2 pi
        ra, va = 1.0 + e, np.sqrt((1.0 - e) / (1.0 + e))
        P[s] = [[0.5 * ra, 0, 0, 0.5], [-0.5 * ra, 0, 0, 0.5]]
        V[s] = [[0, 0.5 * va, 0, 0], [0, -0.5 * va, 0, 0]]
    dt_max = float(np.float32(2 * np.pi / 64))
    with nb.BatchedSystem(B, 2, integrator="hermite") as batch:
        walls = []
        for _ in range(1 + args.repeats):           # the first run warms up (allocations, kernel attributes)
            batch.set_state(P, V)
            e0 = batch.energy(0.0)[:, 2]
            batch.sync()
            t0 = time.perf_counter()
            res = batch.evolve(64, dt_max, levels=12, eta=0.01, eta_start=0.01, softening=0.0)
            walls.append(time.perf_counter() - t0)
            de = np.abs(batch.energy(0.0)[:, 2] / e0 - 1.0)
        wall = statistics.median(walls[1:])
        q = [int(x) for x in np.percentile(res.steps, [0, 25, 50, 75, 90, 99, 100])]
        print(json.dumps({"scattering_pairs": B, "eccentricities": "0 .. 0.99", "wall_ms_median": round(wall * 1e3, 3),
                          "wall_ms_repeats": [round(w * 1e3, 3) for w in walls[1:]],
                          "steps_percentiles_0_25_50_75_90_99_100": q, "steps_total": int(res.steps.sum()),
                          "max_level": int(res.max_level.max()), "clamped": int(res.clamped.sum()),
                          "worst_rel_energy_error": float(f"{de.max():.3g}"),
                          "median_rel_energy_error": float(f"{np.median(de):.3g}")}), flush=True)
        # fixed steps to the same end time: double the step count until the worst error is the adaptive run's
        target, k, bound = float(de.max()), 1024, 1 << 18
        while True:
            batch.set_state(P, V)
            batch.sync()
            t0 = time.perf_counter()
            batch.step_n(k, float(np.float32(64.0 * dt_max / k)), 0.0)
            batch.sync()
            wall_f = time.perf_counter() - t0
            de_f = float(np.nanmax(np.abs(batch.energy(0.0)[:, 2] / e0 - 1.0)))
            print(json.dumps({"fixed_steps": k, "wall_ms": round(wall_f * 1e3, 3), "worst_rel_energy_error": float(f"{de_f:.3g}"),
                              "reaches_adaptive_worst": bool(de_f <= target)}), flush=True)
            if de_f <= target or k >= bound:
                break
            k *= 2


def scattering_pairs(B=1024):
    ecc = np.linspace(0.0, 0.99, B)
    P = np.zeros((B, 2, 4), np.float32)
    V = np.zeros((B, 2, 4), np.float32)
    for s, e in enumerate(ecc):                 # two half masses, semi-major axis 1, at apocentre (G = 1): period 2 pi
        ra, va = 1.0 + e, np.sqrt((1.0 - e) / (1.0 + e))
        P[s] = [[0.5 * ra, 0, 0, 0.5], [-0.5 * ra, 0, 0, 0.5]]
        V[s] = [[0, 0.5 * va, 0, 0], [0, -0.5 * va, 0, 0]]
    return P, V, float(np.float32(2 * np.pi / 64))


def stops_lines():
    import time
    for case in args.cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        inter = B * n * n
        k = int(min(400, max(10, 2e11 // inter)))
        dt = float(np.float32(args.dt))
        with nb.BatchedSystem(B, n, integrator="hermite") as plain, nb.BatchedSystem(B, n, integrator="hermite") as watched:
            plain.set_state(P, V)
            watched.set_state(P, V)
            watched.set_stop_conditions(collision_radius=1e-6, escape_radius=1e6)

            def without():
                plain.evolve(k, dt, levels=0, softening=args.eps)

            def with_conditions():
                watched.evolve(k, dt, levels=0, softening=args.eps)

            without()
            with_conditions()
            torch.cuda.synchronize()
            tp, tw = [], []
            for _ in range(args.repeats):      # alternated
                tp.append(timed(without) / k)
                tw.append(timed(with_conditions) / k)
            mp, mw = statistics.median(tp), statistics.median(tw)
            stopped = int(watched.stops().stopped.sum())
        print(json.dumps({"n": n, "B": B, "k": k, "evolve_ms_per_step": round(mp, 5), "evolve_with_conditions_ms_per_step": round(mw, 5),
                          "ratio": round(mw / mp, 4), "stopped": stopped, "evolve_repeats": [round(x, 5) for x in tp],
                          "with_conditions_repeats": [round(x, 5) for x in tw]}), flush=True)
    P, V, dt_max = scattering_pairs()
    with nb.BatchedSystem(P.shape[0], 2, integrator="hermite") as batch:
        out = {}
        for name, rc in (("to_completion", 0.0), ("collision_radius_0.05", 0.05)):
            walls = []
            for _ in range(1 + args.repeats):       # the first run warms up
                batch.set_state(P, V)
                batch.set_stop_conditions(collision_radius=rc)
                batch.sync()
                t0 = time.perf_counter()
                res = batch.evolve(64, dt_max, levels=12, eta=0.01, eta_start=0.01, softening=0.0)
                walls.append(time.perf_counter() - t0)
            st = batch.stops()
            steps = res.steps[st.stopped] if st.stopped.any() else res.steps
            out[name] = {"wall_ms_median": round(statistics.median(walls[1:]) * 1e3, 3),
                         "wall_ms_repeats": [round(w * 1e3, 3) for w in walls[1:]], "stopped": int(st.stopped.sum()),
                         "steps_total": int(res.steps.sum()),
                         ("steps_of_stopped_percentiles_0_25_50_75_100" if st.stopped.any() else "steps_percentiles_0_25_50_75_100"):
                             [int(x) for x in np.percentile(steps, [0, 25, 50, 75, 100])]}
            if st.stopped.any():
                idx = np.nonzero(st.stopped)[0]
                out[name]["first_stopped_pair_eccentricity"] = round(float(np.linspace(0.0, 0.99, P.shape[0])[idx[0]]), 4)
                out[name]["separation_min_max"] = [float(f"{st.separation[idx].min():.4g}"), float(f"{st.separation[idx].max():.4g}")]
        print(json.dumps({"scattering_pairs": P.shape[0], "eccentricities": "0 .. 0.99", **out}), flush=True)


def merges_lines():
    import time
    for case in args.cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        inter = B * n * n
        k = int(min(400, max(10, 2e11 // inter)))
        dt = float(np.float32(args.dt))
        with nb.BatchedSystem(B, n, integrator="hermite") as stopping, nb.BatchedSystem(B, n, integrator="hermite") as merging:
            for batch, action in ((stopping, "stop"), (merging, "merge")):
                batch.set_state(P, V)
                batch.set_stop_conditions(collision_radius=1e-6, escape_radius=1e6)
                batch.set_collision_action(action)

            def stop_kernel():
                stopping.evolve(k, dt, levels=0, softening=args.eps)

            def merge_kernel():
                merging.evolve(k, dt, levels=0, softening=args.eps)

            stop_kernel()
            merge_kernel()
            torch.cuda.synchronize()
            ts, tm = [], []
            for _ in range(args.repeats):      # alternated
                ts.append(timed(stop_kernel) / k)
                tm.append(timed(merge_kernel) / k)
            ms, mm = statistics.median(ts), statistics.median(tm)
            merged = int(merging.mergers().count.sum())
        print(json.dumps({"n": n, "B": B, "k": k, "evolve_stop_ms_per_step": round(ms, 5), "evolve_merge_ms_per_step": round(mm, 5),
                          "ratio": round(mm / ms, 4), "mergers": merged, "stop_repeats": [round(x, 5) for x in ts],
                          "merge_repeats": [round(x, 5) for x in tm]}), flush=True)
    P, V, dt_max = scattering_pairs()
    with nb.BatchedSystem(P.shape[0], 2, integrator="hermite") as batch:
        out = {}
        for action in ("stop", "merge"):
            walls = []
            for _ in range(1 + args.repeats):       # the first run warms up
                batch.set_counts([2] * P.shape[0])
                batch.set_state(P, V)
                batch.set_stop_conditions(collision_radius=0.05)
                batch.set_collision_action(action)
                batch.sync()
                t0 = time.perf_counter()
                res = batch.evolve(64, dt_max, levels=12, eta=0.01, eta_start=0.01, softening=0.0)
                walls.append(time.perf_counter() - t0)
            st, mg = batch.stops(), batch.mergers()
            hit = st.stopped if action == "stop" else mg.count > 0
            out[action] = {"wall_ms_median": round(statistics.median(walls[1:]) * 1e3, 3),
                           "wall_ms_repeats": [round(w * 1e3, 3) for w in walls[1:]], "stopped": int(st.stopped.sum()),
                           "merged": int((mg.count > 0).sum()), "at_the_end_time": int((res.ticks == 64 << 12).sum()),
                           "steps_total": int(res.steps.sum()),
                           "steps_of_colliding_pairs_percentiles_0_25_50_75_100":
                               [int(x) for x in np.percentile(res.steps[hit], [0, 25, 50, 75, 100])] if hit.any() else []}
            if action == "merge" and hit.any():
                ticks = mg.events["tick"][hit, 0]
                out[action]["merger_ticks_min_max"] = [int(ticks.min()), int(ticks.max())]
        print(json.dumps({"scattering_pairs": P.shape[0], "eccentricities": "0 .. 0.99", "collision_radius": 0.05, **out}), flush=True)


def radii_lines():
    import time
    for case in args.cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        inter = B * n * n
        k = int(min(400, max(10, 2e11 // inter)))
        dt = float(np.float32(args.dt))
        with nb.BatchedSystem(B, n, integrator="hermite") as uniform, nb.BatchedSystem(B, n, integrator="hermite") as radii:
            uniform.set_state(P, V)
            uniform.set_stop_conditions(collision_radius=1e-6, escape_radius=1e6)
            radii.set_state(P, V)
            radii.set_stop_conditions(escape_radius=1e6)
            radii.set_radii(np.full((B, n), 5e-7, np.float32))

            def stop_kernel():
                uniform.evolve(k, dt, levels=0, softening=args.eps)

            def radii_kernel():
                radii.evolve(k, dt, levels=0, softening=args.eps)

            stop_kernel()
            radii_kernel()
            torch.cuda.synchronize()
            ts, tr = [], []
            for _ in range(args.repeats):      # alternated
                ts.append(timed(stop_kernel) / k)
                tr.append(timed(radii_kernel) / k)
            ms, mr = statistics.median(ts), statistics.median(tr)
            stopped = int(uniform.stops().stopped.sum()) + int(radii.stops().stopped.sum())
        print(json.dumps({"n": n, "B": B, "k": k, "evolve_stop_ms_per_step": round(ms, 5), "evolve_radii_ms_per_step": round(mr, 5),
                          "ratio": round(mr / ms, 4), "stopped": stopped, "stop_repeats": [round(x, 5) for x in ts],
                          "radii_repeats": [round(x, 5) for x in tr]}), flush=True)
    P, V, dt_max = scattering_pairs()
    R = np.tile(np.float32([0.03, 0.02]), (P.shape[0], 1))
    with nb.BatchedSystem(P.shape[0], 2, integrator="hermite") as batch:
        out = {}
        for action in ("stop", "merge"):
            walls = []
            for _ in range(1 + args.repeats):       # the first run warms up
                batch.set_counts([2] * P.shape[0])
                batch.set_state(P, V)
                batch.set_collision_action(action)
                batch.set_radii(R)
                batch.sync()
                t0 = time.perf_counter()
                res = batch.evolve(64, dt_max, levels=12, eta=0.01, eta_start=0.01, softening=0.0)
                walls.append(time.perf_counter() - t0)
            st, mg, rr = batch.stops(), batch.mergers(), batch.radii()
            hit = st.stopped if action == "stop" else mg.count > 0
            out[action] = {"wall_ms_median": round(statistics.median(walls[1:]) * 1e3, 3),
                           "wall_ms_repeats": [round(w * 1e3, 3) for w in walls[1:]], "stopped": int(st.stopped.sum()),
                           "merged": int((mg.count > 0).sum()), "at_the_end_time": int((res.ticks == 64 << 12).sum()),
                           "steps_total": int(res.steps.sum()),
                           "steps_of_colliding_pairs_percentiles_0_25_50_75_100":
                               [int(x) for x in np.percentile(res.steps[hit], [0, 25, 50, 75, 100])] if hit.any() else []}
            if action == "merge" and hit.any():
                out[action]["merged_radius_min_max"] = [float(f"{rr[hit, 0].min():.6g}"), float(f"{rr[hit, 0].max():.6g}")]
        print(json.dumps({"scattering_pairs": P.shape[0], "eccentricities": "0 .. 0.99", "radii": [0.03, 0.02], **out}), flush=True)


def massive_lines():
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["4096x256", "1024x1024"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        k = int(min(400, max(10, 2e11 // (B * n * n))))
        dt = float(np.float32(args.dt))
        for m in sorted({min(m, n) for m in (1, 8, 64, 512, n)}):
            Z = P.copy()
            Z[:, m:, 3] = 0.0
            for mode in ("step_n", "evolve_levels0"):
                with nb.BatchedSystem(B, n, integrator="hermite") as on, nb.BatchedSystem(B, n, integrator="hermite") as off:
                    on.set_state(Z, V)
                    on.set_massive_counts([m] * B)
                    off.set_state(Z, V)

                    def run(batch):
                        if mode == "step_n":
                            batch.step_n(k, dt, args.eps)
                        else:
                            batch.evolve(k, dt, levels=0, softening=args.eps)

                    run(on)
                    run(off)
                    torch.cuda.synchronize()
                    t_on, t_off = [], []
                    for _ in range(args.repeats):      # alternated
                        t_on.append(timed(lambda: run(on)) / k)
                        t_off.append(timed(lambda: run(off)) / k)
                    m_on, m_off = statistics.median(t_on), statistics.median(t_off)
                    same = bool(torch.equal(on.positions, off.positions) and torch.equal(on.velocities, off.velocities))
                print(json.dumps({"n": n, "B": B, "m": m, "call": mode, "k": k, "massive_ms_per_step": round(m_on, 5),
                                  "off_zero_mass_ms_per_step": round(m_off, 5), "off_over_massive": round(m_off / m_on, 3),
                                  "massive_spread": round((max(t_on) - min(t_on)) / m_on, 4),
                                  "off_spread": round((max(t_off) - min(t_off)) / m_off, 4),
                                  "interactions_per_step": nb.batch.interactions_per_step([n] * B, [m] * B),
                                  "states_equal_bit_for_bit": same, "massive_repeats": [round(x, 5) for x in t_on],
                                  "off_repeats": [round(x, 5) for x in t_off]}), flush=True)


def field_lines():
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["4096x256", "1024x1024"]
    galaxy = [("plummer", 0.3, 0.05, 0.0), ("miyamoto_nagai", 1.0, 0.5, 0.1), ("log_halo", 0.7, 1.0, 0.9)]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        dt = float(np.float32(args.dt))
        for m in sorted({min(m, n) for m in (1, 8, 64, n)}):
            k = int(min(400, max(10, 2e11 // (B * n * m))))
            with nb.BatchedSystem(B, n, integrator="hermite") as on, nb.BatchedSystem(B, n, integrator="hermite") as off:
                for batch in (on, off):
                    batch.set_state(P, V)
                    batch.set_massive_counts([m] * B)
                on.set_external_field(galaxy)

                def run(batch):
                    batch.evolve(k, dt, levels=0, softening=args.eps)

                run(on)
                run(off)
                torch.cuda.synchronize()
                t_on, t_off = [], []
                for _ in range(args.repeats):      # alternated
                    t_on.append(timed(lambda: run(on)) / k)
                    t_off.append(timed(lambda: run(off)) / k)
                m_on, m_off = statistics.median(t_on), statistics.median(t_off)
            print(json.dumps({"n": n, "B": B, "m": m, "call": "evolve_levels0", "k": k, "components": [c[0] for c in galaxy],
                              "field_ms_per_step": round(m_on, 5), "off_ms_per_step": round(m_off, 5),
                              "field_over_off": round(m_on / m_off, 3),
                              "field_ns_per_body_step": round((m_on - m_off) * 1e6 / (B * n), 4),
                              "field_spread": round((max(t_on) - min(t_on)) / m_on, 4),
                              "off_spread": round((max(t_off) - min(t_off)) / m_off, 4),
                              "interactions_per_step": nb.batch.interactions_per_step([n] * B, [m] * B),
                              "field_repeats": [round(x, 5) for x in t_on], "off_repeats": [round(x, 5) for x in t_off]}), flush=True)


def fates_lines():
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["4096x256", "1024x1024"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        dt = float(np.float32(args.dt))
        for m in sorted({min(m, n) for m in (1, 8, 64)}):
            k = int(min(400, max(10, 2e11 // (B * n * m))))
            with nb.BatchedSystem(B, n, integrator="hermite") as on, nb.BatchedSystem(B, n, integrator="hermite") as off:
                for batch in (on, off):
                    batch.set_state(P, V)
                    batch.set_massive_counts([m] * B)
                on.set_tracer_action("remove")
                on.set_stop_conditions(collision_radius=1e-9, escape_radius=1e9)   # conditions that never trigger

                def run(batch):
                    batch.evolve(k, dt, levels=0, softening=args.eps)

                run(on)
                run(off)
                torch.cuda.synchronize()
                t_on, t_off = [], []
                for _ in range(args.repeats):      # alternated
                    t_on.append(timed(lambda: run(on)) / k)
                    t_off.append(timed(lambda: run(off)) / k)
                m_on, m_off = statistics.median(t_on), statistics.median(t_off)
                same = bool(torch.equal(on.positions, off.positions) and torch.equal(on.velocities, off.velocities))
                f = on.fates()
            print(json.dumps({"n": n, "B": B, "m": m, "call": "evolve_levels0", "k": k, "fates_ms_per_step": round(m_on, 5),
                              "off_ms_per_step": round(m_off, 5), "fates_over_off": round(m_on / m_off, 3),
                              "fates_spread": round((max(t_on) - min(t_on)) / m_on, 4),
                              "off_spread": round((max(t_off) - min(t_off)) / m_off, 4),
                              "interactions_per_step": nb.batch.interactions_per_step([n] * B, [m] * B),
                              "states_equal_bit_for_bit": same, "removed": int(f.hit.sum() + f.escaped.sum()),
                              "fates_repeats": [round(x, 5) for x in t_on], "off_repeats": [round(x, 5) for x in t_off]}), flush=True)


def accrete_lines():
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    dt = float(np.float32(args.dt))
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        for m in sorted({min(m, n) for m in (1, 8, 64)}):
            k = int(min(400, max(10, 2e11 // (B * n * m))))
            with nb.BatchedSystem(B, n, integrator="hermite") as acc, nb.BatchedSystem(B, n, integrator="hermite") as rem:
                for batch, action in ((acc, "accrete"), (rem, "remove")):
                    batch.set_state(P, V)
                    batch.set_massive_counts([m] * B)
                    batch.set_tracer_action("remove")
                    batch.set_hit_action(action)
                    batch.set_stop_conditions(collision_radius=1e-9, escape_radius=1e9)   # conditions that never trigger

                def run(batch):
                    batch.evolve(k, dt, levels=0, softening=args.eps)

                run(acc)
                run(rem)
                torch.cuda.synchronize()
                t_acc, t_rem = [], []
                for _ in range(args.repeats):      # alternated
                    t_acc.append(timed(lambda: run(acc)) / k)
                    t_rem.append(timed(lambda: run(rem)) / k)
                m_acc, m_rem = statistics.median(t_acc), statistics.median(t_rem)
                same = bool(torch.equal(acc.positions, rem.positions) and torch.equal(acc.velocities, rem.velocities))
                f, a = acc.fates(), acc.accretions()
            print(json.dumps({"n": n, "B": B, "m": m, "call": "evolve_levels0", "k": k, "accrete_ms_per_step": round(m_acc, 5),
                              "remove_ms_per_step": round(m_rem, 5), "accrete_over_remove": round(m_acc / m_rem, 4),
                              "accrete_spread": round((max(t_acc) - min(t_acc)) / m_acc, 4),
                              "remove_spread": round((max(t_rem) - min(t_rem)) / m_rem, 4),
                              "interactions_per_step": nb.batch.interactions_per_step([n] * B, [m] * B),
                              "states_equal_bit_for_bit": same, "removed": int(f.hit.sum() + f.escaped.sum()),
                              "accretions": int(a.count.sum()), "accrete_repeats": [round(x, 5) for x in t_acc],
                              "remove_repeats": [round(x, 5) for x in t_rem]}), flush=True)
    # about 1 % of the tracers accrete: the tracers' mass words are 1e-3 of the massive bodies'
    n, B, m, k = 1024, 256, 8, 200
    P, V = ensemble(n, B)
    P[:, m:, 3] = P[:, :m, 3].mean() * 1e-3
    with nb.BatchedSystem(B, n, integrator="hermite") as batch:
        batch.set_massive_counts([m] * B)
        batch.set_tracer_action("remove")

        def fresh(action, rc):
            batch.set_state(P, V)
            batch.set_hit_action(action)
            batch.set_stop_conditions(collision_radius=rc, escape_radius=1e9)
            batch.sync()

        def evolve():
            batch.evolve(k, dt, levels=0, softening=args.eps)

        lo, hi = 1e-4, 1.0                         # bisection on the run that removes, geometric: hits grow with the radius
        for _ in range(12):
            rc = float(np.sqrt(lo * hi))
            fresh("remove", rc)
            evolve()
            frac = float(batch.fates().hit.sum()) / (B * (n - m))
            lo, hi = (rc, hi) if frac < 0.01 else (lo, rc)
        rc = float(np.sqrt(lo * hi))
        t_acc, t_rem = [], []
        for _ in range(1 + args.repeats):          # the first pair warms up; alternated
            fresh("accrete", rc)
            t_acc.append(timed(evolve) / k)
            f, a, st = batch.fates(), batch.accretions(), batch.stops()
            fresh("remove", rc)
            t_rem.append(timed(evolve) / k)
        t_acc, t_rem = t_acc[1:], t_rem[1:]
        m_acc, m_rem = statistics.median(t_acc), statistics.median(t_rem)
    print(json.dumps({"n": n, "B": B, "m": m, "call": "evolve_levels0", "k": k, "collision_radius": float(f"{rc:.4g}"),
                      "tracers_hit_fraction": round(float(f.hit.sum()) / (B * (n - m)), 5), "accretions": int(a.count.sum()),
                      "systems_stopped": int(st.stopped.sum()), "accrete_ms_per_step": round(m_acc, 5),
                      "remove_ms_per_step": round(m_rem, 5), "accrete_over_remove": round(m_acc / m_rem, 4),
                      "accrete_spread": round((max(t_acc) - min(t_acc)) / m_acc, 4),
                      "remove_spread": round((max(t_rem) - min(t_rem)) / m_rem, 4),
                      "accrete_repeats": [round(x, 5) for x in t_acc], "remove_repeats": [round(x, 5) for x in t_rem]}), flush=True)


def pairs_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            wall(batch.pairs)                           # the first call allocates the records and sets the kernel's LDS limit
            wall(lambda: batch.energy(0.0))
            tp, te = [], []
            for _ in range(args.repeats):               # alternated
                t, res = wall(batch.pairs)
                tp.append(t)
                te.append(wall(lambda: batch.energy(0.0))[0])
            mp, me = statistics.median(tp), statistics.median(te)
        print(json.dumps({"n": n, "B": B, "pairs_ms": round(mp, 3), "energy_ms": round(me, 3), "pairs_over_energy": round(mp / me, 3),
                          "pair_evaluations_per_s": float(f"{B * n * n / (mp * 1e-3):.4g}"), "record_megabytes": round(B * n * 48 / 1e6, 1),
                          "binaries_found": int(res.binaries.sum()), "pairs_spread": round((max(tp) - min(tp)) / mp, 4),
                          "energy_spread": round((max(te) - min(te)) / me, 4), "pairs_repeats": [round(x, 3) for x in tp],
                          "energy_repeats": [round(x, 3) for x in te]}), flush=True)


def structure_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"structure": batch.structure, "structure_lean": lambda: batch.structure(bodies=False),
                     "energy": lambda: batch.energy(0.0), "pairs": batch.pairs}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    if name == "structure":
                        res = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        line.update({"lean_over_energy": round(med["structure_lean"] / med["energy"], 3),
                     "pair_walks_per_s": float(f"{3 * B * n * n / (med['structure_lean'] * 1e-3):.4g}"),
                     "record_megabytes": round(B * n * 40 / 1e6, 1), "system_kilobytes": round(B * 120 / 1e3, 1),
                     "median_core_radius": round(float(np.median(res.core_radius)), 4),
                     "median_half_weight_radius": round(float(np.median(res.lagrangian[:, 1])), 4)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def boosted_ensemble(n, B):
    """B boosted Plummer spheres of n bodies, the state of tests/hermite_members_ref.py: plummer(n, seed=100 + s) with the
    velocities of a random 35 % of the bodies (default_rng(s)) multiplied by a uniform 1.5 ... 4 and a bulk velocity added, one
    sphere per seed for the first 64 systems, then copies jittered by 1e-4.  Iterative unbinding drops 20 - 30 % of them."""
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    jitter = np.random.default_rng(n * 7 + B)
    for s in range(B):
        if s < 64:
            P[s], V[s] = nb.plummer(n, seed=100 + s)
            rng = np.random.default_rng(s)
            fast = rng.random(n) < 0.35
            factor = np.where(fast, rng.uniform(1.5, 4.0, size=n), 1.0)
            V[s, :, :3] = (V[s, :, :3].astype(np.float64) * factor[:, None] + np.asarray((0.3, -0.2, 0.1))).astype(np.float32)
        else:
            P[s], V[s] = P[s % 64], V[s % 64]
            P[s, :, :3] += jitter.normal(0, 1e-4, (n, 3)).astype(np.float32)
    return P, V


def members_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = boosted_ensemble(n, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"members": lambda: batch.members(0.0), "members_lean": lambda: batch.members(0.0, bodies=False),
                     "members_lean_one_iteration": lambda: batch.members(0.0, max_iterations=1, bodies=False),
                     "energy": lambda: batch.energy(0.0), "pairs": batch.pairs}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    if name == "members_lean":
                        res = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        # One iteration of every system is the one-iteration call.  The two lean calls differ in the iterations after the first
        # alone (the launch, the loads, the final sums and the copies cancel): where all B workgroups are resident at once the
        # system with the most iterations sets that difference, in a larger batch the mean does, so both quotients are given.
        more = med["members_lean"] - med["members_lean_one_iteration"]
        line.update({"iterations_mean": round(float(res.iterations.mean()), 3), "iterations_max": int(res.iterations.max()),
                     "converged": int(res.converged.sum()),
                     "one_iteration_over_energy": round(med["members_lean_one_iteration"] / med["energy"], 3),
                     "pair_evaluations_per_s_one_iteration": float(f"{B * n * n / (med['members_lean_one_iteration'] * 1e-3):.4g}"),
                     "ms_per_further_iteration_of_the_slowest": round(more / max(int(res.iterations.max()) - 1, 1), 4),
                     "ms_per_further_iteration_of_the_mean": round(more / max(float(res.iterations.mean()) - 1.0, 1e-9), 4),
                     "record_megabytes": round(B * n * 24 / 1e6, 1), "system_kilobytes": round(B * 88 / 1e3, 1),
                     "median_bound_fraction": round(float(np.median(res.bound_fraction())), 4)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def nested_ensemble(n, B):
    """B systems of n bodies from the generator of tests/hermite_hierarchy_ref.py: objects(n, seed=s), 64 distinct systems, the
    rest copies."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import hermite_hierarchy_ref as href
    P = np.zeros((B, n, 4), np.float32)
    V = np.zeros((B, n, 4), np.float32)
    for s in range(B):
        if s < 64:
            P[s], V[s] = href.objects(n, 500 + s)
        else:
            P[s], V[s] = P[s % 64], V[s % 64]
    return P, V


def hierarchy_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = nested_ensemble(n, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"hierarchy": lambda: batch.hierarchy(max_levels=16),
                     "hierarchy_lean": lambda: batch.hierarchy(max_levels=16, nodes=False, bodies=False),
                     "hierarchy_lean_tolerance_0.01": lambda: batch.hierarchy(0.01, max_levels=16, nodes=False, bodies=False),
                     "pairs": batch.pairs}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            kept = {}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    kept[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        free, strict = kept["hierarchy_lean"], kept["hierarchy_lean_tolerance_0.01"]
        line.update({"levels_mean": round(float(free.levels.mean()), 3), "levels_max": int(free.levels.max()),
                     "levels_mean_tolerance_0.01": round(float(strict.levels.mean()), 3),
                     "levels_max_tolerance_0.01": int(strict.levels.max()), "converged": int(free.converged.sum()),
                     "nodes_mean": round(float(free.nodes.mean()), 1), "multiplicity_mean": free.multiplicity().mean(axis=0).round(1).tolist(),
                     "unstable_mean": round(float(free.unstable.mean()), 1),
                     "lean_over_pairs_call": round(med["hierarchy_lean"] / med["pairs"], 3),
                     "record_megabytes": round(B * n * (128 + 16) / 1e6, 1), "system_kilobytes": round(B * 40 / 1e3, 1)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def gravity_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]

    def measure(batch, calls):
        def wall(fn):
            batch.sync()
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        for fn in calls.values():                       # the first calls allocate the records and set the kernels' LDS limits
            wall(fn)
        times = {name: [] for name in calls}
        for _ in range(args.repeats):                   # alternated
            for name, fn in calls.items():
                times[name].append(wall(fn))
        return times, {name: statistics.median(ts) for name, ts in times.items()}

    def report(line, calls, times, med):
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)

    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = boosted_ensemble(n, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)
            calls = {"gravity_own_tidal": lambda: batch.gravity_at(softening=args.eps, tidal=True),
                     "gravity_own": lambda: batch.gravity_at(softening=args.eps),
                     "members_lean_one_iteration": lambda: batch.members(args.eps, max_iterations=1, bodies=False),
                     "members_one_iteration": lambda: batch.members(args.eps, max_iterations=1),
                     "energy": lambda: batch.energy(args.eps)}
            times, med = measure(batch, calls)
        line = {"n": n, "B": B, "softening": args.eps,
                "own_over_members_one_iteration": round(med["gravity_own"] / med["members_one_iteration"], 3),
                "tidal_over_own": round(med["gravity_own_tidal"] / med["gravity_own"], 3),
                "pair_evaluations_per_s_own": float(f"{B * n * n / (med['gravity_own'] * 1e-3):.4g}"),
                "record_megabytes": round(B * n * 24 / 1e6, 1), "tidal_megabytes": round(B * n * 24 / 1e6, 1)}
        report(line, calls, times, med)
    n, B, side = 1024, 64, 256                          # a 256 x 256 grid in the plane z = 0 of every system
    P, V = boosted_ensemble(n, B)
    axis = np.linspace(-2.0, 2.0, side, dtype=np.float32)
    grid = torch.zeros((B, side * side, 4), dtype=torch.float32, device="cuda")
    grid[:, :, 0] = torch.as_tensor(np.repeat(axis, side)).to("cuda")
    grid[:, :, 1] = torch.as_tensor(np.tile(axis, side)).to("cuda")
    with nb.BatchedSystem(B, n) as batch:
        batch.set_state(P, V)
        calls = {"gravity_grid_tidal": lambda: batch.gravity_at(grid, softening=args.eps, tidal=True),
                 "gravity_grid": lambda: batch.gravity_at(grid, softening=args.eps)}
        times, med = measure(batch, calls)
    line = {"n": n, "B": B, "points_per_system": side * side, "softening": args.eps,
            "pair_evaluations_per_s_grid": float(f"{B * side * side * n / (med['gravity_grid'] * 1e-3):.4g}"),
            "record_megabytes": round(B * side * side * 24 / 1e6, 1), "tidal_megabytes": round(B * side * side * 24 / 1e6, 1)}
    report(line, calls, times, med)


def groups_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        # the mean interparticle spacing within the half-mass radius (1.3048 scale radii) of a Plummer sphere of n bodies
        spacing = (4.0 / 3.0 * np.pi * 1.3048 ** 3 / (n / 2.0)) ** (1.0 / 3.0)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"pairs": batch.pairs}
            for tag, f in (("0.2", 0.2), ("1.0", 1.0)):
                b = float(np.float32(f * spacing))
                calls["groups_lean_" + tag] = lambda b=b: batch.groups(b, records=False, bodies=False)
                calls["groups_bodies_" + tag] = lambda b=b: batch.groups(b, records=False)
                calls["groups_" + tag] = lambda b=b: batch.groups(b)
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    if name.startswith("groups_lean_"):
                        found[name[len("groups_lean_"):]] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B, "mean_spacing": round(spacing, 5)}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for tag, res in found.items():
            line.update({f"sweeps_mean_{tag}": round(float(res.sweeps.mean()), 3), f"sweeps_max_{tag}": int(res.sweeps.max()),
                         f"converged_{tag}": int(res.converged.sum()), f"groups_mean_{tag}": round(float(res.groups.mean()), 1),
                         f"largest_count_mean_{tag}": round(float(res.largest_count.mean()), 1),
                         f"lean_over_pairs_{tag}": round(med["groups_lean_" + tag] / med["pairs"], 3),
                         f"ms_per_walk_{tag}": round(med["groups_lean_" + tag] / (float(res.sweeps.mean()) + 1.0), 4)})
        line.update({"record_megabytes": round(B * n * 64 / 1e6, 1), "body_megabytes": round(B * n * 8 / 1e6, 1),
                     "system_kilobytes": round(B * 32 / 1e3, 1)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def span_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        spacing = (4.0 / 3.0 * np.pi * 1.3048 ** 3 / (n / 2.0)) ** (1.0 / 3.0)   # as in --groups
        rng = np.random.default_rng(7)
        subset = np.zeros((B, n), np.uint8)
        for s in range(B):
            subset[s, rng.choice(n, size=min(20, n), replace=False)] = 1
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            b = float(np.float32(spacing))
            calls = {"pairs": batch.pairs,
                     "groups_lean": lambda: batch.groups(b, records=False, bodies=False),
                     "span_lean": lambda: batch.spanning_tree(edges=False, bodies=False),
                     "span_lean_separations": lambda: batch.spanning_tree(separations=True, edges=False, bodies=False),
                     "span": lambda: batch.spanning_tree(),
                     "span_subsets_of_20": lambda: batch.spanning_tree(subset=subset, edges=False, bodies=False)}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        tree, sweeps = found["span_lean"], found["groups_lean"].sweeps
        line.update({"rounds_mean": round(float(tree.rounds.mean()), 3), "rounds_max": int(tree.rounds.max()),
                     "rounds_subsets_mean": round(float(found["span_subsets_of_20"].rounds.mean()), 3),
                     "groups_sweeps_mean": round(float(sweeps.mean()), 3),
                     "ms_per_round": round(med["span_lean"] / max(float(tree.rounds.mean()), 1.0), 4),
                     "ms_per_groups_walk": round(med["groups_lean"] / (float(sweeps.mean()) + 1.0), 4),
                     "separations_ms": round(med["span_lean_separations"] - med["span_lean"], 3),
                     "lean_over_pairs": round(med["span_lean"] / med["pairs"], 3),
                     "lean_over_groups_lean": round(med["span_lean"] / med["groups_lean"], 3),
                     "edge_megabytes": round(B * n * 16 / 1e6, 1), "body_megabytes": round(B * n * 8 / 1e6, 1),
                     "system_kilobytes": round(B * 40 / 1e3, 1)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def neighbours_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        spacing = float(np.float32((4.0 / 3.0 * np.pi * 1.3048 ** 3 / (n / 2.0)) ** (1.0 / 3.0)))   # as in --groups
        massive = np.zeros((B, n), np.uint8)
        massive[:, :8] = 1
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"pairs": batch.pairs,
                     "structure_lean_k6": lambda: batch.structure(k=6, bodies=False),
                     "neighbours_lean_k1": lambda: batch.neighbours(k=1, lists=False, bodies=False),
                     "neighbours_lean_k6": lambda: batch.neighbours(k=6, lists=False, bodies=False),
                     "neighbours_lean_k8": lambda: batch.neighbours(k=8, lists=False, bodies=False),
                     "neighbours_lean_k6_radius": lambda: batch.neighbours(k=6, radius=spacing, lists=False, bodies=False),
                     "neighbours_lean_k6_sources_8": lambda: batch.neighbours(k=6, sources=massive, lists=False, bodies=False),
                     "neighbours_k6": lambda: batch.neighbours(k=6, radius=spacing)}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        res = found["neighbours_k6"]
        line.update({"lean_k6_over_structure_lean": round(med["neighbours_lean_k6"] / med["structure_lean_k6"], 3),
                     "lean_k6_over_pairs": round(med["neighbours_lean_k6"] / med["pairs"], 3),
                     "lists_ms": round(med["neighbours_k6"] - med["neighbours_lean_k6_radius"], 3),
                     "pair_walks_per_s": float(f"{B * n * n / (med['neighbours_lean_k6'] * 1e-3):.4g}"),
                     "mutual_fraction": round(float(res.mutual.sum()) / float(res.bodies.sum()), 4),
                     "mean_within": round(float(res.within.mean()), 3),
                     "median_mean_nearest": round(float(np.median(res.mean_nearest)), 5),
                     "median_mean_kth": round(float(np.median(res.mean_kth)), 5),
                     "list_megabytes": round(B * n * 6 * 8 / 1e6, 1), "body_megabytes": round(B * n * 8 / 1e6, 1),
                     "system_kilobytes": round(B * 40 / 1e3, 1)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def correlation_lines():
    import time
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        edges = {bins: np.geomspace(0.02, 5.0, bins + 1).astype(np.float32) for bins in (8, 16, 32)}
        massive = np.zeros((B, n), np.uint8)
        massive[:, :8] = 1
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            calls = {"pairs": batch.pairs,
                     "neighbours_lean_k6": lambda: batch.neighbours(k=6, lists=False, bodies=False),
                     "correlation_lean_8": lambda: batch.correlation(edges[8], counts=False),
                     "correlation_lean_16": lambda: batch.correlation(edges[16], counts=False),
                     "correlation_lean_32": lambda: batch.correlation(edges[32], counts=False),
                     "correlation_lean_32_sources_8": lambda: batch.correlation(edges[32], sources=massive, counts=False),
                     "correlation_32": lambda: batch.correlation(edges[32])}
            for fn in calls.values():                   # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):               # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree")}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        res = found["correlation_32"]
        for bins in (8, 16, 32):
            line[f"lean_{bins}_over_neighbours_lean"] = round(med[f"correlation_lean_{bins}"] / med["neighbours_lean_k6"], 3)
        line.update({"pair_walks_per_s": float(f"{B * n * n / (med['correlation_lean_32'] * 1e-3):.4g}"),
                     "counted_fraction": round(float(res.counts.sum()) / float(res.pairs.sum()), 4),
                     "below_fraction": round(float(res.below.sum()) / float(res.pairs.sum()), 6),
                     "above_fraction": round(float(res.above.sum()) / float(res.pairs.sum()), 6),
                     "fullest_bin_fraction": round(float(res.counts.sum(axis=0).max()) / float(res.pairs.sum()), 4),
                     "count_kilobytes": round(B * 32 * 4 / 1e3, 1), "system_kilobytes": round(B * 48 / 1e3, 1)})
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
            line[name + "_repeats"] = [round(x, 3) for x in times[name]]
        print(json.dumps(line), flush=True)


def contacts_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "256x4096"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        spacing = float(np.float32((4.0 / 3.0 * np.pi * 1.3048 ** 3 / (n / 2.0)) ** (1.0 / 3.0)))   # as in --groups
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"), "mean_spacing": round(spacing, 5)}
            for f in (0.2, 1.0):
                b = float(np.float32(f * spacing))
                half = np.full((B, n), 0.5 * b, np.float32)
                room = int(batch.contacts(b, lists=False, bodies=False).pairs.max())
                calls = {"pairs": batch.pairs,
                         "neighbours_lean_k1_radius": lambda: batch.neighbours(k=1, radius=b, lists=False, bodies=False),
                         "contacts_count": lambda: batch.contacts(b, lists=False, bodies=False),
                         "contacts_list_lean": lambda: batch.contacts(b, capacity=room, bodies=False),
                         "contacts_list": lambda: batch.contacts(b, capacity=room),
                         "contacts_list_lean_radii": lambda: batch.contacts(radii=half, capacity=room, bodies=False)}
                for fn in calls.values():                           # the first calls allocate the records and set the kernels' LDS limits
                    wall(fn)
                times = {name: [] for name in calls}
                found = {}
                for _ in range(args.repeats):                       # alternated
                    for name, fn in calls.items():
                        t, out = wall(fn)
                        times[name].append(t)
                        found[name] = out
                med = {name: statistics.median(ts) for name, ts in times.items()}
                res, tag = found["contacts_list"], f"b{f}"
                line[tag] = {"radius": round(b, 5), "capacity": room, "pairs_per_system": round(float(res.pairs.mean()), 1),
                             "max_degree": int(res.max_degree.max()), "list_megabytes": round(B * room * 12 / 1e6, 2),
                             "list_crc32": zlib.crc32(res.entries.tobytes()),
                             "radii_same_list": bool(found["contacts_list_lean_radii"].entries.tobytes() == res.entries.tobytes())}
                for name in calls:
                    line[tag][name + "_ms"] = round(med[name], 3)
                for name in ("contacts_count", "contacts_list_lean", "contacts_list"):
                    line[tag][name + "_over_neighbours"] = round(med[name] / med["neighbours_lean_k1_radius"], 3)
                for name in calls:
                    line[tag][name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
        print(json.dumps(line), flush=True)


def approaches_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        spacing = float(np.float32((4.0 / 3.0 * np.pi * 1.3048 ** 3 / (n / 2.0)) ** (1.0 / 3.0)))   # as in --contacts
        b = float(np.float32(0.2 * spacing))
        speed = float(np.sqrt((V[..., :3].astype(np.float64) ** 2).sum(axis=-1).mean()))             # the rms speed
        H = float(np.float32(b / speed))
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            room = int(batch.approaches(H, b, lists=False, bodies=False).pairs.max())
            room0 = int(batch.contacts(b, lists=False, bodies=False).pairs.max())
            calls = {"contacts_count": lambda: batch.contacts(b, lists=False, bodies=False),
                     "contacts_list_lean": lambda: batch.contacts(b, capacity=room0, bodies=False),
                     "approaches_count": lambda: batch.approaches(H, b, lists=False, bodies=False),
                     "approaches_list_lean": lambda: batch.approaches(H, b, capacity=room, bodies=False),
                     "approaches_count_h0": lambda: batch.approaches(0.0, b, lists=False, bodies=False),
                     "approaches_list_lean_h0": lambda: batch.approaches(0.0, b, capacity=room0, bodies=False)}
            for fn in calls.values():                               # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):                           # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        res, still, touching = found["approaches_list_lean"], found["approaches_list_lean_h0"], found["contacts_list_lean"]
        for name in ("i", "j", "r2"):                               # the H = 0 list is contacts()' list
            assert getattr(still, name).tobytes() == getattr(touching, name).tobytes(), name
        assert np.array_equal(still.pairs, touching.pairs) and not still.passing.any() and not still.ending.any()
        line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"), "mean_spacing": round(spacing, 5),
                "radius": round(b, 5), "rms_speed": round(speed, 5), "horizon": round(H, 5), "capacity": room, "capacity_h0": room0,
                "pairs_per_system": round(float(res.pairs.mean()), 1), "now_per_system": round(float(res.now_pairs.mean()), 1),
                "passing_per_system": round(float(res.passing.mean()), 1), "ending_per_system": round(float(res.ending.mean()), 1),
                "list_megabytes": round(B * room * 24 / 1e6, 2), "list_crc32": zlib.crc32(res.entries.tobytes()), "h0_is_contacts": True}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for name in ("count", "list_lean"):
            line[f"approaches_{name}_over_contacts"] = round(med[f"approaches_{name}"] / med[f"contacts_{name}"], 3)
            line[f"approaches_{name}_h0_over_contacts"] = round(med[f"approaches_{name}_h0"] / med[f"contacts_{name}"], 3)
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
        print(json.dumps(line), flush=True)


def radial_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        edges = {32: np.geomspace(0.05, 10.0, 33), 8: np.geomspace(0.05, 10.0, 9)}
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            def download_and_bin():
                """What the call replaces: both arrays to the host, then the mass per shell of every system in numpy."""
                p, v = batch.positions.cpu().numpy(), batch.velocities.cpu().numpy()
                x = p[..., :3].astype(np.float64)
                r = np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])
                shell = np.searchsorted(edges[32], r, side="left")                  # 0 below, 1 ... 32 the shells, 33 above
                flat = (np.arange(B)[:, None] * 34 + shell).ravel()
                return np.bincount(flat, weights=p[..., 3].astype(np.float64).ravel(), minlength=B * 34).reshape(B, 34), v

            calls = {"radial32": lambda: batch.radial_profile(edges[32]),
                     "radial32_bodies": lambda: batch.radial_profile(edges[32], bodies=True),
                     "radial32_systems_only": lambda: batch.radial_profile(edges[32], shells=False),
                     "radial8": lambda: batch.radial_profile(edges[8]),
                     "radial8_bodies": lambda: batch.radial_profile(edges[8], bodies=True),
                     "structure_lean": lambda: batch.structure(bodies=False),
                     "download_and_bin": download_and_bin}
            for fn in calls.values():                               # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):                           # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        res, binned = found["radial32"], found["download_and_bin"][0]
        assert np.array_equal(res.count.sum(axis=1) + res.below + res.above + res.unmeasured, res.selected)
        assert np.allclose(res.weight_sum, binned[:, 1:33], rtol=1e-9, atol=1e-12)                 # the same profile, summed in another order
        assert found["radial32_bodies"].shell_records.tobytes() == res.shell_records.tobytes()
        line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"),
                "members_per_system": round(float(res.count.sum(axis=1).mean()), 1),
                "shells_megabytes": round(B * 32 * 192 / 1e6, 3), "bodies_megabytes": round(B * n * 24 / 1e6, 2),
                "download_megabytes": round(2 * B * n * 16 / 1e6, 2), "shells_crc32": zlib.crc32(res.shell_records.tobytes()),
                "shells8_crc32": zlib.crc32(found["radial8"].shell_records.tobytes())}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for name in ("radial32", "radial32_bodies", "radial8"):
            line[name + "_over_structure"] = round(med[name] / med["structure_lean"], 3)
            line[name + "_over_download_and_bin"] = round(med[name] / med["download_and_bin"], 3)
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
        print(json.dumps(line), flush=True)


def surface_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        edges = {side: nb.SurfaceMapResult.grid(2.0, side) for side in (16, 32, 64)}
        shells = np.geomspace(0.05, 10.0, 33)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            def download_and_bin():
                """What the call replaces: both arrays to the host, then the mass per cell of every system, one numpy.histogram2d each."""
                p, v = batch.positions.cpu().numpy(), batch.velocities.cpu().numpy()
                maps = np.empty((B, 64, 64))
                for s in range(B):
                    maps[s] = np.histogram2d(p[s, :, 0], p[s, :, 1], bins=(edges[64], edges[64]), weights=p[s, :, 3])[0].T
                return maps, v

            calls = {}
            for side in (16, 32, 64):
                calls[f"surface{side}"] = lambda side=side: batch.surface_map(edges[side])
                calls[f"surface{side}_systems_only"] = lambda side=side: batch.surface_map(edges[side], cells=False)
            calls["surface64_bodies"] = lambda: batch.surface_map(edges[64], bodies=True)
            calls["radial32"] = lambda: batch.radial_profile(shells)
            calls["pairs"] = batch.pairs
            calls["download_and_bin"] = download_and_bin
            for fn in calls.values():                               # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(args.repeats):                           # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        res, binned = found["surface64"], found["download_and_bin"][0]
        assert np.array_equal(res.count.sum(axis=(1, 2)) + res.outside + res.unmeasured, res.selected)
        p = P.astype(np.float64)
        assert not (p[..., 0] == 2.0).any() and not (p[..., 1] == 2.0).any()                       # nobody on numpy's closed last edge
        assert np.allclose(res.weight_sum, binned, rtol=1e-6, atol=1e-9)                            # numpy bins in fp32 weights, another order
        assert found["surface64_bodies"].cell_records.tobytes() == res.cell_records.tobytes()
        assert found["surface64_systems_only"].systems.tobytes() == res.systems.tobytes()
        line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"),
                "members_per_system": round(float(res.count.sum(axis=(1, 2)).mean()), 1),
                "occupied_per_system": round(float(res.occupied.mean()), 1), "peak_count_per_system": round(float(res.peak_count.mean()), 1),
                "cells64_megabytes": round(B * 4096 * 64 / 1e6, 2), "bodies_megabytes": round(B * n * 24 / 1e6, 2),
                "download_megabytes": round(2 * B * n * 16 / 1e6, 2), "cells64_crc32": zlib.crc32(res.cell_records.tobytes()),
                "cells16_crc32": zlib.crc32(found["surface16"].cell_records.tobytes())}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for name in ("surface16", "surface32", "surface64", "surface64_systems_only", "surface64_bodies"):
            line[name + "_over_download_and_bin"] = round(med[name] / med["download_and_bin"], 4)
            line[name + "_over_radial32"] = round(med[name] / med["radial32"], 3)
            line[name + "_over_pairs"] = round(med[name] / med["pairs"], 3)
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
        print(json.dumps(line), flush=True)


def host_shape(x, w, radius, tol=1e-3, max_iterations=64, min_members=10):
    """The iteration of include/nbody_batch_shape.h for one system and one aperture as numpy would be asked to do it on the
    host: the reduced tensor by einsum, numpy.linalg.eigh, no pinned order.  Returns q, s and the passes made."""
    axes, w2, w3, q0, s0 = np.eye(3), 1.0, 1.0, 1.0, 1.0
    out2 = radius * radius
    for k in range(1, max_iterations + 1):
        y = x @ axes.T
        r2e = y[:, 0] ** 2 + w2 * y[:, 1] ** 2 + w3 * y[:, 2] ** 2
        inside = (r2e > 0.0) & (r2e <= out2)
        if inside.sum() < min_members:
            break
        xi = x[inside]
        values, vectors = np.linalg.eigh(np.einsum("i,ia,ib->ab", w[inside] / r2e[inside], xi, xi))
        if not values[0] > 0.0:
            break
        q, s = np.sqrt(values[1] / values[2]), np.sqrt(values[0] / values[2])
        axes, w2, w3 = vectors[:, ::-1].T, values[2] / values[1], values[2] / values[0]
        done = abs(q - q0) <= tol * q0 and abs(s - s0) <= tol * s0
        q0, s0 = q, s
        if done:
            break
    return q0, s0, k


def shape_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    repeats = max(args.repeats, 15)
    radii = np.array([0.5, 1.0, 2.0, 4.0])
    shells = np.geomspace(0.05, 10.0, 33)
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        P[:, :, :3] *= np.array([1.0, 0.7, 0.4], dtype=np.float32)   # Plummer spheres flattened to 1 : 0.7 : 0.4
        few = min(args.subset, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            def download():
                return batch.positions.cpu().numpy(), batch.velocities.cpu().numpy()

            def host_iteration():
                """The host's part of what the call replaces, on the first `few` systems only: four apertures each."""
                return [[host_shape(P[s, :, :3].astype(np.float64), P[s, :, 3].astype(np.float64), R) for R in radii] for s in range(few)]

            calls = {"shape4": lambda: batch.shape(radii),
                     "shape4_bodies": lambda: batch.shape(radii, bodies=True),
                     "shape4_systems_only": lambda: batch.shape(radii, apertures=False),
                     "radial32": lambda: batch.radial_profile(shells),
                     "download": download,
                     "host_iteration_subset": host_iteration}
            for fn in calls.values():                               # the first calls allocate the records and set the kernels' LDS limits
                wall(fn)
            times = {name: [] for name in calls}
            found = {}
            for _ in range(repeats):                                # alternated
                for name, fn in calls.items():
                    t, out = wall(fn)
                    times[name].append(t)
                    found[name] = out
            med = {name: statistics.median(ts) for name, ts in times.items()}
        res, host = found["shape4"], found["host_iteration_subset"]
        assert found["shape4_bodies"].aperture_records.tobytes() == res.aperture_records.tobytes()
        assert found["shape4_systems_only"].systems.tobytes() == res.systems.tobytes()
        for s in range(few):                                        # the same shapes, summed in another order
            for a in range(len(radii)):
                if res.status[s, a] == 0:
                    assert abs(res.q[s, a] - host[s][a][0]) < 1e-2 and abs(res.s[s, a] - host[s][a][1]) < 1e-2, (s, a)
        # measured: the download of the whole batch and the host iteration of `few` systems; the product with B is extrapolated
        replaced = med["download"] + med["host_iteration_subset"] * B / few
        line = {"n": n, "B": B, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"), "apertures": len(radii), "repeats": repeats,
                "status_counts": np.bincount(res.status.ravel(), minlength=4).tolist(),
                "passes_mean": round(float(res.iterations.mean()), 2), "passes_of_the_slowest_system": int(res.iterations.max()),
                "q_mean": round(float(res.q[res.status == 0].mean()), 4), "s_mean": round(float(res.s[res.status == 0].mean()), 4),
                "apertures_megabytes": round(B * len(radii) * 256 / 1e6, 3), "bodies_megabytes": round(B * n * 8 / 1e6, 2),
                "download_megabytes": round(2 * B * n * 16 / 1e6, 2), "apertures_crc32": zlib.crc32(res.aperture_records.tobytes()),
                "host_systems_timed": few, "host_iteration_ms_per_system": round(med["host_iteration_subset"] / few, 3),
                "replaced_ms_extrapolated_to_B": round(replaced, 2)}
        for name in calls:
            line[name + "_ms"] = round(med[name], 3)
        for name in ("shape4", "shape4_bodies", "shape4_systems_only"):
            line[name + "_over_replaced"] = round(med[name] / replaced, 5)
            line[name + "_over_download"] = round(med[name] / med["download"], 4)
            line[name + "_over_radial32"] = round(med[name] / med["radial32"], 3)
        for name in calls:
            line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
        print(json.dumps(line), flush=True)


def host_pair_walk(p, v, edges):
    """What pair_velocities() replaces, for one system: all ordered pairs in numpy, nine weighted histograms."""
    x, u = p[:, :3].astype(np.float64), v[:, :3].astype(np.float64)
    d, w = x[None, :, :] - x[:, None, :], u[None, :, :] - u[:, None, :]
    keep = ~np.eye(len(x), dtype=bool)
    s, rv, v2 = (d * d).sum(-1)[keep], (d * w).sum(-1)[keep], (w * w).sum(-1)[keep]
    r = np.sqrt(s)
    vr = rv / r
    words = (np.ones_like(r), r, s, rv, vr, vr * vr, np.maximum(v2 - vr * vr, 0.0), np.sqrt(v2), v2)
    return np.stack([np.histogram(r, bins=edges, weights=word)[0] for word in words], axis=1)


def pair_velocities_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    terms = ("weight", "r1", "r2", "rv", "vr1", "vr2", "vt2", "v1", "v2")
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        few = min(args.subset, B)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            for bins in (8, 32):
                edges = np.geomspace(0.05, 10.0, bins + 1).astype(np.float32)

                def download():
                    return batch.positions.cpu().numpy(), batch.velocities.cpu().numpy()

                def host_walk():
                    """The host's part of what the call replaces, on the first `few` systems only."""
                    return [host_pair_walk(P[s], V[s], edges.astype(np.float64)) for s in range(few)]

                calls = {"lean": lambda: batch.pair_velocities(edges, bins=False),
                         "records": lambda: batch.pair_velocities(edges),
                         "correlation": lambda: batch.correlation(edges),
                         "download": download,
                         "host_walk_subset": host_walk}
                for name, fn in calls.items():                      # the first calls allocate the records and set the kernels' LDS limits
                    if name != "host_walk_subset":
                        wall(fn)
                times = {name: [] for name in calls}
                found = {}
                for round_ in range(args.repeats):                  # alternated; the numpy walk, seconds long and on no GPU, once
                    for name, fn in calls.items():
                        if name == "host_walk_subset" and round_ > 0:
                            continue
                        t, out = wall(fn)
                        times[name].append(t)
                        found[name] = out
                med = {name: statistics.median(ts) for name, ts in times.items()}
                res, host = found["records"], found["host_walk_subset"]
                assert found["lean"].systems.tobytes() == res.systems.tobytes()
                assert np.array_equal(res.count, found["correlation"].counts) and np.array_equal(res.above, found["correlation"].above)
                for s in range(few):                                # the same sums in another order; pairs on an edge's rounding aside
                    if np.array_equal(host[s][:, 0], res.count[s]):
                        for c, word in enumerate(terms):
                            scale = np.abs(host[s][:, c]) + host[s][:, 8] + host[s][:, 2]
                            assert (np.abs(res.bin_records[word][s] - host[s][:, c]) <= 1e-9 * scale).all(), (s, word)
                replaced = med["download"] + med["host_walk_subset"] * B / few
                line = {"n": n, "B": B, "bins": bins, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"), "repeats": args.repeats,
                        "pairs_in_bins_share": round(float(res.count.sum() / res.pairs.sum()), 4),
                        "records_megabytes": round(B * bins * 96 / 1e6, 3), "download_megabytes": round(2 * B * n * 16 / 1e6, 2),
                        "records_crc32": zlib.crc32(res.bin_records.tobytes()), "host_systems_timed": few,
                        "host_walk_ms_per_system": round(med["host_walk_subset"] / few, 3),
                        "replaced_ms_extrapolated_to_B": round(replaced, 2)}
                for name in calls:
                    line[name + "_ms"] = round(med[name], 3)
                for name in ("lean", "records"):
                    line[name + "_over_correlation"] = round(med[name] / med["correlation"], 3)
                    line[name + "_over_replaced"] = round(med[name] / replaced, 6)
                for name in calls:
                    line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
                print(json.dumps(line), flush=True)


def host_mutual_walk(p, v, labels, sets, eps):
    """What mutual_gravity() replaces, for one system: all ordered pairs in numpy, summed by the sets of row and source."""
    x, u, m = p[:, :3].astype(np.float64), v[:, :3].astype(np.float64), p[:, 3].astype(np.float64)
    d = x[None, :, :] - x[:, None, :]
    s2 = (d * d).sum(-1) + eps * eps
    np.fill_diagonal(s2, np.inf)
    inv = 1.0 / np.sqrt(s2)
    phi = m[None, :] * inv
    acc = (phi * inv * inv)[:, :, None] * d
    out = np.zeros((sets, sets, 9))
    for b in range(sets):
        source = labels == b
        P, f = phi[:, source].sum(1), m[:, None] * acc[:, source].sum(1)
        words = np.concatenate([(-m * P)[:, None], f, np.cross(x, f), (x * f).sum(1)[:, None], (u * f).sum(1)[:, None]], axis=1)
        for a in range(sets):
            out[a, b] = words[labels == a].sum(0)
    return out


def mutual_gravity_lines():
    import time
    import zlib
    cases = args.cases if args.cases != [f"{n}x{b}" for n, b in CASES] else ["1024x1024", "4096x256", "256x4096"]
    for case in cases:
        n, B = (int(x) for x in case.lower().split("x"))
        P, V = ensemble(n, B)
        few = min(args.subset, B)
        edges = np.geomspace(0.05, 10.0, 9).astype(np.float32)
        with nb.BatchedSystem(B, n) as batch:
            batch.set_state(P, V)

            def wall(fn):
                batch.sync()
                t0 = time.perf_counter()
                out = fn()
                return (time.perf_counter() - t0) * 1e3, out

            for sets in (2, 8):
                labels = np.tile(np.arange(n) % sets, (B, 1))

                def download():
                    return batch.positions.cpu().numpy(), batch.velocities.cpu().numpy()

                def host_walk():
                    """The host's part of what the call replaces, on the first `few` systems only."""
                    return [host_mutual_walk(P[s], V[s], labels[s], sets, args.eps) for s in range(few)]

                calls = {"matrix": lambda: batch.mutual_gravity(labels, sets=sets, softening=args.eps),
                         "lean": lambda: batch.mutual_gravity(labels, sets=sets, softening=args.eps, matrix=False),
                         "pair_velocities8": lambda: batch.pair_velocities(edges),
                         "download": download,
                         "host_walk_subset": host_walk}
                for name, fn in calls.items():                      # the first calls allocate the records and set the kernels' LDS limits
                    if name != "host_walk_subset":
                        wall(fn)
                times = {name: [] for name in calls}
                found = {}
                for round_ in range(args.repeats):                  # alternated; the numpy walk, seconds long and on no GPU, once
                    for name, fn in calls.items():
                        if name == "host_walk_subset" and round_ > 0:
                            continue
                        t, out = wall(fn)
                        times[name].append(t)
                        found[name] = out
                med = {name: statistics.median(ts) for name, ts in times.items()}
                res, host = found["matrix"], found["host_walk_subset"]
                assert found["lean"].systems.tobytes() == res.systems.tobytes()
                assert (res.selected == n).all() and int(res.total_pairs[0]) == n * (n - 1)
                for s in range(few):                                # the same sums in another order
                    got = np.concatenate([res.potential[s][..., None], res.force[s], res.torque[s], res.virial[s][..., None],
                                          res.power[s][..., None]], axis=-1)
                    scale = np.abs(host[s][:, :, :1]) * (1.0 + np.abs(P[s, :, :3]).max() + np.abs(V[s, :, :3]).max()) / args.eps
                    assert (np.abs(got - host[s]) <= 1e-9 * scale).all(), s
                replaced = med["download"] + med["host_walk_subset"] * B / few
                pairs = float(res.total_pairs.sum())
                line = {"n": n, "B": B, "sets": sets, "softening": args.eps, "library": os.environ.get("NBODY_AMD_LIBRARY", "in-tree"),
                        "repeats": args.repeats, "pairs": int(pairs), "pairs_per_ns_matrix": round(pairs / (med["matrix"] * 1e6), 3),
                        "matrix_megabytes": round(B * sets * sets * 80 / 1e6, 3), "download_megabytes": round(2 * B * n * 16 / 1e6, 2),
                        "matrix_crc32": zlib.crc32(res.entries.tobytes()), "host_systems_timed": few,
                        "host_walk_ms_per_system": round(med["host_walk_subset"] / few, 3),
                        "replaced_ms_extrapolated_to_B": round(replaced, 2)}
                for name in calls:
                    line[name + "_ms"] = round(med[name], 3)
                for name in ("matrix", "lean"):
                    line[name + "_over_pair_velocities8"] = round(med[name] / med["pair_velocities8"], 3)
                    line[name + "_over_replaced"] = round(med[name] / replaced, 6)
                for name in calls:
                    line[name + "_spread"] = round((max(times[name]) - min(times[name])) / med[name], 4)
                print(json.dumps(line), flush=True)


if args.mutual_gravity:
    mutual_gravity_lines()
    sys.exit(0)
if args.pair_velocities:
    pair_velocities_lines()
    sys.exit(0)
if args.shape:
    shape_lines()
    sys.exit(0)
if args.surface:
    surface_lines()
    sys.exit(0)
if args.radial:
    radial_lines()
    sys.exit(0)
if args.approaches:
    approaches_lines()
    sys.exit(0)
if args.contacts:
    contacts_lines()
    sys.exit(0)
if args.correlation:
    correlation_lines()
    sys.exit(0)
if args.neighbours:
    neighbours_lines()
    sys.exit(0)
if args.span:
    span_lines()
    sys.exit(0)
if args.groups:
    groups_lines()
    sys.exit(0)
if args.gravity:
    gravity_lines()
    sys.exit(0)
if args.hierarchy:
    hierarchy_lines()
    sys.exit(0)
if args.members:
    members_lines()
    sys.exit(0)
if args.structure:
    structure_lines()
    sys.exit(0)
if args.pairs:
    pairs_lines()
    sys.exit(0)
if args.field:
    field_lines()
    sys.exit(0)
if args.accrete:
    accrete_lines()
    sys.exit(0)
if args.massive:
    massive_lines()
    sys.exit(0)
if args.fates:
    fates_lines()
    sys.exit(0)
if args.radii:
    radii_lines()
    sys.exit(0)
if args.adaptive:
    adaptive_lines()
    sys.exit(0)
if args.merges:
    merges_lines()
    sys.exit(0)
if args.stops:
    stops_lines()
    sys.exit(0)

for case in args.cases:
    n, B = (int(x) for x in case.lower().split("x"))
    P, V = ensemble(n, B)
    inter = B * n * n
    k = int(min(400, max(10, 2e11 // inter)))   # ~60 ms per batched call at 3e12 interactions/s
    for integrator in args.integrators:
        batch = nb.BatchedSystem(B, n, integrator=integrator)
        batch.set_state(P, V)
        subset = min(args.subset, B) if integrator != "hermite" else 0
        singles = []
        for s in range(subset):
            one = nb.NBodySystem(n)
            one.set_force_mode("auto")          # the faster force mode at this size (the pair-once kernels at every size)
            one.set_integrator(integrator)
            one.setParticlesPosition(P[s])
            one.setParticlesVelocity(V[s])
            singles.append(one)
        k_single = max(5, k // 4)

        def run_batch():
            batch.step_n(k, args.dt, args.eps)

        def run_singles():
            for one in singles:
                one.step_n(k_single, args.dt, args.eps)

        run_batch()
        run_singles()
        torch.cuda.synchronize()
        tb, ts = [], []
        for _ in range(args.repeats):          # alternated
            tb.append(timed(run_batch) / k)
            if singles:
                ts.append(timed(run_singles) / k_single * B / subset)
        batch.sync()
        ms = statistics.median(tb)
        rate = inter / (ms * 1e-3)
        flop = FLOP_PER_INTERACTION[integrator]
        line = {
            "n": n, "B": B, "integrator": integrator, "k": k, "ms_per_step": round(ms, 5),
            "ms_per_step_repeats": [round(x, 5) for x in tb],
            "interactions_per_s": float(f"{rate:.4g}"),
            "flop_per_interaction": flop,
            "frac_of_fp32_peak": round(flop * rate / PEAK_FP32, 4)}
        if ts:
            ms_sq = statistics.median(ts)
            line.update({
                "status_quo_ms_per_step": round(ms_sq, 4), "status_quo_systems_timed": subset, "status_quo_k": k_single,
                "status_quo_interactions_per_s": float(f"{inter / (ms_sq * 1e-3):.4g}"),
                "speedup_vs_status_quo": round(ms_sq / ms, 1)})
        print(json.dumps(line), flush=True)
        batch.close()
        for one in singles:
            one.close()
