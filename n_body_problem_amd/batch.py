"""Batched ensembles: many independent small systems stepped together, one launch per call (``nbody_batch_*`` of
``include/nbody.h``, kernels in ``csrc/nbody_batch.hip`` and ``csrc/nbody_batch_analysis.hip``, the integrators' host code in
``csrc/nbody_batch_capi.hip``).

One :class:`NBodySystem` below a few thousand bodies cannot fill the GPU: its step is ~0.02 ms of launch overhead.  A
:class:`BatchedSystem` holds ``B`` systems of up to ``max_bodies`` (at most :data:`BATCH_MAX_BODIES`) bodies each -- system
``s`` has ``counts[s]`` bodies -- and steps them all in one workgroup per system, ``k`` steps per launch.  A system's result
depends on that system alone (its slot, ``B``, ``max_bodies`` and the other systems change no bit).  Device memory and the
stream come from PyTorch-ROCm; the arithmetic is the HIP kernels'.  There is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import NBodyError
from .system import SOFTENING_VERSION3, TIME_TICK, _ptr, _torch

#: NBODY_BATCH_MAX_BODIES: the largest system a batch holds (64 KiB of positions in LDS); larger ones belong to NBodySystem
BATCH_MAX_BODIES = 4096
INTEGRATORS = {"kick_drift": 0, "kdk": 1, "hermite": 2}
COLLISION_ACTIONS = {"stop": _lib.BATCH_ON_COLLISION_STOP, "merge": _lib.BATCH_ON_COLLISION_MERGE}
TRACER_ACTIONS = {"refuse": _lib.BATCH_TRACERS_REFUSE, "remove": _lib.BATCH_TRACERS_REMOVE}
HIT_ACTIONS = {"remove": _lib.BATCH_ON_HIT_REMOVE, "accrete": _lib.BATCH_ON_HIT_ACCRETE}
FIELD_KINDS = {"none": _lib.BATCH_FIELD_NONE, "plummer": _lib.BATCH_FIELD_PLUMMER, "log_halo": _lib.BATCH_FIELD_LOG_HALO,
               "miyamoto_nagai": _lib.BATCH_FIELD_MIYAMOTO_NAGAI}
#: one merger of the log: numpy's view of ``nbody_batch_merge_event``
MERGE_EVENT_DTYPE = np.dtype([("tick", np.int64), ("survivor", np.int32), ("absorbed", np.int32), ("count_before", np.int32),
                              ("separation", np.float32), ("relative_speed", np.float32), ("mass_survivor", np.float32),
                              ("mass_absorbed", np.float32), ("reserved", np.int32)])
assert MERGE_EVENT_DTYPE.itemsize == ctypes.sizeof(_lib.BatchMergeEvent)
#: one record of :meth:`BatchedSystem.pairs`: numpy's view of ``nbody_batch_pair_record``
PAIR_RECORD_DTYPE = np.dtype([("partner", np.int32), ("mutual", np.int32), ("energy", np.float64), ("semi_major_axis", np.float64),
                              ("eccentricity", np.float64), ("inclination", np.float64), ("separation", np.float64)])
assert PAIR_RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BatchPairRecord) == 48
#: the records of :meth:`BatchedSystem.structure`: numpy's views of ``nbody_batch_structure_body`` and ``_system``
STRUCTURE_BODY_DTYPE = np.dtype([("density", np.float64), ("radius", np.float64), ("enclosed", np.float64), ("neighbour_r2", np.float32),
                                 ("neighbour_weight", np.float32), ("inside", np.int32), ("reserved", np.int32)])
STRUCTURE_SYSTEM_DTYPE = np.dtype([("centre", np.float64, 3), ("core_radius", np.float64), ("core_density", np.float64),
                                   ("total_weight", np.float64), ("lagrange", np.float64, 8), ("estimated", np.int32),
                                   ("reserved", np.int32)])
assert STRUCTURE_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchStructureBody) == 40
assert STRUCTURE_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchStructureSystem) == 120
#: the records of :meth:`BatchedSystem.members`: numpy's views of ``nbody_batch_member_body`` and ``_system``
MEMBER_BODY_DTYPE = np.dtype([("potential", np.float64), ("energy", np.float64), ("member", np.int32), ("removed_at", np.int32)])
MEMBER_SYSTEM_DTYPE = np.dtype([("bound_mass", np.float64), ("centre", np.float64, 3), ("velocity", np.float64, 3),
                                ("kinetic", np.float64), ("potential", np.float64), ("members", np.int32), ("sources", np.int32),
                                ("iterations", np.int32), ("converged", np.int32)])
assert MEMBER_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchMemberBody) == 24
assert MEMBER_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchMemberSystem) == 88
#: the records of :meth:`BatchedSystem.hierarchy`: numpy's views of ``nbody_batch_hierarchy_node``, ``_body`` and ``_system``
HIERARCHY_NODE_DTYPE = np.dtype([("child", np.int32, 2), ("parent", np.int32), ("level", np.int32), ("leaves", np.int32),
                                 ("slot", np.int32), ("stable", np.int32), ("reserved", np.int32), ("mass", np.float64),
                                 ("energy", np.float64), ("semi_major_axis", np.float64), ("eccentricity", np.float64),
                                 ("inclination", np.float64), ("separation", np.float64), ("perturbation", np.float64),
                                 ("mutual_inclination", np.float64, 2), ("h", np.float64, 3)])
HIERARCHY_BODY_DTYPE = np.dtype([("parent", np.int32), ("root", np.int32), ("depth", np.int32), ("reserved", np.int32)])
HIERARCHY_SYSTEM_DTYPE = np.dtype([(name, np.int32) for name in ("nodes", "roots", "levels", "converged", "singles", "binaries",
                                                                 "triples", "higher", "unstable", "reserved")])
assert HIERARCHY_NODE_DTYPE.itemsize == ctypes.sizeof(_lib.BatchHierarchyNode) == 128
assert HIERARCHY_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchHierarchyBody) == 16
assert HIERARCHY_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchHierarchySystem) == 40
#: one record of :meth:`BatchedSystem.gravity_at`: numpy's view of ``nbody_batch_gravity_record``
GRAVITY_RECORD_DTYPE = np.dtype([("acceleration", np.float32, 3), ("reserved", np.float32), ("potential", np.float64)])
assert GRAVITY_RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BatchGravityRecord) == 24
#: the records of :meth:`BatchedSystem.groups`: numpy's views of ``nbody_batch_group_body``, ``_record`` and ``_system``
GROUP_BODY_DTYPE = np.dtype([("group", np.int32), ("size", np.int32)])
GROUP_RECORD_DTYPE = np.dtype([("weight", np.float64), ("centre", np.float64, 3), ("velocity", np.float64, 3),
                               ("count", np.int32), ("sources", np.int32)])
GROUP_SYSTEM_DTYPE = np.dtype([(name, np.int32) for name in ("groups", "grouped", "singles", "largest", "largest_count", "sweeps",
                                                             "converged", "reserved")])
assert GROUP_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchGroupBody) == 8
assert GROUP_RECORD_DTYPE.itemsize == ctypes.sizeof(_lib.BatchGroupRecord) == 64
assert GROUP_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchGroupSystem) == 32
#: the records of :meth:`BatchedSystem.spanning_tree`: numpy's views of ``nbody_batch_span_system``, ``_edge`` and ``_body``
SPAN_SYSTEM_DTYPE = np.dtype([("edges", np.int32), ("selected", np.int32), ("rounds", np.int32), ("reserved", np.int32),
                              ("total_length", np.float64), ("longest", np.float64), ("mean_separation", np.float64)])
SPAN_EDGE_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("r2", np.float32), ("reserved", np.int32)])
SPAN_BODY_DTYPE = np.dtype([("degree", np.int32), ("nearest", np.int32)])
assert SPAN_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSpanSystem) == 40
assert SPAN_EDGE_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSpanEdge) == 16
assert SPAN_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSpanBody) == 8
#: the records of :meth:`BatchedSystem.neighbours`: numpy's views of ``nbody_batch_neighbour_system`` and ``_body``
NEIGHBOUR_SYSTEM_DTYPE = np.dtype([("bodies", np.int32), ("sources", np.int32), ("listed", np.int32), ("complete", np.int32),
                                   ("mutual", np.int32), ("reserved", np.int32), ("mean_nearest", np.float64),
                                   ("mean_kth", np.float64)])
NEIGHBOUR_BODY_DTYPE = np.dtype([("found", np.int32), ("within", np.int32)])
assert NEIGHBOUR_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchNeighbourSystem) == 40
assert NEIGHBOUR_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchNeighbourBody) == 8
#: the record of :meth:`BatchedSystem.correlation`: numpy's view of ``nbody_batch_correlation_system``
CORRELATION_SYSTEM_DTYPE = np.dtype([("rows", np.int32), ("sources", np.int32), ("both", np.int32), ("bins", np.int32),
                                     ("pairs", np.int64), ("below", np.int64), ("above", np.int64), ("unmeasured", np.int64)])
assert CORRELATION_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchCorrelationSystem) == 48
#: the records of :meth:`BatchedSystem.contacts`: numpy's views of ``nbody_batch_contact_system``, ``_body`` and ``nbody_batch_contact``
CONTACT_SYSTEM_DTYPE = np.dtype([("bodies", np.int32), ("touching", np.int32), ("max_degree", np.int32), ("reserved", np.int32),
                                 ("pairs", np.int64), ("stored", np.int64), ("closest_i", np.int32), ("closest_j", np.int32),
                                 ("closest_r2", np.float32), ("reserved2", np.int32)])
CONTACT_BODY_DTYPE = np.dtype([("degree", np.int32), ("upper", np.int32), ("first", np.int32), ("nearest", np.int32)])
CONTACT_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("r2", np.float32)])
assert CONTACT_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchContactSystem) == 48
assert CONTACT_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchContactBody) == 16
assert CONTACT_DTYPE.itemsize == ctypes.sizeof(_lib.BatchContact) == 12
#: the records of :meth:`BatchedSystem.approaches`: numpy's views of ``nbody_batch_approach_system``, ``_body`` and ``nbody_batch_approach``
APPROACH_SYSTEM_DTYPE = np.dtype([("bodies", np.int32), ("approaching", np.int32), ("max_degree", np.int32), ("reserved", np.int32),
                                  ("pairs", np.int64), ("stored", np.int64), ("now", np.int32), ("passing", np.int32),
                                  ("ending", np.int32), ("reserved2", np.int32)])
APPROACH_BODY_DTYPE = np.dtype([("degree", np.int32), ("upper", np.int32), ("first", np.int32), ("now", np.int32)])
APPROACH_DTYPE = np.dtype([("i", np.int32), ("j", np.int32), ("r2", np.float32), ("rv", np.float32), ("v2", np.float32),
                           ("phase", np.int32)])
assert APPROACH_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchApproachSystem) == 48
assert APPROACH_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchApproachBody) == 16
assert APPROACH_DTYPE.itemsize == ctypes.sizeof(_lib.BatchApproach) == 24
#: the records of :meth:`BatchedSystem.radial_profile`: numpy's views of ``nbody_batch_radial_system``, ``_shell`` and ``_body``
RADIAL_SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("below", np.int32), ("above", np.int32), ("unmeasured", np.int32),
                                ("shells", np.int32), ("projected", np.int32), ("total_weight", np.float64),
                                ("centre", np.float64, 3), ("velocity", np.float64, 3)])
RADIAL_SHELL_DTYPE = np.dtype([("count", np.int64), ("weight", np.float64), ("radius", np.float64), ("vr1", np.float64),
                               ("vr2", np.float64), ("vt2", np.float64), ("L", np.float64, 3), ("U", np.float64, 3),
                               ("M", np.float64, 6), ("V", np.float64, 6)])
RADIAL_BODY_DTYPE = np.dtype([("shell", np.int32), ("reserved", np.int32), ("radius", np.float64), ("radial_velocity", np.float64)])
assert RADIAL_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchRadialSystem) == 80
assert RADIAL_SHELL_DTYPE.itemsize == ctypes.sizeof(_lib.BatchRadialShell) == 192
assert RADIAL_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchRadialBody) == 24
#: the records of :meth:`BatchedSystem.surface_map`: numpy's views of ``nbody_batch_surface_system``, ``_cell`` and ``_body``
SURFACE_SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("outside", np.int32), ("unmeasured", np.int32), ("columns", np.int32),
                                 ("rows", np.int32), ("occupied", np.int32), ("peak", np.int32), ("peak_count", np.int32),
                                 ("total_weight", np.float64), ("centre", np.float64, 3), ("velocity", np.float64, 3)])
SURFACE_CELL_DTYPE = np.dtype([("count", np.int64), ("weight", np.float64), ("v1", np.float64), ("v2", np.float64),
                               ("pa", np.float64), ("pb", np.float64), ("z1", np.float64), ("z2", np.float64)])
SURFACE_BODY_DTYPE = np.dtype([("cell", np.int32), ("reserved", np.int32), ("a", np.float64), ("b", np.float64)])
assert SURFACE_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSurfaceSystem) == 88
assert SURFACE_CELL_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSurfaceCell) == 64
assert SURFACE_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchSurfaceBody) == 24
#: the weight of a body in :meth:`BatchedSystem.structure` and :meth:`BatchedSystem.groups`: its mass word, or 1#: the records of :meth:`BatchedSystem.shape`: numpy's views of ``nbody_batch_shape_system``, ``_aperture`` and ``_body``
SHAPE_SYSTEM_DTYPE = np.dtype([("selected", np.int32), ("unmeasured", np.int32), ("apertures", np.int32), ("reduced", np.int32),
                               ("converged", np.int32), ("reserved", np.int32), ("total_weight", np.float64),
                               ("centre", np.float64, 3), ("velocity", np.float64, 3)])
SHAPE_APERTURE_DTYPE = np.dtype([("status", np.int32), ("iterations", np.int32), ("count", np.int64), ("radius", np.float64),
                                 ("inner", np.float64), ("q", np.float64), ("s", np.float64), ("change", np.float64),
                                 ("eigenvalues", np.float64, 3), ("axes", np.float64, 9), ("weight", np.float64),
                                 ("D", np.float64, 3), ("M", np.float64, 6), ("L", np.float64, 3)])
SHAPE_BODY_DTYPE = np.dtype([("inside", np.uint32), ("reserved", np.int32)])
assert SHAPE_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchShapeSystem) == 80
assert SHAPE_APERTURE_DTYPE.itemsize == ctypes.sizeof(_lib.BatchShapeAperture) == 256
assert SHAPE_BODY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchShapeBody) == 8
#: the records of :meth:`BatchedSystem.pair_velocities`: numpy's views of ``nbody_batch_pair_velocities_system`` and ``_bin``
PAIR_VELOCITIES_SYSTEM_DTYPE = np.dtype([("rows", np.int32), ("sources", np.int32), ("both", np.int32), ("bins", np.int32),
                                         ("weight", np.int32), ("reserved", np.int32), ("pairs", np.int64), ("below", np.int64),
                                         ("above", np.int64), ("unmeasured", np.int64)])
PAIR_VELOCITIES_BIN_DTYPE = np.dtype([("count", np.int64), ("approaching", np.int64), ("receding", np.int64)] +
                                     [(name, np.float64) for name in ("weight", "r1", "r2", "rv", "vr1", "vr2", "vt2", "v1", "v2")])
assert PAIR_VELOCITIES_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchPairVelocitiesSystem) == 56
assert PAIR_VELOCITIES_BIN_DTYPE.itemsize == ctypes.sizeof(_lib.BatchPairVelocitiesBin) == 96
#: the records of :meth:`BatchedSystem.mutual_gravity`: numpy's views of ``nbody_batch_mutual_gravity_system`` and ``_entry``
MUTUAL_GRAVITY_SYSTEM_DTYPE = np.dtype([("sets", np.int32), ("selected", np.int32), ("left_out", np.int32), ("unmeasured", np.int32),
                                        ("pairs", np.int64), ("coincident", np.int64), ("members", np.int32, 8), ("mass", np.float64, 8)])
MUTUAL_GRAVITY_ENTRY_DTYPE = np.dtype([("pairs", np.int64), ("potential", np.float64), ("force", np.float64, 3), ("torque", np.float64, 3),
                                       ("virial", np.float64), ("power", np.float64)])
assert MUTUAL_GRAVITY_SYSTEM_DTYPE.itemsize == ctypes.sizeof(_lib.BatchMutualGravitySystem) == 128
assert MUTUAL_GRAVITY_ENTRY_DTYPE.itemsize == ctypes.sizeof(_lib.BatchMutualGravityEntry) == 80

WEIGHTS = {"mass": _lib.BATCH_WEIGHT_MASS, "number": _lib.BATCH_WEIGHT_NUMBER}


def _check(lib, status: int, handle) -> None:
    if status != _lib.NBODY_OK:
        msg = lib.nbody_batch_last_error(handle) or b""
        raise NBodyError(status, msg.decode("utf-8", "replace") or lib.nbody_status_string(status).decode())


class BatchedSystem:
    """``num_systems`` independent systems of up to ``max_bodies`` bodies on one GPU.

    ``positions`` / ``velocities`` are ``(B, max_bodies, 4)`` float32 device tensors used by the kernels in place (zero
    copy): ``positions[s, i] = {x, y, z, mass}``, ``velocities[s, i] = {vx, vy, vz, w}`` (``w`` preserved).  Slots
    ``i >= counts[s]`` are never read or written.  ``integrator``: ``"kick_drift"`` (the reference's scheme, first order),
    ``"kdk"`` (velocity Verlet, second order, with the accelerations cached across calls) or ``"hermite"`` (the
    fourth-order Hermite predictor-corrector of direct-summation codes such as NBODY6: one force-and-jerk evaluation per
    step, about twice a force evaluation, with the accelerations and jerks cached across calls; ``nbody.h`` states the
    scheme).  :meth:`step_n` takes a fixed step shared by all systems; :meth:`evolve` (Hermite only) gives every system
    its own adaptive step and brings all of them to a common time.
    """

    def __init__(self, num_systems: int, max_bodies: int, device: int = 0, counts=None, integrator: str = "kick_drift"):
        if integrator not in INTEGRATORS:
            raise ValueError(f"integrator must be one of {tuple(INTEGRATORS)}")
        self._lib = _lib.load()
        self._h = ctypes.c_void_p(None)
        h = ctypes.c_void_p(None)
        _check(self._lib, self._lib.nbody_batch_create(ctypes.byref(h), int(device), int(num_systems), int(max_bodies)), None)
        self._h = h
        torch = _torch()
        if not torch.cuda.is_available():
            self.close()
            raise NBodyError(_lib.NBODY_ERR_NO_DEVICE, "no HIP device visible to PyTorch; there is no CPU path")
        self.num_systems, self.max_bodies = int(num_systems), int(max_bodies)
        self.device = torch.device("cuda", int(device))
        self.positions = torch.zeros((self.num_systems, self.max_bodies, 4), dtype=torch.float32, device=self.device)
        self.velocities = torch.zeros_like(self.positions)
        self._counts = np.full(self.num_systems, self.max_bodies, dtype=np.int64)
        self.integrator = "kick_drift"
        self._log_capacity = 0
        self.set_integrator(integrator)
        if counts is not None:
            self.set_counts(counts)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nbody_batch_destroy(self._h)
            self._h = ctypes.c_void_p(None)

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _use_current_stream(self) -> None:
        s = _torch().cuda.current_stream(self.device).cuda_stream
        _check(self._lib, self._lib.nbody_batch_set_stream(self._h, ctypes.c_void_p(s)), self._h)

    # -- configuration -----------------------------------------------------------------------
    @property
    def counts(self) -> np.ndarray:
        """Bodies per system (a copy); :meth:`evolve` refreshes them, since mergers lower them."""
        return self._counts.copy()

    def _refresh_counts(self) -> None:
        c = np.zeros(self.num_systems, dtype=np.int64)
        _check(self._lib, self._lib.nbody_batch_get_counts(self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), self._h)
        self._counts = c

    def set_counts(self, counts) -> None:
        """``B`` body counts in ``[0, max_bodies]``; forgets the cached accelerations (and Hermite jerks)."""
        c = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
        if c.shape[0] != self.num_systems:
            raise ValueError(f"expected {self.num_systems} counts, got {c.shape[0]}")
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_set_counts(self._h, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), self._h)
        self._counts = c.copy()

    def set_integrator(self, name: str) -> None:
        """``"kick_drift"``, ``"kdk"`` or ``"hermite"``; a change forgets the cached accelerations (and jerks)."""
        if name not in INTEGRATORS:
            raise ValueError(f"integrator must be one of {tuple(INTEGRATORS)}")
        _check(self._lib, self._lib.nbody_batch_set_integrator(self._h, INTEGRATORS[name]), self._h)
        self.integrator = name

    def invalidate_forces(self) -> None:
        """Forget the cached accelerations of KDK and Hermite, and Hermite's jerks (after editing ``positions`` or
        ``velocities`` in place: the next step evaluates them afresh)."""
        _check(self._lib, self._lib.nbody_batch_invalidate_forces(self._h), self._h)

    # -- state -------------------------------------------------------------------------------
    def set_state(self, pos, vel, counts=None) -> None:
        """Copy ``(B, n, 4)`` positions and velocities (numpy or torch, ``n <= max_bodies``) into slots ``[0, n)`` of every
        system; ``counts`` (optional) sets the body counts first.  Every count must be at most ``n``.  Forgets the cached
        accelerations and jerks."""
        torch = _torch()
        p = torch.as_tensor(np.asarray(pos) if not isinstance(pos, torch.Tensor) else pos, dtype=torch.float32)
        v = torch.as_tensor(np.asarray(vel) if not isinstance(vel, torch.Tensor) else vel, dtype=torch.float32)
        if p.dim() != 3 or p.shape[0] != self.num_systems or p.shape[2] != 4 or p.shape[1] > self.max_bodies:
            raise ValueError(f"positions must have shape ({self.num_systems}, n <= {self.max_bodies}, 4), got {tuple(p.shape)}")
        if tuple(v.shape) != tuple(p.shape):
            raise ValueError(f"velocities must have the shape of the positions {tuple(p.shape)}, got {tuple(v.shape)}")
        if counts is not None:
            self.set_counts(counts)
        n = p.shape[1]
        if int(self._counts.max(initial=0)) > n:
            raise ValueError(f"a system has more bodies ({int(self._counts.max())}) than set_state provides ({n}): set_counts first")
        self._use_current_stream()
        self.positions[:, :n].copy_(p.to(self.device), non_blocking=False)
        self.velocities[:, :n].copy_(v.to(self.device), non_blocking=False)
        self.invalidate_forces()

    def download(self):
        """``(positions, velocities)`` as ``(B, max_bodies, 4)`` float32 numpy arrays (waits for the queued steps)."""
        self._use_current_stream()
        self.sync()
        return self.positions.cpu().numpy(), self.velocities.cpu().numpy()

    # -- stepping ----------------------------------------------------------------------------
    def step_n(self, k: int, dt: float = TIME_TICK, softening: float = SOFTENING_VERSION3) -> None:
        """``k`` steps of every system, enqueued on torch's current stream (one launch per 128 steps)."""
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_step_n_async(self._h, _ptr(self.positions), _ptr(self.velocities), int(k),
                                                             float(dt), float(softening)), self._h)

    def evolve(self, n_intervals: int, dt_max: float, levels: int = 12, eta: float = 0.01, eta_start: float = 0.01,
               softening: float = SOFTENING_VERSION3, max_steps: int = 0) -> "EvolveResult":
        """Advance every system by ``n_intervals * dt_max``, each on its own step ``dt_max * 2**-L`` (``0 <= L <= levels``)
        chosen after every step from Aarseth's criterion with accuracy parameter ``eta`` (``eta_start``: the first step);
        Hermite batches only, ``include/nbody_batch_evolve.h`` states the scheme.  Time is counted in integer ticks of
        ``dt_max * 2**-levels``, so every system lands on the end time exactly.  ``max_steps`` bounds every system's steps
        in this call (``0``: the library's default); when a system runs out, :class:`NBodyError` with
        ``NBODY_ERR_STATE`` is raised, :meth:`evolve_stats` tells where each system stands, and the same call again
        continues.  Returns with the work complete."""
        self._use_current_stream()
        cfg = _lib.BatchEvolveConfig(float(dt_max), int(levels), float(eta), float(eta_start), float(softening), int(max_steps))
        status = self._lib.nbody_batch_evolve_on(self._h, _ptr(self.positions), _ptr(self.velocities), int(n_intervals),
                                                 ctypes.byref(cfg))
        self._refresh_counts()  # also after a call that ran out of steps: its mergers have happened
        _check(self._lib, status, self._h)
        return self.evolve_stats()

    def evolve_stats(self) -> "EvolveResult":
        """Per-system figures of the last :meth:`evolve` call (also after one that ran out of steps)."""
        B = self.num_systems
        steps, clamped, ticks = (np.zeros(B, dtype=np.int64) for _ in range(3))
        lo, hi = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        i64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)
        _check(self._lib, self._lib.nbody_batch_evolve_stats(self._h, steps.ctypes.data_as(i64), lo.ctypes.data_as(i32),
                                                             hi.ctypes.data_as(i32), clamped.ctypes.data_as(i64),
                                                             ticks.ctypes.data_as(i64)), self._h)
        return EvolveResult(steps, lo, hi, clamped, ticks)

    def set_evolve_launch_steps(self, steps_per_launch: int) -> None:
        """Steps one launch of :meth:`evolve` takes per system at most (default 128); results do not depend on it."""
        _check(self._lib, self._lib.nbody_batch_evolve_launch_steps(self._h, int(steps_per_launch)), self._h)

    def set_stop_conditions(self, collision_radius: float = 0.0, escape_radius: float = 0.0) -> None:
        """Stopping conditions of :meth:`evolve` (``include/nbody_batch_stop.h`` states them): a system's run ends after the
        step in which two of its bodies come within ``collision_radius`` of each other, or a body is farther than
        ``escape_radius`` from the coordinate origin (centre the systems); ``0`` switches a condition off, both ``0`` (the
        default) all of it.  With per-body radii (:meth:`set_radii`) collisions are judged by those instead and
        ``collision_radius`` must stay ``0``: :meth:`evolve` refuses both together.  A stop is a result, not an error:
        :meth:`stops` tells which systems stopped, when and which bodies; a stopped system stays frozen in later
        :meth:`evolve` calls.  Forgets earlier stops and the cached accelerations and jerks (as :meth:`set_state`,
        :meth:`invalidate_forces` and :meth:`step_n` forget the stops)."""
        cfg = _lib.BatchStopConfig(float(collision_radius), float(escape_radius))
        _check(self._lib, self._lib.nbody_batch_stop_set(self._h, ctypes.byref(cfg)), self._h)

    def stops(self) -> "StopResult":
        """What the stopping conditions found, per system (waits for the queued work)."""
        B = self.num_systems
        reason, pi, pj, esc = (np.zeros(B, dtype=np.int32) for _ in range(4))
        ticks, sep = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float32)
        i32 = ctypes.POINTER(ctypes.c_int)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_stop_read(self._h, reason.ctypes.data_as(i32),
                                                          ticks.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                          pi.ctypes.data_as(i32), pj.ctypes.data_as(i32),
                                                          sep.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                          esc.ctypes.data_as(i32)), self._h)
        return StopResult(reason, ticks, np.stack([pi, pj], axis=1), sep, esc)

    def set_collision_action(self, action: str = "stop", log_capacity: int = 8) -> None:
        """What :meth:`evolve` does with a collision (``include/nbody_batch_merge.h`` states the rules): ``"stop"`` (the
        default) ends the system's run as :meth:`set_stop_conditions` describes; ``"merge"`` merges the colliding pair --
        the mass is the sum, position and velocity the mass-weighted means, the survivor keeps the lower slot, the absorbed
        body's last state moves to the first slot beyond the count -- lowers :attr:`counts` by one, evaluates the system
        afresh and carries the run on.  :meth:`mergers` tells how many mergers each system had and logs the first
        ``log_capacity`` of them.  Acts while a collision radius or per-body radii (:meth:`set_radii`) are set; with radii
        the merged body's radius is ``cbrt(R_i**3 + R_j**3)`` and the radii move with their bodies.  Forgets stops, the log
        and the cached accelerations and jerks, as :meth:`set_stop_conditions` does."""
        if action not in COLLISION_ACTIONS:
            raise ValueError(f"action must be one of {tuple(COLLISION_ACTIONS)}")
        cfg = _lib.BatchMergeConfig(COLLISION_ACTIONS[action], int(log_capacity))
        _check(self._lib, self._lib.nbody_batch_merge_set(self._h, ctypes.byref(cfg)), self._h)
        self._log_capacity = int(log_capacity)

    def set_radii(self, radii) -> None:
        """Per-body collision radii of :meth:`evolve` (``include/nbody_batch_radii.h`` states the rules): ``(B, n)``, numpy or
        torch, ``n <= max_bodies``, one radius ``>= 0`` per slot (slots from ``n`` on get ``0``); ``None`` switches them off.
        With radii set two bodies collide when they come within the sum of their radii, whether or not a collision radius is
        set (both together are refused by :meth:`evolve`); the collision action is :meth:`set_collision_action`'s, and a
        merged body's radius is ``cbrt(R_i**3 + R_j**3)``.  Radii belong to the slots: :meth:`set_state` and
        :meth:`set_counts` leave them alone.  The shape is checked here, the values by the library (negative or non-finite
        below a system's count: :class:`NBodyError`).  Forgets stops, the merger log and the cached accelerations and
        jerks, as :meth:`set_stop_conditions` does."""
        if radii is None:
            _check(self._lib, self._lib.nbody_batch_radii_set(self._h, None), self._h)
            return
        if hasattr(radii, "detach"):  # a torch tensor
            radii = radii.detach().cpu().numpy()
        r = np.asarray(radii, dtype=np.float32)
        if r.ndim != 2 or r.shape[0] != self.num_systems or r.shape[1] > self.max_bodies:
            raise ValueError(f"radii must have shape ({self.num_systems}, n <= {self.max_bodies}), got {tuple(r.shape)}")
        full = np.zeros((self.num_systems, self.max_bodies), dtype=np.float32)
        full[:, :r.shape[1]] = r
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_radii_set(self._h, full.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._h)

    def radii(self) -> np.ndarray:
        """The radii as the library left them, ``(B, max_bodies)`` float32 (waits for the queued work): after mergers the
        survivors have grown and the absorbed bodies' radii lie with their last states beyond the counts.  Raises
        :class:`NBodyError` (``NBODY_ERR_STATE``) when no radii are set."""
        out = np.zeros((self.num_systems, self.max_bodies), dtype=np.float32)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_radii_read(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))), self._h)
        return out

    def set_massive_counts(self, massive) -> None:
        """Test particles (``include/nbody_batch_massive.h`` states the rules): ``B`` integers in ``[0, max_bodies]``, or
        ``None`` to switch the feature off (the default).  The first ``min(massive[s], counts[s])`` bodies of system ``s``
        are massive; the bodies after them feel the massive ones and exert no force.  They are stepped like any other body
        by :meth:`step_n` (every integrator) and :meth:`evolve`, and count in its time-step criterion, but no body receives
        a force from them, at ``n * m`` interactions per step instead of ``n * n``.  Their mass words
        ``positions[s, i, 3]`` are read by no force kernel and are preserved; :meth:`energy` and :meth:`momentum` keep
        reading them, so zero mass words give the massive bodies' energy.  The values belong to the handle:
        :meth:`set_state` and :meth:`set_counts` leave them alone.  With the default tracer action :meth:`evolve` refuses
        massive counts together with stopping conditions or radii; :meth:`set_tracer_action` ``"remove"`` runs them, and
        :meth:`set_hit_action` says what a hit does to the body hit.  The length is checked here, the values by the
        library.  Forgets what :meth:`set_counts` forgets: the cached accelerations and jerks, the levels and the stops."""
        self._use_current_stream()
        if massive is None:
            _check(self._lib, self._lib.nbody_batch_massive_set(self._h, None), self._h)
            return
        m = np.ascontiguousarray(np.asarray(massive).reshape(-1), dtype=np.int64)
        if m.shape[0] != self.num_systems:
            raise ValueError(f"expected {self.num_systems} massive counts, got {m.shape[0]}")
        _check(self._lib, self._lib.nbody_batch_massive_set(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), self._h)

    @property
    def massive_counts(self):
        """The massive counts as they were set (a copy), or ``None`` while the feature is off."""
        m = np.zeros(self.num_systems, dtype=np.int64)
        status = self._lib.nbody_batch_massive_read(self._h, m.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
        if status == _lib.NBODY_ERR_STATE:
            return None
        _check(self._lib, status, self._h)
        return m

    def set_tracer_action(self, action: str = "refuse") -> None:
        """What :meth:`evolve` does with massive counts (:meth:`set_massive_counts`) together with stopping conditions or
        radii (``include/nbody_batch_fate.h`` states the rules): ``"refuse"`` (the default) refuses the call, as
        :meth:`set_massive_counts` says; ``"remove"`` runs it.  A test particle that comes within the collision radius (or
        the sum of the two radii) of a massive body, or leaves the escape radius, is then removed from that step on: frozen
        where it is, with a fate that :meth:`fates` reports, while its system carries on.  A collision between two massive
        bodies or a massive escaper stops the system as :meth:`set_stop_conditions` describes.  The collision action
        ``"merge"`` stays refused together with massive counts.  Without massive counts ``"remove"`` changes nothing.
        Forgets stops, fates and the cached accelerations and jerks, as :meth:`set_stop_conditions` does."""
        if action not in TRACER_ACTIONS:
            raise ValueError(f"action must be one of {tuple(TRACER_ACTIONS)}")
        cfg = _lib.BatchFateConfig(TRACER_ACTIONS[action])
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_fate_set(self._h, ctypes.byref(cfg)), self._h)

    def fates(self) -> "FateResult":
        """What became of the test particles, per body (waits for the queued work).  Raises :class:`NBodyError`
        (``NBODY_ERR_STATE``) while the tracer action is ``"refuse"``."""
        B, n = self.num_systems, self.max_bodies
        fate, target = np.zeros((B, n), dtype=np.int32), np.zeros((B, n), dtype=np.int32)
        ticks = np.zeros((B, n), dtype=np.int64)
        sep, speed = np.zeros((B, n), dtype=np.float32), np.zeros((B, n), dtype=np.float32)
        hit, escaped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        i32, i64, f32 = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_fate_read(self._h, fate.ctypes.data_as(i32), ticks.ctypes.data_as(i64),
                                                          target.ctypes.data_as(i32), sep.ctypes.data_as(f32),
                                                          speed.ctypes.data_as(f32)), self._h)
        _check(self._lib, self._lib.nbody_batch_fate_count(self._h, hit.ctypes.data_as(i64), escaped.ctypes.data_as(i64)), self._h)
        return FateResult(fate, ticks, target, sep, speed, hit, escaped)

    def set_hit_action(self, action: str = "remove") -> None:
        """What a test particle's hit does to the massive body it hits, where :meth:`set_tracer_action` ``"remove"`` acts and
        collisions are watched (``include/nbody_batch_accrete.h`` states the rules): ``"remove"`` (the default) leaves the
        body as it is; ``"accrete"`` merges the tracer's mass word ``positions[s, i, 3]`` into it -- the mass is the sum,
        position and velocity the mass-weighted means, with radii the body's radius becomes ``cbrt(R_t**3 + R_i**3)`` --
        zeroes the tracer's mass word, evaluates the system afresh and carries the run on; a tracer with a zero mass word
        is removed as before.  Slots and counts do not change.  :meth:`accretions` tells what every tracer gave.  With an
        escape radius alone or without massive counts ``"accrete"`` changes nothing.  Forgets stops, fates, accretions and
        the cached accelerations and jerks, as :meth:`set_stop_conditions` does."""
        if action not in HIT_ACTIONS:
            raise ValueError(f"action must be one of {tuple(HIT_ACTIONS)}")
        cfg = _lib.BatchAccreteConfig(HIT_ACTIONS[action])
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_accrete_set(self._h, ctypes.byref(cfg)), self._h)

    def accretions(self) -> "AccretionResult":
        """What the test particles gave the bodies they hit (waits for the queued work).  Raises :class:`NBodyError`
        (``NBODY_ERR_STATE``) while the hit action is ``"remove"``."""
        given = np.zeros((self.num_systems, self.max_bodies), dtype=np.float32)
        count = np.zeros(self.num_systems, dtype=np.int64)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_accrete_read(self._h, given.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                             count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), self._h)
        return AccretionResult(given, count)

    def set_external_field(self, components) -> None:
        """A static background potential centred on the origin, felt by every body of :meth:`evolve` next to the pair forces
        (``include/nbody_batch_field.h`` states the formulas and the fp32 operation order): the sum of up to four
        components, ``G = 1``.  ``components`` is a list of ``(kind, p0, p1, p2)`` applied to every system, ``kind`` one of
        ``"plummer"`` ``(M, b, -)``, ``"log_halo"`` ``(v0, rc, q)``, ``"miyamoto_nagai"`` ``(M, a, b)`` or ``"none"``
        (skipped); or an array ``(B, C, 4)`` with a numeric kind (``FIELD_KINDS``) in ``[..., 0]``, one set per system; or
        ``None`` to switch the field off (the default).  The field counts in the time-step criterion; it reads no mass
        word, so test particles (:meth:`set_massive_counts`) feel it like any other body.  A Plummer term is bit for bit a
        body of mass ``M`` fixed at the origin with softening ``b``.  :meth:`evolve` takes the field with or without
        massive counts (``levels=0`` gives fixed steps) and refuses it together with stopping conditions, radii, mergers
        or tracer fates; :meth:`step_n` refuses it.  The shape is checked here, the values by the library
        (:class:`NBodyError`).  Forgets what :meth:`set_massive_counts` forgets."""
        self._use_current_stream()
        if components is None:
            _check(self._lib, self._lib.nbody_batch_field_set(self._h, None, 0), self._h)
            return
        if isinstance(components, (list, tuple)) and all(isinstance(c, (list, tuple)) and len(c) > 0 and isinstance(c[0], str)
                                                         for c in components):
            rows = []
            for c in components:
                if c[0] not in FIELD_KINDS:
                    raise ValueError(f"field kind must be one of {tuple(FIELD_KINDS)}, got {c[0]!r}")
                p = [float(u) for u in c[1:]]
                if len(p) > 3:
                    raise ValueError(f"a field component has at most three parameters, got {c!r}")
                rows.append([float(FIELD_KINDS[c[0]])] + p + [0.0] * (3 - len(p)))
            arr = np.broadcast_to(np.asarray(rows, dtype=np.float64).reshape(1, len(rows), 4), (self.num_systems, len(rows), 4))
        else:
            arr = np.asarray(components, dtype=np.float64)
        if arr.ndim != 3 or arr.shape[0] != self.num_systems or arr.shape[2] != 4:
            raise ValueError(f"field components must have shape ({self.num_systems}, C, 4), got {tuple(arr.shape)}")
        kinds = arr[..., 0]
        if not np.all(np.isfinite(kinds)) or not np.all(kinds == np.round(kinds)):
            raise ValueError("field kinds (components[..., 0]) must be integers")
        C = arr.shape[1]
        buf = (_lib.BatchFieldComponent * (self.num_systems * C))()
        for s in range(self.num_systems):
            for c in range(C):
                u = buf[s * C + c]
                u.kind = int(kinds[s, c])
                u.p[0], u.p[1], u.p[2] = (float(np.float32(v)) for v in arr[s, c, 1:])
        _check(self._lib, self._lib.nbody_batch_field_set(self._h, buf, int(C)), self._h)

    def external_field(self):
        """The field's components as they were set, ``(B, C, 4)`` float32 with the kind in ``[..., 0]``, or ``None`` while no
        field is set."""
        buf = (_lib.BatchFieldComponent * (self.num_systems * _lib.BATCH_FIELD_MAX_COMPONENTS))()
        n = ctypes.c_int(0)
        status = self._lib.nbody_batch_field_read(self._h, buf, ctypes.byref(n))
        if status == _lib.NBODY_ERR_STATE:
            return None
        _check(self._lib, status, self._h)
        C = n.value
        out = np.zeros((self.num_systems, C, 4), dtype=np.float32)
        for s in range(self.num_systems):
            for c in range(C):
                u = buf[s * C + c]
                out[s, c] = (u.kind, u.p[0], u.p[1], u.p[2])
        return out

    def field_potential(self) -> np.ndarray:
        """``(B, max_bodies)`` float64: the field's potential at every body's position (fp64 from the fp32 positions and
        parameters; 0 beyond the counts and while no field is set; waits for the queued work)."""
        out = np.zeros((self.num_systems, self.max_bodies), dtype=np.float64)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_field_potential(self._h, _ptr(self.positions),
                                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), self._h)
        return out

    def field_energy(self) -> np.ndarray:
        """``(B,)`` float64: per system the sum of mass word times field potential over its bodies -- the field's part of the
        energy, which :meth:`energy` (the pair energy) does not contain."""
        phi = self.field_potential()
        m = self.positions[:, :, 3].cpu().numpy().astype(np.float64)
        live = np.arange(self.max_bodies)[None, :] < self._counts[:, None]
        return np.where(live, m * phi, 0.0).sum(axis=1)

    def mergers(self) -> "MergeResult":
        """The mergers so far, per system (waits for the queued work)."""
        B, cap = self.num_systems, self._log_capacity
        count = np.zeros(B, dtype=np.int64)
        events = np.zeros((B, cap), dtype=MERGE_EVENT_DTYPE)
        self._use_current_stream()
        ev = events.ctypes.data_as(ctypes.POINTER(_lib.BatchMergeEvent)) if cap > 0 else None
        _check(self._lib, self._lib.nbody_batch_merge_read(self._h, count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ev), self._h)
        return MergeResult(count, events)

    def pairs(self) -> "PairResult":
        """Every body's partner and the orbital elements of the pair (``include/nbody_batch_pairs.h`` states the rules), found
        on the device from the current state (waits for the queued work).  The partner of body ``i`` is the body ``j`` of
        its system with the smallest two-body energy ``v_ij**2 / 2 - (m_i + m_j) / r_ij`` (``G = 1``, no softening); with
        massive counts (:meth:`set_massive_counts`) only massive bodies are partners and a test particle's own mass word
        does not count.  The search runs in fp32, the elements of the chosen pair in fp64.  Changes nothing: an
        :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        rec = np.zeros((self.num_systems, self.max_bodies), dtype=PAIR_RECORD_DTYPE)
        binaries = np.zeros(self.num_systems, dtype=np.int64)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_pairs(self._h, _ptr(self.positions), _ptr(self.velocities),
                                                      rec.ctypes.data_as(ctypes.POINTER(_lib.BatchPairRecord))), self._h)
        _check(self._lib, self._lib.nbody_batch_pairs_binaries(self._h, binaries.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               self._h)
        return PairResult(rec, binaries)

    def structure(self, k: int = 6, weight: str = "mass", fractions=(0.1, 0.5, 0.9), bodies: bool = True) -> "StructureResult":
        """How every system is built (``include/nbody_batch_structure.h`` states the rules), found on the device from the
        current positions (waits for the queued work): every body's density from its ``k``-th neighbour (Casertano & Hut's
        unbiased estimator, ``1 <= k <= 8``), and per system the density centre, the core radius and density, and the
        Lagrangian radii about the centre that enclose the given ``fractions`` (up to eight, each in ``(0, 1]``) of the
        total weight.  ``weight``: ``"mass"`` (the mass words) or ``"number"`` (every body weighs 1, so that test particles
        count).  All ``counts[s]`` bodies of a system take part, whatever the massive counts.  ``bodies=False`` skips the 40
        bytes per body on their way to the host: the per-body arrays of the result are ``None``, the per-system ones the same
        bits.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")
        f = np.ascontiguousarray(np.asarray(fractions, dtype=np.float64).reshape(-1))
        systems = np.zeros(self.num_systems, dtype=STRUCTURE_SYSTEM_DTYPE)
        rec = np.zeros((self.num_systems, self.max_bodies), dtype=STRUCTURE_BODY_DTYPE) if bodies else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_structure(
            self._h, _ptr(self.positions), int(k), WEIGHTS[weight],
            f.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if f.size else None, int(f.size),
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchStructureSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchStructureBody)) if bodies else None), self._h)
        return StructureResult(systems, rec, f, int(k), weight, self.counts)

    def members(self, softening: float, max_iterations: int = 32, initial=None, bodies: bool = True) -> "MemberResult":
        """Which bodies still belong to their system, and how much mass that is (``include/nbody_batch_members.h`` states the
        rules): iterative unbinding on the device from the current state (waits for the queued work).  Every body's
        potential from the member sources (fp32 pair terms as :meth:`energy` forms them, fp64 sums) and its energy in their
        centre-of-mass frame; the bodies with energy ``>= 0`` leave; again with the survivors until nothing changes or
        ``max_iterations`` (1 ... 64) are done.  With massive counts (:meth:`set_massive_counts`) only massive bodies are
        sources; test particles can be members and their mass words are not read.  ``initial``: a ``(B, max_bodies)`` bool
        or uint8 array that picks the starting set, or ``None`` for every body.  The criterion is the self-gravity of the
        set alone: an external field is not part of it.  ``bodies=False`` skips the 24 bytes per body on their way to the
        host: the per-body arrays of the result are ``None``, the per-system ones the same bits.  Changes nothing: an
        :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        init = None
        if initial is not None:
            init = np.ascontiguousarray(np.asarray(initial))
            if init.dtype != np.bool_ and init.dtype != np.uint8:
                raise ValueError(f"initial must be bool or uint8, not {init.dtype}")
            if init.shape != (self.num_systems, self.max_bodies):
                raise ValueError(f"initial must have shape ({self.num_systems}, {self.max_bodies}), got {tuple(init.shape)}")
            init = init.view(np.uint8)
        systems = np.zeros(self.num_systems, dtype=MEMBER_SYSTEM_DTYPE)
        rec = np.zeros((self.num_systems, self.max_bodies), dtype=MEMBER_BODY_DTYPE) if bodies else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_members(
            self._h, _ptr(self.positions), _ptr(self.velocities), float(softening), int(max_iterations),
            init.ctypes.data_as(ctypes.c_void_p) if init is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchMemberSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchMemberBody)) if bodies else None), self._h)
        return MemberResult(systems, rec, self._source_mass())

    def hierarchy(self, tidal_tolerance: float = np.inf, max_levels: int = 8, nodes: bool = True,
                  bodies: bool = True) -> "HierarchyResult":
        """What every system has become, as nested bound pairs such as ``[[0 1] 2] 3`` (``include/nbody_batch_hierarchy.h``
        states the rules), found on the device from the current state (waits for the queued work).  Level by level the live
        roots look for partners as :meth:`pairs` does; two roots that choose each other, are bound, and whose worst
        perturber's tide at apocentre is at most ``tidal_tolerance`` of their own attraction become a node with the merged
        body's state, and the search runs again, ``max_levels`` (1 ... 16) times at the most.  Nested pairs are judged by the
        stability criterion of Mardling & Aarseth (2001).  With massive counts (:meth:`set_massive_counts`) only massive
        bodies are leaves.  ``nodes=False`` and ``bodies=False`` skip the 128 and 16 bytes per slot on their way to the host:
        those arrays of the result are ``None``, the per-system ones the same bits.  Changes nothing: an :meth:`evolve` after
        it is bit for bit the :meth:`evolve` without it."""
        systems = np.zeros(self.num_systems, dtype=HIERARCHY_SYSTEM_DTYPE)
        node = np.zeros((self.num_systems, self.max_bodies), dtype=HIERARCHY_NODE_DTYPE) if nodes else None
        body = np.zeros((self.num_systems, self.max_bodies), dtype=HIERARCHY_BODY_DTYPE) if bodies else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_hierarchy(
            self._h, _ptr(self.positions), _ptr(self.velocities), float(tidal_tolerance), int(max_levels),
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchHierarchySystem)),
            node.ctypes.data_as(ctypes.POINTER(_lib.BatchHierarchyNode)) if nodes else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchHierarchyBody)) if bodies else None), self._h)
        return HierarchyResult(systems, node, body, self.counts)

    def gravity_at(self, points=None, softening: float = SOFTENING_VERSION3, tidal: bool = False,
                   point_counts=None) -> "GravityResult":
        """The field of every system at its own bodies or at sample points (``include/nbody_batch_gravity.h`` states the
        rules), summed on the device from the current state (waits for the queued work): the acceleration (the fp32 pair
        terms and chains of the step kernels, so the bits a ``kick_drift`` step uses), the potential (:meth:`members`' fp32
        terms in fp64 sums) and, with ``tidal``, the tidal tensor ``T_ab = d a_a / d x_b``.  ``points=None``: the rows are the
        bodies of every system, test particles included, each skipping itself, and ``P = max_bodies``.  Otherwise ``points``
        is ``(B, P, 3)`` or ``(B, P, 4)`` (a fourth word is ignored), numpy or torch, with ``1 <= P <= 1048576``; a float32
        device tensor of shape ``(B, P, 4)`` is used in place.  ``point_counts``: ``B`` values in ``[0, P]`` for ragged point
        sets, or ``None`` for ``P`` everywhere.  With massive counts (:meth:`set_massive_counts`) only massive bodies are
        sources.  An external field (:meth:`set_external_field`) is not part of it.  Changes nothing: an :meth:`evolve` after
        it is bit for bit the :meth:`evolve` without it."""
        torch = _torch()
        B = self.num_systems
        dev, P = None, self.max_bodies
        if points is not None:
            p = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
            if p.dim() != 3 or p.shape[0] != B or p.shape[2] not in (3, 4) or p.shape[1] < 1:
                raise ValueError(f"points must have shape ({B}, P >= 1, 3) or ({B}, P >= 1, 4), got {tuple(p.shape)}")
            P = int(p.shape[1])
            if p.shape[2] == 4 and p.dtype == torch.float32 and p.device == self.device and p.is_contiguous():
                dev = p                                            # in place
            else:
                dev = torch.zeros((B, P, 4), dtype=torch.float32, device=self.device)
                dev[:, :, :p.shape[2]].copy_(p.to(device=self.device, dtype=torch.float32))
        pc = None
        if point_counts is not None:
            pc = np.ascontiguousarray(np.asarray(point_counts).reshape(-1), dtype=np.int64)
            if pc.shape[0] != B:
                raise ValueError(f"expected {B} point counts, got {pc.shape[0]}")
        rec = np.zeros((B, P), dtype=GRAVITY_RECORD_DTYPE)
        tid = np.zeros((B, P, 6), dtype=np.float32) if tidal else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_gravity(
            self._h, _ptr(self.positions), _ptr(dev) if dev is not None else None, P if dev is not None else 0,
            pc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) if pc is not None else None, float(softening),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchGravityRecord)),
            tid.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if tidal else None), self._h)
        return GravityResult(rec, tid)

    def groups(self, linking_length, min_members: int = 2, weight: str = "mass", max_sweeps: int = _lib.BATCH_GROUPS_MAX_SWEEPS,
               records: bool = True, bodies: bool = True) -> "BatchGroups":
        """Into which pieces every system has fallen (``include/nbody_batch_groups.h`` states the rules): friends-of-friends
        groups on the device from the current state (waits for the queued work).  Two bodies are friends where their fp32
        distance is at most ``linking_length`` (a scalar, or ``B`` values, one per system); a group is a connected set of
        friends, named by the lowest index among its members.  All bodies link, test particles included; with massive counts
        (:meth:`set_massive_counts`) and ``weight="mass"`` only massive bodies weigh, and the tracers' mass words are not read;
        ``weight="number"`` weighs every body 1.  ``min_members`` sets which groups ``groups`` and ``grouped`` count and
        :meth:`BatchGroups.groups_of` lists; the labels and records do not depend on it.  ``max_sweeps`` (1 ... 64) bounds the
        label sweeps; a handful converge.  ``records=False`` and ``bodies=False`` skip the 64 bytes per slot and the 8 bytes
        per body on their way to the host: those arrays of the result are ``None``, the per-system ones the same bits.  Changes
        nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")
        b = np.asarray(linking_length, dtype=np.float32)
        if b.ndim == 0:
            b = np.full(self.num_systems, b, dtype=np.float32)
        b = np.ascontiguousarray(b.reshape(-1))
        if b.shape[0] != self.num_systems:
            raise ValueError(f"expected one linking length or {self.num_systems}, got {b.shape[0]}")
        systems = np.zeros(self.num_systems, dtype=GROUP_SYSTEM_DTYPE)
        rec = np.zeros((self.num_systems, self.max_bodies), dtype=GROUP_RECORD_DTYPE) if records else None
        body = np.zeros((self.num_systems, self.max_bodies), dtype=GROUP_BODY_DTYPE) if bodies else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_groups(
            self._h, _ptr(self.positions), _ptr(self.velocities), b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
            int(min_members), WEIGHTS[weight], int(max_sweeps), systems.ctypes.data_as(ctypes.POINTER(_lib.BatchGroupSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchGroupRecord)) if records else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchGroupBody)) if bodies else None), self._h)
        return BatchGroups(systems, rec, body, b, int(min_members), weight)

    def spanning_tree(self, subset=None, separations: bool = False, edges: bool = True, bodies: bool = True) -> "SpanResult":
        """The Euclidean minimum spanning tree of every system (``include/nbody_batch_span.h`` states the rules), found on the
        device from the current state (waits for the queued work).  All bodies below the count are vertices, test particles
        included; ``subset``, a ``(B, max_bodies)`` bool or uint8 array, selects the vertices of each system instead.  Edges are
        ordered by their fp32 squared length, ties by the lower first and then the lower second index, so the tree is unique
        and its edges come sorted: cut those longer than ``b`` and the pieces are :meth:`groups` at ``b``.
        ``separations=True`` also gives the mean separation of the selected bodies, which :meth:`SpanResult.q_parameter`
        needs, for one more pass over the pairs.  ``edges=False`` and ``bodies=False`` skip the 16 bytes per slot and the 8
        bytes per body on their way to the host: those arrays of the result are ``None``, the per-system ones the same bits.
        Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        sub = None
        if subset is not None:
            sub = np.ascontiguousarray(np.asarray(subset))
            if sub.dtype != np.bool_ and sub.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {sub.dtype}")
            if sub.shape != (self.num_systems, self.max_bodies):
                raise ValueError(f"subset must have shape ({self.num_systems}, {self.max_bodies}), got {tuple(sub.shape)}")
            sub = sub.view(np.uint8)
        systems = np.zeros(self.num_systems, dtype=SPAN_SYSTEM_DTYPE)
        edge = np.zeros((self.num_systems, self.max_bodies), dtype=SPAN_EDGE_DTYPE) if edges else None
        body = np.zeros((self.num_systems, self.max_bodies), dtype=SPAN_BODY_DTYPE) if bodies else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_span(
            self._h, _ptr(self.positions), sub.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if sub is not None else None,
            1 if separations else 0, systems.ctypes.data_as(ctypes.POINTER(_lib.BatchSpanSystem)),
            edge.ctypes.data_as(ctypes.POINTER(_lib.BatchSpanEdge)) if edges else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchSpanBody)) if bodies else None), self._h)
        vertices = np.arange(self.max_bodies)[None, :] < np.asarray(self.counts).reshape(-1, 1)
        if sub is not None:
            vertices = vertices & (sub != 0)
        return SpanResult(systems, edge, body, bool(separations), vertices)

    def neighbours(self, k: int = 6, radius=None, sources=None, lists: bool = True, bodies: bool = True) -> "NeighbourResult":
        """Who is next to whom (``include/nbody_batch_neighbours.h`` states the rules): for every body of every system the
        indices and fp32 squared distances of its ``k`` (1 ... 8) nearest sources, found on the device from the current state
        (waits for the queued work).  All bodies below the count are rows, test particles included.  ``sources``, a
        ``(B, max_bodies)`` bool or uint8 array, selects the bodies that can be neighbours (all, without it); every body gets a
        list all the same, so with the massive bodies as sources the lists are every planetesimal's nearest planets.  A list
        is ordered by distance, ties by the lower index; a coincident body is a neighbour, the body itself never.  ``radius``
        (a scalar, or ``B`` values, one per system) also counts the sources within it, ``within``; without it that is 0.
        ``lists=False`` and ``bodies=False`` skip the ``8 k`` bytes and the 8 bytes per body on their way to the host: those
        arrays of the result are ``None``, the per-system ones the same bits.  Changes nothing: an :meth:`evolve` after it is
        bit for bit the :meth:`evolve` without it."""
        k = int(k)
        if not 1 <= k <= _lib.BATCH_NEIGHBOURS_MAX:
            raise ValueError(f"k must be 1 ... {_lib.BATCH_NEIGHBOURS_MAX}, not {k}")
        B, n = self.num_systems, self.max_bodies
        b = None
        if radius is not None:
            b = np.asarray(radius, dtype=np.float32)
            if b.ndim == 0:
                b = np.full(B, b, dtype=np.float32)
            b = np.ascontiguousarray(b.reshape(-1))
            if b.shape[0] != B:
                raise ValueError(f"expected one radius or {B}, got {b.shape[0]}")
        src = None
        if sources is not None:
            src = np.ascontiguousarray(np.asarray(sources))
            if src.dtype != np.bool_ and src.dtype != np.uint8:
                raise ValueError(f"sources must be bool or uint8, not {src.dtype}")
            if src.shape != (B, n):
                raise ValueError(f"sources must have shape ({B}, {n}), got {tuple(src.shape)}")
            src = src.view(np.uint8)
        systems = np.zeros(B, dtype=NEIGHBOUR_SYSTEM_DTYPE)
        body = np.zeros((B, n), dtype=NEIGHBOUR_BODY_DTYPE) if bodies else None
        index = np.zeros((B, n, k), dtype=np.int32) if lists else None
        r2 = np.zeros((B, n, k), dtype=np.float32) if lists else None
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_neighbours(
            self._h, _ptr(self.positions), k, b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if b is not None else None,
            src.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if src is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchNeighbourSystem)),
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchNeighbourBody)) if bodies else None,
            index.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if lists else None,
            r2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if lists else None), self._h)
        return NeighbourResult(systems, body, index, r2, k)

    def correlation(self, edges, rows=None, sources=None, counts: bool = True) -> "CorrelationResult":
        """How many pairs lie at which separation (``include/nbody_batch_correlation.h`` states the rules): for every system
        the number of ordered pairs (row, source) in each bin of separation, counted on the device from the current state
        (waits for the queued work).  ``edges`` holds the ``bins + 1`` (2 ... 33) ascending bin edges, ``>= 0``: one set
        ``(bins + 1,)`` for all systems or ``(B, bins + 1)``, one per system.  Bin ``t`` holds the pairs with
        ``edges[t] < r <= edges[t + 1]``, compared as fp32 squares, which is :meth:`neighbours`' ``within`` and :meth:`groups`'
        link.  ``rows`` and ``sources``, ``(B, max_bodies)`` bool or uint8 arrays (numpy or torch), select who is counted
        around whom (all bodies, without them); a body is never paired with itself.  With the same mask on both sides every
        unordered pair is counted twice.  Two different masks give a cross-count: planetesimals around planets, the stars of
        one cluster around those of another.  ``counts=False`` skips the bins on their way to the host: ``counts`` of the
        result is ``None``, the per-system words (``pairs``, ``below``, ``above``, ``unmeasured``) the same bits.  Changes
        nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if hasattr(edges, "detach"):  # a torch tensor
            edges = edges.detach().cpu().numpy()
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float32))
        if e.ndim == 1:
            per_system = 0
        elif e.ndim == 2 and e.shape[0] == B:
            per_system = 1
        else:
            raise ValueError(f"edges must have shape (bins + 1,) or ({B}, bins + 1), got {tuple(e.shape)}")
        bins = e.shape[-1] - 1
        if not 1 <= bins <= _lib.BATCH_CORRELATION_MAX_BINS:
            raise ValueError(f"bins must be 1 ... {_lib.BATCH_CORRELATION_MAX_BINS}, not {bins}")

        def mask(name, m):
            if m is None:
                return None
            if hasattr(m, "detach"):
                m = m.detach().cpu().numpy()
            m = np.ascontiguousarray(np.asarray(m))
            if m.dtype != np.bool_ and m.dtype != np.uint8:
                raise ValueError(f"{name} must be bool or uint8, not {m.dtype}")
            if m.shape != (B, n):
                raise ValueError(f"{name} must have shape ({B}, {n}), got {tuple(m.shape)}")
            return m.view(np.uint8)

        row, src = mask("rows", rows), mask("sources", sources)
        systems = np.zeros(B, dtype=CORRELATION_SYSTEM_DTYPE)
        out = np.zeros((B, bins), dtype=np.uint32) if counts else None
        ubyte = ctypes.POINTER(ctypes.c_ubyte)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_correlation(
            self._h, _ptr(self.positions), bins, e.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), per_system,
            row.ctypes.data_as(ubyte) if row is not None else None, src.ctypes.data_as(ubyte) if src is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchCorrelationSystem)),
            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)) if counts else None), self._h)
        return CorrelationResult(systems, out.astype(np.int64) if counts else None, e)

    def contacts(self, radius=None, *, radii=None, subset=None, capacity=None, lists: bool = True,
                 bodies: bool = True) -> "ContactsResult":
        """Which pairs are within a distance of each other (``include/nbody_batch_contacts.h`` states the rules): for every
        system every unordered pair of bodies that is a contact, listed on the device from the current state (waits for the
        queued work) as ``(i, j, r2)`` with ``i < j``, ascending in ``i`` and then in ``j``.  Exactly one threshold: ``radius``,
        a scalar or ``(B,)``, makes a contact of every pair with ``r <= radius`` (compared as fp32 squares, which is
        :meth:`neighbours`' ``within``, :meth:`correlation`'s edge and :meth:`groups`' link); ``radii``, ``(B, max_bodies)``
        float32, of every pair with ``r <= R_i + R_j``, :meth:`set_radii`'s own rule at no softening -- ``radii=b.radii()``
        asks which bodies overlap now.  ``subset``, a ``(B, max_bodies)`` bool or uint8 array (numpy or torch), selects the
        bodies that take part (all, without it).  ``capacity`` is the number of list entries kept per system: a system with
        more contacts is ``truncated`` to the first ``capacity`` of them, its ``pairs`` exact all the same.  ``capacity=None``
        makes one counting call and then one with room for the fullest system.  ``lists=False`` only counts (one call at
        capacity 0: ``i``, ``j``, ``r2`` are ``None`` and ``stored`` is 0); ``bodies=False`` skips the per-body records on their
        way to the host.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if (radius is None) == (radii is None):
            raise ValueError("exactly one of radius and radii must be given")
        rad = rr = None
        if radius is not None:
            if hasattr(radius, "detach"):  # a torch tensor
                radius = radius.detach().cpu().numpy()
            rad = np.asarray(radius, dtype=np.float32)
            if rad.ndim == 0:
                rad = np.full(B, rad, dtype=np.float32)
            if rad.shape != (B,):
                raise ValueError(f"radius must be a scalar or have shape ({B},), got {tuple(rad.shape)}")
            rad = np.ascontiguousarray(rad)
        else:
            if hasattr(radii, "detach"):
                radii = radii.detach().cpu().numpy()
            rr = np.ascontiguousarray(np.asarray(radii, dtype=np.float32))
            if rr.shape != (B, n):
                raise ValueError(f"radii must have shape ({B}, {n}), got {tuple(rr.shape)}")
        sub = None
        if subset is not None:
            if hasattr(subset, "detach"):
                subset = subset.detach().cpu().numpy()
            sub = np.ascontiguousarray(np.asarray(subset))
            if sub.dtype != np.bool_ and sub.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {sub.dtype}")
            if sub.shape != (B, n):
                raise ValueError(f"subset must have shape ({B}, {n}), got {tuple(sub.shape)}")
            sub = sub.view(np.uint8)
        if capacity is not None:
            if int(capacity) != capacity or capacity < 0:
                raise ValueError(f"capacity must be an integer >= 0, not {capacity!r}")
            if B * int(capacity) > _lib.BATCH_CONTACTS_MAX_ENTRIES:
                raise ValueError(f"{B} systems x capacity {capacity} exceed 2^28 list entries")
        fp, ubyte = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)

        def call(cap, want_bodies):
            systems = np.zeros(B, dtype=CONTACT_SYSTEM_DTYPE)
            body = np.zeros((B, n), dtype=CONTACT_BODY_DTYPE) if want_bodies else None
            entries = np.zeros((B, cap), dtype=CONTACT_DTYPE) if cap > 0 else None
            self._use_current_stream()
            _check(self._lib, self._lib.nbody_batch_contacts(
                self._h, _ptr(self.positions), rad.ctypes.data_as(fp) if rad is not None else None,
                rr.ctypes.data_as(fp) if rr is not None else None, sub.ctypes.data_as(ubyte) if sub is not None else None,
                cap, systems.ctypes.data_as(ctypes.POINTER(_lib.BatchContactSystem)),
                body.ctypes.data_as(ctypes.POINTER(_lib.BatchContactBody)) if want_bodies else None,
                entries.ctypes.data_as(ctypes.POINTER(_lib.BatchContact)) if cap > 0 else None), self._h)
            return systems, body, entries

        if not lists:
            systems, body, _ = call(0, bodies)
            return ContactsResult(systems, body, None)
        if capacity is None:
            systems, body, _ = call(0, bodies)
            capacity = int(systems["pairs"].max()) if B else 0
            if capacity == 0:
                return ContactsResult(systems, body, np.zeros((B, 0), dtype=CONTACT_DTYPE))
            if B * capacity > _lib.BATCH_CONTACTS_MAX_ENTRIES:
                raise ValueError(f"{B} systems x {capacity} contacts in the fullest exceed 2^28 list entries: pass a capacity")
        systems, body, entries = call(int(capacity), bodies)
        return ContactsResult(systems, body, entries if entries is not None else np.zeros((B, 0), dtype=CONTACT_DTYPE))

    def approaches(self, horizon, radius=None, *, radii=None, subset=None, capacity=None, lists: bool = True,
                   bodies: bool = True) -> "ApproachesResult":
        """Which pairs will come within a distance of each other (``include/nbody_batch_approaches.h`` states the rules): for
        every system every unordered pair of bodies whose separation, with both bodies moved on straight lines at their current
        velocities, is within the threshold at some time in ``[0, horizon]``, listed on the device from the current state
        (waits for the queued work) as ``(i, j, r2, rv, v2, phase)`` with ``i < j``, ascending in ``i`` and then in ``j``.
        ``horizon`` is a scalar or ``(B,)``, finite and ``>= 0``.  The thresholds, ``subset``, ``capacity``, ``lists`` and
        ``bodies`` are :meth:`contacts`' own: exactly one of ``radius`` (a scalar or ``(B,)``) and ``radii``
        (``(B, max_bodies)`` float32, a pair within ``R_i + R_j``); ``capacity=None`` makes one counting call and then one with
        room for the fullest system; ``lists=False`` only counts.  ``phase`` is 0 for a pair within reach now (a
        :meth:`contacts` pair), 1 for one whose closest passage falls before the horizon and within reach, 2 for one still
        closing at the horizon and within reach there.  With a horizon of 0, or with all velocities equal, the approaches are
        the contacts.  The device computes no time and no distance: the result derives ``time`` and ``miss_distance`` in float64
        from the entries' words.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if (radius is None) == (radii is None):
            raise ValueError("exactly one of radius and radii must be given")

        def per_system(value, name):
            if hasattr(value, "detach"):  # a torch tensor
                value = value.detach().cpu().numpy()
            out = np.asarray(value, dtype=np.float32)
            if out.ndim == 0:
                out = np.full(B, out, dtype=np.float32)
            if out.shape != (B,):
                raise ValueError(f"{name} must be a scalar or have shape ({B},), got {tuple(out.shape)}")
            return np.ascontiguousarray(out)
        hor = per_system(horizon, "horizon")
        rad = rr = None
        if radius is not None:
            rad = per_system(radius, "radius")
        else:
            if hasattr(radii, "detach"):
                radii = radii.detach().cpu().numpy()
            rr = np.ascontiguousarray(np.asarray(radii, dtype=np.float32))
            if rr.shape != (B, n):
                raise ValueError(f"radii must have shape ({B}, {n}), got {tuple(rr.shape)}")
        sub = None
        if subset is not None:
            if hasattr(subset, "detach"):
                subset = subset.detach().cpu().numpy()
            sub = np.ascontiguousarray(np.asarray(subset))
            if sub.dtype != np.bool_ and sub.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {sub.dtype}")
            if sub.shape != (B, n):
                raise ValueError(f"subset must have shape ({B}, {n}), got {tuple(sub.shape)}")
            sub = sub.view(np.uint8)
        if capacity is not None:
            if int(capacity) != capacity or capacity < 0:
                raise ValueError(f"capacity must be an integer >= 0, not {capacity!r}")
            if B * int(capacity) > _lib.BATCH_APPROACHES_MAX_ENTRIES:
                raise ValueError(f"{B} systems x capacity {capacity} exceed 2^27 list entries")
        fp, ubyte = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_ubyte)

        def call(cap, want_bodies):
            systems = np.zeros(B, dtype=APPROACH_SYSTEM_DTYPE)
            body = np.zeros((B, n), dtype=APPROACH_BODY_DTYPE) if want_bodies else None
            entries = np.zeros((B, cap), dtype=APPROACH_DTYPE) if cap > 0 else None
            self._use_current_stream()
            _check(self._lib, self._lib.nbody_batch_approaches(
                self._h, _ptr(self.positions), _ptr(self.velocities), hor.ctypes.data_as(fp),
                rad.ctypes.data_as(fp) if rad is not None else None, rr.ctypes.data_as(fp) if rr is not None else None,
                sub.ctypes.data_as(ubyte) if sub is not None else None, cap,
                systems.ctypes.data_as(ctypes.POINTER(_lib.BatchApproachSystem)),
                body.ctypes.data_as(ctypes.POINTER(_lib.BatchApproachBody)) if want_bodies else None,
                entries.ctypes.data_as(ctypes.POINTER(_lib.BatchApproach)) if cap > 0 else None), self._h)
            return systems, body, entries

        if not lists:
            systems, body, _ = call(0, bodies)
            return ApproachesResult(systems, body, None, hor)
        if capacity is None:
            systems, body, _ = call(0, bodies)
            capacity = int(systems["pairs"].max()) if B else 0
            if capacity == 0:
                return ApproachesResult(systems, body, np.zeros((B, 0), dtype=APPROACH_DTYPE), hor)
            if B * capacity > _lib.BATCH_APPROACHES_MAX_ENTRIES:
                raise ValueError(f"{B} systems x {capacity} approaches in the fullest exceed 2^27 list entries: pass a capacity")
        systems, body, entries = call(int(capacity), bodies)
        return ApproachesResult(systems, body, entries if entries is not None else np.zeros((B, 0), dtype=APPROACH_DTYPE), hor)

    def radial_profile(self, edges, *, centre=None, velocity=None, weight: str = "mass", subset=None, projected=None,
                       shells: bool = True, bodies: bool = False) -> "RadialProfileResult":
        """How every system is built as a function of radius (``include/nbody_batch_radial.h`` states the rules): the bodies
        binned on the device into up to 32 shells about a centre, from the current state (waits for the queued work), and per
        shell the count and the 23 float64 sums that density, mean radial velocity, velocity dispersions, anisotropy,
        rotation and shape are made of.  ``edges`` holds the ``shells + 1`` (2 ... 33) ascending float64 edges, ``>= 0``: one
        set ``(shells + 1,)`` for all systems or ``(B, shells + 1)``, one per system.  Shell ``t`` holds the bodies with
        ``edges[t] < r <= edges[t + 1]``, compared as float64 squares.  ``centre`` and ``velocity`` give the frame: ``None``
        (zeros), ``(3,)``, ``(B, 3)``, for ``centre`` also a :class:`StructureResult` (its ``centre``) or ``"density"``, which
        calls ``structure(weight=weight, bodies=False)`` first and takes its density centre.  ``weight``: ``"mass"`` or
        ``"number"``.  ``subset``, a ``(B, max_bodies)`` bool or uint8 array (numpy or torch), selects who takes part (all
        bodies below the count, without it), whatever the massive counts.  ``projected``: ``None`` for spherical shells, or the
        axis 0, 1 or 2 that the radius and the radial velocity leave out: annuli in the plane of the other two.  Every sum
        runs over the shell's members in ascending body index, so a system's records are the same bits in any slot, batch and
        capacity.  ``shells=False`` skips the 192 bytes per shell on their way to the host and ``bodies=True`` adds the 24
        bytes per body (``body_shell``, ``body_radius``, ``body_radial_velocity``); the remaining records are the same bits
        either way.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")
        if projected is not None and projected not in (0, 1, 2):
            raise ValueError(f"projected must be None, 0, 1 or 2, not {projected!r}")
        if hasattr(edges, "detach"):  # a torch tensor
            edges = edges.detach().cpu().numpy()
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64))
        if e.ndim == 1:
            per_system = 0
        elif e.ndim == 2 and e.shape[0] == B:
            per_system = 1
        else:
            raise ValueError(f"edges must have shape (shells + 1,) or ({B}, shells + 1), got {tuple(e.shape)}")
        count = e.shape[-1] - 1
        if not 1 <= count <= _lib.BATCH_RADIAL_MAX_SHELLS:
            raise ValueError(f"shells must be 1 ... {_lib.BATCH_RADIAL_MAX_SHELLS}, not {count}")

        def frame(name, value):
            if value is None:
                return None
            if hasattr(value, "detach"):
                value = value.detach().cpu().numpy()
            v = np.asarray(value, dtype=np.float64)
            if v.shape == (3,):
                v = np.broadcast_to(v, (B, 3))
            if v.shape != (B, 3):
                raise ValueError(f"{name} must have shape (3,) or ({B}, 3), got {tuple(v.shape)}")
            return np.ascontiguousarray(v)

        if isinstance(centre, str):
            if centre != "density":
                raise ValueError(f"centre must be an array, a StructureResult or 'density', not {centre!r}")
            centre = self.structure(weight=weight, bodies=False).centre
        elif isinstance(centre, StructureResult):
            centre = centre.centre
        c, v0 = frame("centre", centre), frame("velocity", velocity)
        mask = None
        if subset is not None:
            mask = subset.detach().cpu().numpy() if hasattr(subset, "detach") else subset
            mask = np.ascontiguousarray(np.asarray(mask))
            if mask.dtype != np.bool_ and mask.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {mask.dtype}")
            if mask.shape != (B, n):
                raise ValueError(f"subset must have shape ({B}, {n}), got {tuple(mask.shape)}")
            mask = mask.view(np.uint8)
        systems = np.zeros(B, dtype=RADIAL_SYSTEM_DTYPE)
        rec = np.zeros((B, count), dtype=RADIAL_SHELL_DTYPE) if shells else None
        body = np.zeros((B, n), dtype=RADIAL_BODY_DTYPE) if bodies else None
        dbl = ctypes.POINTER(ctypes.c_double)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_radial_profile(
            self._h, _ptr(self.positions), _ptr(self.velocities), count, e.ctypes.data_as(dbl), per_system,
            c.ctypes.data_as(dbl) if c is not None else None, v0.ctypes.data_as(dbl) if v0 is not None else None,
            WEIGHTS[weight], -1 if projected is None else int(projected),
            mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if mask is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchRadialSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchRadialShell)) if shells else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchRadialBody)) if bodies else None), self._h)
        return RadialProfileResult(systems, rec, body, e, weight)

    def surface_map(self, edges_a, edges_b=None, *, centre=None, velocity=None, axes=None, projected: int = 2, weight: str = "mass",
                    subset=None, cells: bool = True, bodies: bool = False) -> "SurfaceMapResult":
        """What every system looks like from a direction (``include/nbody_batch_surface.h`` states the rules): the bodies
        binned on the device into a grid of ``columns x rows`` cells (1 ... 64 each) in the plane of a view, from the current
        state (waits for the queued work), and per cell the count and the seven float64 sums that the surface density, the
        line-of-sight velocity and its dispersion, the velocity in the plane and the depth are made of.  ``edges_a`` holds the
        ``columns + 1`` ascending float64 edges of the map's first axis and ``edges_b`` the ``rows + 1`` of its second
        (``None``: ``edges_a`` again): each ``(bins + 1,)`` for all systems or ``(B, bins + 1)``, one set per system
        (:meth:`SurfaceMapResult.grid` makes evenly spaced ones).  Cell ``(j, i)`` holds the bodies with ``edges_a[i] <= a <
        edges_a[i + 1]`` and ``edges_b[j] <= b < edges_b[j + 1]``: half-open on the right, the last edge included.
        ``centre``, ``velocity``, ``weight`` and ``subset`` are :meth:`radial_profile`'s: the frame (``None``, ``(3,)``, ``(B,
        3)``, for ``centre`` also a :class:`StructureResult` or ``"density"``), ``"mass"`` or ``"number"``, and a ``(B,
        max_bodies)`` bool or uint8 mask (numpy or torch).  The view is three float64 row vectors per system, ``A`` (the first
        axis), ``B`` (the second) and ``Q`` (the line of sight), as ``axes`` of shape ``(3, 3)`` or ``(B, 3, 3)``
        (:meth:`SurfaceMapResult.view` builds an orthonormal triple for a direction; only finiteness is checked).  Without
        ``axes``, ``projected = p`` takes the unit vectors of the two axes that are not ``p``, in ascending order, and ``p``
        itself as ``Q``.  Every sum runs over the cell's members in ascending body index, so a system's records are the same
        bits in any slot, batch and capacity.  ``cells=False`` skips the 64 bytes per cell on their way to the host and
        ``bodies=True`` adds the 24 bytes per body (``body_cell``, ``body_a``, ``body_b``); the remaining records are the same
        bits either way.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")

        def host(value):
            return value.detach().cpu().numpy() if hasattr(value, "detach") else value

        def edge_set(name, value):
            e = np.asarray(host(value), dtype=np.float64)
            if not (e.ndim == 1 or (e.ndim == 2 and e.shape[0] == B)):
                raise ValueError(f"{name} must have shape (bins + 1,) or ({B}, bins + 1), got {tuple(e.shape)}")
            if not 1 <= e.shape[-1] - 1 <= _lib.BATCH_SURFACE_MAX_SIDE:
                raise ValueError(f"columns and rows must be 1 ... {_lib.BATCH_SURFACE_MAX_SIDE}, not {e.shape[-1] - 1}")
            return e

        ea = edge_set("edges_a", edges_a)
        eb = ea if edges_b is None else edge_set("edges_b", edges_b)
        per_system = int(ea.ndim == 2 or eb.ndim == 2)
        if per_system:
            ea, eb = (np.broadcast_to(e, (B, e.shape[-1])) for e in (ea, eb))
        ea, eb = np.ascontiguousarray(ea), np.ascontiguousarray(eb)
        columns, rows = ea.shape[-1] - 1, eb.shape[-1] - 1

        def frame(name, value):
            if value is None:
                return None
            v = np.asarray(host(value), dtype=np.float64)
            if v.shape == (3,):
                v = np.broadcast_to(v, (B, 3))
            if v.shape != (B, 3):
                raise ValueError(f"{name} must have shape (3,) or ({B}, 3), got {tuple(v.shape)}")
            return np.ascontiguousarray(v)

        if isinstance(centre, str):
            if centre != "density":
                raise ValueError(f"centre must be an array, a StructureResult or 'density', not {centre!r}")
            centre = self.structure(weight=weight, bodies=False).centre
        elif isinstance(centre, StructureResult):
            centre = centre.centre
        c, v0 = frame("centre", centre), frame("velocity", velocity)
        if axes is None:
            if projected not in (0, 1, 2):
                raise ValueError(f"projected must be 0, 1 or 2, not {projected!r}")
            kept = [k for k in range(3) if k != projected]
            view = np.eye(3)[[kept[0], kept[1], projected]]
        else:
            view = np.asarray(host(axes), dtype=np.float64)
            if view.shape != (3, 3) and view.shape != (B, 3, 3):
                raise ValueError(f"axes must have shape (3, 3) or ({B}, 3, 3), got {tuple(view.shape)}")
        view = np.ascontiguousarray(np.broadcast_to(view, (B, 3, 3)))
        mask = None
        if subset is not None:
            mask = np.ascontiguousarray(np.asarray(host(subset)))
            if mask.dtype != np.bool_ and mask.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {mask.dtype}")
            if mask.shape != (B, n):
                raise ValueError(f"subset must have shape ({B}, {n}), got {tuple(mask.shape)}")
            mask = mask.view(np.uint8)
        systems = np.zeros(B, dtype=SURFACE_SYSTEM_DTYPE)
        rec = np.zeros((B, rows, columns), dtype=SURFACE_CELL_DTYPE) if cells else None
        body = np.zeros((B, n), dtype=SURFACE_BODY_DTYPE) if bodies else None
        dbl = ctypes.POINTER(ctypes.c_double)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_surface_map(
            self._h, _ptr(self.positions), _ptr(self.velocities), columns, rows, ea.ctypes.data_as(dbl), eb.ctypes.data_as(dbl),
            per_system, c.ctypes.data_as(dbl) if c is not None else None, v0.ctypes.data_as(dbl) if v0 is not None else None,
            view.ctypes.data_as(dbl), WEIGHTS[weight],
            mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if mask is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchSurfaceSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchSurfaceCell)) if cells else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchSurfaceBody)) if bodies else None), self._h)
        return SurfaceMapResult(systems, rec, body, ea, eb, view, weight)

    def shape(self, radii, *, inner=None, centre=None, velocity=None, weight: str = "mass", subset=None, reduced: bool = True,
              tol: float = 1e-3, max_iterations: int = 64, min_members: int = 10, apertures: bool = True,
              bodies: bool = False) -> "ShapeResult":
        """How every system is shaped and oriented (``include/nbody_batch_shape.h`` states the rules): for each of up to 8
        apertures the ellipsoid that the iterated moment tensor converges to, found on the device from the current state
        (waits for the queued work).  ``radii`` holds the major semi-axes, ``> 0``: ``(apertures,)`` for all systems or ``(B,
        apertures)``; ``inner``, of the same shape, makes ellipsoidal shells ``inner < r_ell <= radius`` (``None``: full
        ellipsoids).  Each aperture starts as the sphere of its radius; a pass takes the bodies inside the current ellipsoid,
        diagonalises their moment tensor -- the reduced one, every body's term divided by its squared elliptical radius, or
        with ``reduced=False`` the plain one -- and deforms the ellipsoid to the axis ratios found, keeping the major axis at
        the radius, until ``q`` (middle over major) and ``s`` (minor over major) change by at most ``tol`` of themselves
        (status 0) or ``max_iterations`` (1 ... 64) passes are made (status 1).  A pass with fewer than ``min_members`` (>= 4)
        members ends the aperture with status 2 and a tensor without three positive eigenvalues with status 3, both with the
        state of the pass before.  ``centre``, ``velocity``, ``weight`` and ``subset`` are :meth:`radial_profile`'s: the frame
        (``None``, ``(3,)``, ``(B, 3)``, for ``centre`` also a :class:`StructureResult` or ``"density"``), ``"mass"`` or
        ``"number"``, and a ``(B, max_bodies)`` bool or uint8 mask (numpy or torch).  Every sum runs over blocks of 64 bodies in
        ascending index and then over the blocks, so a system's records are the same bits in any slot, batch and capacity.
        ``apertures=False`` skips the 256 bytes per aperture on their way to the host and ``bodies=True`` adds the 8 bytes per
        body (``inside``: bit ``a`` set for a member of aperture ``a``'s final ellipsoid); the remaining records are the same
        bits either way.  Changes nothing: an :meth:`evolve` after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")

        def host(value):
            return value.detach().cpu().numpy() if hasattr(value, "detach") else value

        R = np.atleast_1d(np.asarray(host(radii), dtype=np.float64))
        if not (R.ndim == 1 or (R.ndim == 2 and R.shape[0] == B)):
            raise ValueError(f"radii must have shape (apertures,) or ({B}, apertures), got {tuple(R.shape)}")
        count = R.shape[-1]
        if not 1 <= count <= _lib.BATCH_SHAPE_MAX_APERTURES:
            raise ValueError(f"apertures must be 1 ... {_lib.BATCH_SHAPE_MAX_APERTURES}, not {count}")
        Rin = None
        if inner is not None:
            Rin = np.atleast_1d(np.asarray(host(inner), dtype=np.float64))
            if Rin.shape[-1] != count or not (Rin.ndim == 1 or (Rin.ndim == 2 and Rin.shape[0] == B)):
                raise ValueError(f"inner must have shape ({count},) or ({B}, {count}), got {tuple(Rin.shape)}")
        per_system = int(R.ndim == 2 or (Rin is not None and Rin.ndim == 2))
        if per_system:
            R = np.broadcast_to(R, (B, count))
            Rin = None if Rin is None else np.broadcast_to(Rin, (B, count))
        R = np.ascontiguousarray(R)
        Rin = None if Rin is None else np.ascontiguousarray(Rin)

        def frame(name, value):
            if value is None:
                return None
            v = np.asarray(host(value), dtype=np.float64)
            if v.shape == (3,):
                v = np.broadcast_to(v, (B, 3))
            if v.shape != (B, 3):
                raise ValueError(f"{name} must have shape (3,) or ({B}, 3), got {tuple(v.shape)}")
            return np.ascontiguousarray(v)

        if isinstance(centre, str):
            if centre != "density":
                raise ValueError(f"centre must be an array, a StructureResult or 'density', not {centre!r}")
            centre = self.structure(weight=weight, bodies=False).centre
        elif isinstance(centre, StructureResult):
            centre = centre.centre
        c, v0 = frame("centre", centre), frame("velocity", velocity)
        mask = None
        if subset is not None:
            mask = np.ascontiguousarray(np.asarray(host(subset)))
            if mask.dtype != np.bool_ and mask.dtype != np.uint8:
                raise ValueError(f"subset must be bool or uint8, not {mask.dtype}")
            if mask.shape != (B, n):
                raise ValueError(f"subset must have shape ({B}, {n}), got {tuple(mask.shape)}")
            mask = mask.view(np.uint8)
        systems = np.zeros(B, dtype=SHAPE_SYSTEM_DTYPE)
        rec = np.zeros((B, count), dtype=SHAPE_APERTURE_DTYPE) if apertures else None
        body = np.zeros((B, n), dtype=SHAPE_BODY_DTYPE) if bodies else None
        dbl = ctypes.POINTER(ctypes.c_double)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_shape(
            self._h, _ptr(self.positions), _ptr(self.velocities), count, R.ctypes.data_as(dbl),
            Rin.ctypes.data_as(dbl) if Rin is not None else None, per_system,
            c.ctypes.data_as(dbl) if c is not None else None, v0.ctypes.data_as(dbl) if v0 is not None else None,
            WEIGHTS[weight], 1 if reduced else 0, float(tol), int(max_iterations), int(min_members),
            mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if mask is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchShapeSystem)),
            rec.ctypes.data_as(ctypes.POINTER(_lib.BatchShapeAperture)) if apertures else None,
            body.ctypes.data_as(ctypes.POINTER(_lib.BatchShapeBody)) if bodies else None), self._h)
        return ShapeResult(systems, rec, body, weight)

    def pair_velocities(self, edges, rows=None, sources=None, weight: str = "number", bins: bool = True) -> "PairVelocityResult":
        """How pairs move at which separation (``include/nbody_batch_pair_velocities.h`` states the rules): for every system
        and each bin of separation the number of ordered pairs (row, source), how many approach and recede, and the fp64 sums
        of separation, radial velocity and its square, tangential and whole relative velocity over them, summed on the device
        from the current state in a pinned order (waits for the queued work).  ``edges``, ``rows`` and ``sources`` are
        :meth:`correlation`'s: ``(bins + 1,)`` or ``(B, bins + 1)`` ascending edges ``>= 0`` (1 ... 32 bins) and
        ``(B, max_bodies)`` bool or uint8 masks (numpy or torch); the bin of a pair is decided by :meth:`correlation`'s code, so
        on finite velocities the counts are :meth:`correlation`'s.  ``weight``: ``"number"`` (every pair weighs 1) or
        ``"mass"`` (the product of the two mass words).  ``bins=False`` skips the bin records on their way to the host:
        ``bin_records`` of the result is ``None``, the per-system words the same bits.  Changes nothing: an :meth:`evolve`
        after it is bit for bit the :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if weight not in WEIGHTS:
            raise ValueError(f"weight must be one of {sorted(WEIGHTS)}, not {weight!r}")
        if hasattr(edges, "detach"):  # a torch tensor
            edges = edges.detach().cpu().numpy()
        e = np.ascontiguousarray(np.asarray(edges, dtype=np.float32))
        if e.ndim == 1:
            per_system = 0
        elif e.ndim == 2 and e.shape[0] == B:
            per_system = 1
        else:
            raise ValueError(f"edges must have shape (bins + 1,) or ({B}, bins + 1), got {tuple(e.shape)}")
        nbins = e.shape[-1] - 1
        if not 1 <= nbins <= _lib.BATCH_PAIR_VELOCITIES_MAX_BINS:
            raise ValueError(f"bins must be 1 ... {_lib.BATCH_PAIR_VELOCITIES_MAX_BINS}, not {nbins}")

        def mask(name, m):
            if m is None:
                return None
            if hasattr(m, "detach"):
                m = m.detach().cpu().numpy()
            m = np.ascontiguousarray(np.asarray(m))
            if m.dtype != np.bool_ and m.dtype != np.uint8:
                raise ValueError(f"{name} must be bool or uint8, not {m.dtype}")
            if m.shape != (B, n):
                raise ValueError(f"{name} must have shape ({B}, {n}), got {tuple(m.shape)}")
            return m.view(np.uint8)

        row, src = mask("rows", rows), mask("sources", sources)
        systems = np.zeros(B, dtype=PAIR_VELOCITIES_SYSTEM_DTYPE)
        out = np.zeros((B, nbins), dtype=PAIR_VELOCITIES_BIN_DTYPE) if bins else None
        ubyte = ctypes.POINTER(ctypes.c_ubyte)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_pair_velocities(
            self._h, _ptr(self.positions), _ptr(self.velocities), nbins, e.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), per_system,
            row.ctypes.data_as(ubyte) if row is not None else None, src.ctypes.data_as(ubyte) if src is not None else None,
            WEIGHTS[weight], systems.ctypes.data_as(ctypes.POINTER(_lib.BatchPairVelocitiesSystem)),
            out.ctypes.data_as(ctypes.POINTER(_lib.BatchPairVelocitiesBin)) if bins else None), self._h)
        return PairVelocityResult(systems, out, e, weight)

    def mutual_gravity(self, labels, sets=None, softening: float = 0.0, centre=None, velocity=None,
                       matrix: bool = True) -> "MutualGravityResult":
        """What the parts of every system do to each other (``include/nbody_batch_mutual_gravity.h`` states the rules): for
        every ordered pair ``(a, b)`` of up to 8 disjoint sets of bodies the potential energy between them, the net force of
        ``b`` on ``a``, its torque and Clausius virial about ``centre`` and the power it puts into ``a`` in the frame moving
        with ``velocity``, as fp64 pair sums on the device from the current state in a pinned order (waits for the queued
        work).  ``labels`` is ``(B, max_bodies)`` integers (numpy or torch): a value ``a`` in ``[0, sets)`` puts the body in set
        ``a`` and any negative value leaves it out -- ``groups().label``, ``members().member`` or a mask as integers all do --
        or a tuple of ``(B, max_bodies)`` boolean masks, mask ``a`` being set ``a`` (overlapping masks are refused).  ``sets``
        (1 ... 8) defaults to ``max(label) + 1``.  ``centre`` and ``velocity`` are what :meth:`radial_profile` takes: ``None``
        (zeros), ``(3,)``, ``(B, 3)``, for ``centre`` also a :class:`StructureResult` or ``"density"``.  ``softening`` follows
        :meth:`energy`'s rule.  Only bodies below the count take part, whatever the massive counts; a labelled body with a NaN
        or infinite word is taken out and counted in ``unmeasured``.  ``matrix=False`` skips the entries on their way to the
        host: the per-system words are the same bits.  Changes nothing: an :meth:`evolve` after it is bit for bit the
        :meth:`evolve` without it."""
        B, n = self.num_systems, self.max_bodies
        if isinstance(labels, (tuple, list)) and len(labels) and np.asarray(
                labels[0].detach().cpu().numpy() if hasattr(labels[0], "detach") else labels[0]).dtype == np.bool_:
            labels = MutualGravityResult.labels_from_masks(*labels)
        if hasattr(labels, "detach"):  # a torch tensor
            labels = labels.detach().cpu().numpy()
        lab = np.asarray(labels)
        if lab.dtype == np.bool_ or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"labels must be integers or a tuple of bool masks, not {lab.dtype}")
        if lab.shape != (B, n):
            raise ValueError(f"labels must have shape ({B}, {n}), got {tuple(lab.shape)}")
        lab = lab.astype(np.int64)
        top = int(lab.max()) if lab.size else -1
        if sets is None:
            sets = max(top + 1, 1)
        sets = int(sets)
        if not 1 <= sets <= _lib.BATCH_MUTUAL_GRAVITY_MAX_SETS:
            raise ValueError(f"sets must be 1 ... {_lib.BATCH_MUTUAL_GRAVITY_MAX_SETS}, not {sets}")
        if top >= sets:
            s, i = np.argwhere(lab >= sets)[0]
            raise ValueError(f"the label {lab[s, i]} of body {i} of system {s} must be below sets ({sets}) or negative")
        wire = np.ascontiguousarray(np.where(lab < 0, _lib.BATCH_MUTUAL_GRAVITY_NO_SET, lab).astype(np.uint8))

        def frame(name, value):
            if value is None:
                return None
            if hasattr(value, "detach"):
                value = value.detach().cpu().numpy()
            v = np.asarray(value, dtype=np.float64)
            if v.shape == (3,):
                v = np.broadcast_to(v, (B, 3))
            if v.shape != (B, 3):
                raise ValueError(f"{name} must have shape (3,) or ({B}, 3), got {tuple(v.shape)}")
            return np.ascontiguousarray(v)

        if isinstance(centre, str):
            if centre != "density":
                raise ValueError(f"centre must be an array, a StructureResult or 'density', not {centre!r}")
            centre = self.structure(bodies=False).centre
        elif isinstance(centre, StructureResult):
            centre = centre.centre
        c, v0 = frame("centre", centre), frame("velocity", velocity)
        systems = np.zeros(B, dtype=MUTUAL_GRAVITY_SYSTEM_DTYPE)
        out = np.zeros((B, sets, sets), dtype=MUTUAL_GRAVITY_ENTRY_DTYPE) if matrix else None
        dbl = ctypes.POINTER(ctypes.c_double)
        self._use_current_stream()
        _check(self._lib, self._lib.nbody_batch_mutual_gravity(
            self._h, _ptr(self.positions), _ptr(self.velocities), sets, wire.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
            float(softening), c.ctypes.data_as(dbl) if c is not None else None, v0.ctypes.data_as(dbl) if v0 is not None else None,
            systems.ctypes.data_as(ctypes.POINTER(_lib.BatchMutualGravitySystem)),
            out.ctypes.data_as(ctypes.POINTER(_lib.BatchMutualGravityEntry)) if matrix else None), self._h)
        return MutualGravityResult(systems, out, sets)

    def _source_mass(self) -> np.ndarray:
        """``(B,)`` float64: the mass of all sources of :meth:`members` -- :meth:`momentum`'s mass, and with massive counts the
        fp64 sum of the massive bodies' mass words alone."""
        massive = self.massive_counts
        if massive is None:
            return self.momentum()[:, 3]
        m = self.positions[:, :, 3].cpu().numpy().astype(np.float64)
        source = np.arange(self.max_bodies)[None, :] < np.minimum(massive, self._counts)[:, None]
        return np.where(source, m, 0.0).sum(axis=1)

    def sync(self) -> None:
        """Wait for the queued work and report a kernel failure."""
        _check(self._lib, self._lib.nbody_batch_sync(self._h), self._h)

    # -- diagnostics -------------------------------------------------------------------------
    def energy(self, softening: float) -> np.ndarray:
        """``(B, 3)``: per system ``[kinetic, potential, total]`` (fp32 pair terms, fp64 sums; ``nbody_energy``'s definition)."""
        self._use_current_stream()
        out = np.zeros((self.num_systems, 3), dtype=np.float64)
        _check(self._lib, self._lib.nbody_batch_energy(self._h, _ptr(self.positions), _ptr(self.velocities), float(softening),
                                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), self._h)
        return out

    def momentum(self) -> np.ndarray:
        """``(B, 4)``: per system ``[px, py, pz, mass]`` (fp64)."""
        self._use_current_stream()
        out = np.zeros((self.num_systems, 4), dtype=np.float64)
        _check(self._lib, self._lib.nbody_batch_momentum(self._h, _ptr(self.positions), _ptr(self.velocities),
                                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), self._h)
        return out


class EvolveResult:
    """What :meth:`BatchedSystem.evolve` did, per system (``(B,)`` arrays): ``steps`` taken, ``min_level`` and ``max_level``
    stepped at, ``clamped`` steps (still longer than requested at the finest level) and the ``ticks`` reached, in units of
    ``dt_max * 2**-levels`` (``n_intervals * 2**levels`` when finished)."""

    def __init__(self, steps, min_level, max_level, clamped, ticks):
        self.steps, self.min_level, self.max_level, self.clamped, self.ticks = steps, min_level, max_level, clamped, ticks

    def __repr__(self):
        return (f"EvolveResult(steps={self.steps.tolist()}, min_level={self.min_level.tolist()}, "
                f"max_level={self.max_level.tolist()}, clamped={self.clamped.tolist()}, ticks={self.ticks.tolist()})")


class StopResult:
    """What the stopping conditions of :meth:`BatchedSystem.set_stop_conditions` found, per system (``(B,)`` arrays, all zero
    for a system that has not stopped): ``reason`` (bit 1: collision, bit 2: escape), ``ticks`` (the tick of the stop, in
    the units of the :meth:`BatchedSystem.evolve` call that found it), ``pair`` (``(B, 2)``: the colliding bodies
    ``i < j``), their ``separation``, the ``escaper`` (the escaping body of smallest index) and ``stopped`` (boolean).  A
    stop for one reason only has ``-1`` for the other's indices."""

    def __init__(self, reason, ticks, pair, separation, escaper):
        self.reason, self.ticks, self.pair, self.separation, self.escaper = reason, ticks, pair, separation, escaper
        self.stopped = reason != 0

    def __repr__(self):
        return (f"StopResult(reason={self.reason.tolist()}, ticks={self.ticks.tolist()}, pair={self.pair.tolist()}, "
                f"separation={self.separation.tolist()}, escaper={self.escaper.tolist()})")


class MergeResult:
    """What the collision action ``"merge"`` did, per system: ``count`` (``(B,)``, the number of mergers) and ``events``
    (``(B, log_capacity)``, structured: ``tick``, in the units of the :meth:`BatchedSystem.evolve` call that found the
    collision, ``survivor`` and ``absorbed`` (the pair ``i < j`` before the swap), ``count_before``, ``separation``,
    ``relative_speed``, ``mass_survivor`` and ``mass_absorbed``; entries from a system's count on are zero)."""

    def __init__(self, count, events):
        self.count, self.events = count, events

    def __repr__(self):
        return f"MergeResult(count={self.count.tolist()}, events={self.events.tolist()})"


class FateResult:
    """What became of the test particles under the tracer action ``"remove"`` (:meth:`BatchedSystem.set_tracer_action`).
    ``(B, max_bodies)`` arrays: ``fate`` (0 alive, 1 hit a massive body, 2 escaped), ``ticks`` (the tick of the step that
    found it, in the units of the :meth:`BatchedSystem.evolve` call that found it), ``target`` (the massive body hit, ``-1``
    otherwise), ``separation`` and ``relative_speed`` at the evaluation that found the hit (0 otherwise); massive bodies, live
    tracers and empty slots read ``0, 0, -1, 0, 0``.  ``(B,)`` arrays: ``hit`` and ``escaped``, the totals per system."""

    def __init__(self, fate, ticks, target, separation, relative_speed, hit, escaped):
        self.fate, self.ticks, self.target, self.separation, self.relative_speed = fate, ticks, target, separation, relative_speed
        self.hit, self.escaped = hit, escaped

    def __repr__(self):
        return f"FateResult(hit={self.hit.tolist()}, escaped={self.escaped.tolist()})"


class AccretionResult:
    """What the hit action ``"accrete"`` did (:meth:`BatchedSystem.set_hit_action`): ``given`` (``(B, max_bodies)`` float32,
    the mass word each test particle gave the body it hit, 0 elsewhere; the body is the fate's ``target``) and ``count``
    (``(B,)`` int64, the accretions per system)."""

    def __init__(self, given, count):
        self.given, self.count = given, count

    def __repr__(self):
        return f"AccretionResult(count={self.count.tolist()})"


class PairResult:
    """What :meth:`BatchedSystem.pairs` found.  ``(B, max_bodies)`` arrays: ``partner`` (int32, ``-1`` for a body without a
    candidate), ``mutual`` (bool: the partner's partner is the body itself) and, float64, the pair's ``energy``
    (``v**2 / 2 - mu / r``), ``semi_major_axis`` (negative for a hyperbolic pair, ``inf`` at zero energy), ``eccentricity``,
    ``inclination`` (radians, against the z axis) and ``separation``; bodies without a partner and slots from the count on
    read ``-1, False, 0, 0, 0, 0, 0``.  ``binaries`` (``(B,)`` int64): the mutual pairs with negative energy per system, each
    counted once."""

    def __init__(self, records, binaries):
        self.partner = np.ascontiguousarray(records["partner"])
        self.mutual = records["mutual"] != 0
        self.energy, self.semi_major_axis, self.eccentricity, self.inclination, self.separation = (
            np.ascontiguousarray(records[k]) for k in ("energy", "semi_major_axis", "eccentricity", "inclination", "separation"))
        self.binaries = binaries

    def bound_pairs(self, s: int) -> np.ndarray:
        """The binaries of system ``s``: one row ``(i, j, a, e, energy)`` per mutual pair ``i < j`` with negative energy
        (float64, ``(binaries[s], 5)``)."""
        i = np.nonzero(self.mutual[s] & (self.energy[s] < 0.0) & (np.arange(self.partner.shape[1]) < self.partner[s]))[0]
        return np.stack([i.astype(np.float64), self.partner[s, i].astype(np.float64), self.semi_major_axis[s, i],
                         self.eccentricity[s, i], self.energy[s, i]], axis=1)

    def __repr__(self):
        return f"PairResult(binaries={self.binaries.tolist()})"


class StructureResult:
    """What :meth:`BatchedSystem.structure` found.  Per system: ``centre`` ``(B, 3)``, ``core_radius``, ``core_density``,
    ``total_weight`` (float64, ``(B,)``), ``estimated`` (int32: the bodies that have a ``k``-th neighbour), ``fractions`` as
    given and ``lagrangian`` ``(B, len(fractions))``, the radii about the centre that enclose them.  Per body, ``(B,
    max_bodies)`` arrays or ``None`` without ``bodies``: ``density``, ``radius`` (from the centre), ``enclosed`` (the weight
    within that radius, the body included), ``neighbour_distance`` (float64, to the ``k``-th neighbour; ``inf`` without one),
    ``neighbour_weight`` (float32) and ``inside`` (int32), the weight and number of the bodies strictly nearer than that;
    slots from the count on read 0.  ``k`` and ``weight`` as given, ``counts`` the systems' live counts at the call."""

    def __init__(self, systems, bodies, fractions, k, weight, counts):
        self.k, self.weight = k, weight
        self.counts = np.array(counts, dtype=np.int64)
        self.fractions = np.array(fractions, dtype=np.float64)
        self.centre = np.ascontiguousarray(systems["centre"])
        self.core_radius, self.core_density, self.total_weight, self.estimated = (
            np.ascontiguousarray(systems[name]) for name in ("core_radius", "core_density", "total_weight", "estimated"))
        self.lagrangian = np.ascontiguousarray(systems["lagrange"][:, :len(self.fractions)])
        self.density = self.radius = self.enclosed = self.neighbour_distance = self.neighbour_weight = self.inside = None
        if bodies is not None:
            self.density, self.radius, self.enclosed, self.neighbour_weight, self.inside = (
                np.ascontiguousarray(bodies[name]) for name in ("density", "radius", "enclosed", "neighbour_weight", "inside"))
            self.neighbour_distance = np.sqrt(bodies["neighbour_r2"].astype(np.float64))

    def lagrangian_radii(self, fractions) -> np.ndarray:
        """The header's rule applied on the host to the per-body records, for fractions beyond eight or chosen afterwards:
        ``(B, len(fractions))``, per fraction ``f`` the smallest ``radius`` whose ``enclosed`` is at least ``f * total_weight``,
        the largest radius where no body qualifies, 0 for a system of no weight or no bodies.  Needs ``bodies=True``."""
        if self.radius is None:
            raise ValueError("lagrangian_radii needs the per-body records: structure(bodies=True)")
        f = np.asarray(fractions, dtype=np.float64).reshape(-1)
        if not np.all((f > 0.0) & (f <= 1.0)):
            raise ValueError("a fraction must be in (0, 1]")
        out = np.zeros((self.radius.shape[0], f.size))
        for s in range(self.radius.shape[0]):
            n = int(self.counts[s])
            if self.total_weight[s] == 0.0 or n == 0:
                continue
            radius, enclosed = self.radius[s, :n], self.enclosed[s, :n]
            for q, fq in enumerate(f):
                ok = enclosed >= fq * self.total_weight[s]
                out[s, q] = radius[ok].min() if ok.any() else radius.max()
        return out

    def __repr__(self):
        return f"StructureResult(k={self.k}, weight={self.weight!r}, core_radius={self.core_radius.tolist()})"


class MemberResult:
    """What :meth:`BatchedSystem.members` found.  Per system (``(B,)`` arrays): ``bound_mass`` (float64, the mass words of the
    final member sources), ``centre`` and ``velocity`` (``(B, 3)``, their centre of mass and its velocity; 0 where nothing is
    bound), ``kinetic_energy`` and ``potential_energy`` (over the final member sources, in the last iteration's frame and
    potential: exact for the final set when converged), ``count`` (int32: the final members, test particles included),
    ``sources`` (int32: the final member sources), ``iterations`` (int32: those evaluated) and ``converged`` (bool: the last one
    removed nobody or left no member).  ``source_mass`` (float64): the mass of all sources, members or not, as
    :meth:`BatchedSystem.momentum` counts it.  Per body, ``(B, max_bodies)`` arrays or ``None`` without ``bodies``: ``member``
    (bool), ``removed_at`` (int32: the iteration that removed the body; 0 for a member and for a body outside ``initial``),
    ``potential`` and ``energy`` (float64, the last iteration's); slots from the count on read 0."""

    def __init__(self, systems, bodies, source_mass):
        self.source_mass = np.array(source_mass, dtype=np.float64)
        self.bound_mass = np.ascontiguousarray(systems["bound_mass"])
        self.centre, self.velocity = np.ascontiguousarray(systems["centre"]), np.ascontiguousarray(systems["velocity"])
        self.kinetic_energy, self.potential_energy = np.ascontiguousarray(systems["kinetic"]), np.ascontiguousarray(systems["potential"])
        self.count, self.sources, self.iterations = (np.ascontiguousarray(systems[name]) for name in ("members", "sources", "iterations"))
        self.converged = systems["converged"] != 0
        self.member = self.removed_at = self.potential = self.energy = None
        if bodies is not None:
            self.member = bodies["member"] != 0
            self.removed_at, self.potential, self.energy = (np.ascontiguousarray(bodies[name]) for name in ("removed_at", "potential", "energy"))

    def bound_fraction(self) -> np.ndarray:
        """``(B,)`` float64: ``bound_mass`` over the mass of all sources; 0 for a system without source mass."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.source_mass != 0.0, self.bound_mass / self.source_mass, 0.0)

    def __repr__(self):
        return (f"MemberResult(bound_mass={self.bound_mass.tolist()}, count={self.count.tolist()}, "
                f"iterations={self.iterations.tolist()}, converged={self.converged.tolist()})")


class GravityResult:
    """What :meth:`BatchedSystem.gravity_at` found, per system and row (``P`` rows: the points given, or ``max_bodies``
    without points): ``acceleration`` (``(B, P, 3)`` float32, ``G = 1``), ``potential`` (``(B, P)`` float64, ``<= 0``) and
    ``tidal`` (``(B, P, 3, 3)`` float32, symmetric: ``T_ab = d a_a / d x_b``, whose trace is ``-3 eps^2 sum m (r^2 + eps^2)^-5/2``
    and zero without softening), or ``None`` without ``tidal``.  Rows from the point count or body count on read 0."""

    #: where the six words {xx, xy, xz, yy, yz, zz} of a row go in its 3 x 3 tensor
    TIDAL_INDEX = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])

    def __init__(self, records, tidal):
        self.acceleration = np.ascontiguousarray(records["acceleration"])
        self.potential = np.ascontiguousarray(records["potential"])
        self.tidal = None if tidal is None else np.ascontiguousarray(tidal[..., self.TIDAL_INDEX])

    def __repr__(self):
        B, P = self.potential.shape
        return f"GravityResult(systems={B}, rows={P}, tidal={self.tidal is not None})"


class BatchGroups:
    """What :meth:`BatchedSystem.groups` found.  Per system (``(B,)`` int32 arrays): ``groups`` (those with at least
    ``min_members`` members), ``grouped`` (the bodies in them), ``singles`` (groups of one body), ``largest`` (the root of the
    group with the most members, ties to the lower root; -1 for an empty system), ``largest_count``, ``sweeps`` (the label
    sweeps run) and ``converged`` (bool: the last sweep lowered no label).  Per body, ``(B, max_bodies)`` int32 arrays or ``None``
    without ``bodies``: ``group`` (the root of the body's group, the lowest index among its members; -1 from the count on) and
    ``size`` (its members; 0 from the count on).  Per slot, ``(B, max_bodies)`` arrays or ``None`` without ``records``, filled
    at a group's root and 0 elsewhere: ``weight`` (float64), ``centre`` and ``velocity`` (``(B, max_bodies, 3)`` float64: the
    weighted means; 0 where the weight is 0), ``count`` and ``sources`` (int32: all members, and the massive ones).
    ``linking_length`` (``(B,)`` float32), ``min_members`` and ``weight_kind`` are the call's arguments."""

    def __init__(self, systems, records, bodies, linking_length, min_members, weight):
        self.systems, self.group_records, self.body_records = systems, records, bodies
        self.linking_length, self.min_members, self.weight_kind = np.asarray(linking_length, dtype=np.float32), int(min_members), weight
        for name in ("groups", "grouped", "singles", "largest", "largest_count", "sweeps"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.converged = systems["converged"] != 0
        self.group = self.size = None
        if bodies is not None:
            self.group, self.size = np.ascontiguousarray(bodies["group"]), np.ascontiguousarray(bodies["size"])
        self.weight = self.centre = self.velocity = self.count = self.sources = None
        if records is not None:
            for name in ("weight", "centre", "velocity", "count", "sources"):
                setattr(self, name, np.ascontiguousarray(records[name]))

    def _need_bodies(self, what):
        if self.group is None:
            raise ValueError(f"{what} needs the per-body records: call groups(bodies=True)")

    def roots(self, s: int) -> np.ndarray:
        """The roots of all groups of system ``s`` in ascending order, groups of one body included."""
        self._need_bodies("roots")
        g = self.group[s]
        return np.flatnonzero(g == np.arange(g.shape[0])).astype(np.int32)

    def groups_of(self, s: int) -> list:
        """The member index arrays (ascending) of system ``s``'s groups with at least ``min_members`` members, the largest
        group first, ties by the lower root."""
        self._need_bodies("groups_of")
        g, size = self.group[s], self.size[s]
        roots = [int(r) for r in self.roots(s) if size[r] >= self.min_members]
        roots.sort(key=lambda r: (-int(size[r]), r))
        return [np.flatnonzero(g == r) for r in roots]

    def largest_mask(self) -> np.ndarray:
        """``(B, max_bodies)`` bool: the members of every system's largest group -- a starting set for
        :meth:`BatchedSystem.members` (``initial=``)."""
        self._need_bodies("largest_mask")
        return (self.group == self.largest[:, None]) & (self.group >= 0)

    def __repr__(self):
        return (f"BatchGroups(groups={self.groups.tolist()}, largest_count={self.largest_count.tolist()}, "
                f"sweeps={self.sweeps.tolist()}, converged={self.converged.tolist()})")


class SpanResult:
    """What :meth:`BatchedSystem.spanning_tree` found.  Per system (``(B,)`` arrays): ``edges`` (int32: ``selected - 1``, or 0
    below two selected bodies), ``selected`` (int32: the vertices), ``rounds`` (int32: the rounds the search ran),
    ``total_length`` and ``longest`` (float64: the sum of the edge lengths in ascending order, and the last of them) and
    ``mean_separation`` (float64: the mean distance of two selected bodies; 0 without ``separations``).  Per slot,
    ``(B, max_bodies)`` arrays or ``None`` without ``edges``: ``i``, ``j`` (int32, ``i < j``) and ``r2`` (float32: the squared
    length) of the ``e``-th shortest edge; -1, -1 and 0 from ``edges`` on.  Per body, ``(B, max_bodies)`` int32 arrays or
    ``None`` without ``bodies``: ``degree`` (the tree edges at the body) and ``nearest`` (its nearest selected body, always a
    tree neighbour); 0 and -1 for a body that is not selected, beyond the count or alone."""

    def __init__(self, systems, edges, bodies, separations, vertices):
        self.systems, self.edge_records, self.body_records, self.separations = systems, edges, bodies, bool(separations)
        self.vertices = vertices
        for name in ("edges", "selected", "rounds", "total_length", "longest", "mean_separation"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.i = self.j = self.r2 = self.degree = self.nearest = None
        if edges is not None:
            self.i, self.j, self.r2 = (np.ascontiguousarray(edges[name]) for name in ("i", "j", "r2"))
        if bodies is not None:
            self.degree, self.nearest = np.ascontiguousarray(bodies["degree"]), np.ascontiguousarray(bodies["nearest"])

    def _need_edges(self, what):
        if self.i is None:
            raise ValueError(f"{what} needs the per-slot records: call spanning_tree(edges=True)")

    def edges_of(self, s: int):
        """``(ends, lengths)`` of system ``s``: an ``(E, 2)`` int32 array of the edges' ends in ascending order of length, and
        their float64 lengths, the terms of ``total_length``."""
        self._need_edges("edges_of")
        E = int(self.edges[s])
        ends = np.stack([self.i[s, :E], self.j[s, :E]], axis=1).astype(np.int32)
        return ends, np.sqrt(self.r2[s, :E].astype(np.float64))

    def _b2(self, b):
        """The fp32 product ``b b`` that :meth:`BatchedSystem.groups` compares with; a scalar or one value per system."""
        b = np.asarray(b, dtype=np.float32)
        if b.ndim == 0:
            b = np.full(self.edges.shape[0], b, dtype=np.float32)
        b = b.reshape(-1)
        if b.shape[0] != self.edges.shape[0]:
            raise ValueError(f"expected one linking length or {self.edges.shape[0]}, got {b.shape[0]}")
        return b * b

    def group_count(self, b) -> np.ndarray:
        """``(B,)`` int32: into how many pieces every system falls at the linking length ``b`` (a scalar, or one per system):
        1 + the edges with ``r2 > b2``; 0 without selected bodies.  This is ``groups(b, min_members=1).groups`` where all
        bodies are selected."""
        self._need_edges("group_count")
        b2 = self._b2(b)
        live = np.arange(self.r2.shape[1])[None, :] < self.edges[:, None]
        cut = (live & (self.r2 > b2[:, None])).sum(axis=1)
        return np.where(self.selected > 0, 1 + cut, 0).astype(np.int32)

    def labels_at(self, s: int, b) -> np.ndarray:
        """``(max_bodies,)`` int32: for every selected body of system ``s`` the lowest index of its piece at the linking length
        ``b`` -- :meth:`BatchedSystem.groups`' ``group`` where all bodies are selected; -1 for a body that is not selected or
        beyond the count.  A union-find over the edges with ``r2 <= b2``."""
        self._need_edges("labels_at")
        b2 = self._b2(b)[s]
        n = self.r2.shape[1]
        parent = list(range(n))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        E = int(self.edges[s])
        for a, c, r2 in zip(self.i[s, :E].tolist(), self.j[s, :E].tolist(), self.r2[s, :E].tolist()):
            if np.float32(r2) <= b2:
                ra, rc = find(a), find(c)
                parent[max(ra, rc)] = min(ra, rc)
        labels = np.array([find(a) for a in range(n)], dtype=np.int32)
        return np.where(self.vertices[s], labels, -1).astype(np.int32)

    def linking_length_for(self, pieces: int) -> np.ndarray:
        """``(B,)`` float64: the length of the ``(pieces - 1)``-th longest edge: at linking lengths below it, down to the next
        edge, a system is in ``pieces`` pieces.  NaN where a system has fewer than ``pieces - 1`` edges."""
        self._need_edges("linking_length_for")
        if pieces < 2:
            raise ValueError("pieces must be at least 2")
        at = self.edges.astype(np.int64) - (pieces - 1)
        r2 = np.take_along_axis(self.r2, np.clip(at, 0, self.r2.shape[1] - 1)[:, None], axis=1)[:, 0].astype(np.float64)
        return np.where(at >= 0, np.sqrt(r2), np.nan)

    def q_parameter(self, radius) -> np.ndarray:
        """``(B,)`` float64: the Q of Cartwright & Whitworth (2004), ``m / s`` with ``m = total_length / (N^2 V)^(1/3)``,
        ``V = 4 pi R^3 / 3``, ``s = mean_separation / R`` and ``N = selected``.  ``radius`` is the cluster radius ``R``, a
        scalar or one value per system.  Needs ``spanning_tree(separations=True)``.  Q above 0.8 speaks for a central
        concentration, below for substructure.  NaN below two selected bodies."""
        if not self.separations:
            raise ValueError("q_parameter needs the mean separation: call spanning_tree(separations=True)")
        R = np.broadcast_to(np.asarray(radius, dtype=np.float64), self.total_length.shape)
        N = self.selected.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = self.total_length / np.cbrt(N * N * (4.0 * np.pi * R ** 3 / 3.0))
            s = self.mean_separation / R
            return np.where(self.selected >= 2, m / s, np.nan)

    def __repr__(self):
        return (f"SpanResult(edges={self.edges.tolist()}, total_length={self.total_length.tolist()}, "
                f"rounds={self.rounds.tolist()})")


class NeighbourResult:
    """What :meth:`BatchedSystem.neighbours` found.  Per list slot, ``(B, max_bodies, k)`` arrays or ``None`` without
    ``lists``: ``index`` (int32: the ``t``-th nearest source of the body; -1 from ``found`` on and beyond the count), ``r2``
    (float32: its squared distance; +inf there) and ``distance`` (float64: ``sqrt`` of it, formed on the host).  Per body,
    ``(B, max_bodies)`` int32 arrays or ``None`` without ``bodies``: ``found`` (the filled slots, ``min(k, candidates)``) and
    ``within`` (the sources within ``radius``; 0 without one).  Per system (``(B,)`` arrays): ``bodies`` (int32: the rows),
    ``sources`` (the selected bodies), ``listed`` (rows with a neighbour), ``complete`` (rows with ``k``), ``mutual`` (rows
    whose nearest body's nearest they are), ``mean_nearest`` and ``mean_kth`` (float64: the mean distance to the nearest
    source over the listed rows, and to the ``k``-th over the complete ones).  ``systems`` and ``body_records`` are the
    records themselves; ``k`` is the list length asked for."""

    def __init__(self, systems, bodies, index, r2, k):
        self.systems, self.body_records, self.index, self.r2, self.k = systems, bodies, index, r2, int(k)
        for name in ("bodies", "sources", "listed", "complete", "mutual", "mean_nearest", "mean_kth"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.distance = None if r2 is None else np.sqrt(r2.astype(np.float64))
        self.found = self.within = None
        if bodies is not None:
            self.found, self.within = np.ascontiguousarray(bodies["found"]), np.ascontiguousarray(bodies["within"])

    def gather(self, values, fill=np.nan) -> np.ndarray:
        """``values``, a ``(B, max_bodies, ...)`` array of one entry per body, at the neighbours' indices:
        ``(B, max_bodies, k, ...)``, with ``fill`` where a slot is empty.  The velocity dispersion about every body's
        neighbours is ``res.gather(v).std(axis=2)``.  Integer ``values`` need an integer ``fill``."""
        if self.index is None:
            raise ValueError("gather needs the lists: call neighbours(lists=True)")
        values = np.asarray(values)
        B, n, k = self.index.shape
        if values.shape[:2] != (B, n):
            raise ValueError(f"values must have shape ({B}, {n}, ...), got {tuple(values.shape)}")
        empty = self.index < 0
        out = values[np.arange(B)[:, None, None], np.where(empty, 0, self.index)]
        out = out.astype(np.result_type(out.dtype, np.asarray(fill).dtype), copy=True)
        out[empty] = fill
        return out

    def __repr__(self):
        return (f"NeighbourResult(k={self.k}, listed={self.listed.tolist()}, complete={self.complete.tolist()}, "
                f"mutual={self.mutual.tolist()}, mean_nearest={self.mean_nearest.tolist()})")


class CorrelationResult:
    """What :meth:`BatchedSystem.correlation` counted.  ``edges`` are the bin edges as given (float32, ``(bins + 1,)`` or
    ``(B, bins + 1)``); ``counts`` is ``(B, bins)`` int64, the ordered pairs (row, source) with
    ``edges[t] < r <= edges[t + 1]``, or ``None`` without ``counts``.  Per system (``(B,)`` arrays): ``rows`` and ``sources``
    (int32: the selected bodies below the count), ``both`` (those that are a row and a source), ``pairs`` (int64: the pairs
    examined, ``rows * sources - both``), ``below`` (within the first edge; with a first edge of 0 the coincident pairs),
    ``above`` (beyond the last edge) and ``unmeasured`` (a NaN or infinite coordinate), so that
    ``below + counts.sum(axis=1) + above + unmeasured == pairs``.  ``auto`` (bool) tells where rows and sources are the same
    bodies: there every unordered pair was counted twice, every count is even and ``unordered`` is ``counts // 2`` (-1
    elsewhere).  ``systems`` is the records themselves, ``bins`` the number of bins."""

    def __init__(self, systems, counts, edges):
        self.systems, self.counts, self.edges = systems, counts, edges
        for name in ("rows", "sources", "both", "pairs", "below", "above", "unmeasured"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.bins = int(edges.shape[-1]) - 1
        self.auto = (self.rows == self.both) & (self.sources == self.both)

    def _need_counts(self):
        if self.counts is None:
            raise ValueError("this needs the bins: call correlation(counts=True)")

    def _edges(self) -> np.ndarray:
        """``(B, bins + 1)`` float64."""
        return np.broadcast_to(self.edges.astype(np.float64), (len(self.systems), self.bins + 1))

    @property
    def unordered(self) -> np.ndarray:
        """``(B, bins)`` int64: the unordered pairs per bin where ``auto``, -1 in the systems where not."""
        self._need_counts()
        return np.where(self.auto[:, None], self.counts // 2, -1)

    def cumulative(self) -> np.ndarray:
        """``(B, bins)`` int64: the ordered pairs within the upper edge of every bin, ``below + cumsum(counts)``: what
        ``neighbours(radius=edge).within`` sums to over the rows.  Divided by ``pairs`` it is the correlation integral."""
        self._need_counts()
        return self.below[:, None] + np.cumsum(self.counts, axis=1)

    def shell_volumes(self) -> np.ndarray:
        """``(B, bins)`` float64: ``4 pi / 3 (hi^3 - lo^3)`` of every bin."""
        e = self._edges()
        return 4.0 / 3.0 * np.pi * (e[:, 1:] ** 3 - e[:, :-1] ** 3)

    def density(self) -> np.ndarray:
        """``(B, bins)`` float64: the ordered counts per row and shell volume -- the mean number density of sources around a
        row at that separation.  NaN in a system without rows."""
        self._need_counts()
        rows = np.where(self.rows > 0, self.rows, 1).astype(np.float64)[:, None]
        return np.where(self.rows[:, None] > 0, self.counts / rows / self.shell_volumes(), np.nan)

    def xi(self, mean_density) -> np.ndarray:
        """``(B, bins)`` float64: the two-point correlation function against a mean source density (a scalar or ``B`` values):
        ``density() / mean_density - 1``."""
        mean = np.asarray(mean_density, dtype=np.float64)
        return self.density() / (mean[:, None] if mean.ndim == 1 else mean) - 1.0

    def correlation_dimension(self, lo: int = 0, hi=None) -> np.ndarray:
        """``(B,)`` float64: the slope of ``log cumulative()`` against the log of the bins' upper edges over the bins
        ``lo ... hi`` (both included; ``hi`` defaults to the last), by least squares: the correlation dimension D2 where the
        correlation integral is a power law.  NaN where a cumulative count in the range is 0."""
        hi = self.bins - 1 if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi < self.bins:
            raise ValueError(f"need 0 <= lo < hi < {self.bins}, got {lo} and {hi}")
        c = self.cumulative()[:, lo:hi + 1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(c > 0, np.log(np.where(c > 0, c, 1.0)), np.nan)
            x = np.log(self._edges()[:, lo + 1:hi + 2])
            x = x - x.mean(axis=1, keepdims=True)
            return (x * (y - y.mean(axis=1, keepdims=True))).sum(axis=1) / (x * x).sum(axis=1)

    @staticmethod
    def landy_szalay(dd, dr, rr, n_d, n_r) -> np.ndarray:
        """The Landy-Szalay estimator ``(DD - 2 DR + RR) / RR`` of xi from three ordered counts as :meth:`correlation` gives
        them -- ``dd`` data around data, ``dr`` data around randoms (or randoms around data), ``rr`` randoms around randoms --
        each normalised by its ordered pairs: ``n_d (n_d - 1)``, ``n_d n_r`` and ``n_r (n_r - 1)``.  NaN where ``rr`` is 0."""
        dd, dr, rr = (np.asarray(a, dtype=np.float64) for a in (dd, dr, rr))
        n_d, n_r = np.asarray(n_d, dtype=np.float64), np.asarray(n_r, dtype=np.float64)
        n_d, n_r = (n[:, None] if n.ndim == 1 else n for n in (n_d, n_r))
        DD, DR, RR = dd / (n_d * (n_d - 1.0)), dr / (n_d * n_r), rr / (n_r * (n_r - 1.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(RR > 0, (DD - 2.0 * DR + RR) / np.where(RR > 0, RR, 1.0), np.nan)

    def __repr__(self):
        return (f"CorrelationResult(bins={self.bins}, pairs={self.pairs.tolist()}, below={self.below.tolist()}, "
                f"above={self.above.tolist()}, unmeasured={self.unmeasured.tolist()})")


class ContactsResult:
    """What :meth:`BatchedSystem.contacts` listed.  Per system (``(B,)`` arrays): ``pairs`` (int64: the contacts, exact
    whatever the capacity), ``stored`` (int64: those in the list, ``min(pairs, capacity)``), ``truncated`` (bool:
    ``stored < pairs``), ``bodies`` (int32: the bodies taking part), ``touching`` (those with a contact), ``max_degree``,
    ``closest`` (``(B, 2)`` int32: the contact of smallest separation, ``i < j``, -1 without one) and ``closest_distance``
    (float64, ``inf`` without one).  Per body (``(B, max_bodies)`` int32, ``None`` without ``bodies``): ``degree`` (its
    contacts), ``upper`` (those of higher index), ``first`` (where its entries start in the list: the exclusive sum of
    ``upper``) and ``nearest`` (the partner of smallest separation, ties to the lower index, -1 without one).  The list
    (``(B, capacity)``, ``None`` without ``lists``): ``i``, ``j`` (int32, -1 from ``stored`` on), ``r2`` (float32, ``inf`` from
    ``stored`` on) and ``distance`` (float64).  ``systems``, ``body_records`` and ``entries`` are the records themselves."""

    def __init__(self, systems, bodies, entries):
        self.systems, self.body_records, self.entries = systems, bodies, entries
        for name in ("pairs", "stored", "bodies", "touching", "max_degree"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.truncated = self.stored < self.pairs
        self.closest = np.stack([systems["closest_i"], systems["closest_j"]], axis=1)
        self.closest_r2 = np.ascontiguousarray(systems["closest_r2"])
        self.closest_distance = np.sqrt(self.closest_r2.astype(np.float64))
        for name in ("degree", "upper", "first", "nearest"):
            setattr(self, name, None if bodies is None else np.ascontiguousarray(bodies[name]))
        for name in ("i", "j", "r2"):
            setattr(self, name, None if entries is None else np.ascontiguousarray(entries[name]))
        self.distance = None if entries is None else np.sqrt(self.r2.astype(np.float64))
        self.capacity = 0 if entries is None else int(entries.shape[1])

    def _need_list(self):
        if self.entries is None:
            raise ValueError("this needs the list: call contacts(lists=True)")

    def pairs_of(self, s: int) -> np.ndarray:
        """``(stored[s], 2)`` int32: the listed contacts of system ``s`` as rows ``(i, j)``, ``i < j``, in the list's order."""
        self._need_list()
        m = int(self.stored[s])
        return np.stack([self.i[s, :m], self.j[s, :m]], axis=1)

    def partners_of(self, s: int, i: int) -> np.ndarray:
        """int32, ascending: every body in contact with body ``i`` of system ``s``, from the list, in both directions.  Raises
        where the system is truncated: the list would not hold them all."""
        self._need_list()
        if self.truncated[s]:
            raise ValueError(f"system {s} is truncated ({int(self.stored[s])} of {int(self.pairs[s])} contacts): call again with more capacity")
        p = self.pairs_of(s)
        return np.sort(np.concatenate([p[p[:, 0] == i, 1], p[p[:, 1] == i, 0]]))

    def __repr__(self):
        return (f"ContactsResult(pairs={self.pairs.tolist()}, stored={self.stored.tolist()}, touching={self.touching.tolist()}, "
                f"max_degree={self.max_degree.tolist()}, closest={self.closest.tolist()})")


class ApproachesResult:
    """What :meth:`BatchedSystem.approaches` listed.  Per system (``(B,)`` arrays): ``pairs`` (int64: the approaches, exact
    whatever the capacity), ``stored`` (int64: those in the list, ``min(pairs, capacity)``), ``truncated`` (bool:
    ``stored < pairs``), ``bodies`` (int32: the bodies taking part), ``approaching`` (those with an approach), ``max_degree``,
    ``now_pairs``, ``passing`` and ``ending`` (int32: the pairs of phase 0, 1 and 2, which add up to ``pairs``) and ``horizon``
    (float64: the call's).  Per body (``(B, max_bodies)`` int32, ``None`` without ``bodies``): ``degree`` (its approaches),
    ``upper`` (those of higher index), ``first`` (where its entries start in the list: the exclusive sum of ``upper``) and
    ``now`` (those of phase 0: its :meth:`BatchedSystem.contacts` degree).  The list (``(B, capacity)``, ``None`` without
    ``lists``): ``i``, ``j`` (int32, -1 from ``stored`` on), ``r2``, ``rv``, ``v2`` (float32: the separation squared, ``d . w``
    and the relative speed squared, from ``i`` to ``j``), ``phase`` (int32: 0 now, 1 passage, 2 end, -1 from ``stored`` on) and,
    derived here in float64 from those words, ``time`` (0, ``-rv / v2`` and the horizon by phase) and ``miss_distance``
    (``sqrt(r2)``, ``sqrt(max(0, r2 - rv^2 / v2))`` and ``sqrt(r2 + 2 rv H + v2 H^2)``), both ``inf`` from ``stored`` on.
    ``systems``, ``body_records`` and ``entries`` are the records themselves."""

    def __init__(self, systems, bodies, entries, horizon):
        self.systems, self.body_records, self.entries = systems, bodies, entries
        self.horizon = np.asarray(horizon, dtype=np.float64)
        for name in ("pairs", "stored", "bodies", "approaching", "max_degree", "passing", "ending"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.now_pairs = np.ascontiguousarray(systems["now"])
        self.truncated = self.stored < self.pairs
        for name in ("degree", "upper", "first", "now"):
            setattr(self, name, None if bodies is None else np.ascontiguousarray(bodies[name]))
        for name in ("i", "j", "r2", "rv", "v2", "phase"):
            setattr(self, name, None if entries is None else np.ascontiguousarray(entries[name]))
        self.capacity = 0 if entries is None else int(entries.shape[1])
        self.time = self.miss_distance = None
        if entries is not None:
            r2, rv, v2 = (getattr(self, name).astype(np.float64) for name in ("r2", "rv", "v2"))
            H = np.broadcast_to(self.horizon[:, None], r2.shape)
            with np.errstate(divide="ignore", invalid="ignore"):
                passage = -rv / v2
                time = np.select([self.phase == 0, self.phase == 1, self.phase == 2], [0.0, passage, H], np.inf)
                miss2 = np.select([self.phase == 0, self.phase == 1, self.phase == 2],
                                  [r2, r2 - rv * rv / v2, r2 + 2.0 * rv * H + v2 * H * H], np.inf)
            self.time, self.miss_distance = time, np.sqrt(np.maximum(miss2, 0.0))

    def _need_list(self):
        if self.entries is None:
            raise ValueError("this needs the list: call approaches(lists=True)")

    def pairs_of(self, s: int) -> np.ndarray:
        """``(stored[s], 2)`` int32: the listed approaches of system ``s`` as rows ``(i, j)``, ``i < j``, in the list's order."""
        self._need_list()
        m = int(self.stored[s])
        return np.stack([self.i[s, :m], self.j[s, :m]], axis=1)

    def partners_of(self, s: int, i: int) -> np.ndarray:
        """int32, ascending: every body that approaches body ``i`` of system ``s``, from the list, in both directions.  Raises
        where the system is truncated: the list would not hold them all."""
        self._need_list()
        if self.truncated[s]:
            raise ValueError(f"system {s} is truncated ({int(self.stored[s])} of {int(self.pairs[s])} approaches): call again with more capacity")
        p = self.pairs_of(s)
        return np.sort(np.concatenate([p[p[:, 0] == i, 1], p[p[:, 1] == i, 0]]))

    def soonest(self, s: int):
        """``(entries, time, miss_distance)`` of system ``s``'s listed approaches ordered by ``time``, ties in the list's order:
        the records, and the two float64 arrays that go with them.  The first is the next encounter."""
        self._need_list()
        m = int(self.stored[s])
        order = np.argsort(self.time[s, :m], kind="stable")
        return self.entries[s, :m][order], self.time[s, :m][order], self.miss_distance[s, :m][order]

    def __repr__(self):
        return (f"ApproachesResult(pairs={self.pairs.tolist()}, stored={self.stored.tolist()}, now={self.now_pairs.tolist()}, "
                f"passing={self.passing.tolist()}, ending={self.ending.tolist()}, approaching={self.approaching.tolist()})")


class RadialProfileResult:
    """What :meth:`BatchedSystem.radial_profile` found.  ``edges`` as given (float64, ``(shells + 1,)`` or ``(B, shells + 1)``),
    ``shells`` their number less one, ``weight`` as given and ``projected`` (``None``, or the axis left out).  Per system
    (``(B,)`` arrays): ``selected`` (int32: the bodies taking part), ``below`` (within the first edge), ``above`` (beyond the
    last) and ``unmeasured`` (a NaN or infinite coordinate or velocity), so that ``below + count.sum(axis=1) + above +
    unmeasured == selected``; ``total_weight`` (float64: the weight of all measured bodies taking part, ``below`` and ``above``
    included); ``centre`` and ``velocity`` ``(B, 3)``, the frame as used.  Per shell, ``None`` without ``shells``: ``count``
    ``(B, shells)`` int64, and the float64 sums over the shell's members in ascending body index ``weight_sum`` (w), ``radius``
    (w r), ``vr1`` (w vr), ``vr2`` (w vr vr), ``vt2`` (w vt2), all ``(B, shells)``; ``L`` (w d x u) and ``U`` (w u), ``(B,
    shells, 3)``; ``M`` (w d_a d_b) and ``V`` (w u_a u_b), ``(B, shells, 6)`` in the order xx, yy, zz, xy, xz, yz.  Per body,
    ``(B, max_bodies)`` or ``None`` without ``bodies``: ``body_shell`` (int32: the shell, -1 below, ``shells`` above, -2
    unmeasured, -3 not taking part), ``body_radius`` and ``body_radial_velocity`` (float64).  ``systems``, ``shell_records`` and
    ``body_records`` are the records themselves.  The derived values below are computed on the host in float64; one that
    divides by a shell's weight is NaN where the shell is empty (or weighs nothing)."""

    def __init__(self, systems, shells, bodies, edges, weight):
        self.systems, self.shell_records, self.body_records, self.edges, self.weight = systems, shells, bodies, edges, weight
        for name in ("selected", "below", "above", "unmeasured", "total_weight", "centre", "velocity"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.shells = int(edges.shape[-1]) - 1
        p = int(systems["projected"][0]) if len(systems) else -1
        self.projected = None if p < 0 else p
        self.count = self.weight_sum = self.radius = self.vr1 = self.vr2 = self.vt2 = self.L = self.U = self.M = self.V = None
        if shells is not None:
            self.count = np.ascontiguousarray(shells["count"])
            self.weight_sum = np.ascontiguousarray(shells["weight"])
            for name in ("radius", "vr1", "vr2", "vt2", "L", "U", "M", "V"):
                setattr(self, name, np.ascontiguousarray(shells[name]))
        self.body_shell = self.body_radius = self.body_radial_velocity = None
        if bodies is not None:
            self.body_shell, self.body_radius, self.body_radial_velocity = (
                np.ascontiguousarray(bodies[name]) for name in ("shell", "radius", "radial_velocity"))

    def _need_shells(self):
        if self.count is None:
            raise ValueError("this needs the shell records: call radial_profile(shells=True)")

    def _edges(self) -> np.ndarray:
        """``(B, shells + 1)`` float64."""
        return np.broadcast_to(self.edges, (len(self.systems), self.shells + 1))

    def _per_weight(self, total) -> np.ndarray:
        """``total / weight_sum`` with the weight broadcast over trailing axes, NaN where the weight is not > 0."""
        self._need_shells()
        w = self.weight_sum.reshape(self.weight_sum.shape + (1,) * (total.ndim - 2))
        ok = w > 0.0
        return np.where(ok, total / np.where(ok, w, 1.0), np.nan)

    @staticmethod
    def _tensor(t6) -> np.ndarray:
        """``(..., 6)`` in the order xx, yy, zz, xy, xz, yz as symmetric ``(..., 3, 3)``."""
        return t6[..., [0, 3, 4, 3, 1, 5, 4, 5, 2]].reshape(t6.shape[:-1] + (3, 3))

    def mean_radius(self) -> np.ndarray:
        """``(B, shells)``: the weighted mean radius of every shell's members."""
        return self._per_weight(self.radius)

    def volume(self) -> np.ndarray:
        """``(B, shells)``: ``4 pi / 3 (hi^3 - lo^3)`` of every shell; in projected mode the area ``pi (hi^2 - lo^2)`` of the
        annulus."""
        e = self._edges()
        if self.projected is not None:
            return np.pi * (e[:, 1:] ** 2 - e[:, :-1] ** 2)
        return 4.0 / 3.0 * np.pi * (e[:, 1:] ** 3 - e[:, :-1] ** 3)

    def density(self) -> np.ndarray:
        """``(B, shells)``: the weight per volume (per area, projected); 0 in an empty shell."""
        self._need_shells()
        return self.weight_sum / self.volume()

    def number_density(self) -> np.ndarray:
        """``(B, shells)``: the members per volume (per area, projected); 0 in an empty shell."""
        self._need_shells()
        return self.count / self.volume()

    def cumulative_weight(self) -> np.ndarray:
        """``(B, shells)``: the weight between the first edge and the outer edge of every shell.  The bodies within the first
        edge (``below``) are not in it: ``total_weight`` is the weight of all measured bodies, those and ``above`` included."""
        self._need_shells()
        return np.cumsum(self.weight_sum, axis=1)

    def radial_velocity(self) -> np.ndarray:
        """``(B, shells)``: the weighted mean radial velocity."""
        return self._per_weight(self.vr1)

    def sigma_r(self) -> np.ndarray:
        """``(B, shells)``: the radial velocity dispersion, ``sqrt(<vr^2> - <vr>^2)``."""
        return np.sqrt(np.maximum(self._per_weight(self.vr2) - self.radial_velocity() ** 2, 0.0))

    def sigma_t(self, rotation: bool = False) -> np.ndarray:
        """``(B, shells)``: the tangential velocity dispersion per tangential direction, ``sqrt(<vt^2> / 2)``.  With
        ``rotation`` the mean rotation is taken off first: ``sqrt((<vt^2> - v_rot^2) / 2)`` with the streaming speed ``v_rot =
        |L| / (sum of w r)``, the shell's angular momentum over its weighted radius."""
        vt2 = self._per_weight(self.vt2)
        if rotation:
            ok = self.radius > 0.0
            v_rot = np.where(ok, np.linalg.norm(self.L, axis=2) / np.where(ok, self.radius, 1.0), np.nan)
            vt2 = np.maximum(vt2 - v_rot ** 2, 0.0)
        return np.sqrt(vt2 / 2.0)

    def anisotropy(self) -> np.ndarray:
        """``(B, shells)``: Binney's ``beta = 1 - <vt^2> / (2 <vr^2>)``: 0 isotropic, 1 radial, negative tangential.  NaN where
        ``<vr^2>`` is 0.  Spherical shells only."""
        if self.projected is not None:
            raise ValueError("the anisotropy needs spherical shells: radial_profile(projected=None)")
        vr2, vt2 = self._per_weight(self.vr2), self._per_weight(self.vt2)
        ok = vr2 > 0.0
        return np.where(ok, 1.0 - vt2 / (2.0 * np.where(ok, vr2, 1.0)), np.nan)

    def specific_angular_momentum(self) -> np.ndarray:
        """``(B, shells, 3)``: ``L / W``, the weighted mean of ``d x u``."""
        return self._per_weight(self.L)

    def dispersion_tensor(self) -> np.ndarray:
        """``(B, shells, 3, 3)``: ``V / W - (U / W)(U / W)^T``, the velocity dispersion tensor about the shell's mean velocity."""
        mean = self._per_weight(self.U)
        return self._tensor(self._per_weight(self.V)) - mean[..., :, None] * mean[..., None, :]

    def axis_ratios(self) -> np.ndarray:
        """``(B, shells, 2)``: ``b / a`` and ``c / a`` of every shell, the square roots of the ratios of the eigenvalues
        (``numpy.linalg.eigvalsh``) of the shape tensor ``M / W`` to its largest.  NaN where the shell is empty."""
        m = self._tensor(self._per_weight(self.M))
        ok = np.isfinite(m).all(axis=(2, 3))
        lam = np.linalg.eigvalsh(np.where(ok[..., None, None], m, np.eye(3)))  # ascending
        top = lam[..., 2]
        good = ok & (top > 0.0)
        ratio = np.maximum(lam[..., 1::-1], 0.0) / np.where(good, top, 1.0)[..., None]
        return np.where(good[..., None], np.sqrt(ratio), np.nan)

    def circular_velocity(self) -> np.ndarray:
        """``(B, shells)``: ``sqrt(cumulative_weight() / outer edge)``, the circular speed at every shell's outer edge from the
        weight between the first edge and it (``below`` is not in it), with G = 1."""
        return np.sqrt(self.cumulative_weight() / self._edges()[:, 1:])

    def __repr__(self):
        return (f"RadialProfileResult(shells={self.shells}, weight={self.weight!r}, projected={self.projected}, "
                f"selected={self.selected.tolist()}, below={self.below.tolist()}, above={self.above.tolist()}, "
                f"unmeasured={self.unmeasured.tolist()})")


class SurfaceMapResult:
    """What :meth:`BatchedSystem.surface_map` found.  ``edges_a`` and ``edges_b`` as used (float64, ``(bins + 1,)`` or ``(B,
    bins + 1)``), ``columns`` and ``rows`` their numbers less one, ``axes`` ``(B, 3, 3)`` the rows ``A``, ``B`` and ``Q`` of
    every system and ``weight`` as given.  Per system (``(B,)`` arrays): ``selected`` (int32: the bodies taking part),
    ``outside`` (beyond the grid) and ``unmeasured`` (a word that is not finite), so that ``outside + count.sum(axis=(1, 2)) +
    unmeasured == selected``; ``occupied`` (the cells with a member), ``peak`` (the cell ``j * columns + i`` with the most
    members, ties to the lower index, -1 if there is none) and ``peak_count``; ``total_weight`` (float64: the weight of all
    measured bodies taking part, ``outside`` included); ``centre`` and ``velocity`` ``(B, 3)``, the frame as used.  Per cell,
    ``(B, rows, columns)`` or ``None`` without ``cells``: ``count`` (int64) and the float64 sums over the cell's members in
    ascending body index ``weight_sum`` (w), ``v1`` (w uq), ``v2`` (w uq uq), ``pa`` (w ua), ``pb`` (w ub), ``z1`` (w q) and
    ``z2`` (w q q), with ``uq`` the velocity along the line of sight, ``ua`` and ``ub`` those in the plane and ``q`` the depth.
    Per body, ``(B, max_bodies)`` or ``None`` without ``bodies``: ``body_cell`` (int32: the cell, -1 outside, -2 unmeasured, -3
    not taking part), ``body_a`` and ``body_b`` (float64: the rotated coordinates).  ``systems``, ``cell_records`` and
    ``body_records`` are the records themselves.  The derived values below are computed on the host in float64; the moments
    are NaN where a cell is empty (or weighs nothing)."""

    def __init__(self, systems, cells, bodies, edges_a, edges_b, axes, weight):
        self.systems, self.cell_records, self.body_records = systems, cells, bodies
        self.edges_a, self.edges_b, self.axes, self.weight = edges_a, edges_b, axes, weight
        for name in ("selected", "outside", "unmeasured", "occupied", "peak", "peak_count", "total_weight", "centre", "velocity"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.columns, self.rows = int(edges_a.shape[-1]) - 1, int(edges_b.shape[-1]) - 1
        self.count = self.weight_sum = self.v1 = self.v2 = self.pa = self.pb = self.z1 = self.z2 = None
        if cells is not None:
            self.count = np.ascontiguousarray(cells["count"])
            self.weight_sum = np.ascontiguousarray(cells["weight"])
            for name in ("v1", "v2", "pa", "pb", "z1", "z2"):
                setattr(self, name, np.ascontiguousarray(cells[name]))
        self.body_cell = self.body_a = self.body_b = None
        if bodies is not None:
            self.body_cell, self.body_a, self.body_b = (np.ascontiguousarray(bodies[name]) for name in ("cell", "a", "b"))

    @staticmethod
    def grid(extent, bins) -> np.ndarray:
        """``bins + 1`` evenly spaced float64 edges (``numpy.linspace``): ``extent`` is ``(lo, hi)``, or one number for ``(-extent,
        extent)``.  With ``(B, 2)`` extents, ``(B, bins + 1)``: one set per system."""
        e = np.asarray(extent, dtype=np.float64)
        if e.ndim == 0:
            e = np.array([-float(e), float(e)])
        if e.shape[-1] != 2 or int(bins) < 1:
            raise ValueError(f"extent must be a number, (lo, hi) or (B, 2) and bins >= 1, got {extent!r} and {bins!r}")
        return np.ascontiguousarray(np.linspace(e[..., 0], e[..., 1], int(bins) + 1, axis=-1))

    @staticmethod
    def view(direction, up=(0.0, 0.0, 1.0)) -> np.ndarray:
        """The right-handed orthonormal triple ``(A, B, Q)`` of an observer who looks along ``direction``: ``Q = direction /
        |direction|`` (the line of sight, pointing away from the observer), ``A = up x Q`` normalised (the map's first axis,
        to the right of an observer whose head points along ``up``), ``B = Q x A``, so that ``A x B = Q``.  Where ``up`` is
        parallel to the direction the coordinate axis least aligned with it stands in.  ``direction`` ``(3,)`` gives ``(3, 3)``
        and ``(B, 3)`` gives ``(B, 3, 3)``: one view per system."""
        d = np.asarray(direction, dtype=np.float64)
        if d.shape[-1:] != (3,) or d.ndim > 2:
            raise ValueError(f"direction must have shape (3,) or (B, 3), got {tuple(d.shape)}")
        norm = np.linalg.norm(d, axis=-1, keepdims=True)
        if not np.all(np.isfinite(d)) or not np.all(norm > 0.0):
            raise ValueError("direction must be finite and not zero")
        q = d / norm
        u = np.broadcast_to(np.asarray(up, dtype=np.float64), q.shape)
        a = np.cross(u, q)
        flat = np.linalg.norm(a, axis=-1) < 1.0e-12 * np.linalg.norm(u, axis=-1)
        if np.any(flat):
            spare = np.eye(3)[np.argmin(np.abs(q), axis=-1)]
            a = np.where(flat[..., None], np.cross(spare, q), a)
        a = a / np.linalg.norm(a, axis=-1, keepdims=True)
        return np.ascontiguousarray(np.stack([a, np.cross(q, a), q], axis=-2))

    def _need_cells(self):
        if self.count is None:
            raise ValueError("this needs the cell records: call surface_map(cells=True)")

    def area(self) -> np.ndarray:
        """``(B, rows, columns)``: the area of every cell."""
        B = len(self.systems)
        wa = np.diff(np.broadcast_to(self.edges_a, (B, self.columns + 1)), axis=1)
        wb = np.diff(np.broadcast_to(self.edges_b, (B, self.rows + 1)), axis=1)
        return wb[:, :, None] * wa[:, None, :]

    def _per_weight(self, total) -> np.ndarray:
        """``total / weight_sum``, NaN where the weight is not > 0."""
        self._need_cells()
        ok = self.weight_sum > 0.0
        return np.where(ok, total / np.where(ok, self.weight_sum, 1.0), np.nan)

    def surface_density(self) -> np.ndarray:
        """``(B, rows, columns)``: the weight per area; 0 in an empty cell."""
        self._need_cells()
        return self.weight_sum / self.area()

    def number_density(self) -> np.ndarray:
        """``(B, rows, columns)``: the members per area; 0 in an empty cell."""
        self._need_cells()
        return self.count / self.area()

    def mean_velocity(self) -> np.ndarray:
        """``(B, rows, columns)``: ``v1 / weight``, the weighted mean velocity along the line of sight (the first moment)."""
        return self._per_weight(self.v1)

    def dispersion(self) -> np.ndarray:
        """``(B, rows, columns)``: ``sqrt(max(v2 / weight - mean^2, 0))``, the line-of-sight velocity dispersion (the second
        moment)."""
        return np.sqrt(np.maximum(self._per_weight(self.v2) - self.mean_velocity() ** 2, 0.0))

    def plane_velocity(self):
        """Two ``(B, rows, columns)`` arrays: ``(pa / weight, pb / weight)``, the weighted mean velocity in the plane of the
        map, along its first and second axis."""
        return self._per_weight(self.pa), self._per_weight(self.pb)

    def mean_depth(self) -> np.ndarray:
        """``(B, rows, columns)``: ``z1 / weight``, the weighted mean of ``q``, the coordinate along the line of sight."""
        return self._per_weight(self.z1)

    def depth_dispersion(self) -> np.ndarray:
        """``(B, rows, columns)``: ``sqrt(max(z2 / weight - mean_depth^2, 0))``, the spread of ``q`` in every cell."""
        return np.sqrt(np.maximum(self._per_weight(self.z2) - self.mean_depth() ** 2, 0.0))

    def image(self, s: int = 0, quantity: str = "surface_density"):
        """System ``s``'s map ready for ``matplotlib``: ``(array, extent)`` with the ``(rows, columns)`` array of ``quantity``
        (the name of one of the single-valued helpers above, or ``"count"``) and ``extent = (a_lo, a_hi, b_lo, b_hi)``, for
        ``imshow(array, extent=extent, origin="lower")``: row ``j`` of the array is the ``j``-th interval of the second axis."""
        self._need_cells()
        if quantity not in ("count", "surface_density", "number_density", "mean_velocity", "dispersion", "mean_depth", "depth_dispersion"):
            raise ValueError(f"quantity must be count or a single-valued helper of SurfaceMapResult, not {quantity!r}")
        values = self.count if quantity == "count" else getattr(self, quantity)()
        B = len(self.systems)
        ea, eb = np.broadcast_to(self.edges_a, (B, self.columns + 1))[s], np.broadcast_to(self.edges_b, (B, self.rows + 1))[s]
        return np.array(values[s]), (float(ea[0]), float(ea[-1]), float(eb[0]), float(eb[-1]))

    def __repr__(self):
        return (f"SurfaceMapResult(columns={self.columns}, rows={self.rows}, weight={self.weight!r}, selected={self.selected.tolist()}, "
                f"outside={self.outside.tolist()}, unmeasured={self.unmeasured.tolist()}, occupied={self.occupied.tolist()})")


class ShapeResult:
    """What :meth:`BatchedSystem.shape` found.  ``weight_kind`` as given.  Per system (``(B,)`` arrays): ``selected`` (int32: the
    bodies taking part), ``unmeasured`` (a word that is not finite), ``converged`` (the apertures with status 0),
    ``total_weight`` (float64: the weight of all measured bodies taking part); ``centre`` and ``velocity`` ``(B, 3)``, the frame
    as used; ``reduced`` (bool) the tensor used.  Per aperture, ``(B, apertures)`` or ``None`` without ``apertures``: ``status``
    (int32: 0 converged, 1 the iteration limit, 2 too few members, 3 degenerate), ``iterations`` (the passes made), ``count``
    (int64: the members of the final ellipsoid), ``radius`` and ``inner`` as given, ``q`` and ``s`` (middle and minor over
    major), ``change`` (the last relative change of the two), ``eigenvalues`` ``(B, apertures, 3)`` descending, ``axes`` ``(B,
    apertures, 3, 3)`` with the major, middle and minor axis as rows (right-handed), and the float64 sums over the members:
    ``weight`` (w), ``D`` ``(..., 3)`` (w d), ``M`` ``(..., 6)`` (w d_a d_b: xx, yy, zz, xy, xz, yz, not reduced) and ``L``
    ``(..., 3)`` (w d x u).  Per body, ``(B, max_bodies)`` or ``None`` without ``bodies``: ``inside`` (uint32: bit ``a`` set for a
    member of aperture ``a``).  ``systems``, ``aperture_records`` and ``body_records`` are the records themselves.  The derived
    values below are computed on the host in float64."""

    def __init__(self, systems, apertures, bodies, weight):
        self.systems, self.aperture_records, self.body_records, self.weight_kind = systems, apertures, bodies, weight
        for name in ("selected", "unmeasured", "converged", "total_weight", "centre", "velocity"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.reduced = bool(systems["reduced"][0]) if len(systems) else True
        self.apertures = int(systems["apertures"][0]) if len(systems) else 0
        names = ("status", "iterations", "count", "radius", "inner", "q", "s", "change", "eigenvalues", "weight", "D", "M", "L")
        for name in names + ("axes",):
            setattr(self, name, None)
        if apertures is not None:
            for name in names:
                setattr(self, name, np.ascontiguousarray(apertures[name]))
            self.axes = np.ascontiguousarray(apertures["axes"]).reshape(apertures.shape + (3, 3))
        self.inside = None if bodies is None else np.ascontiguousarray(bodies["inside"])

    def _need_apertures(self):
        if self.q is None:
            raise ValueError("this needs the aperture records: call shape(apertures=True)")

    def triaxiality(self) -> np.ndarray:
        """``(B, apertures)``: ``T = (1 - q^2) / (1 - s^2)``: 0 oblate, 1 prolate.  NaN where ``s == 1``."""
        self._need_apertures()
        den = 1.0 - self.s * self.s
        return np.where(den != 0.0, (1.0 - self.q * self.q) / np.where(den != 0.0, den, 1.0), np.nan)

    def ellipticity(self) -> np.ndarray:
        """``(B, apertures)``: ``1 - s``, the flattening of the minor against the major axis."""
        self._need_apertures()
        return 1.0 - self.s

    def offset(self) -> np.ndarray:
        """``(B, apertures, 3)``: ``D / weight``, the members' centre relative to the frame's.  NaN where the weight is not
        ``> 0``."""
        self._need_apertures()
        ok = self.weight > 0.0
        return np.where(ok[..., None], self.D / np.where(ok, self.weight, 1.0)[..., None], np.nan)

    def spin_axis(self) -> np.ndarray:
        """``(B, apertures, 3)``: ``L / |L|``, the direction of the members' angular momentum.  NaN where ``L == 0``."""
        self._need_apertures()
        norm = np.linalg.norm(self.L, axis=-1)
        ok = norm > 0.0
        return np.where(ok[..., None], self.L / np.where(ok, norm, 1.0)[..., None], np.nan)

    def misalignment(self) -> np.ndarray:
        """``(B, apertures)``: the angle in radians, 0 ... pi, between ``L`` and the minor axis ``e3``.  NaN where ``L == 0``."""
        cosine = np.einsum("...k,...k->...", self.spin_axis(), self.axes[..., 2, :])
        return np.arccos(np.clip(cosine, -1.0, 1.0))

    def view(self, a: int = 0, kind: str = "face_on") -> np.ndarray:
        """``(B, 3, 3)``: a right-handed view of every system for :meth:`BatchedSystem.surface_map`'s ``axes``, from aperture
        ``a``'s axes.  ``"face_on"``: the map's axes are the major and the middle axis and the line of sight is the minor one,
        ``(e1, e2, e3)``.  ``"edge_on"``: the major axis across, the minor axis up and the line of sight against the middle
        one, ``(e1, e3, -e2)``."""
        self._need_apertures()
        e = self.axes[:, a]
        if kind == "face_on":
            return np.ascontiguousarray(e)
        if kind == "edge_on":
            return np.ascontiguousarray(np.stack([e[:, 0], e[:, 2], -e[:, 1]], axis=1))
        raise ValueError(f"kind must be 'face_on' or 'edge_on', not {kind!r}")

    def members_mask(self, a: int = 0) -> np.ndarray:
        """``(B, max_bodies)`` bool: the members of aperture ``a``'s final ellipsoid, for :meth:`BatchedSystem.members`'
        ``initial`` and the ``subset`` arguments."""
        if self.inside is None:
            raise ValueError("this needs the per-body records: call shape(bodies=True)")
        if not 0 <= int(a) < max(self.apertures, 1):
            raise ValueError(f"a must be 0 ... {self.apertures - 1}, not {a!r}")
        return np.ascontiguousarray((self.inside >> np.uint32(int(a))) & np.uint32(1)).astype(np.bool_)

    def __repr__(self):
        return (f"ShapeResult(apertures={self.apertures}, reduced={self.reduced}, weight={self.weight_kind!r}, "
                f"selected={self.selected.tolist()}, converged={self.converged.tolist()})")


def interactions_per_step(counts, massive=None) -> int:
    """Ordered body-body interactions one step of these systems evaluates (``sum n_s^2``, the one-sided convention); with
    ``massive`` (:meth:`BatchedSystem.set_massive_counts`) ``sum n_s * min(m_s, n_s)``: every body against the massive ones."""
    c = np.asarray(counts, dtype=np.int64)
    if massive is None:
        return int((c * c).sum())
    m = np.minimum(np.asarray(massive, dtype=np.int64), c)
    return int((c * m).sum())


SYSTEM_FIELDS = ("nodes", "roots", "levels", "singles", "binaries", "triples", "higher", "unstable")
NODE_FIELDS = ("child", "parent", "level", "leaves", "slot", "mass", "energy", "semi_major_axis", "eccentricity", "inclination",
               "separation", "perturbation", "mutual_inclination", "h")


class PairVelocityResult:
    """What :meth:`BatchedSystem.pair_velocities` summed.  ``edges`` are the bin edges as given (float32, ``(bins + 1,)`` or
    ``(B, bins + 1)``); ``bin_records`` is ``(B, bins)`` of ``PAIR_VELOCITIES_BIN_DTYPE`` (``None`` without ``bins``), and each
    of its words a ``(B, bins)`` array of that name: ``count``, ``approaching``, ``receding`` (int64) and the sums ``weight``,
    ``r1``, ``r2``, ``rv``, ``vr1``, ``vr2``, ``vt2``, ``v1``, ``v2`` (float64) over the ordered pairs (row, source) with
    ``edges[t] < r <= edges[t + 1]``.  Per system (``(B,)`` arrays): ``rows``, ``sources``, ``both``, ``pairs``, ``below``,
    ``above`` and ``unmeasured`` as in :class:`CorrelationResult` (a pair with a NaN or infinite velocity word is unmeasured
    too).  ``auto`` (bool) tells where rows and sources are the same bodies.  ``systems`` is the records themselves, ``bins``
    the number of bins, ``weight`` the weight's name.  The derived quantities are NaN where a bin is empty."""

    WORDS = ("count", "approaching", "receding", "weight", "r1", "r2", "rv", "vr1", "vr2", "vt2", "v1", "v2")

    def __init__(self, systems, bin_records, edges, weight="number"):
        self.systems, self.bin_records, self.edges, self.weight_name = systems, bin_records, edges, weight
        for name in ("rows", "sources", "both", "pairs", "below", "above", "unmeasured"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.bins = int(edges.shape[-1]) - 1
        self.auto = (self.rows == self.both) & (self.sources == self.both)
        for name in self.WORDS:
            setattr(self, name, None if bin_records is None else np.ascontiguousarray(bin_records[name]))

    def _need_bins(self):
        if self.bin_records is None:
            raise ValueError("this needs the bins: call pair_velocities(bins=True)")

    def _per_weight(self, total) -> np.ndarray:
        self._need_bins()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.count > 0, total / np.where(self.count > 0, self.weight, 1.0), np.nan)

    def mean_separation(self) -> np.ndarray:
        """``(B, bins)``: the weighted mean separation of the pairs of every bin, ``r1 / weight``."""
        return self._per_weight(self.r1)

    def mean_radial_velocity(self) -> np.ndarray:
        """``(B, bins)``: the mean pairwise radial velocity v12(r), ``vr1 / weight``; negative where pairs approach."""
        return self._per_weight(self.vr1)

    def sigma_radial(self) -> np.ndarray:
        """``(B, bins)``: the pairwise dispersion along the separation, ``sqrt(max(vr2 / weight - v12^2, 0))``."""
        return np.sqrt(np.maximum(self._per_weight(self.vr2) - self.mean_radial_velocity() ** 2, 0.0))

    def sigma_tangential(self) -> np.ndarray:
        """``(B, bins)``: the pairwise dispersion across the separation per component, ``sqrt(vt2 / (2 weight))``."""
        return np.sqrt(self._per_weight(self.vt2) / 2.0)

    def anisotropy(self) -> np.ndarray:
        """``(B, bins)``: ``1 - sigma_tangential^2 / sigma_radial^2``; NaN where the radial dispersion is 0."""
        st, sr = self.sigma_tangential(), self.sigma_radial()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(sr > 0, 1.0 - st * st / np.where(sr > 0, sr * sr, 1.0), np.nan)

    def structure_function(self, order: int = 2) -> np.ndarray:
        """``(B, bins)``: the velocity structure function of order 1 (``v1 / weight``, the mean relative speed) or 2
        (``v2 / weight``, its mean square)."""
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, not {order}")
        return self._per_weight(self.v1 if order == 1 else self.v2)

    def approaching_fraction(self) -> np.ndarray:
        """``(B, bins)``: the fraction of the pairs of every bin that approach, ``approaching / count``."""
        self._need_bins()
        return np.where(self.count > 0, self.approaching / np.where(self.count > 0, self.count, 1), np.nan)

    def expansion_rate(self) -> np.ndarray:
        """``(B, bins)``: the least-squares expansion rate ``sum(d.w) / sum(d.d)`` of the pairs of every bin, ``rv / r2``."""
        self._need_bins()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.count > 0, self.rv / np.where(self.count > 0, self.r2, 1.0), np.nan)

    def unordered(self) -> np.ndarray:
        """``(B, bins)`` of ``PAIR_VELOCITIES_BIN_DTYPE``: the records over unordered pairs where ``auto`` -- every pair was
        summed twice there, as (i, j) and (j, i) with the same terms, so counts and sums are halved -- and the records as
        they are in the systems where rows and sources differ."""
        self._need_bins()
        out = self.bin_records.copy()
        for name in self.WORDS:
            half = out[name] // 2 if out[name].dtype == np.int64 else out[name] / 2.0
            out[name] = np.where(self.auto[:, None], half, out[name])
        return out

    def __repr__(self):
        return (f"PairVelocityResult(bins={self.bins}, weight={self.weight_name!r}, pairs={self.pairs.tolist()}, "
                f"below={self.below.tolist()}, above={self.above.tolist()}, unmeasured={self.unmeasured.tolist()})")


class MutualGravityResult:
    """What :meth:`BatchedSystem.mutual_gravity` summed.  ``entries`` is ``(B, K, K)`` of ``MUTUAL_GRAVITY_ENTRY_DTYPE``
    (``None`` without ``matrix``), entry ``[s, a, b]`` what set ``b`` does to set ``a`` in system ``s``, and each of its words a
    view of that name: ``pairs`` (int64), ``potential``, ``virial``, ``power`` (``(B, K, K)`` float64), ``force`` and
    ``torque`` (``(B, K, K, 3)``).  Per system (``(B,)`` arrays): ``selected``, ``left_out``, ``unmeasured``, ``total_pairs``,
    ``coincident``; ``members`` (``(B, K)`` int32) and ``mass`` (``(B, K)`` float64).  ``systems`` is the records themselves,
    ``sets`` is ``K``.  The derived quantities are NaN where a set is empty."""

    WORDS = ("pairs", "potential", "force", "torque", "virial", "power")

    def __init__(self, systems, entries, sets):
        self.systems, self.entries, self.sets = systems, entries, int(sets)
        for name in ("selected", "left_out", "unmeasured", "coincident"):
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.total_pairs = np.ascontiguousarray(systems["pairs"])
        self.members = np.ascontiguousarray(systems["members"][:, :self.sets])
        self.mass = np.ascontiguousarray(systems["mass"][:, :self.sets])
        for name in self.WORDS:
            setattr(self, name, None if entries is None else entries[name])

    def _need_matrix(self):
        if self.entries is None:
            raise ValueError("this needs the entries: call mutual_gravity(matrix=True)")

    def _set(self, a):
        if not 0 <= int(a) < self.sets:
            raise ValueError(f"set must be 0 ... {self.sets - 1}, not {a}")
        return int(a)

    def _where_both(self, a, b, value):
        full = (self.members[:, a] > 0) & (self.members[:, b] > 0)
        return np.where(full.reshape(full.shape + (1,) * (value.ndim - 1)), value, np.nan)

    def _others(self, a, word):
        self._need_matrix()
        a = self._set(a)
        value = sum((word[:, a, b] for b in range(self.sets) if b != a), np.zeros_like(word[:, a, a]))
        return np.where((self.members[:, a] > 0).reshape((-1,) + (1,) * (value.ndim - 1)), value, np.nan)

    def interaction_energy(self, a, b) -> np.ndarray:
        """``(B,)``: the potential energy between sets ``a`` and ``b != a``, ``potential[:, a, b]`` (``potential[:, b, a]`` is
        the same sum in another order)."""
        self._need_matrix()
        a, b = self._set(a), self._set(b)
        if a == b:
            raise ValueError("interaction_energy is between two different sets: self_energy(a) is the energy of one")
        return self._where_both(a, b, self.potential[:, a, b])

    def self_energy(self, a) -> np.ndarray:
        """``(B,)``: the potential energy of set ``a`` in its own field, ``potential[:, a, a] / 2`` (every unordered pair was
        summed twice)."""
        self._need_matrix()
        a = self._set(a)
        return self._where_both(a, a, self.potential[:, a, a] / 2.0)

    def total_potential_energy(self) -> np.ndarray:
        """``(B,)``: the potential energy of all selected bodies, the sum of all entries' ``potential`` halved; NaN where no
        body is selected."""
        self._need_matrix()
        return np.where(self.selected > 0, self.potential.sum(axis=(1, 2)) / 2.0, np.nan)

    def force_on(self, a) -> np.ndarray:
        """``(B, 3)``: the net force of all other sets on set ``a``."""
        return self._others(a, self.force)

    def torque_on(self, a) -> np.ndarray:
        """``(B, 3)``: the torque of all other sets on set ``a`` about the centre."""
        return self._others(a, self.torque)

    def power_into(self, a) -> np.ndarray:
        """``(B,)``: the rate at which all other sets do work on set ``a`` in the frame of ``velocity``."""
        return self._others(a, self.power)

    def acceleration_of(self, a) -> np.ndarray:
        """``(B, 3)``: the acceleration of the centre of mass of set ``a`` by all other sets, ``force_on(a) / mass[:, a]``;
        NaN where the set's mass is 0."""
        force = self.force_on(a)
        m = self.mass[:, self._set(a)]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where((m != 0)[:, None], force / np.where(m != 0, m, 1.0)[:, None], np.nan)

    def two_body_energy(self, a, b, centres, velocities) -> np.ndarray:
        """``(B,)``: the orbital energy of sets ``a`` and ``b`` as two point masses and nothing else:
        ``mu |v_a - v_b|^2 / 2 - M_a M_b / |x_a - x_b|`` with ``mu = M_a M_b / (M_a + M_b)`` from ``mass``.  ``centres`` and
        ``velocities`` are ``(B, K, 3)``: where each set is and how it moves, by the caller's choice (no softening enters).
        It knows nothing of the sets' extent: compare it with :meth:`interaction_energy`, which sums over the bodies."""
        a, b = self._set(a), self._set(b)
        x, v = np.asarray(centres, np.float64), np.asarray(velocities, np.float64)
        want = (self.mass.shape[0], self.sets, 3)
        if x.shape != want or v.shape != want:
            raise ValueError(f"centres and velocities must have shape {want}, got {tuple(x.shape)} and {tuple(v.shape)}")
        ma, mb = self.mass[:, a], self.mass[:, b]
        with np.errstate(divide="ignore", invalid="ignore"):
            mu = ma * mb / (ma + mb)
            r = np.sqrt(((x[:, a] - x[:, b]) ** 2).sum(axis=1))
            w2 = ((v[:, a] - v[:, b]) ** 2).sum(axis=1)
            return self._where_both(a, b, 0.5 * mu * w2 - ma * mb / r)

    @staticmethod
    def labels_from_masks(*masks) -> np.ndarray:
        """``(B, max_bodies)`` int64 labels from boolean masks of that shape (numpy or torch): mask ``a`` is set ``a``, a
        body in no mask is -1.  Overlapping masks are refused."""
        if not masks:
            raise ValueError("labels_from_masks needs at least one mask")
        ms = [np.asarray(m.detach().cpu().numpy() if hasattr(m, "detach") else m) for m in masks]
        for m in ms:
            if m.dtype != np.bool_ or m.shape != ms[0].shape:
                raise ValueError("the masks must be bool arrays of one shape")
        if (np.sum([m.astype(np.int64) for m in ms], axis=0) > 1).any():
            raise ValueError("the masks overlap: a body is in one set at most")
        labels = np.full(ms[0].shape, -1, np.int64)
        for a, m in enumerate(ms):
            labels[m] = a
        return labels

    def __repr__(self):
        return (f"MutualGravityResult(sets={self.sets}, members={self.members.tolist()}, pairs={self.total_pairs.tolist()}, "
                f"coincident={self.coincident.tolist()}, unmeasured={self.unmeasured.tolist()})")


class HierarchyResult:
    """What :meth:`BatchedSystem.hierarchy` found.  Per system (``(B,)`` int32 arrays): ``nodes`` (made), ``roots`` (live at the
    end, leaves only), ``levels`` (evaluated), ``singles``, ``binaries``, ``triples``, ``higher`` (roots with 1, 2, 3 and >= 4
    leaves), ``unstable`` (roots with ``stable == 0``), and ``converged`` (bool).  ``counts``: the body counts the call saw; a
    leaf's id is its index and node ``k`` of system ``s`` has the id ``counts[s] + k``.  Per node, ``(B, max_bodies)`` arrays
    or ``None`` without ``nodes`` (entry ``k`` is node ``k``; beyond ``nodes[s]`` zeros, ``child`` and ``parent`` -1):
    ``child`` (``(B, max_bodies, 2)``, the lower slot's first), ``node_parent``, ``level``, ``leaves``, ``slot``, ``stable``
    (bool), ``mass``, ``energy``, ``semi_major_axis``, ``eccentricity``, ``inclination``, ``separation``, ``perturbation``,
    ``mutual_inclination`` (``(B, max_bodies, 2)``) and ``h`` (``(B, max_bodies, 3)``).  Per body, ``(B, max_bodies)`` int32
    arrays or ``None`` without ``bodies``: ``parent``, ``root`` and ``depth``.  ``systems``, ``node_records`` and
    ``body_records`` are the records themselves."""

    def __init__(self, systems, nodes, bodies, counts):
        self.systems, self.node_records, self.body_records = systems, nodes, bodies
        self.counts = np.asarray(counts, dtype=np.int64)
        for name in SYSTEM_FIELDS:
            setattr(self, name, np.ascontiguousarray(systems[name]))
        self.converged = systems["converged"] != 0
        for name in NODE_FIELDS:
            setattr(self, "node_parent" if name == "parent" else name, None if nodes is None else np.ascontiguousarray(nodes[name]))
        self.stable = None if nodes is None else nodes["stable"] != 0
        self.nodes = np.ascontiguousarray(systems["nodes"])       # the per-system count, not the records
        self.parent = self.root = self.depth = None
        if bodies is not None:
            self.parent, self.root, self.depth = (np.ascontiguousarray(bodies[name]) for name in ("parent", "root", "depth"))

    def multiplicity(self) -> np.ndarray:
        """``(B, 4)`` int32: singles, binaries, triples and higher multiples among the roots of every system."""
        return np.stack([self.singles, self.binaries, self.triples, self.higher], axis=1)

    def roots_of(self, s: int) -> list:
        """The ids of system ``s``'s roots in ascending slot (needs the node records)."""
        if self.node_records is None:
            raise ValueError("roots_of needs the node records: call hierarchy(nodes=True)")
        n, made = int(self.counts[s]), int(self.nodes[s])
        rec = self.node_records[s, :made]
        leaves = made + int(self.roots[s])              # every node takes one root away; test particles are no roots
        child = set(rec["child"].ravel().tolist())
        roots = [(i, i) for i in range(leaves) if i not in child]
        roots += [(int(rec["slot"][k]), n + k) for k in range(made) if rec["parent"][k] < 0]
        return [i for _, i in sorted(roots)]

    def describe(self, s: int) -> str:
        """System ``s`` Fewbody style: the roots in ascending slot, a node as ``[a b]`` with the lower-slot child first, e.g.
        ``"[[0 2] 5] 1 [3 4]"``."""
        n = int(self.counts[s])

        def text(i):
            if i < n:
                return str(i)
            a, b = self.node_records[s, i - n]["child"]
            return f"[{text(int(a))} {text(int(b))}]"
        return " ".join(text(i) for i in self.roots_of(s))

    def __repr__(self):
        return (f"HierarchyResult(multiplicity={self.multiplicity().tolist()}, unstable={self.unstable.tolist()}, "
                f"levels={self.levels.tolist()}, converged={self.converged.tolist()})")


__all__ = ["BatchedSystem", "EvolveResult", "StopResult", "MergeResult", "FateResult", "AccretionResult", "PairResult", "StructureResult", "MemberResult", "HierarchyResult", "GravityResult", "GRAVITY_RECORD_DTYPE", "BatchGroups", "GROUP_BODY_DTYPE", "GROUP_RECORD_DTYPE", "GROUP_SYSTEM_DTYPE", "SpanResult", "SPAN_SYSTEM_DTYPE", "SPAN_EDGE_DTYPE", "SPAN_BODY_DTYPE", "NeighbourResult", "NEIGHBOUR_SYSTEM_DTYPE", "NEIGHBOUR_BODY_DTYPE", "CorrelationResult", "CORRELATION_SYSTEM_DTYPE", "ContactsResult", "CONTACT_SYSTEM_DTYPE", "CONTACT_BODY_DTYPE", "CONTACT_DTYPE", "ApproachesResult", "APPROACH_SYSTEM_DTYPE", "APPROACH_BODY_DTYPE", "APPROACH_DTYPE", "WEIGHTS", "MERGE_EVENT_DTYPE", "PAIR_RECORD_DTYPE", "STRUCTURE_BODY_DTYPE", "STRUCTURE_SYSTEM_DTYPE", "MEMBER_BODY_DTYPE", "MEMBER_SYSTEM_DTYPE", "HIERARCHY_NODE_DTYPE", "HIERARCHY_BODY_DTYPE", "HIERARCHY_SYSTEM_DTYPE", "BATCH_MAX_BODIES", "INTEGRATORS", "FIELD_KINDS", "interactions_per_step", "PairVelocityResult", "PAIR_VELOCITIES_SYSTEM_DTYPE", "PAIR_VELOCITIES_BIN_DTYPE", "MutualGravityResult", "MUTUAL_GRAVITY_SYSTEM_DTYPE", "MUTUAL_GRAVITY_ENTRY_DTYPE"]
