"""ctypes binding of ``libnbody_amd.so`` -- one prototype per entry point of ``include/nbody.h``.

There is no fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_void_p

from .build import LIB_PATH

NBODY_OK = 0
NBODY_ERR_INVALID = -1
NBODY_ERR_ALLOC = -2
NBODY_ERR_DEVICE = -3
NBODY_ERR_NO_DEVICE = -4
NBODY_ERR_STATE = -5


class NBodyError(RuntimeError):
    """A C-ABI call returned a negative ``nbody_status``."""

    def __init__(self, status: int, message: str):
        super().__init__(f"nbody status {status}: {message}")
        self.status = status


_PROTOTYPES = {
    # name: (restype, argtypes)
    "nbody_abi_version": (c_int, []),
    "nbody_status_string": (c_char_p, [c_int]),
    "nbody_create": (c_int, [POINTER(c_void_p), c_int, c_int64]),
    "nbody_create_shard": (c_int, [POINTER(c_void_p), c_int, c_int64, c_int64, c_int64, c_int64]),
    "nbody_destroy": (c_int, [c_void_p]),
    "nbody_last_error": (c_char_p, [c_void_p]),
    "nbody_default_split_len": (c_int64, [c_int64]),
    "nbody_split_len": (c_int64, [c_void_p]),
    "nbody_n_total": (c_int64, [c_void_p]),
    "nbody_set_positions": (c_int, [c_void_p, c_void_p]),
    "nbody_set_velocities": (c_int, [c_void_p, c_void_p]),
    "nbody_download": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nbody_positions_device": (c_void_p, [c_void_p]),
    "nbody_velocities_device": (c_void_p, [c_void_p]),
    "nbody_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float]),
    "nbody_step_async": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float]),
    "nbody_step_n": (c_int, [c_void_p, c_int, c_float, c_float]),
    "nbody_step_n_on": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float]),
    "nbody_set_graph_replay": (c_int, [c_void_p, c_int]),
    "nbody_set_strip_len": (c_int, [c_void_p, c_int]),
    "nbody_sync": (c_int, [c_void_p]),
    "nbody_forces": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_float]),
    "nbody_forces_complement": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_float]),
    "nbody_update": (c_int, [c_void_p, c_void_p, c_void_p, c_float]),
    "nbody_set_integrator": (c_int, [c_void_p, c_int]),
    "nbody_invalidate_forces": (c_int, [c_void_p]),
    "nbody_kdk_prepare": (c_int, [c_void_p]),
    "nbody_kdk_kick_drift": (c_int, [c_void_p, c_void_p, c_void_p, c_float]),
    "nbody_kdk_kick": (c_int, [c_void_p, c_void_p, c_float]),
    "nbody_set_stream": (c_int, [c_void_p, c_void_p]),
    "nbody_reset_stream": (c_int, [c_void_p]),
    "nbody_energy": (c_int, [c_void_p, c_void_p, c_void_p, c_float, POINTER(c_double)]),
    "nbody_momentum": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double)]),
    "nbody_timing_enable": (c_int, [c_void_p, c_int]),
    "nbody_timing_read": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64), POINTER(c_double),
                                  POINTER(c_int64)]),
    "nbody_timing_read_ex": (c_int, [c_void_p, POINTER(c_double)]),
    "nbody_set_force_mode": (c_int, [c_void_p, c_int]),
    "nbody_pair_once_split_len": (ctypes.c_int64, [ctypes.c_int64]),
    "nbody_sym_set_colparts": (c_int, [c_void_p, c_void_p]),
    "nbody_sym_groups": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                 ctypes.POINTER(ctypes.c_int64)]),
    "nbody_sym_reduce": (c_int, [c_void_p]),
    "nbody_sym_rowsum": (c_int, [c_void_p]),
    "nbody_set_particle_softening": (c_int, [c_void_p, c_void_p]),
    "nbody_upload_particle_softening": (c_int, [c_void_p, c_void_p]),
    "nbody_set_rows_per_lane": (c_int, [c_void_p, c_int]),
    "nbody_set_equal_mass_path": (c_int, [c_void_p, c_int]),
    "nbody_set_early_summation": (c_int, [c_void_p, c_int]),
    "nbody_set_summation_parts": (c_int, [c_void_p, c_int]),
    "nbody_morton_order": (c_int, [c_void_p, c_int64, c_void_p]),
    "nbody_create_auto": (c_int, [POINTER(c_void_p), c_int, c_int64]),
    "nbody_force_mode": (c_int, [c_void_p]),
    "nbody_reorder": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "nbody_morton_order_device": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "nbody_order_compute": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "nbody_order_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int]),
    "nbody_order_read": (c_int, [c_void_p, c_void_p]),
    "nbody_order_identity": (c_int, [c_void_p, c_void_p, c_int64]),
    "nbody_order_set": (c_int, [c_void_p, c_void_p, c_int64, c_int]),
    "nbody_order_permute_softening": (c_int, [c_void_p]),
    "nbody_multi_set_positions": (c_int, [c_void_p, c_void_p]),
    "nbody_multi_set_velocities": (c_int, [c_void_p, c_void_p]),
    "nbody_multi_timing_enable": (c_int, [c_void_p, c_int]),
    "nbody_multi_timing_read": (c_int, [c_void_p, c_int, POINTER(c_double)]),
    "nbody_multi_order": (c_int, [c_void_p, c_void_p]),
    "nbody_multi_reorder": (c_int, [c_void_p]),
    "nbody_multi_set_reorder_period": (c_int, [c_void_p, c_int64]),
    "nbody_partial_sum_bytes": (c_int64, [c_void_p]),
    "nbody_device_info": (c_int, [c_void_p, POINTER(c_int64), c_char_p, c_int]),
    # multi-GPU (csrc/nbody_multi.hip)
    "nbody_multi_geometry": (c_int, [c_int64, c_int, c_int, c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "nbody_multi_ring_schedule": (c_int, [c_int, c_int, c_int, POINTER(c_int), POINTER(c_int)]),
    "nbody_multi_unique_id": (c_int, [c_void_p]),
    "nbody_multi_create": (c_int, [POINTER(c_void_p), c_void_p, POINTER(c_int), c_int]),
    "nbody_multi_create_rank": (c_int, [POINTER(c_void_p), c_void_p, c_int, c_int, c_int, c_void_p]),
    "nbody_multi_destroy": (c_int, [c_void_p]),
    "nbody_multi_last_error": (c_char_p, [c_void_p]),
    "nbody_multi_set_timeout": (c_int, [c_void_p, c_double]),
    "nbody_multi_set_state": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nbody_multi_set_particle_softening": (c_int, [c_void_p, c_void_p]),
    "nbody_multi_download": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nbody_multi_step": (c_int, [c_void_p, c_float, c_float]),
    "nbody_multi_step_n": (c_int, [c_void_p, c_int, c_float, c_float]),
    "nbody_multi_step_async": (c_int, [c_void_p, c_float, c_float]),
    "nbody_multi_sync": (c_int, [c_void_p]),
    "nbody_multi_energy": (c_int, [c_void_p, c_float, POINTER(c_double)]),
    "nbody_multi_momentum": (c_int, [c_void_p, POINTER(c_double)]),
    "nbody_multi_replica_checksums": (c_int, [c_void_p, POINTER(ctypes.c_uint64)]),
    "nbody_multi_info": (c_int, [c_void_p, POINTER(c_int64)]),
    "nbody_multi_shard": (c_void_p, [c_void_p, c_int]),
    "nbody_multi_positions_device": (c_void_p, [c_void_p, c_int]),
    "nbody_multi_velocities_device": (c_void_p, [c_void_p, c_int]),
    # batched ensembles (csrc/nbody_batch_capi.hip over csrc/nbody_batch.hip, csrc/nbody_batch_analysis.hip)
    "nbody_batch_create": (c_int, [POINTER(c_void_p), c_int, c_int64, c_int64]),
    "nbody_batch_destroy": (c_int, [c_void_p]),
    "nbody_batch_last_error": (c_char_p, [c_void_p]),
    "nbody_batch_set_counts": (c_int, [c_void_p, POINTER(c_int64)]),
    "nbody_batch_set_integrator": (c_int, [c_void_p, c_int]),
    "nbody_batch_invalidate_forces": (c_int, [c_void_p]),
    "nbody_batch_set_stream": (c_int, [c_void_p, c_void_p]),
    "nbody_batch_step_n_on": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float]),
    "nbody_batch_step_n_async": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_float, c_float]),
    "nbody_batch_sync": (c_int, [c_void_p]),
    "nbody_batch_energy": (c_int, [c_void_p, c_void_p, c_void_p, c_float, POINTER(c_double)]),
    "nbody_batch_momentum": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_double)]),
}


class BatchEvolveConfig(ctypes.Structure):
    """``nbody_batch_evolve_config`` of include/nbody_batch_evolve.h."""
    _fields_ = [("dt_max", c_float), ("levels", c_int), ("eta", c_float), ("eta_start", c_float), ("softening", c_float),
                ("max_steps", c_int)]


#: the entry points of include/nbody_batch_evolve.h (adaptive shared steps for Hermite batches), which nbody.h includes
_EVOLVE_PROTOTYPES = {
    "nbody_batch_evolve_on": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(BatchEvolveConfig)]),
    "nbody_batch_evolve_stats": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int), POINTER(c_int), POINTER(c_int64),
                                         POINTER(c_int64)]),
    "nbody_batch_evolve_launch_steps": (c_int, [c_void_p, c_int]),
}
BATCH_EVOLVE_MAX_LEVELS = 20
BATCH_EVOLVE_DEFAULT_MAX_STEPS = 1048576


class BatchStopConfig(ctypes.Structure):
    """``nbody_batch_stop_config`` of include/nbody_batch_stop.h."""
    _fields_ = [("collision_radius", c_float), ("escape_radius", c_float)]


#: the entry points of include/nbody_batch_stop.h (stopping conditions for Hermite batches), which nbody.h includes
_STOP_PROTOTYPES = {
    "nbody_batch_stop_set": (c_int, [c_void_p, POINTER(BatchStopConfig)]),
    "nbody_batch_stop_read": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int64), POINTER(c_int), POINTER(c_int), POINTER(c_float),
                                      POINTER(c_int)]),
    "nbody_batch_stop_count": (c_int, [c_void_p, POINTER(c_int64)]),
}
BATCH_STOP_COLLISION = 1
BATCH_STOP_ESCAPE = 2


class BatchMergeConfig(ctypes.Structure):
    """``nbody_batch_merge_config`` of include/nbody_batch_merge.h."""
    _fields_ = [("on_collision", c_int), ("log_capacity", c_int)]


class BatchMergeEvent(ctypes.Structure):
    """``nbody_batch_merge_event`` of include/nbody_batch_merge.h."""
    _fields_ = [("tick", c_int64), ("survivor", c_int), ("absorbed", c_int), ("count_before", c_int), ("separation", c_float),
                ("relative_speed", c_float), ("mass_survivor", c_float), ("mass_absorbed", c_float), ("reserved", c_int)]


#: the entry points of include/nbody_batch_merge.h (mergers for Hermite batches), which nbody.h includes
_MERGE_PROTOTYPES = {
    "nbody_batch_merge_set": (c_int, [c_void_p, POINTER(BatchMergeConfig)]),
    "nbody_batch_merge_read": (c_int, [c_void_p, POINTER(c_int64), POINTER(BatchMergeEvent)]),
    "nbody_batch_get_counts": (c_int, [c_void_p, POINTER(c_int64)]),
}
BATCH_ON_COLLISION_STOP = 0
BATCH_ON_COLLISION_MERGE = 1


#: the entry points of include/nbody_batch_radii.h (per-body collision radii for Hermite batches), which nbody.h includes
_RADII_PROTOTYPES = {
    "nbody_batch_radii_set": (c_int, [c_void_p, POINTER(c_float)]),
    "nbody_batch_radii_read": (c_int, [c_void_p, POINTER(c_float)]),
}


#: the entry points of include/nbody_batch_massive.h (test particles for batched ensembles), which nbody.h includes
_MASSIVE_PROTOTYPES = {
    "nbody_batch_massive_set": (c_int, [c_void_p, POINTER(c_int64)]),
    "nbody_batch_massive_read": (c_int, [c_void_p, POINTER(c_int64)]),
}


class BatchFateConfig(ctypes.Structure):
    """``nbody_batch_fate_config`` of include/nbody_batch_fate.h."""
    _fields_ = [("action", c_int)]


#: the entry points of include/nbody_batch_fate.h (tracer fates for Hermite batches), which nbody.h includes
_FATE_PROTOTYPES = {
    "nbody_batch_fate_set": (c_int, [c_void_p, POINTER(BatchFateConfig)]),
    "nbody_batch_fate_read": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int64), POINTER(c_int), POINTER(c_float), POINTER(c_float)]),
    "nbody_batch_fate_count": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
}
BATCH_TRACERS_REFUSE = 0
BATCH_TRACERS_REMOVE = 1
BATCH_FATE_ALIVE = 0
BATCH_FATE_HIT = 1
BATCH_FATE_ESCAPED = 2


class BatchAccreteConfig(ctypes.Structure):
    """``nbody_batch_accrete_config`` of include/nbody_batch_accrete.h."""
    _fields_ = [("on_hit", c_int)]


#: the entry points of include/nbody_batch_accrete.h (accreting tracers for Hermite batches), which nbody.h includes
_ACCRETE_PROTOTYPES = {
    "nbody_batch_accrete_set": (c_int, [c_void_p, POINTER(BatchAccreteConfig)]),
    "nbody_batch_accrete_read": (c_int, [c_void_p, POINTER(c_float), POINTER(c_int64)]),
}
BATCH_ON_HIT_REMOVE = 0
BATCH_ON_HIT_ACCRETE = 1


class BatchFieldComponent(ctypes.Structure):
    """``nbody_batch_field_component`` of include/nbody_batch_field.h."""
    _fields_ = [("kind", c_int), ("p", c_float * 3)]


#: the entry points of include/nbody_batch_field.h (external fields for Hermite batches), which nbody.h includes
_FIELD_PROTOTYPES = {
    "nbody_batch_field_set": (c_int, [c_void_p, POINTER(BatchFieldComponent), c_int]),
    "nbody_batch_field_read": (c_int, [c_void_p, POINTER(BatchFieldComponent), POINTER(c_int)]),
    "nbody_batch_field_potential": (c_int, [c_void_p, c_void_p, POINTER(c_double)]),
}
BATCH_FIELD_MAX_COMPONENTS = 4
BATCH_FIELD_NONE = 0
BATCH_FIELD_PLUMMER = 1
BATCH_FIELD_LOG_HALO = 2
BATCH_FIELD_MIYAMOTO_NAGAI = 3


class BatchPairRecord(ctypes.Structure):
    """``nbody_batch_pair_record`` of include/nbody_batch_pairs.h."""
    _fields_ = [("partner", c_int), ("mutual", c_int), ("energy", c_double), ("semi_major_axis", c_double),
                ("eccentricity", c_double), ("inclination", c_double), ("separation", c_double)]


#: the entry points of include/nbody_batch_pairs.h (bound pairs of batched ensembles), which nbody.h includes
_PAIRS_PROTOTYPES = {
    "nbody_batch_pairs": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(BatchPairRecord)]),
    "nbody_batch_pairs_binaries": (c_int, [c_void_p, POINTER(c_int64)]),
}


BATCH_WEIGHT_MASS = 0
BATCH_WEIGHT_NUMBER = 1
BATCH_STRUCTURE_MAX_NEIGHBOUR = 8
BATCH_STRUCTURE_FRACTIONS = 8


class BatchStructureBody(ctypes.Structure):
    """``nbody_batch_structure_body`` of include/nbody_batch_structure.h."""
    _fields_ = [("density", c_double), ("radius", c_double), ("enclosed", c_double), ("neighbour_r2", c_float),
                ("neighbour_weight", c_float), ("inside", c_int), ("reserved", c_int)]


class BatchStructureSystem(ctypes.Structure):
    """``nbody_batch_structure_system`` of include/nbody_batch_structure.h."""
    _fields_ = [("centre", c_double * 3), ("core_radius", c_double), ("core_density", c_double), ("total_weight", c_double),
                ("lagrange", c_double * 8), ("estimated", c_int), ("reserved", c_int)]


#: the entry point of include/nbody_batch_structure.h (cluster structure of batched ensembles), which nbody.h includes
_STRUCTURE_PROTOTYPES = {
    "nbody_batch_structure": (c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_double), c_int, POINTER(BatchStructureSystem),
                                      POINTER(BatchStructureBody)]),
}


BATCH_MEMBERS_MAX_ITERATIONS = 64


class BatchMemberBody(ctypes.Structure):
    """``nbody_batch_member_body`` of include/nbody_batch_members.h."""
    _fields_ = [("potential", c_double), ("energy", c_double), ("member", c_int), ("removed_at", c_int)]


class BatchMemberSystem(ctypes.Structure):
    """``nbody_batch_member_system`` of include/nbody_batch_members.h."""
    _fields_ = [("bound_mass", c_double), ("centre", c_double * 3), ("velocity", c_double * 3), ("kinetic", c_double),
                ("potential", c_double), ("members", c_int), ("sources", c_int), ("iterations", c_int), ("converged", c_int)]


#: the entry point of include/nbody_batch_members.h (bound members of batched ensembles), which nbody.h includes
_MEMBERS_PROTOTYPES = {
    "nbody_batch_members": (c_int, [c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, POINTER(BatchMemberSystem),
                                    POINTER(BatchMemberBody)]),
}


BATCH_HIERARCHY_MAX_LEVELS = 16


class BatchHierarchyNode(ctypes.Structure):
    """``nbody_batch_hierarchy_node`` of include/nbody_batch_hierarchy.h."""
    _fields_ = [("child", c_int * 2), ("parent", c_int), ("level", c_int), ("leaves", c_int), ("slot", c_int), ("stable", c_int),
                ("reserved", c_int), ("mass", c_double), ("energy", c_double), ("semi_major_axis", c_double),
                ("eccentricity", c_double), ("inclination", c_double), ("separation", c_double), ("perturbation", c_double),
                ("mutual_inclination", c_double * 2), ("h", c_double * 3)]


class BatchHierarchyBody(ctypes.Structure):
    """``nbody_batch_hierarchy_body`` of include/nbody_batch_hierarchy.h."""
    _fields_ = [("parent", c_int), ("root", c_int), ("depth", c_int), ("reserved", c_int)]


class BatchHierarchySystem(ctypes.Structure):
    """``nbody_batch_hierarchy_system`` of include/nbody_batch_hierarchy.h."""
    _fields_ = [("nodes", c_int), ("roots", c_int), ("levels", c_int), ("converged", c_int), ("singles", c_int),
                ("binaries", c_int), ("triples", c_int), ("higher", c_int), ("unstable", c_int), ("reserved", c_int)]


#: the entry point of include/nbody_batch_hierarchy.h (hierarchies of batched ensembles), which nbody.h includes
_HIERARCHY_PROTOTYPES = {
    "nbody_batch_hierarchy": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_int, POINTER(BatchHierarchySystem),
                                      POINTER(BatchHierarchyNode), POINTER(BatchHierarchyBody)]),
}


BATCH_GRAVITY_MAX_POINTS = 1048576


class BatchGravityRecord(ctypes.Structure):
    """``nbody_batch_gravity_record`` of include/nbody_batch_gravity.h."""
    _fields_ = [("acceleration", c_float * 3), ("reserved", c_float), ("potential", c_double)]


#: the entry point of include/nbody_batch_gravity.h (gravity at points of batched ensembles), which nbody.h includes
_GRAVITY_PROTOTYPES = {
    "nbody_batch_gravity": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, POINTER(c_int64), c_float, POINTER(BatchGravityRecord),
                                    POINTER(c_float)]),
}


BATCH_GROUPS_MAX_SWEEPS = 64


class BatchGroupBody(ctypes.Structure):
    """``nbody_batch_group_body`` of include/nbody_batch_groups.h."""
    _fields_ = [("group", c_int), ("size", c_int)]


class BatchGroupRecord(ctypes.Structure):
    """``nbody_batch_group_record`` of include/nbody_batch_groups.h."""
    _fields_ = [("weight", c_double), ("centre", c_double * 3), ("velocity", c_double * 3), ("count", c_int), ("sources", c_int)]


class BatchGroupSystem(ctypes.Structure):
    """``nbody_batch_group_system`` of include/nbody_batch_groups.h."""
    _fields_ = [("groups", c_int), ("grouped", c_int), ("singles", c_int), ("largest", c_int), ("largest_count", c_int),
                ("sweeps", c_int), ("converged", c_int), ("reserved", c_int)]


#: the entry point of include/nbody_batch_groups.h (friends-of-friends groups of batched ensembles), which nbody.h includes
_GROUPS_PROTOTYPES = {
    "nbody_batch_groups": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_float), c_int, c_int, c_int, POINTER(BatchGroupSystem),
                                   POINTER(BatchGroupRecord), POINTER(BatchGroupBody)]),
}


BATCH_SPAN_MAX_ROUNDS = 13


class BatchSpanSystem(ctypes.Structure):
    """``nbody_batch_span_system`` of include/nbody_batch_span.h."""
    _fields_ = [("edges", c_int), ("selected", c_int), ("rounds", c_int), ("reserved", c_int), ("total_length", c_double),
                ("longest", c_double), ("mean_separation", c_double)]


class BatchSpanEdge(ctypes.Structure):
    """``nbody_batch_span_edge`` of include/nbody_batch_span.h."""
    _fields_ = [("i", c_int), ("j", c_int), ("r2", c_float), ("reserved", c_int)]


class BatchSpanBody(ctypes.Structure):
    """``nbody_batch_span_body`` of include/nbody_batch_span.h."""
    _fields_ = [("degree", c_int), ("nearest", c_int)]


#: the entry point of include/nbody_batch_span.h (minimum spanning trees of batched ensembles), which nbody.h includes
_SPAN_PROTOTYPES = {
    "nbody_batch_span": (c_int, [c_void_p, c_void_p, POINTER(ctypes.c_ubyte), c_int, POINTER(BatchSpanSystem),
                                 POINTER(BatchSpanEdge), POINTER(BatchSpanBody)]),
}


BATCH_NEIGHBOURS_MAX = 8


class BatchNeighbourSystem(ctypes.Structure):
    """``nbody_batch_neighbour_system`` of include/nbody_batch_neighbours.h."""
    _fields_ = [("bodies", c_int), ("sources", c_int), ("listed", c_int), ("complete", c_int), ("mutual", c_int),
                ("reserved", c_int), ("mean_nearest", c_double), ("mean_kth", c_double)]


class BatchNeighbourBody(ctypes.Structure):
    """``nbody_batch_neighbour_body`` of include/nbody_batch_neighbours.h."""
    _fields_ = [("found", c_int), ("within", c_int)]


#: the entry point of include/nbody_batch_neighbours.h (nearest-neighbour lists of batched ensembles), which nbody.h includes
_NEIGHBOURS_PROTOTYPES = {
    "nbody_batch_neighbours": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_float), POINTER(ctypes.c_ubyte),
                                       POINTER(BatchNeighbourSystem), POINTER(BatchNeighbourBody), POINTER(c_int),
                                       POINTER(c_float)]),
}


BATCH_CORRELATION_MAX_BINS = 32


class BatchCorrelationSystem(ctypes.Structure):
    """``nbody_batch_correlation_system`` of include/nbody_batch_correlation.h."""
    _fields_ = [("rows", c_int), ("sources", c_int), ("both", c_int), ("bins", c_int), ("pairs", ctypes.c_longlong),
                ("below", ctypes.c_longlong), ("above", ctypes.c_longlong), ("unmeasured", ctypes.c_longlong)]


#: the entry point of include/nbody_batch_correlation.h (pair-separation counts of batched ensembles), which nbody.h includes
_CORRELATION_PROTOTYPES = {
    "nbody_batch_correlation": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_float), c_int, POINTER(ctypes.c_ubyte),
                                        POINTER(ctypes.c_ubyte), POINTER(BatchCorrelationSystem), POINTER(ctypes.c_uint)]),
}


BATCH_CONTACTS_MAX_ENTRIES = 1 << 28


class BatchContactSystem(ctypes.Structure):
    """``nbody_batch_contact_system`` of include/nbody_batch_contacts.h."""
    _fields_ = [("bodies", c_int), ("touching", c_int), ("max_degree", c_int), ("reserved", c_int), ("pairs", ctypes.c_longlong),
                ("stored", ctypes.c_longlong), ("closest_i", c_int), ("closest_j", c_int), ("closest_r2", c_float),
                ("reserved2", c_int)]


class BatchContactBody(ctypes.Structure):
    """``nbody_batch_contact_body`` of include/nbody_batch_contacts.h."""
    _fields_ = [("degree", c_int), ("upper", c_int), ("first", c_int), ("nearest", c_int)]


class BatchContact(ctypes.Structure):
    """``nbody_batch_contact`` of include/nbody_batch_contacts.h."""
    _fields_ = [("i", c_int), ("j", c_int), ("r2", c_float)]


#: the entry point of include/nbody_batch_contacts.h (contact lists of batched ensembles), which nbody.h includes
_CONTACTS_PROTOTYPES = {
    "nbody_batch_contacts": (c_int, [c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), POINTER(ctypes.c_ubyte),
                                     ctypes.c_longlong, POINTER(BatchContactSystem), POINTER(BatchContactBody),
                                     POINTER(BatchContact)]),
}


BATCH_APPROACHES_MAX_ENTRIES = 1 << 27
BATCH_APPROACH_NOW, BATCH_APPROACH_PASSAGE, BATCH_APPROACH_END = 0, 1, 2


class BatchApproachSystem(ctypes.Structure):
    """``nbody_batch_approach_system`` of include/nbody_batch_approaches.h."""
    _fields_ = [("bodies", c_int), ("approaching", c_int), ("max_degree", c_int), ("reserved", c_int), ("pairs", ctypes.c_longlong),
                ("stored", ctypes.c_longlong), ("now", c_int), ("passing", c_int), ("ending", c_int), ("reserved2", c_int)]


class BatchApproachBody(ctypes.Structure):
    """``nbody_batch_approach_body`` of include/nbody_batch_approaches.h."""
    _fields_ = [("degree", c_int), ("upper", c_int), ("first", c_int), ("now", c_int)]


class BatchApproach(ctypes.Structure):
    """``nbody_batch_approach`` of include/nbody_batch_approaches.h."""
    _fields_ = [("i", c_int), ("j", c_int), ("r2", c_float), ("rv", c_float), ("v2", c_float), ("phase", c_int)]


#: the entry point of include/nbody_batch_approaches.h (approach lists of batched ensembles), which nbody.h includes
_APPROACHES_PROTOTYPES = {
    "nbody_batch_approaches": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), POINTER(c_float),
                                       POINTER(ctypes.c_ubyte), ctypes.c_longlong, POINTER(BatchApproachSystem),
                                       POINTER(BatchApproachBody), POINTER(BatchApproach)]),
}


BATCH_RADIAL_MAX_SHELLS = 32
BATCH_RADIAL_BELOW, BATCH_RADIAL_UNMEASURED, BATCH_RADIAL_NOT_TAKING = -1, -2, -3


class BatchRadialShell(ctypes.Structure):
    """``nbody_batch_radial_shell`` of include/nbody_batch_radial.h."""
    _fields_ = [("count", ctypes.c_longlong), ("weight", c_double), ("radius", c_double), ("vr1", c_double), ("vr2", c_double),
                ("vt2", c_double), ("L", c_double * 3), ("U", c_double * 3), ("M", c_double * 6), ("V", c_double * 6)]


class BatchRadialSystem(ctypes.Structure):
    """``nbody_batch_radial_system`` of include/nbody_batch_radial.h."""
    _fields_ = [("selected", c_int), ("below", c_int), ("above", c_int), ("unmeasured", c_int), ("shells", c_int), ("projected", c_int),
                ("total_weight", c_double), ("centre", c_double * 3), ("velocity", c_double * 3)]


class BatchRadialBody(ctypes.Structure):
    """``nbody_batch_radial_body`` of include/nbody_batch_radial.h."""
    _fields_ = [("shell", c_int), ("reserved", c_int), ("radius", c_double), ("radial_velocity", c_double)]


#: the entry point of include/nbody_batch_radial.h (radial profiles of batched ensembles), which nbody.h includes
_RADIAL_PROTOTYPES = {
    "nbody_batch_radial_profile": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_double), c_int, POINTER(c_double),
                                           POINTER(c_double), c_int, c_int, POINTER(ctypes.c_ubyte), POINTER(BatchRadialSystem),
                                           POINTER(BatchRadialShell), POINTER(BatchRadialBody)]),
}


BATCH_SURFACE_MAX_SIDE = 64
BATCH_SURFACE_OUTSIDE, BATCH_SURFACE_UNMEASURED, BATCH_SURFACE_NOT_TAKING = -1, -2, -3


class BatchSurfaceCell(ctypes.Structure):
    """``nbody_batch_surface_cell`` of include/nbody_batch_surface.h."""
    _fields_ = [("count", ctypes.c_longlong), ("weight", c_double), ("v1", c_double), ("v2", c_double), ("pa", c_double),
                ("pb", c_double), ("z1", c_double), ("z2", c_double)]


class BatchSurfaceSystem(ctypes.Structure):
    """``nbody_batch_surface_system`` of include/nbody_batch_surface.h."""
    _fields_ = [("selected", c_int), ("outside", c_int), ("unmeasured", c_int), ("columns", c_int), ("rows", c_int), ("occupied", c_int),
                ("peak", c_int), ("peak_count", c_int), ("total_weight", c_double), ("centre", c_double * 3), ("velocity", c_double * 3)]


class BatchSurfaceBody(ctypes.Structure):
    """``nbody_batch_surface_body`` of include/nbody_batch_surface.h."""
    _fields_ = [("cell", c_int), ("reserved", c_int), ("a", c_double), ("b", c_double)]


#: the entry point of include/nbody_batch_surface.h (surface maps of batched ensembles), which nbody.h includes
_SURFACE_PROTOTYPES = {
    "nbody_batch_surface_map": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_double), POINTER(c_double), c_int,
                                        POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int, POINTER(ctypes.c_ubyte),
                                        POINTER(BatchSurfaceSystem), POINTER(BatchSurfaceCell), POINTER(BatchSurfaceBody)]),
}


BATCH_SHAPE_MAX_APERTURES = 8
BATCH_SHAPE_MAX_ITERATIONS = 64
BATCH_SHAPE_CONVERGED, BATCH_SHAPE_MAX, BATCH_SHAPE_FEW, BATCH_SHAPE_DEGENERATE = 0, 1, 2, 3


class BatchShapeAperture(ctypes.Structure):
    """``nbody_batch_shape_aperture`` of include/nbody_batch_shape.h."""
    _fields_ = [("status", c_int), ("iterations", c_int), ("count", ctypes.c_longlong), ("radius", c_double), ("inner", c_double),
                ("q", c_double), ("s", c_double), ("change", c_double), ("eigenvalues", c_double * 3), ("axes", c_double * 9),
                ("weight", c_double), ("D", c_double * 3), ("M", c_double * 6), ("L", c_double * 3)]


class BatchShapeSystem(ctypes.Structure):
    """``nbody_batch_shape_system`` of include/nbody_batch_shape.h."""
    _fields_ = [("selected", c_int), ("unmeasured", c_int), ("apertures", c_int), ("reduced", c_int), ("converged", c_int),
                ("reserved", c_int), ("total_weight", c_double), ("centre", c_double * 3), ("velocity", c_double * 3)]


class BatchShapeBody(ctypes.Structure):
    """``nbody_batch_shape_body`` of include/nbody_batch_shape.h."""
    _fields_ = [("inside", ctypes.c_uint), ("reserved", c_int)]


#: the entry point of include/nbody_batch_shape.h (shapes of batched ensembles), which nbody.h includes
_SHAPE_PROTOTYPES = {
    "nbody_batch_shape": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_double), POINTER(c_double), c_int, POINTER(c_double),
                                  POINTER(c_double), c_int, c_int, c_double, c_int, c_int, POINTER(ctypes.c_ubyte),
                                  POINTER(BatchShapeSystem), POINTER(BatchShapeAperture), POINTER(BatchShapeBody)]),
}


BATCH_PAIR_VELOCITIES_MAX_BINS = 32


class BatchPairVelocitiesBin(ctypes.Structure):
    """``nbody_batch_pair_velocities_bin`` of include/nbody_batch_pair_velocities.h."""
    _fields_ = [("count", ctypes.c_longlong), ("approaching", ctypes.c_longlong), ("receding", ctypes.c_longlong),
                ("weight", c_double), ("r1", c_double), ("r2", c_double), ("rv", c_double), ("vr1", c_double), ("vr2", c_double),
                ("vt2", c_double), ("v1", c_double), ("v2", c_double)]


class BatchPairVelocitiesSystem(ctypes.Structure):
    """``nbody_batch_pair_velocities_system`` of include/nbody_batch_pair_velocities.h."""
    _fields_ = [("rows", c_int), ("sources", c_int), ("both", c_int), ("bins", c_int), ("weight", c_int), ("reserved", c_int),
                ("pairs", ctypes.c_longlong), ("below", ctypes.c_longlong), ("above", ctypes.c_longlong),
                ("unmeasured", ctypes.c_longlong)]


#: the entry point of include/nbody_batch_pair_velocities.h (pair velocity statistics of batched ensembles), which nbody.h includes
_PAIR_VELOCITIES_PROTOTYPES = {
    "nbody_batch_pair_velocities": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(c_float), c_int, POINTER(ctypes.c_ubyte),
                                            POINTER(ctypes.c_ubyte), c_int, POINTER(BatchPairVelocitiesSystem),
                                            POINTER(BatchPairVelocitiesBin)]),
}


BATCH_MUTUAL_GRAVITY_MAX_SETS = 8
BATCH_MUTUAL_GRAVITY_NO_SET = 255


class BatchMutualGravityEntry(ctypes.Structure):
    """``nbody_batch_mutual_gravity_entry`` of include/nbody_batch_mutual_gravity.h."""
    _fields_ = [("pairs", ctypes.c_longlong), ("potential", c_double), ("force", c_double * 3), ("torque", c_double * 3),
                ("virial", c_double), ("power", c_double)]


class BatchMutualGravitySystem(ctypes.Structure):
    """``nbody_batch_mutual_gravity_system`` of include/nbody_batch_mutual_gravity.h."""
    _fields_ = [("sets", c_int), ("selected", c_int), ("left_out", c_int), ("unmeasured", c_int), ("pairs", ctypes.c_longlong),
                ("coincident", ctypes.c_longlong), ("members", c_int * 8), ("mass", c_double * 8)]


#: the entry point of include/nbody_batch_mutual_gravity.h (mutual gravity of labelled sets of batched ensembles), which nbody.h includes
_MUTUAL_GRAVITY_PROTOTYPES = {
    "nbody_batch_mutual_gravity": (c_int, [c_void_p, c_void_p, c_void_p, c_int, POINTER(ctypes.c_ubyte), c_float, POINTER(c_double),
                                           POINTER(c_double), POINTER(BatchMutualGravitySystem), POINTER(BatchMutualGravityEntry)]),
}


class MultiConfig(ctypes.Structure):
    """``nbody_multi_config`` of include/nbody.h."""
    _fields_ = [("n_bodies", c_int64), ("split_len", c_int64), ("force_mode", c_int), ("integrator", c_int),
                ("exchange", c_int), ("transport", c_int), ("body_order", c_int), ("create_timeout_s", c_int)]

_lib = None


def load() -> ctypes.CDLL:
    """Load the in-tree shared library; raises if it has not been built."""
    global _lib
    if _lib is None:
        path = os.environ.get("NBODY_AMD_LIBRARY", LIB_PATH)  # an A/B build of the same ABI (tools/build_variant.sh)
        if not os.path.exists(path):
            raise ImportError(
                f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc, gfx950).  n_body_problem_amd has no CPU or PyTorch fallback.")
        try:
            # PyTorch-ROCm ships its own HIP runtime: let it load first so that this library binds to the same
            # one (loading the system runtime first and torch's second leaves the process without a device)
            import torch  # noqa: F401
        except ImportError:  # a torch-free host (ctypes only) uses the system runtime
            pass
        lib = ctypes.CDLL(path)
        for name, (res, args) in list(_PROTOTYPES.items()) + list(_EVOLVE_PROTOTYPES.items()) + list(_STOP_PROTOTYPES.items()) + \
                list(_MERGE_PROTOTYPES.items()) + list(_RADII_PROTOTYPES.items()) + list(_MASSIVE_PROTOTYPES.items()) + list(_FATE_PROTOTYPES.items()) + \
                list(_ACCRETE_PROTOTYPES.items()) + list(_FIELD_PROTOTYPES.items()) + list(_PAIRS_PROTOTYPES.items()) + \
                list(_STRUCTURE_PROTOTYPES.items()) + list(_MEMBERS_PROTOTYPES.items()) + list(_HIERARCHY_PROTOTYPES.items()) + \
                list(_GRAVITY_PROTOTYPES.items()) + list(_GROUPS_PROTOTYPES.items()) + list(_SPAN_PROTOTYPES.items()) + \
                list(_NEIGHBOURS_PROTOTYPES.items()) + list(_CORRELATION_PROTOTYPES.items()) + \
                list(_CONTACTS_PROTOTYPES.items()) + list(_APPROACHES_PROTOTYPES.items()) + list(_RADIAL_PROTOTYPES.items()) + \
                list(_SURFACE_PROTOTYPES.items()) + list(_SHAPE_PROTOTYPES.items()) + \
                list(_PAIR_VELOCITIES_PROTOTYPES.items()) + list(_MUTUAL_GRAVITY_PROTOTYPES.items()):
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def exported_names():
    """The entry points nbody.h itself declares."""
    return list(_PROTOTYPES)


def evolve_names():
    """The entry points of nbody_batch_evolve.h."""
    return list(_EVOLVE_PROTOTYPES)


def stop_names():
    """The entry points of nbody_batch_stop.h."""
    return list(_STOP_PROTOTYPES)


def merge_exported_names():
    """The entry points of nbody_batch_merge.h."""
    return list(_MERGE_PROTOTYPES)


def radii_names():
    """The entry points of nbody_batch_radii.h."""
    return list(_RADII_PROTOTYPES)


def massive_names():
    """The entry points of nbody_batch_massive.h."""
    return list(_MASSIVE_PROTOTYPES)


def fate_names():
    """The entry points of nbody_batch_fate.h."""
    return list(_FATE_PROTOTYPES)


def accrete_names():
    """The entry points of nbody_batch_accrete.h."""
    return list(_ACCRETE_PROTOTYPES)


def field_names():
    """The entry points of nbody_batch_field.h."""
    return list(_FIELD_PROTOTYPES)


def pairs_names():
    """The entry points of nbody_batch_pairs.h."""
    return list(_PAIRS_PROTOTYPES)


def structure_names():
    """The entry point of nbody_batch_structure.h."""
    return list(_STRUCTURE_PROTOTYPES)


def members_names():
    """The entry point of nbody_batch_members.h."""
    return list(_MEMBERS_PROTOTYPES)


def hierarchy_names():
    """The entry point of nbody_batch_hierarchy.h."""
    return list(_HIERARCHY_PROTOTYPES)


def gravity_names():
    """The entry point of nbody_batch_gravity.h."""
    return list(_GRAVITY_PROTOTYPES)


def groups_names():
    """The entry point of nbody_batch_groups.h."""
    return list(_GROUPS_PROTOTYPES)


def span_names():
    """The entry point of nbody_batch_span.h."""
    return list(_SPAN_PROTOTYPES)


def neighbours_names():
    """The entry point of nbody_batch_neighbours.h."""
    return list(_NEIGHBOURS_PROTOTYPES)


def correlation_names():
    """The entry point of nbody_batch_correlation.h."""
    return list(_CORRELATION_PROTOTYPES)


def contacts_names():
    """The entry point of nbody_batch_contacts.h."""
    return list(_CONTACTS_PROTOTYPES)


def approaches_names():
    """The entry point of nbody_batch_approaches.h."""
    return list(_APPROACHES_PROTOTYPES)


def radial_names():
    """The entry point of nbody_batch_radial.h."""
    return list(_RADIAL_PROTOTYPES)


def surface_names():
    """The entry point of nbody_batch_surface.h."""
    return list(_SURFACE_PROTOTYPES)


def shape_names():
    """The entry point of nbody_batch_shape.h."""
    return list(_SHAPE_PROTOTYPES)


def pair_velocities_names():
    """The entry point of nbody_batch_pair_velocities.h."""
    return list(_PAIR_VELOCITIES_PROTOTYPES)


def mutual_gravity_names():
    """The entry point of nbody_batch_mutual_gravity.h."""
    return list(_MUTUAL_GRAVITY_PROTOTYPES)


def check(status: int, ctx=None) -> None:
    if status != NBODY_OK:
        lib = load()
        msg = lib.nbody_last_error(ctx) or b""
        text = msg.decode("utf-8", "replace") or lib.nbody_status_string(status).decode()
        raise NBodyError(status, text)
