"""MI355X-native all-pairs N-body step: drop-in for the step path of ctbfl/N_body_problem.

Layout: ``csrc/`` hand-written HIP kernels (gfx950) + the C ABI of ``include/nbody.h``;
``system.py`` the host-side mirror of the reference's step interface; ``multi.py`` rows
sharded over the GPUs of one node (the exchange inside the library); ``batch.py`` many independent small systems stepped
together; ``initial_conditions.py`` seeded synthetic inputs.
"""
from .initial_conditions import plummer, uniform_cube, pad_reference_style, padded_count, CONFIG_SEED  # noqa: F401
from ._lib import NBodyError  # noqa: F401
from .system import (NBodySystem, initialize, step, default_split_len, TIME_TICK, SOFTENING_VERSION3,  # noqa: F401
                     SOFTENING_VERSION1, BLOCK_SIZE, pair_once_split_len, morton_order)
from .batch import BatchedSystem, EvolveResult, StopResult, MergeResult, FateResult, AccretionResult, PairResult, StructureResult, MemberResult, HierarchyResult, GravityResult, GRAVITY_RECORD_DTYPE, BatchGroups, SpanResult, NeighbourResult, CorrelationResult, CORRELATION_SYSTEM_DTYPE, ContactsResult, CONTACT_SYSTEM_DTYPE, CONTACT_BODY_DTYPE, CONTACT_DTYPE, ApproachesResult, APPROACH_SYSTEM_DTYPE, APPROACH_BODY_DTYPE, APPROACH_DTYPE, RadialProfileResult, RADIAL_SYSTEM_DTYPE, RADIAL_SHELL_DTYPE, RADIAL_BODY_DTYPE, SurfaceMapResult, SURFACE_SYSTEM_DTYPE, SURFACE_CELL_DTYPE, SURFACE_BODY_DTYPE, ShapeResult, SHAPE_SYSTEM_DTYPE, SHAPE_APERTURE_DTYPE, SHAPE_BODY_DTYPE, PairVelocityResult, PAIR_VELOCITIES_SYSTEM_DTYPE, PAIR_VELOCITIES_BIN_DTYPE, MutualGravityResult, MUTUAL_GRAVITY_SYSTEM_DTYPE, MUTUAL_GRAVITY_ENTRY_DTYPE, HIERARCHY_NODE_DTYPE, HIERARCHY_BODY_DTYPE, HIERARCHY_SYSTEM_DTYPE, BATCH_MAX_BODIES  # noqa: F401

__all__ = ["NBodySystem", "initialize", "step", "default_split_len", "plummer", "uniform_cube",
           "pad_reference_style", "padded_count", "NBodyError", "TIME_TICK", "SOFTENING_VERSION3",
           "SOFTENING_VERSION1", "BLOCK_SIZE", "CONFIG_SEED", "pair_once_split_len", "morton_order",
           "BatchedSystem", "BATCH_MAX_BODIES", "PairResult", "StructureResult", "MemberResult", "HierarchyResult",
           "HIERARCHY_NODE_DTYPE", "HIERARCHY_BODY_DTYPE", "HIERARCHY_SYSTEM_DTYPE", "GravityResult", "GRAVITY_RECORD_DTYPE",
           "BatchGroups", "SpanResult", "NeighbourResult", "CorrelationResult", "CORRELATION_SYSTEM_DTYPE",
           "ContactsResult", "CONTACT_SYSTEM_DTYPE", "CONTACT_BODY_DTYPE", "CONTACT_DTYPE",
           "ApproachesResult", "APPROACH_SYSTEM_DTYPE", "APPROACH_BODY_DTYPE", "APPROACH_DTYPE",
           "RadialProfileResult", "RADIAL_SYSTEM_DTYPE", "RADIAL_SHELL_DTYPE", "RADIAL_BODY_DTYPE",
           "SurfaceMapResult", "SURFACE_SYSTEM_DTYPE", "SURFACE_CELL_DTYPE", "SURFACE_BODY_DTYPE",
           "ShapeResult", "SHAPE_SYSTEM_DTYPE", "SHAPE_APERTURE_DTYPE", "SHAPE_BODY_DTYPE",
           "PairVelocityResult", "PAIR_VELOCITIES_SYSTEM_DTYPE", "PAIR_VELOCITIES_BIN_DTYPE",
           "MutualGravityResult", "MUTUAL_GRAVITY_SYSTEM_DTYPE", "MUTUAL_GRAVITY_ENTRY_DTYPE"]
