"""MI355X-native Barnes-Hut step behind the reference's file-level interface.

The product is libbhgpu.so (hand-written HIP for gfx950, C-ABI in include/bhgpu.h); this package is
the thin Python host above it: a ctypes binding (`_lib`), the engine object (`engine`), the
reference's text formats (`textio`), its step-loop entry points under their own names (`project`)
and the one-process-per-GPU driver (`distributed`).  There is no CPU fallback: without the HIP
library and a GPU, every compute entry point raises.
"""
from .engine import (BarnesHutEngine, BhConfig, BhError, BhForceError, BhGroups, BhLagrangian, BhMomentMap, BhPairCounts, BhRadialProfile, BhSortSnapshot,  # noqa: F401
                     BhTimestep, LagrangianSelect, Precision, correlation_from, density_centre_from, force_error_stats, lagrangian_from,
                     local_density_from, radial_edges, radial_exponents, radial_profile_from_planes,
                     BhMassSegregation, BhSpanningTree, mass_segregation_from, spanning_tree_from, BhBinaries, binaries_from_records,
                     BhNeighbourLists, neighbour_lists_from, BhAzimuthalModes, BhModeTotal, azimuthal_modes_from_planes,
                     modes_exponents, modes_planes, BhRotationCurve, BhResonances, rotation_curve_from_planes, toomre_q_from,
                     resonances_from, disc_velocity_table_from, epicyclic_from)
from .textio import loadSimulationDataFromText, save_init_files  # noqa: F401

__all__ = ["BarnesHutEngine", "BhConfig", "BhError", "BhForceError", "BhGroups", "BhMomentMap", "BhTimestep", "Precision",
           "force_error_stats", "local_density_from", "density_centre_from", "loadSimulationDataFromText", "save_init_files",
           "BhRadialProfile", "BhLagrangian", "LagrangianSelect", "radial_edges", "radial_exponents",
           "radial_profile_from_planes", "lagrangian_from", "BhPairCounts", "correlation_from", "BhSortSnapshot",
           "BhSpanningTree", "BhMassSegregation", "mass_segregation_from", "spanning_tree_from",
           "BhBinaries", "binaries_from_records", "BhNeighbourLists", "neighbour_lists_from",
           "BhAzimuthalModes", "BhModeTotal", "azimuthal_modes_from_planes", "modes_exponents", "modes_planes",
           "BhRotationCurve", "BhResonances", "rotation_curve_from_planes", "toomre_q_from", "resonances_from",
           "disc_velocity_table_from", "epicyclic_from"]
