"""easyhec_amd -- MI355X-native differentiable silhouette rasterizer for EasyHeC's pose-optimisation hot path.

    import easyhec_amd.dr as dr                       # RasterizeCudaContext / rasterize / interpolate / antialias
    from easyhec_amd.renderer import NVDiffrastRenderer
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.trainer import RBSolverTrainer

The compute path is libehr_hip.so (hand-written HIP for gfx950, C ABI in include/ehr.h); there is no CPU fallback.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # the Levenberg-Marquardt solve (easyhec_amd/lm.py), looked up on first use: importing the package stays free of torch
    if name in ("LevenbergMarquardt", "solve_lm", "LmResult", "LmPrior", "make_prior"):
        from . import lm
        return getattr(lm, name)
    # its multi-start form (easyhec_amd/lm_multi.py), likewise
    if name in ("MultiStartLM", "MultiLmResult", "solve_lm_multi", "solve_global_lm", "group_basins"):
        from . import lm_multi
        return getattr(lm_multi, name)
    # its form for a camera rig (easyhec_amd/lm_rig.py), likewise
    if name in ("RigLM", "solve_lm_rig"):
        from . import lm_rig
        return getattr(lm_rig, name)
    # information-gain exploration (easyhec_amd/info_explorer.py), likewise
    if name in ("InformationExplorer", "information_gain", "greedy_select"):
        from . import info_explorer
        return getattr(info_explorer, name)
    # the feasibility filter in front of the explorers' scoring (easyhec_amd/feasibility.py), likewise
    if name in ("FeasibilityFilter", "link_spheres", "box_planes", "config_clearance", "robot_triangles", "mesh_clearance"):
        from . import feasibility
        return getattr(feasibility, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
