"""ctypes binding of libehr_hip.so (include/ehr.h).  There is NO fallback: if the library is missing, or a tensor
is not on a HIP device, the call raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EHR_LIB") or os.path.join(_HERE, "libehr_hip.so")  # EHR_LIB: A/B builds of the same ABI
_lib = None

c_void_p, c_int, c_size_t, c_float = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float

# name -> (restype, argtypes); mirrors include/ehr.h one to one
SIGNATURES = {
    "ehr_version": (c_int, []),
    "ehr_last_error": (ctypes.c_char_p, []),
    "ehr_device_count": (c_int, []),
    "ehr_device_arch": (ctypes.c_char_p, [c_int]),
    "ehr_ctx_create": (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    "ehr_ctx_destroy": (c_int, [c_void_p]),
    "ehr_ctx_scratch_bytes": (c_size_t, [c_void_p]),
    "ehr_tile_flags_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ehr_rasterize_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "ehr_rasterize_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p]),
    "ehr_rasterize_grad_db": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p]),
    "ehr_interpolate_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p, c_void_p]),
    "ehr_interpolate_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ehr_interpolate_da_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 8 + [c_void_p, c_void_p]),
    "ehr_interpolate_da_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 8 +
                                [c_void_p, c_void_p, c_void_p]),
    "ehr_topology_scratch_bytes": (c_size_t, [c_int]),
    "ehr_antialias_topology": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "ehr_antialias_work_bytes": (c_size_t, [c_int, c_int, c_int]),
    "ehr_antialias_fwd": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ehr_antialias_fwd_zg": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ehr_antialias_grad": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ehr_fused_plan": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "ehr_render_mask_loss": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p]),
    "ehr_mask_information": (c_int, [c_void_p] * 8 + [c_int, c_void_p] + [c_int] * 6 + [c_void_p] * 6),
    "ehr_fused_status": (c_int, [c_void_p]),
    "ehr_fused_bind_ref": (c_int, [c_void_p, c_void_p, c_void_p]),
    "ehr_pose_forward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_float, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_pose_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_float, c_float, c_void_p, c_void_p]),
    "ehr_pose_adam": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_float, c_float, c_float,
                              c_float, c_void_p, c_void_p, c_void_p]),
    "ehr_solver_step": (c_int, [c_void_p] * 9 + [c_int] * 6 + [c_float] * 2 + [c_void_p] * 5 + [c_int, c_void_p] +
                        [c_float] * 5 + [c_void_p] * 8 + [c_int, c_void_p]),
    "ehr_solver_step_multi": (c_int, [c_void_p] * 9 + [c_int] * 7 + [c_float] * 2 + [c_void_p] * 5 + [c_int, c_void_p] +
                              [c_float] * 5 + [c_void_p] * 8 + [c_void_p]),
    "ehr_fused_bind_ref_shared": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_fused_bind_weight": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_mask_variance": (c_int, [c_void_p] * 5 + [c_int] * 7 + [c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_mask_overlap": (c_int, [c_void_p] * 6 + [c_int] * 7 + [c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_mask_distance": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ehr_mask_cost": (c_int, [c_void_p] * 6 + [c_int] * 8 + [c_void_p, c_int, c_void_p]),
    "ehr_comm_unique_id": (c_int, [c_void_p]),
    "ehr_comm_init": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "ehr_comm_allreduce": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "ehr_comm_destroy": (c_int, [c_void_p]),
    "ehr_comm_p2p_export": (c_int, [c_void_p, c_void_p]),
    "ehr_comm_p2p_open": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "ehr_comm_p2p_step": (c_int, [c_void_p] * 6 + [c_float] * 5 + [c_void_p, c_void_p, c_void_p]),
    "ehr_comm_p2p_close": (c_int, [c_void_p]),
    "ehr_graph_begin": (c_int, [c_void_p, ctypes.POINTER(c_void_p)]),
    "ehr_graph_end": (c_int, [c_void_p]),
    "ehr_graph_launch": (c_int, [c_void_p, c_void_p]),
    "ehr_graph_release": (c_int, [c_void_p]),
    "ehr_fused_timing": (c_int, [c_void_p, c_int]),
    "ehr_fused_timing_read": (c_int, [c_void_p, ctypes.POINTER(c_float), ctypes.POINTER(c_int)]),
    "ehr_joint_forward": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ehr_joint_backward_adam": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_float] * 2 + [c_void_p] * 10 + [c_float] * 5 +
                                [c_void_p, c_void_p]),
    "ehr_rig_backward_adam": (c_int, [c_void_p] + [c_int] * 3 + [c_void_p] * 7 + [c_float] * 7 + [c_void_p, c_void_p]),
    "ehr_intrinsics_backward_adam": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p] * 3 + [c_int] + [c_void_p] * 4 +
                                     [c_float] * 5 + [c_void_p] * 3),
    "ehr_lm_linearize": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_float] * 2 + [c_void_p] * 4 + [c_int] * 5 + [c_void_p] * 3),
    "ehr_lm_update": (c_int, [c_void_p] * 4 + [c_int] * 2 + [c_void_p] * 3 + [c_int] * 2 + [c_void_p] + [c_int] * 2 +
                      [c_void_p] * 2 + [c_int] * 2 + [ctypes.c_double] * 2 + [c_int] + [c_void_p] * 2 + [c_int, c_void_p]),
    "ehr_lm_update_prior": (c_int, [c_void_p] * 4 + [c_int] * 2 + [c_void_p] * 3 + [c_int] * 2 + [c_void_p] + [c_int] * 2 +
                            [c_void_p] * 2 + [c_int] * 2 + [ctypes.c_double] * 2 + [c_int] + [c_void_p] * 2 + [c_int] +
                            [c_void_p] * 3),
    "ehr_lm_linearize_multi": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_float] * 2 + [c_void_p] * 3),
    "ehr_lm_update_multi": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p] + [ctypes.c_double] * 2 + [c_int] +
                            [c_void_p] * 2 + [c_int, c_void_p]),
    "ehr_joint_forward_multi": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 3),
    "ehr_joint_forward_mounted": (c_int, [c_void_p] * 6 + [c_int] * 4 + [ctypes.c_uint32, c_void_p, c_void_p, c_int] +
                                  [c_void_p] * 3),
    "ehr_joint_forward_multi_mounted": (c_int, [c_void_p] * 6 + [c_int] * 4 + [ctypes.c_uint32, c_void_p, c_void_p, c_int, c_int] +
                                        [c_void_p] * 3),
    "ehr_lm_linearize_multi_calib": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_float] * 2 + [c_void_p] * 4 + [c_int] * 5 +
                                     [c_void_p] * 3),
    "ehr_lm_update_multi_calib": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 3 + [c_int] * 2 + [c_void_p] +
                                  [c_int] * 2 + [c_void_p] * 2 + [c_int] * 2 + [ctypes.c_double] * 2 + [c_int] +
                                  [c_void_p] * 2 + [c_int] + [c_void_p] * 3),
    "ehr_lm_update_rig": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [ctypes.c_double] * 2 + [c_int] +
                          [c_void_p] * 2 + [c_int, c_void_p]),
    "ehr_lm_update_rig_prior": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [ctypes.c_double] * 2 + [c_int] +
                                [c_void_p] * 2 + [c_int] + [c_void_p] * 3),
    "ehr_lm_update_rig_arrow": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int] + [ctypes.c_double] * 2 + [c_int] +
                                [c_void_p] * 2 + [c_int] + [c_void_p] * 3),
    "ehr_information_gain": (c_int, [c_void_p] * 4 + [c_int] * 3 + [ctypes.c_double, ctypes.c_uint32, c_void_p, c_void_p]),
    "ehr_information_pick": (c_int, [c_void_p] * 2 + [c_int] * 3 + [ctypes.c_double, c_int] + [c_void_p] * 5),
    "ehr_config_clearance": (c_int, [c_void_p] * 6 + [c_int, c_void_p, c_int, ctypes.c_uint32, c_void_p, ctypes.c_double] +
                             [c_int] * 2 + [c_void_p] * 5),
    "ehr_mesh_clearance": (c_int, [c_void_p] * 6 + [c_int, c_void_p, c_int, ctypes.c_uint32, ctypes.c_double] + [c_int] * 2 +
                           [c_void_p] * 2 + [c_int] + [c_void_p] * 5),
    "ehr_segment_clearance": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 +
                              [c_int, c_void_p, c_int, ctypes.c_uint32, c_void_p, ctypes.c_double] + [c_void_p] * 3 +
                              [ctypes.c_double] + [c_int] * 3 + [c_void_p] * 13),
    "ehr_edge_clearance": (c_int, [c_void_p] * 6 + [c_int] * 3 + [c_void_p, c_int] + [c_void_p] * 3 + [c_int] + [c_void_p] * 5 +
                           [c_int, c_void_p, c_int, ctypes.c_uint32, c_void_p, ctypes.c_double] + [c_void_p] * 3 +
                           [ctypes.c_double] + [c_int] * 3 + [c_void_p] * 14),
    "ehr_roadmap_paths": (c_int, [c_void_p] * 3 + [c_int] + [c_void_p] * 2 + [c_int] * 4 + [c_void_p] * 8),
}


def lib():
    """Load libehr_hip.so; raises (loudly) if it has not been built -- there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m easyhec_amd.build` (hipcc --offload-arch=gfx950). "
                "easyhec_amd has no CPU or PyTorch fallback for the render path.")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export a symbol the header declares
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def has_symbols(*names):
    """True if the library exports every one of ``names``.  The ABI version does not change when an entry is added: the
    symbols' presence is the capability check, looked up on the bare library (the loaded one where there is one), so it also
    answers for an ``EHR_LIB`` build that predates them, which :func:`lib` would refuse to bind.  False where the file is
    missing."""
    if not os.path.exists(LIB_PATH):
        return False
    so = _lib if _lib is not None else ctypes.CDLL(LIB_PATH)
    return all(hasattr(so, n) for n in names)


# what each feature needs of the library (the names tests and tools ask by)
def has_multistart():
    return has_symbols("ehr_solver_step_multi")


def has_pose_search():
    return has_symbols("ehr_mask_overlap")


def has_soft_search():
    return has_symbols("ehr_mask_distance", "ehr_mask_cost")


def has_weighted_loss():
    return has_symbols("ehr_fused_bind_weight")


def has_joint_offsets():
    return has_symbols("ehr_joint_forward", "ehr_joint_backward_adam")


def has_rig():
    return has_symbols("ehr_rig_backward_adam")


def has_intrinsics():
    return has_symbols("ehr_intrinsics_backward_adam")


def has_information():
    return has_symbols("ehr_mask_information")


def has_lm():
    return has_symbols("ehr_lm_linearize", "ehr_lm_update")


def has_lm_multi():
    return has_symbols("ehr_lm_linearize_multi", "ehr_lm_update_multi")


def has_lm_multi_calib():
    return has_symbols("ehr_joint_forward_multi", "ehr_lm_linearize_multi_calib", "ehr_lm_update_multi_calib")


def has_mounted():
    return has_symbols("ehr_joint_forward_mounted", "ehr_joint_forward_multi_mounted")


def has_lm_rig():
    return has_symbols("ehr_lm_update_rig")


def has_lm_rig_arrow():
    return has_symbols("ehr_lm_update_rig_arrow")


def has_lm_prior():
    return has_symbols("ehr_lm_update_prior", "ehr_lm_update_rig_prior")


def has_information_gain():
    return has_symbols("ehr_information_gain", "ehr_information_pick")


def has_feasibility():
    return has_symbols("ehr_config_clearance")


def has_mesh_clearance():
    return has_symbols("ehr_mesh_clearance")


def has_segment_clearance():
    return has_symbols("ehr_segment_clearance")


def has_roadmap():
    return has_symbols("ehr_edge_clearance", "ehr_roadmap_paths")


IG_MAX_PARAMS = 32  # include/ehr.h: EHR_IG_MAX_PARAMS
FEAS_MAX_LINKS, FEAS_MAX_SPHERES, FEAS_MAX_PLANES, FEAS_MAX_OBSTACLES = 32, 4096, 16, 1024  # include/ehr.h: EHR_FEAS_*
MESH_MAX_TRIANGLES = 1048576  # include/ehr.h: EHR_MESH_MAX_TRIANGLES
SEG_MAX_DEPTH, SEG_MAX_EVALS, SEG_MAX_SPHERES = 20, 4096, 3264  # include/ehr.h: EHR_SEG_*
ROADMAP_MAX_NODES, ROADMAP_MAX_HOPS = 4096, 8  # include/ehr.h: EHR_ROADMAP_*


# the state block of ehr_lm_update (include/ehr.h: EHR_LM_*), in float64 words
LM_STATE = {"lambda": 0, "nu": 1, "F_acc": 2, "pred": 3, "rho": 4, "F_trial": 5, "iterations": 6, "accepted": 7, "rejected": 8,
            "reported": 9, "done": 10, "why": 11, "last": 12, "count": 13, "retries": 14, "F_prior": 15}
LM_THETA, LM_DELTA, LM_G, LM_H, LM_STATE_DOUBLES, LM_MAX_PARAMS = 16, 48, 80, 112, 1136, 32


# the state block of ehr_lm_update_rig_arrow (include/ehr.h: EHR_LM_ARROW_*): words 0..15 as LM_STATE, then theta, delta, g with
# a capacity of LM_ARROW_MAX_PARAMS, then H_acc packed: per camera a panel [10][36] and the border's other half [26][10], then
# the corner [26][26]
LM_ARROW_MAX_CAMERAS, LM_ARROW_MAX_BLOCK, LM_ARROW_MAX_SHARED, LM_ARROW_MAX_PARAMS = 16, 10, 26, 192
LM_ARROW_THETA, LM_ARROW_DELTA, LM_ARROW_G, LM_ARROW_H = 16, 208, 400, 592
LM_ARROW_PANEL_STRIDE, LM_ARROW_BORDER_T, LM_ARROW_CAMERA_STRIDE = 36, 360, 620
LM_ARROW_CORNER, LM_ARROW_STATE_DOUBLES = 10512, 11188


class RigCamera(ctypes.Structure):
    """``ehr_rig_camera`` of include/ehr.h, field for field."""
    _fields_ = [(k, c_void_p) for k in ("grad_mvp", "tc_jac", "K", "link_poses", "joint_frames", "red", "dof", "adam_m",
                                        "adam_v", "step", "loss_out", "grad_out")] + \
               [("B", c_int), ("H", c_int), ("W", c_int), ("near_plane", c_float), ("far_plane", c_float)]


class LmRigCamera(ctypes.Structure):
    """``ehr_lm_rig_camera`` of include/ehr.h, field for field."""
    _fields_ = [(k, c_void_p) for k in ("info", "grad", "count", "loss", "dof")] + [("B", c_int)]


class LmRigArrowCamera(ctypes.Structure):
    """``ehr_lm_rig_arrow_camera`` of include/ehr.h, field for field."""
    _fields_ = [(k, c_void_p) for k in ("info", "grad", "count", "loss", "dof", "theta", "K0", "K")] + \
               [(k, c_int) for k in ("B", "H", "W", "free4_mask", "tie_focal")]


EHR_ERR_OVERFLOW = -3  # include/ehr.h
EHR_ERR_RETRY = -4


def check(rc, what):
    if rc != 0:
        msg = lib().ehr_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what}: {msg} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else c_void_p(t.data_ptr())
