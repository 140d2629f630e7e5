"""The eye-in-hand scene of the end-to-end tests (tests/test_gpu_mounted.py), whose preconditions
tests/test_mounted_reference.py checks with the oracle on the CPU: xArm7, the camera on the last arm link (link7), 4 views of
160 x 120.  CPU only, numpy; not collected by pytest."""
import functools
import types

import numpy as np

import helpers

H, W, VIEWS, SCALE = 120, 160, 4, 0.125
MOUNT = "link7"


@functools.lru_cache(maxsize=None)
def scene():
    """(robot, mounted view, K [3,3], X = T_cam<-mount [4,4], qpos [4,J] zero-padded, link_poses [4,L,4,4] float32)."""
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.robot import load_robot
    from easyhec_amd.synthetic import make_mounted_views, mounted_camera_X, scaled_K
    rb = load_robot("xarm7")
    view = rb.mounted(MOUNT)
    K = scaled_K(XARM7_K_1280x720, SCALE, W, H, True)
    X = mounted_camera_X()
    q, lp = make_mounted_views(view, VIEWS, K, H, W, X, seed=0)
    qp = np.zeros((VIEWS, rb.chain.dof))
    qp[:, :q.shape[1]] = q
    return rb, view, K, X, qp, lp


def oracle_masks(oracle, links=None):
    """[B,H,W] float32 masks of the scene at the true X by the CPU oracle; ``links``: only these rendered links."""
    rb, view, K, X, qp, lp = scene()
    links = list(range(len(rb.meshes))) if links is None else list(links)
    only = types.SimpleNamespace(meshes=[rb.meshes[l] for l in links])
    verts, tris, toff, voff = helpers.scene_arrays(only)
    mvp = np.ascontiguousarray(helpers.mvp_numpy(K, H, W, X, lp)[:, links])
    ref = np.zeros((VIEWS, H, W), np.float32)
    return oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref, want_grad=False)[0]
