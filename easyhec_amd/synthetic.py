"""Synthetic workloads for the BASELINE.json configs: joint angles, link poses, camera pose and
intrinsics.  There is no network / dataset here, so inputs are generated deterministically (seed 0) from the
packaged robot geometry; reference masks are rendered by the HIP renderer itself at the ground-truth pose."""
import numpy as np

from .config import FRANKA_K_1920x1080, XARM7_K_1280x720

__all__ = ["lookat_pose", "camera_Tc_c2b", "scaled_K", "perturb_pose", "make_views", "mounted_camera_X",
           "make_mounted_views", "WORKLOADS"]


def lookat_pose(phi, theta, radius):
    """Camera-to-base pose looking at the origin (restates /root/reference/easyhec/utils/utils_3d.py:359-394,
    ``calc_pose_from_lookat`` for one view): phi from +z, theta azimuth, OpenCV camera axes."""
    c = np.array([radius * np.sin(theta) * np.sin(phi), -radius * np.cos(theta) * np.sin(phi), radius * np.cos(phi)])
    fwd = c / (np.linalg.norm(c) + 1e-10)
    up = np.array([0.0, 0.0, 1.0])
    right = np.cross(up, fwd)
    right = right / (np.linalg.norm(right) + 1e-10)
    if (right ** 2).sum() < 0.01:
        right = np.array([0.0, 1.0, 0.0])
    up = np.cross(fwd, right)
    up = up / (np.linalg.norm(up) + 1e-10)
    pose = np.eye(4)
    pose[:3, :3] = np.stack([right, up, fwd], axis=-1)
    pose[:3, 3] = c
    return pose @ np.diag([1.0, -1.0, -1.0, 1.0])  # blender -> opencv


def camera_Tc_c2b(phi_deg=60.0, theta_deg=20.0, radius=1.3, lift=0.3):
    """Tc_c2b = inverse of the look-at pose with the camera raised by ``lift`` metres
    (recipe of /root/reference/tools/manual_tune_franka_init.py:20-26)."""
    Tb_b2c = lookat_pose(np.radians(phi_deg), np.radians(theta_deg), radius)
    Tb_b2c[2, 3] += lift
    return np.linalg.inv(Tb_b2c)


def scaled_K(K, scale, W=None, H=None, recentre=False):
    K = np.array(K, dtype=np.float64)
    K[:2] *= scale
    if recentre:
        K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    return K


def perturb_pose(Tc_c2b, dt=(0.02, -0.015, 0.02), drot_deg=(3.0, -2.0, 2.0)):
    """GT o exp([dt, drot]) -- the initial pose error of config 2."""
    w = np.radians(np.asarray(drot_deg, dtype=np.float64))
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / th ** 2) * (K @ K) if th > 0 else np.eye(3)
    D = np.eye(4)
    D[:3, :3] = R
    D[:3, 3] = dt
    return Tc_c2b @ D


def make_views(robot, n_views, seed=0, qpos_scale=0.5):
    """(qpos [n,7], link_poses [n,L,4,4] float32) for n synthetic views of one camera."""
    rng = np.random.default_rng(seed)
    q = robot.sample_qpos(n_views, rng, scale=qpos_scale)
    lp = np.stack([robot.link_poses(qi) for qi in q]).astype(np.float32)
    return q, lp


def mounted_camera_X(position=(0.0, 0.15, 0.15), look=(0.0, -1.0, -0.6), up=(1.0, 0.0, 0.0)):
    """``X = T_cam<-mount`` of a camera bolted to a link (eye-in-hand): the camera's centre at ``position`` in the mount link's
    frame, its optical axis (OpenCV +z) along ``look``, its image x axis along ``up x look``.  The default is a camera on the
    xArm7's last arm link, 15 cm out on the tool side and 15 cm off the axis, that looks back at the arm across the link's
    axis.  It does not look straight back along that axis: every such pose is a half turn of the mount's frame, and a half
    turn is where the rotation-vector coordinates of ``model.dof`` are singular (w and -w are the same rotation) -- no place
    to start a solve from; this X is a turn of 139 degrees."""
    z = np.asarray(look, dtype=np.float64)
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, dtype=np.float64), z)
    x = x / np.linalg.norm(x)
    T = np.eye(4)
    T[:3, :3] = np.stack([x, np.cross(z, x), z], axis=-1)
    T[:3, 3] = position
    return np.linalg.inv(T)


def make_mounted_views(view, n_views, K, H, W, X=None, seed=0, qpos_scale=0.5, min_links=4, min_depth=0.15, tries=10000):
    """(qpos [n,7], link_poses [n,L,4,4] float32 mount<-link) for n synthetic views of a camera that rides on the arm.
    view: ``robot.mounted(link)``; X: the camera's true pose in the mount (default :func:`mounted_camera_X`).  A camera on
    the arm sees nothing of it from most joint vectors, so vectors are drawn like :func:`make_views` draws them and kept
    where the centres of at least ``min_links`` rendered links that do not ride with the mount project inside the image at
    a depth of ``min_depth`` metres or more."""
    X = mounted_camera_X() if X is None else np.asarray(X, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    rng = np.random.default_rng(seed)
    centre = np.array([(v.min(0) + v.max(0)) / 2 for v, _ in view.meshes], dtype=np.float64)
    moving = np.asarray(view.joint_table()["upstream"]) != 0          # (relative mask: the link moves in the mount's frame)
    qs = []
    for _ in range(tries):
        q = view.sample_qpos(1, rng, scale=qpos_scale)[0]
        P = X @ view.link_poses(q)
        p = np.einsum("lrc,lc->lr", P[:, :3, :3], centre) + P[:, :3, 3]
        z = np.where(p[:, 2] > 0, p[:, 2], np.inf)
        u, v = K[0, 0] * p[:, 0] / z + K[0, 2], K[1, 1] * p[:, 1] / z + K[1, 2]
        seen = moving & (p[:, 2] >= min_depth) & (u > 0) & (u < W) & (v > 0) & (v < H)
        if seen.sum() >= min_links:
            qs.append(q)
            if len(qs) == n_views:
                break
    if len(qs) < n_views:
        raise ValueError(f"make_mounted_views: {len(qs)} of {n_views} views found in {tries} draws: the camera sees too little")
    q = np.stack(qs)
    return q, np.stack([view.link_poses(qi) for qi in q]).astype(np.float32)


# name -> (robot, H, W, K, number of views, camera radius, lift)
WORKLOADS = {
    # config 1: plumbing case, single merged mesh is handled by the tests directly (320x240)
    "xarm7_640x480_1view": dict(robot="xarm7", H=480, W=640, K=scaled_K(XARM7_K_1280x720, 0.5, 640, 480, True),
                                views=1, radius=1.3, lift=0.3),
    "xarm7_1280x720_8view": dict(robot="xarm7", H=720, W=1280, K=np.array(XARM7_K_1280x720), views=8, radius=1.3,
                                 lift=0.3),
    "franka_1920x1080_16view": dict(robot="franka", H=1080, W=1920, K=np.array(FRANKA_K_1920x1080), views=16,
                                    radius=2.6, lift=0.5),
    "xarm7_1280x720_64view": dict(robot="xarm7", H=720, W=1280, K=np.array(XARM7_K_1280x720), views=64, radius=1.3,
                                  lift=0.3),
}
