"""Float64 reference of the eye-in-hand kinematics (csrc/ehr_joint_core.h: joint_forward_view's MOUNTED branch;
``UrdfChain.joint_table(mount=...)``): a camera bolted to node ``mount`` of the flat table sees link l at

    P_l = inv(F_m) @ F_l                                F_i: the base-frame frames of ``joint_reference.fk``

CPU only, numpy; not collected by pytest (the tests are tests/test_mounted_reference.py and tests/test_gpu_mounted.py).

``fk_mounted`` composes with ``np.linalg.inv`` (not with R^T and a subtraction, which is what the kernel does).  The analytic
derivative is written from BASE-frame quantities, with u_i(j) = 1 where active joint j lies between the root and node i:

    d P_l / d offset_j = inv(F_m) @ (u_l(j) - u_m(j)) [xi_j]^ @ F_l          [xi]^ F = [ [a]x R | a x (t - p) ]  (revolute)
                                                                                        [ 0      | a           ]  (prismatic)

with (a, p) joint j's BASE-frame axis and point.  What the kernel writes instead is the pair the unchanged downstream kernels
need: the mount-frame poses, ``joint_frames = (sigma_j R_m^T a_j, R_m^T (p_j - t_m))`` with sigma_j = -1 where u_m(j) = 1, and
the host passes ``upstream[l] ^ mount_upstream``; ``folded`` gives that triple, and tests/test_mounted_reference.py holds
``joint_reference.pose_derivatives`` on it against the derivative above.

The functions that take the DEVICE's outputs (``pose_derivatives``, ``offset_gradient``) have the signatures of their twins in
tests/joint_reference.py, so that the error rules of the base-frame tests apply as they are.  They do not use the folded sign
or the XOR-ed mask: they undo the fold (a'' = sigma a') and apply the factor u_l - u_m from ``upstream_base`` and
``mount_upstream``."""
import numpy as np
import torch

import joint_reference as JR
import pose_reference as R

_NP = R._NP


def masks(table, mount, use=None):
    """(u_l [L] uint32 for the rendered links -- or for ``use`` --, u_m uint32), walked on parent / qidx alone."""
    def walk(i):
        m = 0
        while i >= 0:
            if table["qidx"][i] >= 0:
                m |= 1 << int(table["qidx"][i])
            i = int(table["parent"][i])
        return m
    use = table["use"] if use is None else use
    return np.array([walk(int(i)) for i in use], dtype=np.uint32), np.uint32(walk(int(mount)))


def mounted_table(table, mount):
    """``table`` with the keys ``UrdfChain.joint_table(mount=...)`` adds, built here from parent / qidx."""
    ul, um = masks(table, mount)
    return dict(table, mount=int(mount), mount_upstream=um, upstream_base=ul, upstream=ul ^ um)


def fk_mounted(table, qpos, offset, mount, dtype=torch.float64):
    """(frames [B,N,4,4] base frame, link_poses [B,L,4,4] = inv(F_m) F_l, joint_frames [B,J,6] = (a, p) in the BASE frame) in
    ``dtype``: ``joint_reference.fk`` and one ``np.linalg.inv`` per view."""
    frames, _, jf = JR.fk(table, qpos, offset, dtype)
    inv = np.linalg.inv(frames[:, int(mount)])
    return frames, inv[:, None] @ frames[:, table["use"]], jf


def folded(table, qpos, offset, mount, dtype=torch.float64):
    """What the kernel is specified to write, from the composition above (NOT by the kernel's formula): (link_poses,
    joint_frames [B,J,6] = (sigma_j R a_j, R p_j + t) with [R | t] = inv(F_m), the relative mask [L] uint32)."""
    ft = _NP[dtype]
    frames, lp, jf = fk_mounted(table, qpos, offset, mount, dtype)
    inv = np.linalg.inv(frames[:, int(mount)])
    ul, um = masks(table, mount)
    J = jf.shape[1]
    sigma = np.array([-1.0 if (int(um) >> j) & 1 else 1.0 for j in range(J)], dtype=ft)
    a = np.einsum("brc,bjc->bjr", inv[:, :3, :3], jf[:, :, :3]) * sigma[None, :, None]
    p = np.einsum("brc,bjc->bjr", inv[:, :3, :3], jf[:, :, 3:]) + inv[:, None, :3, 3]
    return lp, np.concatenate([a, p], axis=2).astype(ft), ul ^ um


def _twist_times_frame(kind, a, p, Fl, ft, absolute=False):
    """[xi]^ @ F_l (rows 0..2; the last row is zero) for joint (kind, a, p) and the frame F_l."""
    D = np.zeros((4, 4), dtype=ft)
    Rl, tl = Fl[:3, :3], Fl[:3, 3]
    if kind == 1:
        if absolute:
            ax = np.abs(JR._hat(a, ft))
            D[:3, :3] = ax @ np.abs(Rl)
            D[:3, 3] = ax @ (np.abs(tl) + np.abs(p))
        else:
            D[:3, :3] = JR._hat(a, ft) @ Rl
            D[:3, 3] = np.cross(a, tl - p)
    elif kind == 2:
        D[:3, 3] = np.abs(a) if absolute else a
    return D


def analytic_derivatives(table, qpos, offset, mount, dtype=torch.float64):
    """D [B,L,J,4,4] = inv(F_m) (u_l - u_m) [xi_j]^ F_l, from the base-frame frames and joint frames."""
    ft = _NP[dtype]
    frames, _, jf = fk_mounted(table, qpos, offset, mount, dtype)
    ul, um = masks(table, mount)
    kinds = JR.joint_kinds(table)
    B, J, L = frames.shape[0], jf.shape[1], len(table["use"])
    D = np.zeros((B, L, J, 4, 4), dtype=ft)
    for b in range(B):
        inv = np.linalg.inv(frames[b, int(mount)])
        for l in range(L):
            Fl = frames[b, int(table["use"][l])]
            for j in range(J):
                s = ((int(ul[l]) >> j) & 1) - ((int(um) >> j) & 1)
                if s and kinds[j]:
                    D[b, l, j] = ft(s) * (inv @ _twist_times_frame(kinds[j], jf[b, j, :3], jf[b, j, 3:], Fl, ft))
    return D


def difference_derivatives(table, qpos, offset, mount, h=1e-6):
    """D [B,L,J,4,4] by central differences of inv(F_m) F_l in float64."""
    off = np.zeros(np.atleast_2d(qpos).shape[1]) if offset is None else np.asarray(offset, np.float64)
    J = off.shape[0]
    out = []
    for j in range(J):
        e = np.zeros(J)
        e[j] = h
        out.append((fk_mounted(table, qpos, off + e, mount)[1] - fk_mounted(table, qpos, off - e, mount)[1]) / (2 * h))
    return np.stack(out, axis=2)


def pose_derivatives(table, link_poses, joint_frames, dtype=torch.float64, absolute=False):
    """``joint_reference.pose_derivatives`` for a MOUNTED table and the mounted kernel's outputs (mount-frame link_poses,
    sign-folded joint_frames): the fold undone, the factor u_l - u_m applied.  ``absolute``: the scale of the contraction."""
    ft = _NP[dtype]
    lp = np.asarray(link_poses).astype(ft)
    jf = np.asarray(joint_frames).astype(ft)
    B, L = lp.shape[:2]
    J = jf.shape[1]
    kinds = JR.joint_kinds(table)
    ul, um = np.asarray(table["upstream_base"]), int(table["mount_upstream"])
    D = np.zeros((B, L, J, 4, 4), dtype=ft)
    for l in range(L):
        for j in range(J):
            um_j = (um >> j) & 1
            s = ((int(ul[l]) >> j) & 1) - um_j
            if not s or not kinds[j]:
                continue
            for b in range(B):
                a = jf[b, j, :3] * ft(-1 if um_j else 1)       # R_m^T a_j: the fold undone
                d = _twist_times_frame(kinds[j], a, jf[b, j, 3:], lp[b, l], ft, absolute)
                D[b, l, j] = d if absolute else ft(s) * d
    return D


def offset_gradient(table, grad_mvp, Tc, K, H, W, near, far, link_poses, joint_frames, dtype=torch.float64):
    """``joint_reference.offset_gradient`` for a mounted table: (sum [J], scale [J]) with Tc = X = T_cam<-mount."""
    ft = _NP[dtype]
    PF = R._proj_flip(K, H, W, near, far, dtype).numpy()
    A = PF @ np.asarray(Tc).astype(ft).reshape(4, 4)
    Aabs = np.abs(PF) @ np.abs(np.asarray(Tc).astype(ft).reshape(4, 4))
    g = np.asarray(grad_mvp).astype(ft)
    G = np.swapaxes(A, 0, 1)[None, None] @ g
    Gabs = np.swapaxes(Aabs, 0, 1)[None, None] @ np.abs(g)
    D = pose_derivatives(table, link_poses, joint_frames, dtype)
    Dabs = pose_derivatives(table, link_poses, joint_frames, dtype, absolute=True)
    return (G[:, :, None] * D).sum(axis=(0, 1, 3, 4)), (Gabs[:, :, None] * Dabs).sum(axis=(0, 1, 3, 4))


def gauge_joint(table, mount):
    """The active joint nearest ``mount`` on its way to the root (the one that moves the mount link itself), or None."""
    i = int(mount)
    while i >= 0:
        if table["qidx"][i] >= 0:
            return int(table["qidx"][i])
        i = int(table["parent"][i])
    return None


def mounts(name_or_table):
    """The mounts the tests walk: node 1, N/2 and N-1."""
    N = int(name_or_table["parent"].shape[0])
    return sorted({1, N // 2, N - 1})
