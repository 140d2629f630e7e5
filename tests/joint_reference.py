"""Float64 reference of the joint-offset kernels (csrc/ehr_joint.hip): forward kinematics from the flat table of
``UrdfChain.joint_table`` ALONE, the joint frames, the derivative D of a rendered link's pose with respect to an upstream
joint's zero offset, and the offset gradient from a given ``grad_mvp``.  CPU only, numpy; the projection is
tests/pose_reference.py's.

Every function takes ``dtype=`` like tests/pose_reference.py: the same text run in float32 gives ``e32``, the error a float32
evaluation of these formulas has against float64.  Inputs are float32 / float64 VALUES, converted to the working dtype.

    T_child = T_parent @ origin @ motion(q_j + offset_j)              (articulation order)
    revolute :  D = [ [a]x R_l | a x (t_l - p) ; 0 0 ]                a: world axis, p: world point on the axis
    prismatic:  D = [ 0        | a             ; 0 0 ]
    d(sum loss)/d offset_j = sum_{b,l: bit j of upstream[l]} < (PF @ Tc)^T @ grad_mvp[b,l], D_blj >"""
import numpy as np
import torch

import pose_reference as R

_NP = R._NP


def _hat(a, ft):
    z = ft(0)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], dtype=ft)


def motion(kind, axis, q, ft):
    """4x4 motion of a joint of ``kind`` (0 fixed, 1 revolute, 2 prismatic) about / along the unit ``axis`` by q."""
    M = np.eye(4, dtype=ft)
    if kind == 1:
        Kx = _hat(axis, ft)
        M[:3, :3] = np.eye(3, dtype=ft) + np.sin(q) * Kx + (ft(1) - np.cos(q)) * (Kx @ Kx)
    elif kind == 2:
        M[:3, 3] = axis * q
    return M


def fk(table, qpos, offset=None, dtype=torch.float64):
    """(frames [B,N,4,4], link_poses [B,L,4,4], joint_frames [B,J,6]) in ``dtype``.  qpos [B,J] (float64 values), offset [J]
    or None.  joint_frames[b,j] = (a, p): world axis of active joint j and a world point on it (the moved link's origin)."""
    ft = _NP[dtype]
    q = np.atleast_2d(np.asarray(qpos)).astype(ft)
    B, J = q.shape
    if offset is not None:
        q = q + np.asarray(offset).astype(ft)[None]
    N = table["parent"].shape[0]
    origin = table["origin"].astype(ft).reshape(N, 4, 4)
    axis = table["axis"].astype(ft)
    frames = np.zeros((B, N, 4, 4), dtype=ft)
    jf = np.zeros((B, J, 6), dtype=ft)
    for b in range(B):
        for i in range(N):
            p, k, c = int(table["parent"][i]), int(table["kind"][i]), int(table["qidx"][i])
            Tp = np.eye(4, dtype=ft) if p < 0 else frames[b, p]
            frames[b, i] = Tp @ origin[i] @ motion(k if c >= 0 else 0, axis[i], q[b, c] if c >= 0 else ft(0), ft)
            if c >= 0:
                jf[b, c, :3] = frames[b, i, :3, :3] @ axis[i]
                jf[b, c, 3:] = frames[b, i, :3, 3]
    return frames, frames[:, table["use"]], jf


def joint_kinds(table):
    """kind of every active joint, [J] int32 (the kind of the link it moves)."""
    J = int(table["qidx"].max()) + 1
    out = np.zeros(J, dtype=np.int32)
    for i, c in enumerate(table["qidx"]):
        if c >= 0:
            out[c] = table["kind"][i]
    return out


def pose_derivatives(table, link_poses, joint_frames, dtype=torch.float64, absolute=False):
    """D [B,L,J,4,4]: d link_poses[b,l] / d offset_j by the formula above (zero where joint j is not upstream of link l).
    ``absolute``: every product replaced by its absolute value (and t - p by |t| + |p|): the scale of the contraction."""
    ft = _NP[dtype]
    lp = np.asarray(link_poses).astype(ft)
    jf = np.asarray(joint_frames).astype(ft)
    B, L = lp.shape[:2]
    J = jf.shape[1]
    kinds = joint_kinds(table)
    D = np.zeros((B, L, J, 4, 4), dtype=ft)
    for l in range(L):
        for j in range(J):
            if not (int(table["upstream"][l]) >> j) & 1:
                continue
            for b in range(B):
                a, p = jf[b, j, :3], jf[b, j, 3:]
                Rl, tl = lp[b, l, :3, :3], lp[b, l, :3, 3]
                if kinds[j] == 1:
                    if absolute:
                        ax = np.abs(_hat(a, ft))
                        D[b, l, j, :3, :3] = ax @ np.abs(Rl)
                        D[b, l, j, :3, 3] = ax @ (np.abs(tl) + np.abs(p))
                    else:
                        D[b, l, j, :3, :3] = _hat(a, ft) @ Rl
                        D[b, l, j, :3, 3] = np.cross(a, tl - p)
                elif kinds[j] == 2:
                    D[b, l, j, :3, 3] = np.abs(a) if absolute else a
    return D


def offset_gradient(table, grad_mvp, Tc, K, H, W, near, far, link_poses, joint_frames, dtype=torch.float64):
    """(sum [J], scale [J]): d(sum_b loss_b)/d offset_j from grad_mvp [B,L,4,4] and Tc [4,4] (float32 values, e.g. the device's
    own tc_jac[0]), and the sum of the absolute values of every product entering each sum."""
    ft = _NP[dtype]
    PF = R._proj_flip(K, H, W, near, far, dtype).numpy()
    A = PF @ np.asarray(Tc).astype(ft).reshape(4, 4)
    Aabs = np.abs(PF) @ np.abs(np.asarray(Tc).astype(ft).reshape(4, 4))
    g = np.asarray(grad_mvp).astype(ft)
    G = np.swapaxes(A, 0, 1)[None, None] @ g
    Gabs = np.swapaxes(Aabs, 0, 1)[None, None] @ np.abs(g)
    D = pose_derivatives(table, link_poses, joint_frames, dtype)
    Dabs = pose_derivatives(table, link_poses, joint_frames, dtype, absolute=True)
    s = (G[:, :, None] * D).sum(axis=(0, 1, 3, 4))
    scale = (Gabs[:, :, None] * Dabs).sum(axis=(0, 1, 3, 4))
    return s, scale


def adam_step(p, m, v, t, gsum, red, free, lr, b1, b2, eps, wd, dtype=torch.float64):
    """One step of the offsets' Adam group: tests/pose_reference.py's ``adam_step`` (six elements at a time) on the mean-loss
    gradient gsum / red[7], applied where ``free`` only and frozen as a whole where any of red[0..7] is not finite or
    >= 3e38.  p, m, v, gsum, free: [J]; t: int.  Returns (p, m, v, t, grad) after the step; grad is 0 for a joint that is
    not free, NaN for a free joint of a frozen step."""
    ft = _NP[dtype]
    c = lambda x: np.asarray(x).astype(ft)
    p, m, v, gsum, red = c(p), c(m), c(v), c(gsum), c(red)
    free = np.asarray(free).astype(bool)
    J = p.shape[0]
    with np.errstate(all="ignore"):
        ok = bool((np.isfinite(red) & (np.abs(red) < ft(np.float32(3.0e38)))).all())
    if not ok:
        return p, m, v, int(t), np.where(free, ft(np.nan), ft(0))
    n = -(-J // 6) * 6
    pad = lambda x: np.concatenate([x, np.zeros(n - J, dtype=ft)]).reshape(-1, 6)
    red6 = np.zeros((n // 6, 8), dtype=ft)
    red6[:, :6] = pad(gsum)
    red6[:, 6:] = red[6:8]
    p1, m1, v1, _, _, g0 = R.adam_step(pad(p), pad(m), pad(v), int(t), red6, lr, b1, b2, eps, wd, dtype=dtype)
    p1, m1, v1, g0 = (x.reshape(-1)[:J] for x in (p1, m1, v1, g0))
    return (np.where(free, p1, p).astype(ft), np.where(free, m1, m).astype(ft), np.where(free, v1, v).astype(ft),
            int(t) + 1, np.where(free, g0, ft(0)).astype(ft))
