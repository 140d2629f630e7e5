"""Float64 reference of the camera rig's finish stage (csrc/ehr_joint.hip: rig_backward_adam_kernel), built on
tests/joint_reference.py: C cameras watch one arm and share its joint offsets.  CPU only, numpy.

    objective    mean over ALL views of all cameras of the per-view loss
    gradient     g_j = sum_c offset_gradient_c[j] / sum_c B_c         (offset_gradient_c: JR.offset_gradient of camera c)
    Adam         all or nothing: if every red_c[0..7] of every camera is finite and < 3e38, every camera's pose group takes
                 R.adam_step on its own red_c and the offsets' group JR.adam_step on (sum_c S_c, n = sum_c red_c[7]);
                 otherwise nothing moves, every loss is NaN and the free joints' gradient is NaN.

A camera is a dict: g [B,L,4,4] (d loss_b / d mvp), Tc [4,4], K, H, W, near, far, lp [B,L,4,4], jf [B,J,6].  Every function
takes ``dtype=`` like the references it is built on: the same text run in float32 gives ``e32``."""
import numpy as np
import torch

import joint_reference as JR
import pose_reference as R

_NP = R._NP


def camera_sums(table, cams, dtype=torch.float64):
    """[(S_c [J], scale_c [J])]: JR.offset_gradient of every camera alone."""
    return [JR.offset_gradient(table, c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"], c["lp"], c["jf"], dtype=dtype)
            for c in cams]


def rig_sum(table, cams, dtype=torch.float64):
    """(T [J], scale [J]): the sum over the cameras, in camera order, and the sum of the absolute values of every product."""
    ft = _NP[dtype]
    per = camera_sums(table, cams, dtype)
    T, scale = per[0][0].astype(ft), per[0][1].astype(ft)
    for s, sc in per[1:]:
        T, scale = T + s.astype(ft), scale + sc.astype(ft)
    return T, scale


def rig_gradient(table, cams, dtype=torch.float64):
    """(g [J], scale [J]): the gradient of the mean per-view loss over all views of all cameras, sum_c S_c / sum_c B_c."""
    ft = _NP[dtype]
    T, scale = rig_sum(table, cams, dtype)
    n = ft(sum(np.asarray(c["g"]).shape[0] for c in cams))
    return T / n, scale / n


def rig_adam_step(poses, reds, offsets, gsum, free, pose_hyper, offset_hyper, dtype=torch.float64):
    """One all-or-nothing step.  poses: [(p, m, v, t)] per camera ([6] each); reds: [red_c [8]]; offsets: (p, m, v, t) [J];
    gsum [J]: the rig sum; free [J]; the hyper-parameters are (lr, b1, b2, eps, wd) of the pose groups and of the offsets'.
    Returns (poses after: [(p, m, v, t, loss, grad)], offsets after: (p, m, v, t, grad), ok)."""
    ft = _NP[dtype]
    reds = [np.asarray(r).astype(ft) for r in reds]
    free = np.asarray(free).astype(bool)
    with np.errstate(all="ignore"):
        ok = all(bool((np.isfinite(r) & (np.abs(r) < ft(np.float32(3.0e38)))).all()) for r in reds)
    if not ok:
        nan6 = np.full(6, np.nan, dtype=ft)
        out = [(np.asarray(p).astype(ft), np.asarray(m).astype(ft), np.asarray(v).astype(ft), int(t), ft(np.nan), nan6)
               for p, m, v, t in poses]
        p, m, v, t = offsets
        return out, (np.asarray(p).astype(ft), np.asarray(m).astype(ft), np.asarray(v).astype(ft), int(t),
                     np.where(free, ft(np.nan), ft(0))), False
    out = []
    for (p, m, v, t), r in zip(poses, reds):
        p1, m1, v1, t1, loss, grad = R.adam_step(p, m, v, int(t), r, *pose_hyper, dtype=dtype)
        out.append((p1, m1, v1, int(t1), loss, grad))
    n = reds[0][7]
    for r in reds[1:]:
        n = n + r[7]
    red = np.zeros(8, dtype=ft)
    red[7] = n
    return out, JR.adam_step(*offsets, gsum, red, free, *offset_hyper, dtype=dtype), True
