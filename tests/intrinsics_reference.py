"""Float64 reference of the intrinsics kernel (csrc/ehr_intrinsics.hip): the K written for a parameter vector, the gradient
with respect to the parameters from a given ``grad_mvp``, and the parameter group's Adam.  CPU only, numpy; the projection
is tests/pose_reference.py's.

Every function takes ``dtype=`` like tests/pose_reference.py: the same text run in float32 gives ``e32``, the error a float32
evaluation of these formulas has against float64.  Inputs are float32 / float64 VALUES, converted to the working dtype.

    fu = K0[0,0] exp(theta0)    fv = K0[1,1] exp(theta1)    cu = K0[0,2] + W theta2    cv = K0[1,2] + H theta3
    MVP_bl = P(K) @ A_bl,  A_bl = F @ Tc @ link_poses[b,l],  F = diag(1,-1,-1,1)
    d(sum <G_bl, MVP_bl>)/d theta = (fu 2/W Q[0,0], fv 2/H Q[1,1], -2 Q[0,2], 2 Q[1,2]),  Q[r,k] = sum_bl sum_c G_bl[r,c] A_bl[k,c]"""
import numpy as np
import torch

import pose_reference as R

_NP = R._NP
ENTRIES = ((0, 0), (1, 1), (0, 2), (1, 2))   # where fu, fv, cu, cv sit in K


def K_of_theta(K0, theta, H, W, dtype=torch.float64):
    """[3,3] in ``dtype``: K for ``theta`` (not rounded to float32).  An entry whose theta is exactly 0 is K0's, selected."""
    ft = _NP[dtype]
    K0 = np.asarray(K0).astype(ft).reshape(3, 3)
    th = np.asarray(theta).astype(ft).reshape(4)
    K = K0.copy()
    new = (K0[0, 0] * np.exp(th[0]), K0[1, 1] * np.exp(th[1]), K0[0, 2] + ft(W) * th[2], K0[1, 2] + ft(H) * th[3])
    for i, (r, c) in enumerate(ENTRIES):
        if th[i] != 0:
            K[r, c] = new[i]
    return K


def theta_gradient(grad_mvp, Tc, link_poses, K0, theta, H, W, dtype=torch.float64):
    """(sum [4], scale [4]): d(sum_b loss_b)/d theta from grad_mvp [..., 4, 4], Tc [4,4] and link_poses [..., 4, 4] (float32
    values), and the sum of the absolute values of every product entering each sum.  fu, fv are the RENDERED ones: K(theta)
    rounded to float32."""
    ft = _NP[dtype]
    g = np.asarray(grad_mvp).astype(ft).reshape(-1, 4, 4)
    lp = np.asarray(link_poses).astype(ft).reshape(-1, 4, 4)
    T = np.asarray(Tc).astype(ft).reshape(4, 4)
    F = np.diag(np.array([1, -1, -1, 1], dtype=ft))
    A = (F @ T)[None] @ lp
    Aabs = np.abs(T)[None] @ np.abs(lp)
    Q = np.einsum("prc,pkc->rk", g, A)
    Qabs = np.einsum("prc,pkc->rk", np.abs(g), Aabs)
    K = K_of_theta(K0, theta, H, W).astype(np.float32).astype(ft)
    fac = np.array([K[0, 0] * (ft(2) / ft(W)), K[1, 1] * (ft(2) / ft(H)), ft(-2), ft(2)], dtype=ft)
    q = np.array([Q[0, 0], Q[1, 1], Q[0, 2], Q[1, 2]], dtype=ft)
    qabs = np.array([Qabs[0, 0], Qabs[1, 1], Qabs[0, 2], Qabs[1, 2]], dtype=ft)
    return fac * q, np.abs(fac) * qabs


def adam_step(p, m, v, t, gsum, red, free, tie, lr, b1, b2, eps, wd, dtype=torch.float64):
    """One step of the intrinsics' Adam group: tests/pose_reference.py's ``adam_step`` on the mean-loss gradient gsum /
    red[7] (with ``tie``: both focal elements take gsum[0] + gsum[1]), applied where ``free`` only and frozen as a whole
    where any of red[0..7] is not finite or >= 3e38.  p, m, v, gsum, free: [4]; t: int.  Returns (p, m, v, t, grad) after the
    step; grad is +0 for an element that is not free, NaN for a free element of a frozen step."""
    ft = _NP[dtype]
    c = lambda x: np.asarray(x).astype(ft)
    p, m, v, gsum, red = c(p), c(m), c(v), c(gsum).copy(), c(red)
    free = np.asarray(free).astype(bool)
    if tie:
        gsum[:2] = gsum[0] + gsum[1]
    with np.errstate(all="ignore"):
        ok = bool((np.isfinite(red) & (np.abs(red) < ft(np.float32(3.0e38)))).all())
    if not ok:
        return p, m, v, int(t), np.where(free, ft(np.nan), ft(0))
    pad = lambda x: np.concatenate([x, np.zeros(2, dtype=ft)])
    red6 = np.zeros(8, dtype=ft)
    red6[:4] = gsum
    red6[6:] = red[6:8]
    p1, m1, v1, _, _, g0 = R.adam_step(pad(p), pad(m), pad(v), int(t), red6, lr, b1, b2, eps, wd, dtype=dtype)
    p1, m1, v1, g0 = (x[:4] for x in (p1, m1, v1, g0))
    return (np.where(free, p1, p).astype(ft), np.where(free, m1, m).astype(ft), np.where(free, v1, v).astype(ft),
            int(t) + 1, np.where(free, g0, ft(0)).astype(ft))
