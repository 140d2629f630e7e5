"""Float64 reference of the pose head (csrc/ehr_pose_core.h: se3 exponential with partials, pose backward, Adam) and the
inputs its tests sweep.  CPU only, no device code restated: the exponential is easyhec_amd/se3.py run in the requested
dtype under torch.autograd, the projection is the formula of tests/test_host_math.py::test_K_to_projection_matches_formula,
Adam is torch.optim.Adam's update written out.

Every function takes ``dtype=``: the SAME text run in float32 gives the error a float32 evaluation of these formulas has
against float64 (``e32``), which is what the kernels' tolerance is made of (tests/test_gpu_pose_head.py):

    max |Xhip - X64| / s  <=  4 * e32 + 8 * 2^-23        per group of cases

Inputs are float32 VALUES (numpy float32 arrays, or Python floats already rounded with ``f32``): they are converted to the
working dtype exactly, never rounded again."""
import functools
import math

import numpy as np
import torch

from easyhec_amd.se3 import se3_exp_map

U = 2.0 ** -23
_NP = {torch.float64: np.float64, torch.float32: np.float32}


def f32(x):
    """Round a Python float to float32 once (what a ctypes c_float argument does) and return it as a Python float."""
    return float(np.float32(x))


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


# ---- se3 exponential and its Jacobian --------------------------------------------------------------------------------
def _exp(d):
    return se3_exp_map(d[None])[0].transpose(0, 1)  # se3.py stores the transform transposed


def exp_and_jac(dof, dtype=torch.float64):
    """Tc [4,4] and dTc/ddof [6,4,4] (numpy, ``dtype``) from dof given as float32 values; includes the squared-angle
    clamp at 1e-4 and its gradient cut (torch.clamp passes the gradient only where the input is >= the bound)."""
    d = _t(dof, dtype)
    Tc = _exp(d)
    J = torch.autograd.functional.jacobian(_exp, d)  # [4,4,6]
    return Tc.numpy(), J.permute(2, 0, 1).contiguous().numpy()


# ---- projection and MVP ----------------------------------------------------------------------------------------------
def _proj_flip(K, H, W, near, far, dtype):
    """proj @ diag(1,-1,-1,1); camera point (x,y,z) -> NDC x = 2(fu x/z + cu)/W - 1, y = 1 - 2(fv y/z + cv)/H."""
    K = _t(K, dtype)
    n, f = _t(near, dtype), _t(far, dtype)
    P = torch.zeros((4, 4), dtype=dtype)
    P[0, 0] = 2 * K[0, 0] / W
    P[0, 2] = -2 * K[0, 2] / W + 1
    P[1, 1] = 2 * K[1, 1] / H
    P[1, 2] = 2 * K[1, 2] / H - 1
    P[2, 2] = -(f + n) / (f - n)
    P[2, 3] = -2 * f * n / (f - n)
    P[3, 2] = -1
    return P @ torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=dtype))


def mvp(Tc, K, H, W, near, far, link_poses, dtype=torch.float64):
    """[..., 4, 4] = proj @ diag(1,-1,-1,1) @ Tc @ link_pose.  Tc is taken in ``dtype`` as given (the reference's own
    exponential in the same dtype); K, near, far and link_poses are float32 values."""
    PF = _proj_flip(K, H, W, near, far, dtype)
    Tc = torch.as_tensor(np.asarray(Tc)).to(dtype)
    return (PF @ (Tc @ _t(link_poses, dtype))).numpy()


# ---- pose backward ---------------------------------------------------------------------------------------------------
def backward(grad_mvp, loss_b, K, H, W, near, far, link_poses, jac, dtype=torch.float64):
    """red[8] = (sum_{b,l} <jac_i, PF^T G_bl lp_bl^T> for i < 6, sum_b loss_b, B) and scale[7]: the sum of the absolute
    values of every product that enters each of the six contractions, and of the loss sum.  jac: [6,4,4] (float32 values,
    e.g. the device's own tc_jac[1:7]); grad_mvp, link_poses: [B,L,4,4]; loss_b: [B]."""
    PF = _proj_flip(K, H, W, near, far, dtype)
    G = _t(grad_mvp, dtype).reshape(-1, 4, 4)
    lp = _t(link_poses, dtype).reshape(-1, 4, 4)
    J = _t(jac, dtype).reshape(6, 4, 4)
    lb = _t(loss_b, dtype)
    B = int(lb.shape[0])
    # MVP_p = PF @ Tc @ lp_p  =>  d<G_p, MVP_p>/dTc = PF^T @ G_p @ lp_p^T
    D = (PF.transpose(0, 1)[None] @ G @ lp.transpose(1, 2)).sum(0)
    Dabs = (PF.abs().transpose(0, 1)[None] @ G.abs() @ lp.abs().transpose(1, 2)).sum(0)
    red = torch.zeros(8, dtype=dtype)
    red[:6] = (J * D[None]).sum(dim=(1, 2))
    red[6] = lb.sum()
    red[7] = B
    scale = torch.zeros(7, dtype=dtype)
    scale[:6] = (J.abs() * Dabs[None]).sum(dim=(1, 2))
    scale[6] = lb.abs().sum()
    return red.numpy(), scale.numpy()


# ---- Adam ------------------------------------------------------------------------------------------------------------
def adam_step(p, m, v, t, red, lr, b1, b2, eps, wd, dtype=torch.float64):
    """One step of torch.optim.Adam with L2 weight decay on g = red[:6] / red[7], in ``dtype`` (numpy arithmetic).
    p, m, v: [..., 6]; red: [..., 8]; t: steps taken so far (int, or an int array [...]); the hyper-parameters are scalars
    or arrays that broadcast against [..., 1].  Returns (p, m, v, t, loss, grad) after the step.

    A reported failure must not destroy the calibration: where any of the eight ``red`` values is non-finite or
    |x| >= 3e38, p, m, v and t are returned unchanged and loss and grad are NaN."""
    ft = _NP[dtype]
    c = lambda x: np.asarray(x).astype(ft)  # exact for float32 values (and for float64 state when dtype is float64)
    p, m, v, red = c(p), c(m), c(v), c(red)
    lr, b1, b2, eps, wd = c(lr), c(b1), c(b2), c(eps), c(wd)
    t = np.asarray(t, dtype=np.int64)
    one = ft(1)
    with np.errstate(all="ignore"):
        ok = (np.isfinite(red) & (np.abs(red) < ft(np.float32(3.0e38)))).all(axis=-1)
        t1 = t + 1
        tf = t1.astype(ft)[..., None] if t1.ndim else ft(t1)
        g0 = red[..., :6] / red[..., 7:8]
        loss = red[..., 6] / red[..., 7]
        g = g0 + wd * p
        m1 = b1 * m + (one - b1) * g
        v1 = b2 * v + (one - b2) * g * g
        bc1 = one - np.power(b1, tf)
        bc2 = one - np.power(b2, tf)
        step_size = lr / bc1
        denom = np.sqrt(v1) / np.sqrt(bc2) + eps
        p1 = p - step_size * (m1 / denom)
    okv = ok[..., None]
    nan = ft(np.nan)
    return (np.where(okv, p1, p).astype(ft), np.where(okv, m1, m).astype(ft), np.where(okv, v1, v).astype(ft),
            np.where(ok, t1, t), np.where(ok, loss, nan).astype(ft), np.where(okv, g0, nan).astype(ft))


# ---- the error rule --------------------------------------------------------------------------------------------------
def rel_err(x, x64, s):
    """max |x - x64| / s (s a scalar or an array broadcast against x64); 0 where the two agree exactly (so a zero scale
    demands equality and gives inf otherwise)."""
    d = np.abs(np.asarray(x, dtype=np.float64) - np.asarray(x64, dtype=np.float64))
    s = np.broadcast_to(np.asarray(s, dtype=np.float64), d.shape)
    with np.errstate(all="ignore"):
        r = np.where(d == 0, 0.0, d / s)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def bound(e32):
    return 4.0 * e32 + 8.0 * U


# ---- swept inputs (shared by the CPU checks of the input conditions and the GPU tests) ------------------------------------
ANGLES = [0.0, 1e-6, 1e-3, 0.0099, 0.0101, 0.02, 0.05, 0.1, 0.5, 1.0, 2.0, 3.0, float(np.float32(math.pi)), 3.2, 5.0,
          6.28, 7.5]
XARM7_K = np.array([[906.8, 0, 650.2], [0, 906.7, 367.7], [0, 0, 1.0]], dtype=np.float32)  # config.XARM7_K_1280x720
SMALL_K = np.array([[143.5, 0, 31.25], [0, 118.75, 88.5], [0, 0, 1.0]], dtype=np.float32)   # non-square, off-centre
CAMERAS = [(XARM7_K, 720, 1280), (SMALL_K, 131, 97)]  # (K, H, W)
NEAR_FAR = [(f32(0.001), f32(10.0)), (f32(0.05), f32(100.0))]
PAIR_COUNTS = [1, 8, 255, 256, 257, 600]
MVP_COMBOS = [(ci, ni, bl) for ci in range(2) for ni in range(2) for bl in PAIR_COUNTS]  # 24


def random_rigid(rng, n):
    """n random rigid transforms [n,4,4] float32: rotation from a random rotation vector, translation within 1 m."""
    from scipy.spatial.transform import Rotation
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = Rotation.from_rotvec(rng.normal(size=(n, 3)) * 1.2).as_matrix()
    T[:, :3, 3] = rng.uniform(-1.0, 1.0, size=(n, 3))
    return T.astype(np.float32)


def _V64(w):
    th = np.sqrt(max(float(w @ w), 1e-4))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + K * ((1 - np.cos(th)) / th ** 2) + (K @ K) * ((th - np.sin(th)) / th ** 3)


@functools.lru_cache(maxsize=None)
def forward_cases():
    """{angle index: [dof float32 [6], ...]}: per angle 20 draws of a random unit axis and a translation uniform in +-1.5 m,
    the three coordinate axes, and one draw with a zero translation -- 24 poses, one per MVP_COMBOS entry.  Draw 0 of every
    angle has translation z in [1.0, 1.5] and the camera at least 1.3 m from the base origin (|V u| >= 1.3 in float64): the
    pose the fused head is run at."""
    rng = np.random.default_rng(20240917)
    out = {}
    for ai, ang in enumerate(ANGLES):
        cases = []
        for k in range(20):
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            w = (ax * ang).astype(np.float32)
            u = rng.uniform(-1.5, 1.5, size=3)
            if k == 0:
                for _ in range(10000):
                    u = rng.uniform(-1.5, 1.5, size=3)
                    u[2] = rng.uniform(1.0, 1.5)
                    if np.linalg.norm(_V64(w.astype(np.float64)) @ u.astype(np.float32).astype(np.float64)) >= 1.3:
                        break
                else:
                    raise AssertionError("no translation found")
            cases.append(np.concatenate([u.astype(np.float32), w]))
        for a in range(3):
            w = np.zeros(3, np.float32)
            w[a] = np.float32(ang) * (-1 if a == 1 else 1)
            cases.append(np.concatenate([rng.uniform(-1.5, 1.5, size=3).astype(np.float32), w]))
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        cases.append(np.concatenate([np.zeros(3, np.float32), (ax * ang).astype(np.float32)]))
        out[ai] = cases
    return out


def clamp_margin(dof):
    """Smallest relative distance of the squared angle from the clamp bound 1e-4, over a float32 and a float64 evaluation."""
    w32 = np.asarray(dof, dtype=np.float32)[3:]
    n32 = float(np.float32(np.float32(w32[0] * w32[0]) + np.float32(w32[1] * w32[1])) + np.float32(w32[2] * w32[2]))
    w64 = w32.astype(np.float64)
    n64 = float(w64 @ w64)
    return min(abs(n32 - 1e-4), abs(n64 - 1e-4)) / 1e-4


def mvp_inputs(ai, k):
    """(K, H, W, near, far, link_poses [BL,4,4]) of pose k of angle ai: MVP_COMBOS[k], seeded per (ai, k)."""
    ci, ni, bl = MVP_COMBOS[k % len(MVP_COMBOS)]
    K, H, W = CAMERAS[ci]
    near, far = NEAR_FAR[ni]
    rng = np.random.default_rng(1000 * ai + k + 7)
    return K, H, W, near, far, random_rigid(rng, bl)


BACKWARD_SHAPES = [(1, 1), (1, 3), (3, 1), (7, 9), (8, 8), (21, 3), (13, 5), (64, 8), (300, 2), (1000, 1), (16, 32)]
BACKWARD_VARIANTS = [("plain", "uniform"), ("cancel", "uniform"), ("plain", "zero"), ("cancel", "zero")]
BACKWARD_DRAWS = 2


def backward_case(si, vi, draw):
    """Inputs of one pose backward case: dict(B, L, K, H, W, near, far, link_poses [B,L,4,4], grad_mvp [B,L,4,4],
    loss_b [B], dof [6]).  grad_mvp: standard normal times a per-pair scale 10^U(-3,3); "cancel": every odd pair repeats
    the link pose of the pair before it and carries that pair's gradient negated, times (1 + 1e-3 N(0,1))."""
    B, L = BACKWARD_SHAPES[si]
    gkind, lkind = BACKWARD_VARIANTS[vi]
    rng = np.random.default_rng(90000 + 100 * si + 10 * vi + draw)
    K, H, W = CAMERAS[(si + draw) % 2]
    near, far = NEAR_FAR[(si + vi) % 2]
    lp = random_rigid(rng, B * L)
    G = rng.normal(size=(B * L, 4, 4)) * (10.0 ** rng.uniform(-3, 3, size=(B * L, 1, 1)))
    if gkind == "cancel":
        n2 = (B * L) // 2
        lp[1:2 * n2:2] = lp[0:2 * n2:2]
        G[1:2 * n2:2] = -G[0:2 * n2:2] * (1.0 + 1e-3 * rng.normal(size=(n2, 4, 4)))
    loss = rng.uniform(0, 1e6, size=B) if lkind == "uniform" else np.zeros(B)
    poses = forward_cases()
    dof = poses[(3 * si + vi) % len(ANGLES)][(5 * si + draw) % 24]
    return dict(B=B, L=L, K=K, H=H, W=W, near=near, far=far, link_poses=lp.reshape(B, L, 4, 4),
                grad_mvp=G.astype(np.float32).reshape(B, L, 4, 4), loss_b=loss.astype(np.float32), dof=dof)


ADAM_T0 = [0, 1, 9, 999, 99999, 999999]
ADAM_HYPER = {  # lr, b1, b2, eps, wd
    "default": (3e-3, 0.9, 0.999, 1e-8, 5e-4),
    "wd0": (3e-3, 0.9, 0.999, 1e-8, 0.0),
    "wd0.1": (3e-3, 0.9, 0.999, 1e-8, 0.1),
    "eps1e-3": (3e-3, 0.9, 0.999, 1e-3, 5e-4),
    "betas.5.9": (3e-3, 0.5, 0.9, 1e-8, 5e-4),
}
ADAM_GRADS = ["noisy1e3", "zero_fresh", "zero_moving", "tiny1e-6", "huge1e15", "mixed"]
ADAM_DRAWS = 3
ADAM_WARM = 1000     # the state of a case with t0 steps behind it is a float64 trajectory of min(t0, ADAM_WARM) steps
ADAM_NFRAMES = 8.0   # red[7]


def hyper32(name):
    return tuple(f32(x) for x in ADAM_HYPER[name])


def adam_gradients(kind, rng, steps):
    """[steps, 6] float64 mean-loss gradients of one sequence.  zero_fresh: zero throughout; zero_moving: noisy O(1e3)
    with the second half of every 100 steps exactly zero (the moments decay for 50 steps before checkpoints 100, 1000 and
    2000 without leaving float32's normal range); a one-step case uses noisy steps followed by one zero gradient."""
    if kind == "noisy1e3":
        return rng.normal(size=(steps, 6)) * 1e3 + rng.normal(size=6) * 300
    if kind == "zero_fresh":
        return np.zeros((steps, 6))
    if kind == "zero_moving":
        g = rng.normal(size=(steps, 6)) * 1e3
        g[(np.arange(steps) % 100) >= 50] = 0.0
        return g
    if kind == "tiny1e-6":
        return rng.normal(size=(steps, 6)) * 1e-6
    if kind == "huge1e15":
        return rng.normal(size=(steps, 6)) * 1e15
    if kind == "mixed":
        sgn = np.array([1, -1, 1, -1, -1, 1.0])
        mag = np.array([1e-4, 1e-2, 1.0, 1e2, 1e4, 1e6])
        return sgn * mag * (1.0 + 0.3 * rng.normal(size=(steps, 6)))
    raise KeyError(kind)


def red_of(g, loss, nframes=ADAM_NFRAMES):
    """[..., 8] float32 ``red`` whose mean gradient is (about) g: sums over nframes frames."""
    g = np.asarray(g, dtype=np.float64)
    red = np.zeros(g.shape[:-1] + (8,))
    red[..., :6] = g * nframes
    red[..., 6] = np.asarray(loss) * nframes
    red[..., 7] = nframes
    with np.errstate(over="ignore"):
        return red.astype(np.float32)


@functools.lru_cache(maxsize=None)
def adam_one_step_cases():
    """List of dict(t0, hyper, grad, p, m, v [N,6] float32, red [N,8] float32): one group per (t0, hyper, gradient kind),
    N = ADAM_DRAWS states.  The state is where a float64 trajectory of min(t0, ADAM_WARM) steps of that gradient kind,
    started at a random pose with zero moments, stands -- rounded to float32 once (zero_fresh keeps m = v = 0 by starting
    from there with wd's contribution only; at t0 = 0 the moments are zero for every kind)."""
    out = []
    for ti, t0 in enumerate(ADAM_T0):
        for hi, hname in enumerate(ADAM_HYPER):
            h = hyper32(hname)
            for gi, kind in enumerate(ADAM_GRADS):
                rng = np.random.default_rng(500000 + 1000 * ti + 10 * hi + gi)
                n = min(t0, ADAM_WARM)
                p = rng.uniform(-1.5, 1.5, size=(ADAM_DRAWS, 6)).astype(np.float32).astype(np.float64)
                m, v = np.zeros_like(p), np.zeros_like(p)
                seq = np.stack([adam_gradients("noisy1e3" if kind == "zero_moving" else kind, rng, n + 1)
                                for _ in range(ADAM_DRAWS)], axis=1)  # [n+1, N, 6]
                if kind == "zero_moving":
                    seq[n] = 0.0
                if kind == "zero_fresh" and t0 > 0:
                    n = 0  # no gradient has ever arrived: the moments are exactly zero whatever the step count
                tt = 0
                for k in range(n):
                    red = red_of(seq[k], 1.0)
                    p, m, v, tt, _, _ = adam_step(p, m, v, tt, red.astype(np.float64), *h)
                out.append(dict(t0=t0, hyper=hname, grad=kind, p=p.astype(np.float32), m=m.astype(np.float32),
                                v=v.astype(np.float32), red=red_of(seq[-1], rng.uniform(0, 1e5, size=ADAM_DRAWS))))
    return out


TRAJ_STEPS = 2000
TRAJ_CHECKPOINTS = [1, 10, 100, 1000, 2000]


@functools.lru_cache(maxsize=None)
def adam_trajectory_cases():
    """dict(p0 [S,6] float32, red [T,S,8] float32, hyper [S] names): one sequence per (hyper, gradient kind)."""
    p0, red, names = [], [], []
    for hi, hname in enumerate(ADAM_HYPER):
        for gi, kind in enumerate(ADAM_GRADS):
            rng = np.random.default_rng(700000 + 10 * hi + gi)
            p0.append(rng.uniform(-1.5, 1.5, size=6).astype(np.float32))
            red.append(red_of(adam_gradients(kind, rng, TRAJ_STEPS), rng.uniform(0, 1e5, size=TRAJ_STEPS)))
            names.append((hname, kind))
    return dict(p0=np.stack(p0), red=np.stack(red, axis=1), names=names)


def adam_trajectory(dtype):
    """The reference trajectory of adam_trajectory_cases() in ``dtype``: {checkpoint: (p, m, v) [S,6]}."""
    tc = adam_trajectory_cases()
    H = np.array([hyper32(h) for h, _ in tc["names"]], dtype=np.float64)  # float32 values
    hy = [H[:, j:j + 1].astype(np.float32) for j in range(5)]
    p, m, v = tc["p0"], np.zeros_like(tc["p0"]), np.zeros_like(tc["p0"])
    if dtype == torch.float64:
        p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    t = np.zeros(p.shape[0], dtype=np.int64)
    out = {}
    for k in range(TRAJ_STEPS):
        r = tc["red"][k]
        p, m, v, t, _, _ = adam_step(p, m, v, t, r, *hy, dtype=dtype)
        if k + 1 in TRAJ_CHECKPOINTS:
            out[k + 1] = (p.copy(), m.copy(), v.copy())
    return out
