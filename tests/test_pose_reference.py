"""The float64 reference of the pose head (tests/pose_reference.py) against independent statements of the same
mathematics -- scipy's matrix exponential, central differences, the closed form below the squared-angle clamp,
torch.optim.Adam, torch autograd -- and the conditions the swept inputs of tests/test_gpu_pose_head.py must satisfy."""
import numpy as np
import pytest
import torch

import pose_reference as R


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def _expm_twist(d):
    from scipy.linalg import expm
    X = np.zeros((4, 4))
    X[:3, :3] = _hat(d[3:])
    X[:3, 3] = d[:3]
    return expm(X)


@pytest.mark.parametrize("angle", [0.02, 0.5, 2.0, 3.1, 3.2, 7.5])
def test_exp_and_jac_above_the_clamp_is_the_matrix_exponential_and_its_derivative(angle):
    rng = np.random.default_rng(int(angle * 1000))
    for _ in range(5):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        d = np.concatenate([rng.uniform(-1.5, 1.5, size=3), ax * angle]).astype(np.float32)
        Tc, J = R.exp_and_jac(d)
        assert Tc.dtype == np.float64 and Tc.shape == (4, 4) and J.shape == (6, 4, 4)
        d64 = d.astype(np.float64)
        assert np.abs(Tc - _expm_twist(d64)).max() <= 1e-12
        h = 1e-6
        for i in range(6):
            e = np.zeros(6)
            e[i] = h
            fd = (_expm_twist(d64 + e) - _expm_twist(d64 - e)) / (2 * h)
            assert np.abs(J[i] - fd).max() <= 2e-8, (angle, i)


@pytest.mark.parametrize("angle", [0.0, 1e-6, 1e-3, 0.0099])
def test_exp_and_jac_below_the_clamp_is_the_closed_form_with_the_angle_fixed(angle):
    """Squared angle below 1e-4: th = 0.01 is a constant, so R = I + a hat(w) + b hat(w)^2 and V = I + b hat(w) + c hat(w)^2
    with constant a, b, c, and the rotation partials come from hat(w) and hat(w)^2 alone."""
    th = np.sqrt(1e-4)
    a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    rng = np.random.default_rng(11)
    for _ in range(5):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        d = np.concatenate([rng.uniform(-1.5, 1.5, size=3), ax * angle]).astype(np.float32)
        Tc, J = R.exp_and_jac(d)
        u, w = d[:3].astype(np.float64), d[3:].astype(np.float64)
        K = _hat(w)
        V = np.eye(3) + b * K + c * K @ K
        exp = np.eye(4)
        exp[:3, :3] = np.eye(3) + a * K + b * K @ K
        exp[:3, 3] = V @ u
        assert np.abs(Tc - exp).max() <= 1e-14
        for i in range(3):
            dT = np.zeros((4, 4))
            dT[:3, 3] = V[:, i]
            assert np.abs(J[i] - dT).max() <= 1e-14
            E = _hat(np.eye(3)[i])
            dK2 = E @ K + K @ E
            dT = np.zeros((4, 4))
            dT[:3, :3] = a * E + b * dK2
            dT[:3, 3] = (b * E + c * dK2) @ u
            assert np.abs(J[3 + i] - dT).max() <= 1e-14


def test_exp_and_jac_float32_is_the_same_text_in_float32():
    d = R.forward_cases()[9][3]
    T32, J32 = R.exp_and_jac(d, dtype=torch.float32)
    T64, J64 = R.exp_and_jac(d)
    assert T32.dtype == np.float32 and J32.dtype == np.float32
    assert 0 < np.abs(J32 - J64).max() <= 1e-5


def test_mvp_projects_a_camera_point_to_ndc():
    K, H, W = R.CAMERAS[1]
    n, f = R.NEAR_FAR[1]
    lp = np.eye(4, dtype=np.float32)[None]
    M = R.mvp(np.eye(4), K, H, W, n, f, lp)[0]
    x, y, z = 0.1, -0.2, 1.5
    clip = M @ np.array([x, y, z, 1.0])
    fu, fv, cu, cv = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    assert abs(clip[0] / clip[3] - (2 * (fu * x / z + cu) / W - 1)) <= 1e-14
    assert abs(clip[1] / clip[3] - (1 - 2 * (fv * y / z + cv) / H)) <= 1e-14
    assert abs(clip[2] / clip[3] - ((f + n) / (f - n) - 2 * f * n / ((f - n) * z))) <= 1e-14
    import helpers
    assert np.abs(R._proj_flip(K, H, W, n, f, torch.float64).numpy()
                  - helpers.projection(K.astype(np.float64), H, W, n, f) @ np.diag([1.0, -1, -1, 1])).max() <= 1e-15


def test_adam_step_is_torch_optim_adam_over_200_steps():
    rng = np.random.default_rng(5)
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 5e-4
    p0 = rng.uniform(-1.5, 1.5, size=6)
    pt = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v, t = p0.copy(), np.zeros(6), np.zeros(6), 0
    for k in range(200):
        g = rng.normal(size=6) * (1.0 if k % 7 else 0.0)
        red = np.concatenate([g * 4.0, [2.5 * 4.0, 4.0]])
        pt.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v, t, loss, grad = R.adam_step(p, m, v, t, red, lr, b1, b2, eps, wd)
        st = opt.state[pt]
        assert t == k + 1 == int(st["step"]) and loss == 2.5 and np.array_equal(grad, g)
        assert np.abs(p - pt.detach().numpy()).max() <= 1e-12
        assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12
        assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 3.1e38, -3.0e38])
def test_adam_step_leaves_the_state_alone_on_a_non_finite_red(bad):
    p, m, v = np.arange(6) * 0.1, np.full(6, 0.2), np.full(6, 0.3)
    for slot in range(8):
        red = np.array([1, 2, 3, 4, 5, 6, 7, 8], dtype=np.float32)
        red[slot] = bad
        for dtype in (torch.float64, torch.float32):
            out = R.adam_step(p, m, v, 5, red, 3e-3, 0.9, 0.999, 1e-8, 5e-4, dtype=dtype)
            assert np.array_equal(out[0], p.astype(out[0].dtype)) and np.array_equal(out[1], m.astype(out[1].dtype))
            assert np.array_equal(out[2], v.astype(out[2].dtype)) and int(out[3]) == 5
            assert np.isnan(out[4]) and np.isnan(out[5]).all()
    ok = R.adam_step(p, m, v, 5, np.array([1, 2, 3, 4, 5, 6, 7, 2.9e38], dtype=np.float32), 3e-3, 0.9, 0.999, 1e-8, 5e-4)
    assert int(ok[3]) == 6 and np.isfinite(ok[0]).all()


def test_backward_is_autograd_through_the_exponential():
    for si in (3, 6, 8):
        for vi in (0, 1):
            c = R.backward_case(si, vi, 0)
            d = torch.tensor(c["dof"].astype(np.float64), requires_grad=True)
            PF = R._proj_flip(c["K"], c["H"], c["W"], c["near"], c["far"], torch.float64)
            G = torch.tensor(c["grad_mvp"].astype(np.float64))
            M = PF @ (R._exp(d) @ torch.tensor(c["link_poses"].astype(np.float64)))
            (M * G).sum().backward()
            _, J = R.exp_and_jac(c["dof"])
            red, scale = R.backward(c["grad_mvp"], c["loss_b"], c["K"], c["H"], c["W"], c["near"], c["far"],
                                    c["link_poses"], J)
            assert np.abs(red[:6] - d.grad.numpy()).max() <= 1e-13 * scale[:6].max()
            assert (scale[:6] >= np.abs(red[:6])).all()
            assert red[7] == c["B"] and abs(red[6] - c["loss_b"].astype(np.float64).sum()) <= 1e-9 * scale[6]
            assert np.abs(M.detach().numpy() - R.mvp(R.exp_and_jac(c["dof"])[0], c["K"], c["H"], c["W"], c["near"],
                                                     c["far"], c["link_poses"])).max() <= 1e-12 * float(M.detach().abs().max())
            if vi == 1 and c["B"] * c["L"] >= 60:
                assert np.abs(red[:6]).max() <= 0.05 * scale[:6].max()   # the "cancel" variant cancels


# ---- conditions on the swept inputs ---------------------------------------------------------------------------------------
def test_swept_poses_keep_clear_of_the_clamp_tie_and_stay_in_range():
    cases = R.forward_cases()
    assert len(cases) == len(R.ANGLES) == 17
    for ai, ang in enumerate(R.ANGLES):
        assert len(cases[ai]) == 24 == len(R.MVP_COMBOS)
        for k, d in enumerate(cases[ai]):
            assert d.dtype == np.float32 and d.shape == (6,) and np.isfinite(d).all()
            # the squared angle is at least 1 % away from 1e-4 in float32 and in float64: rounding cannot move the decision
            assert R.clamp_margin(d) >= 0.01, (ang, k)
            assert (np.abs(d[:3]) <= 1.5).all()
            assert abs(float(np.linalg.norm(d[3:].astype(np.float64))) - ang) <= 1e-6 * max(ang, 1e-6)
        assert not cases[ai][23][:3].any()                       # the zero translation
        for a in range(3):                                       # the coordinate axes
            w = cases[ai][20 + a][3:]
            assert np.count_nonzero(w) == (1 if ang else 0) and abs(w[a]) == np.float32(ang)
        d0 = cases[ai][0].astype(np.float64)                     # the fused head's pose: in front of the robot, 1.3 m away
        assert 1.0 <= d0[2] <= 1.5
        assert np.linalg.norm(R.exp_and_jac(cases[ai][0])[0][:3, 3]) >= 1.3 - 1e-6
    assert R.ANGLES[0] == 0.0 and R.ANGLES[12] == float(np.float32(np.pi))
    below = [a for a in R.ANGLES if a * a < 1e-4]
    assert below == [0.0, 1e-6, 1e-3, 0.0099]
    assert sorted({bl for _, _, bl in R.MVP_COMBOS}) == [1, 8, 255, 256, 257, 600]


def test_swept_backward_and_adam_inputs_are_valid():
    assert [b * l for b, l in R.BACKWARD_SHAPES] == [1, 3, 3, 63, 64, 63, 65, 512, 600, 1000, 512]
    for si in range(len(R.BACKWARD_SHAPES)):
        for vi in range(len(R.BACKWARD_VARIANTS)):
            c = R.backward_case(si, vi, 0)
            B, L = R.BACKWARD_SHAPES[si]
            assert c["grad_mvp"].shape == c["link_poses"].shape == (B, L, 4, 4) and c["loss_b"].shape == (B,)
            assert np.isfinite(c["grad_mvp"]).all() and np.abs(c["grad_mvp"]).max() < 1e5
            assert (c["loss_b"] >= 0).all() and (c["loss_b"] <= 1e6).all()
            assert (c["loss_b"] == 0).all() == (R.BACKWARD_VARIANTS[vi][1] == "zero")
            lp = c["link_poses"].astype(np.float64).reshape(-1, 4, 4)
            assert np.abs(lp[:, :3, :3] @ lp[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
            assert (lp[:, 3] == [0, 0, 0, 1]).all()
    cases = R.adam_one_step_cases()
    assert len(cases) == len(R.ADAM_T0) * len(R.ADAM_HYPER) * len(R.ADAM_GRADS)
    for c in cases:
        for name in ("p", "m", "v", "red"):
            assert c[name].dtype == np.float32 and np.isfinite(c[name]).all() and (np.abs(c[name]) < 3e38).all()
        assert (c["v"] >= 0).all() and (c["red"][:, 7] == R.ADAM_NFRAMES).all()
        if c["grad"] in ("zero_fresh", "zero_moving"):
            assert not c["red"][:, :6].any()
        if c["grad"] == "zero_fresh" or c["t0"] == 0:
            assert not c["m"].any() and not c["v"].any()
        if c["grad"] == "zero_moving" and c["t0"] > 0:
            assert c["m"].all() and c["v"].all()
    tc = R.adam_trajectory_cases()
    assert tc["red"].shape == (R.TRAJ_STEPS, 30, 8) and np.isfinite(tc["red"]).all() and (np.abs(tc["red"]) < 3e38).all()


def test_bound_and_rel_err():
    assert R.bound(0.0) == 8 * 2.0 ** -23 and R.bound(1e-4) == 4e-4 + 8 * 2.0 ** -23
    assert R.rel_err([1.0, 2.0], [1.0, 2.5], 5.0) == 0.1
    assert R.rel_err([0.0], [0.0], 0.0) == 0.0 and R.rel_err([1e-30], [0.0], 0.0) == np.inf
    assert R.rel_err([np.nan], [0.0], 1.0) == np.inf
