"""The float64 reference of the intrinsics kernel (tests/intrinsics_reference.py) pinned against tests/pose_reference.py: the
gradient is the central difference of the objective through ``_proj_flip``, K at theta = 0 is K0 bit for bit, the package's
host helper is the same function, and the Adam group is the pose head's Adam."""
import numpy as np
import pytest
import torch

import intrinsics_reference as IR
import pose_reference as R


def _case(ci, seed, n=7):
    rng = np.random.default_rng(seed)
    K0, H, W = R.CAMERAS[ci]
    g = rng.normal(size=(n, 4, 4))
    Tc = R.random_rigid(rng, 1)[0].astype(np.float64)
    lp = R.random_rigid(rng, n).astype(np.float64)
    theta = np.array([0.013, -0.021, 0.008, -0.011]) * (1 + ci)
    return K0, H, W, g, Tc, lp, theta


def _phi(K0, H, W, g, Tc, lp, theta, near, far):
    K = IR.K_of_theta(K0, theta, H, W)
    return float((g * R.mvp(Tc, K, H, W, near, far, lp)).sum())


@pytest.mark.parametrize("ci", [0, 1])
def test_theta_gradient_is_the_central_difference_through_the_projection(ci):
    K0, H, W, g, Tc, lp, theta = _case(ci, 40 + ci)
    near, far = R.NEAR_FAR[ci]
    # the reference's fu, fv are K(theta) ROUNDED to float32 (what was rendered); the difference quotient is taken at that K:
    # theta' reproduces the rounded focal lengths exactly enough for the 1e-7 bar below
    K32 = IR.K_of_theta(K0, theta, H, W).astype(np.float32).astype(np.float64)
    theta = theta.copy()
    theta[0] = np.log(K32[0, 0] / np.float64(K0[0, 0]))
    theta[1] = np.log(K32[1, 1] / np.float64(K0[1, 1]))
    s, scale = IR.theta_gradient(g, Tc, lp, K0, theta, H, W)
    h = 1e-6
    for i in range(4):
        e = np.zeros(4)
        e[i] = h
        num = (_phi(K0, H, W, g, Tc, lp, theta + e, near, far) - _phi(K0, H, W, g, Tc, lp, theta - e, near, far)) / (2 * h)
        print(f"camera {ci} element {i}: analytic {s[i]:.9e} central difference {num:.9e} scale {scale[i]:.3e}")
        assert abs(s[i] - num) <= 1e-7 * scale[i], (i, s[i], num)
        assert abs(s[i]) > 1e-5 * scale[i]                         # a sign error would not hide in a vanishing value
    # tied: the derivative with respect to ONE common log-scale
    e = np.array([h, h, 0, 0])
    num = (_phi(K0, H, W, g, Tc, lp, theta + e, near, far) - _phi(K0, H, W, g, Tc, lp, theta - e, near, far)) / (2 * h)
    assert abs((s[0] + s[1]) - num) <= 1e-7 * (scale[0] + scale[1])
    assert (scale >= np.abs(s)).all()
    s32, _ = IR.theta_gradient(g, Tc, lp, K0, theta, H, W, dtype=torch.float32)
    assert s32.dtype == np.float32 and R.rel_err(s32, s, scale) < 1e-5


@pytest.mark.parametrize("ci", [0, 1])
def test_K_at_zero_theta_is_K0_bit_for_bit_and_the_host_helper_agrees(ci):
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    K0, H, W = R.CAMERAS[ci]
    K = IR.K_of_theta(K0, np.zeros(4), H, W).astype(np.float32)
    assert np.array_equal(K.view(np.uint32), np.asarray(K0, np.float32).view(np.uint32))
    assert np.array_equal(intrinsics_from_theta(K0, np.zeros(4), H, W).view(np.uint32), K.view(np.uint32))
    rng = np.random.default_rng(ci)
    for k in range(50):
        th = (rng.normal(size=4) * 0.03).astype(np.float32)
        th[k % 4] = 0.0 if k % 3 == 0 else th[k % 4]          # mixed: some elements exactly zero
        want = IR.K_of_theta(K0, th, H, W).astype(np.float32)
        got = intrinsics_from_theta(K0, th, H, W)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, th)
        for i, (r, c) in enumerate(IR.ENTRIES):
            if th[i] == 0:
                assert got[r, c] == np.float32(K0[r, c])
    # the other five entries are K0's whatever theta is
    got = intrinsics_from_theta(K0, [0.1, -0.1, 0.05, 0.02], H, W)
    rest = np.ones((3, 3), bool)
    for r, c in IR.ENTRIES:
        rest[r, c] = False
    assert np.array_equal(got[rest], np.asarray(K0, np.float32)[rest])
    assert got[0, 0] > K0[0, 0] and got[1, 1] < K0[1, 1] and got[0, 2] > K0[0, 2] and got[1, 2] > K0[1, 2]


@pytest.mark.parametrize("hname", list(R.ADAM_HYPER))
def test_adam_step_with_every_element_free_is_the_pose_heads(hname):
    h = R.hyper32(hname)
    rng = np.random.default_rng(3)
    for t0 in (0, 9, 999):
        p = rng.normal(size=4) * 0.01
        m = rng.normal(size=4) * (t0 > 0)
        v = rng.uniform(1, 4, size=4) * (t0 > 0)
        gsum = rng.normal(size=4) * 100
        red = np.array([1, 2, 3, 4, 5, 6, 7, 3.0])
        for dt in (torch.float64, torch.float32):
            got = IR.adam_step(p, m, v, t0, gsum, red, np.ones(4), 0, *h, dtype=dt)
            pad = lambda x: np.concatenate([x, np.zeros(2)])
            red6 = np.concatenate([gsum, [0, 0], red[6:]])
            want = R.adam_step(pad(p), pad(m), pad(v), t0, red6, *h, dtype=dt)
            for a, b in zip(got[:3], want[:3]):
                assert np.array_equal(a, b[:4])
            assert got[3] == t0 + 1 and np.array_equal(got[4], want[5][:4])
    # not free: kept, +0; tied: both focal elements take the sum; a non-finite red freezes the group
    got = IR.adam_step(p, m, v, 5, gsum, red, [1, 1, 0, 0], 1, *h)
    both = IR.adam_step(p, m, v, 5, np.array([gsum[0] + gsum[1]] * 2 + [0, 0]), red, [1, 1, 0, 0], 0, *h)
    for a, b in zip(got, both):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0][2:], p[2:]) and (got[4][2:] == 0).all() and not np.signbit(got[4][2:]).any()
    red[2] = np.inf
    fz = IR.adam_step(p, m, v, 5, gsum, red, [1, 1, 0, 1], 0, *h)
    assert np.array_equal(fz[0], p) and fz[3] == 5 and np.isnan(fz[4][[0, 1, 3]]).all() and fz[4][2] == 0
