"""The float64 reference of the camera rig (tests/rig_reference.py): its gradient is the concatenation identity where the
cameras coincide, it matches central differences of ``UrdfChain`` kinematics through two DIFFERENT cameras, and its Adam is all
or nothing."""
import numpy as np
import pytest

import joint_reference as JR
import pose_reference as R
import rig_reference as RR


@pytest.fixture(scope="module", params=["xarm7", "franka"])
def robot(request):
    from easyhec_amd.robot import load_robot
    return load_robot(request.param)


def _qpos(robot, n, seed):
    lim = robot.chain.limits()
    q = np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], size=(n, robot.chain.dof))
    return np.where(np.isfinite(q), q, 0.0)


def _camera(robot, t, B, seed, cam, nf, off, Tc=None):
    rng = np.random.default_rng(seed)
    q = _qpos(robot, B, seed + 1)
    K, H, W = R.CAMERAS[cam]
    near, far = R.NEAR_FAR[nf]
    _, lp, jf = JR.fk(t, q, off)
    return dict(q=q, g=rng.normal(size=(B, len(robot.use_links), 4, 4)), K=K, H=H, W=W, near=near, far=far, lp=lp, jf=jf,
                Tc=R.random_rigid(rng, 1)[0].astype(np.float64) if Tc is None else Tc)


def test_rig_sum_of_coinciding_cameras_is_the_gradient_of_the_concatenated_views(robot):
    t = robot.joint_table()
    off = np.random.default_rng(1).uniform(-0.05, 0.05, size=robot.chain.dof)
    a = _camera(robot, t, 2, 10, 0, 0, off)
    cams = [a, _camera(robot, t, 3, 20, 0, 0, off, Tc=a["Tc"]), _camera(robot, t, 1, 30, 0, 0, off, Tc=a["Tc"])]
    T, scale = RR.rig_sum(t, cams)
    cat = lambda k: np.concatenate([c[k] for c in cams])
    s, sc = JR.offset_gradient(t, cat("g"), a["Tc"], a["K"], a["H"], a["W"], a["near"], a["far"], cat("lp"), cat("jf"))
    assert (np.abs(T - s) <= 8 * 2.0 ** -52 * sc).all(), (T, s)       # float64 rounding: the two add in different orders
    assert (np.abs(scale - sc) <= 8 * 2.0 ** -52 * sc).all()
    g, _ = RR.rig_gradient(t, cams)
    assert np.array_equal(g, T / 6.0)                                 # the mean over ALL views: 2 + 3 + 1


def test_rig_gradient_is_the_central_difference_through_two_different_cameras(robot):
    """d/d offset of  (1 / sum B_c) sum_c <g_c, PF_c @ Tc_c @ link_poses(qpos_c + offset)>  with UrdfChain's own kinematics:
    two cameras of different K, size, depth planes, pose and view count."""
    t = robot.joint_table()
    J = robot.chain.dof
    off = np.random.default_rng(2).uniform(-0.05, 0.05, size=J)
    cams = [_camera(robot, t, 2, 40, 0, 0, off), _camera(robot, t, 3, 50, 1, 1, off)]
    g, scale = RR.rig_gradient(t, cams)
    n = sum(c["g"].shape[0] for c in cams)

    def f(o):
        return sum(float((c["g"] * R.mvp(c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"],
                                         robot.link_poses_batch(c["q"] + o[None]))).sum()) for c in cams) / n
    for j in range(J):
        e = np.zeros(J)
        e[j] = 1e-6
        num = (f(off + e) - f(off - e)) / 2e-6
        assert abs(g[j] - num) <= 1e-7 * scale[j], (j, g[j], num)
    # each camera contributes: neither sum alone is the rig's
    (s0, _), (s1, _) = RR.camera_sums(t, cams)
    assert np.abs(s0).max() > 0 and np.abs(s1).max() > 0 and np.array_equal(RR.rig_sum(t, cams)[0], s0 + s1)
    g32, _ = RR.rig_gradient(t, cams, dtype=R.torch.float32)
    assert g32.dtype == np.float32 and R.rel_err(g32, g, scale) < 1e-5


def test_rig_adam_is_all_or_nothing():
    rng = np.random.default_rng(3)
    J = 9
    free = np.array([0, 1, 1, 1, 1, 1, 1, 0, 0], bool)
    h = R.hyper32("default")
    poses = [(rng.normal(size=6), rng.normal(size=6), rng.uniform(1, 4, size=6), 9 + c) for c in range(3)]
    reds = [np.array([1, 2, 3, 4, 5, 6, 7, 2 + c], np.float64) for c in range(3)]
    offs = (rng.normal(size=J) * 0.01, rng.normal(size=J), rng.uniform(1, 4, size=J), 9)
    gsum = rng.normal(size=J)
    out, o, ok = RR.rig_adam_step(poses, reds, offs, gsum, free, h, h)
    assert ok and o[3] == 10 and [x[3] for x in out] == [10, 11, 12]
    assert np.array_equal(o[4], np.where(free, gsum / 9.0, 0.0))                 # n = 2 + 3 + 4 views
    for c in range(3):                                                           # a camera's pose step is its solo step
        want = R.adam_step(*poses[c], reds[c], *h)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(out[c], want))
    solo = JR.adam_step(*offs, gsum, [0, 0, 0, 0, 0, 0, 0, 9.0], free, *h)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(o, solo))
    for bad in (0, 2):
        r2 = [r.copy() for r in reds]
        r2[bad][6] = np.inf
        out, o, ok = RR.rig_adam_step(poses, r2, offs, gsum, free, h, h)
        assert not ok and o[3] == 9 and all(np.array_equal(a, b) for a, b in zip(o[:3], offs[:3]))
        assert np.isnan(o[4][free]).all() and (o[4][~free] == 0).all()
        for c in range(3):
            assert all(np.array_equal(a, b) for a, b in zip(out[c][:3], poses[c][:3])) and out[c][3] == poses[c][3]
            assert np.isnan(out[c][4]) and np.isnan(out[c][5]).all()
