"""The flat kinematic table (``UrdfChain.joint_table``) and the float64 reference of the joint-offset kernels
(tests/joint_reference.py), pinned on both packaged robots: FK from the table alone is ``UrdfChain.link_poses_batch``, the
analytic pose derivative is the central difference of that FK, the ``upstream`` bits are an ancestor walk."""
import numpy as np
import pytest

import joint_reference as JR

ROBOTS = ["xarm7", "franka"]


@pytest.fixture(scope="module", params=ROBOTS)
def robot(request):
    from easyhec_amd.robot import load_robot
    return load_robot(request.param)


def _qpos(robot, n, seed):
    rng = np.random.default_rng(seed)
    lim = robot.chain.limits()
    q = rng.uniform(lim[:, 0], lim[:, 1], size=(n, robot.chain.dof))
    return np.where(np.isfinite(q), q, 0.0)


def test_table_shapes_and_limits(robot):
    t = robot.joint_table()
    N, J, L = len(robot.chain.link_order), robot.chain.dof, len(robot.use_links)
    assert (N, J) == {"xarm7": (14, 9), "franka": (12, 9)}[robot.name]
    assert t["parent"].shape == (N,) and t["parent"].dtype == np.int32
    assert t["origin"].shape == (N, 16) and t["origin"].dtype == np.float64
    assert t["kind"].shape == (N,) and t["kind"].dtype == np.int32
    assert t["axis"].shape == (N, 3) and t["axis"].dtype == np.float64
    assert t["qidx"].shape == (N,) and t["qidx"].dtype == np.int32
    assert t["use"].shape == (L,) and t["use"].dtype == np.int32 and t["use"].tolist() == list(robot.use_links)
    assert t["upstream"].shape == (L,) and t["upstream"].dtype == np.uint32
    assert t["parent"][0] == -1 and (t["parent"][1:] >= 0).all() and (t["parent"][1:] < np.arange(1, N)).all()
    assert np.allclose(np.linalg.norm(t["axis"], axis=1), 1.0, atol=1e-15)
    assert sorted(t["qidx"][t["qidx"] >= 0].tolist()) == list(range(J))
    kinds = JR.joint_kinds(t)
    assert (kinds == 1).sum() == 7 and (kinds == 2).sum() == 2       # seven revolute, two prismatic
    assert ((t["kind"] == 0) == (t["qidx"] < 0)).all()


def test_table_refuses_chains_beyond_the_kernel_limits():
    from easyhec_amd.kinematics import UrdfChain
    eye = np.eye(4).tolist()
    mk = lambda n, typ: UrdfChain(spec={"links": [f"l{i}" for i in range(n + 1)], "joints": [
        {"name": f"j{i}", "type": typ, "parent": f"l{i}", "child": f"l{i + 1}", "origin": eye, "axis": [0, 0, 1],
         "lower": -1.0, "upper": 1.0} for i in range(n)]})
    assert mk(32, "revolute").joint_table([32])["upstream"][0] == 0xFFFFFFFF
    with pytest.raises(ValueError, match="32 joints"):
        mk(33, "revolute").joint_table([1])
    with pytest.raises(ValueError, match="64 links"):
        mk(64, "fixed").joint_table([1])
    assert mk(63, "fixed").joint_table([63])["upstream"][0] == 0


def test_fk_from_the_table_is_link_poses_batch(robot):
    t = robot.joint_table()
    q = _qpos(robot, 6, 1)
    _, lp, _ = JR.fk(t, q)
    want = robot.link_poses_batch(q)
    assert np.abs(lp - want).max() <= 1e-12
    # all links, not only the rendered ones
    frames, _, _ = JR.fk(t, q)
    every = robot.chain.link_poses_batch(q, list(range(len(robot.chain.link_order))))
    assert np.abs(frames - every).max() <= 1e-12


def test_upstream_bits_are_an_ancestor_walk(robot):
    t = robot.joint_table()
    chain = robot.chain
    col = {id(j): i for i, j in enumerate(chain.active)}
    for k, li in enumerate(robot.use_links):
        bits, name = 0, chain.link_order[li]
        while name in chain._joint_of_child:
            j = chain._joint_of_child[name]
            if id(j) in col:
                bits |= 1 << col[id(j)]
            name = j["parent"]
        assert int(t["upstream"][k]) == bits, (k, li)
    if robot.name == "franka":
        assert robot.use_links[0] == 0 and int(t["upstream"][0]) == 0           # the base link: no joint moves it
    # (neither packaged robot renders a link behind a prismatic joint: the fingers are covered through the table of ALL links)
    every = chain.joint_table(range(len(chain.link_order)))
    kinds = JR.joint_kinds(every)
    assert any(int(u) & sum(1 << j for j in range(chain.dof) if kinds[j] == 2) for u in every["upstream"])


def test_analytic_derivative_is_the_central_difference(robot):
    """Every link (the rendered ones and the fingers behind the prismatic joints) x every active joint, at 3 configurations
    and non-zero offsets."""
    every = list(range(len(robot.chain.link_order)))
    t = robot.chain.joint_table(every)
    assert set(robot.use_links) <= set(every)
    J = robot.chain.dof
    q = _qpos(robot, 3, 2)
    off = np.random.default_rng(3).uniform(-0.05, 0.05, size=J)
    _, lp, jf = JR.fk(t, q, off)
    D = JR.pose_derivatives(t, lp, jf)
    h, worst = 1e-6, 0.0
    for j in range(J):
        e = np.zeros(J)
        e[j] = h
        num = (robot.chain.link_poses_batch(q + off + e, every) - robot.chain.link_poses_batch(q + off - e, every)) / (2 * h)
        worst = max(worst, float(np.abs(D[:, :, j] - num).max()))
        up = np.array([(int(u) >> j) & 1 for u in t["upstream"]], dtype=bool)
        assert np.abs(num[:, ~up]).max(initial=0.0) == 0.0, j                   # a joint that is not upstream moves nothing
        assert up.any() and np.abs(num[:, up]).max() > 0.0
    print(f"{robot.name}: worst |D - central difference| = {worst:.2e}")
    assert worst <= 1e-8


def test_offset_gradient_is_the_chain_rule_through_fk(robot):
    """offset_gradient against a central difference of  sum <grad_mvp, PF @ Tc @ link_poses(offset)>."""
    import pose_reference as R
    t = robot.joint_table()
    J, L = robot.chain.dof, len(robot.use_links)
    rng = np.random.default_rng(4)
    q = _qpos(robot, 2, 5)
    off = rng.uniform(-0.05, 0.05, size=J)
    g = rng.normal(size=(2, L, 4, 4))
    Tc = R.random_rigid(rng, 1)[0].astype(np.float64)
    K, H, W = R.CAMERAS[0]
    near, far = R.NEAR_FAR[0]
    _, lp, jf = JR.fk(t, q, off)
    s, scale = JR.offset_gradient(t, g, Tc, K, H, W, near, far, lp, jf)
    f = lambda o: float((g * R.mvp(Tc, K, H, W, near, far, JR.fk(t, q, o)[1])).sum())
    for j in range(J):
        e = np.zeros(J)
        e[j] = 1e-6
        num = (f(off + e) - f(off - e)) / 2e-6
        assert abs(s[j] - num) <= 1e-7 * scale[j], (j, s[j], num)
    assert (scale >= np.abs(s)).all()
    # the float32 run of the same text: what the kernels' bar is made of
    s32, _ = JR.offset_gradient(t, g, Tc, K, H, W, near, far, lp, jf, dtype=R.torch.float32)
    assert s32.dtype == np.float32 and R.rel_err(s32, s, scale) < 1e-5
