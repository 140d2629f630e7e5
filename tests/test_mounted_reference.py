"""Eye-in-hand kinematics on the CPU: the float64 reference of tests/mounted_reference.py against central differences, the
sign-folded joint frames and the XOR-ed mask against that reference, wrong copies of the fold against the bars the GPU tests
use, the host kinematics (``UrdfChain`` with ``mount=``, ``Robot.mounted``) against the reference, the gauge between the
mount's own joint and the camera pose, and the preconditions of the end-to-end scene (tests/mounted_scene.py)."""
import numpy as np
import pytest
import torch

import joint_reference as JR
import joint_table_cases as C
import mounted_reference as MR
import mounted_scene as MS
import pose_reference as R

F32 = torch.float32
U = R.U


def _folded_D(t, q, off, m, mistake=None):
    """``joint_reference.pose_derivatives`` on what the kernel hands on (the folded triple), or on a wrong copy of it."""
    lp, jf, rel = MR.folded(t, q, off, m)
    lp, jf, rel = wrong_fold(t, m, lp, jf, rel, mistake)
    return JR.pose_derivatives(dict(t, upstream=rel), lp, jf)


def wrong_fold(t, m, lp, jf, rel, mistake):
    """The folded triple with one mistake a kernel or its caller could make:
      "axis_kept"   the axes of the joints that move the mount are not negated
      "mask_base"   the host passes the base-frame mask, not upstream ^ mount_upstream
      "point_too"   the point p' is negated together with the axis"""
    ul, um = MR.masks(t, m)
    neg = np.array([(int(um) >> j) & 1 for j in range(jf.shape[1])], bool)
    jf = jf.copy()
    if mistake == "axis_kept":
        jf[:, neg, :3] *= -1
    elif mistake == "mask_base":
        rel = ul
    elif mistake == "point_too":
        jf[:, neg, 3:] *= -1
    else:
        assert mistake is None, mistake
    return lp, jf, rel


# ---- 1. the derivative -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.NAMES)
def test_analytic_derivative_is_the_central_difference_and_the_folded_frames_give_it(name):
    t = C.case(name).table
    q, off = C.qpos(name, 2), C.offsets(name).astype(np.float64)
    for m in MR.mounts(t):
        D = MR.analytic_derivatives(t, q, off, m)
        Dd = MR.difference_derivatives(t, q, off, m)
        Df = _folded_D(t, q, off, m)
        ul, um = MR.masks(t, m)
        negated = bin(int(um)).count("1")
        d_diff, d_fold = float(np.abs(D - Dd).max()), float(np.abs(D - Df).max())
        print(f"[mounted] {name} mount {m} ({negated} negated joints): analytic - differences {d_diff:.2e}, folded - analytic {d_fold:.2e}")
        assert np.abs(D).max() > 0.1 or name == "one"
        assert d_diff <= 1e-7 and d_fold <= 1e-12
        # the reference that takes the kernel's outputs (fold undone, factor u_l - u_m) is the same derivative
        lp, jf, rel = MR.folded(t, q, off, m)
        assert np.abs(MR.pose_derivatives(MR.mounted_table(t, m), lp, jf) - D).max() <= 1e-12
    assert any(int(MR.masks(t, m)[1]) for m in MR.mounts(t))


def forward_miss(name, m, mistake):
    """The wrong copy's joint_frames over the bar of the GPU forward test (``eh <= R.bound(e32)``, B = 1 and 5)."""
    t = C.case(name).table
    worst = 0.0
    for B in (1, 5):
        q, off = C.qpos(name, B), C.offsets(name)
        lp, jf64, rel = MR.folded(t, q, off, m)
        _, jf32, _ = MR.folded(t, q, off, m, dtype=F32)
        _, jfw, _ = wrong_fold(t, m, lp, jf64, rel, mistake)
        s = float(np.abs(jf64).max())
        worst = max(worst, R.rel_err(jfw.astype(np.float32), jf64, s) / R.bound(R.rel_err(jf32, jf64, s)))
    return worst


def gradient_miss(name, m, mistake, B):
    """The wrong copy's offset gradient over the bar of the GPU gradient test."""
    worst = 0.0
    for draw in range(2):
        c = C.bwd_case(name, B, draw)
        t = MR.mounted_table(c["t"], m)
        lp, jf, rel = MR.folded(c["t"], c["q"], c["off"], m)
        lp, jf = lp.astype(np.float32), jf.astype(np.float32)                  # what the forward kernel hands on
        args = (c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"])
        s64, scale = MR.offset_gradient(t, *args, lp, jf)
        s32, _ = MR.offset_gradient(t, *args, lp, jf, dtype=F32)
        _, jfw, relw = wrong_fold(c["t"], m, lp, jf, rel, mistake)
        sw, _ = JR.offset_gradient(dict(c["t"], upstream=relw), *args, lp, jfw)
        live = scale > 0
        e32 = R.rel_err(s32[live], s64[live], scale[live])
        worst = max(worst, R.rel_err(sw[live], s64[live], scale[live]) / R.bound(e32))
    return worst


@pytest.mark.parametrize("name", ["tree", "prismatic_mid", "full", "serial64"])
def test_wrong_copies_of_the_fold_miss_the_gpu_bars(name):
    t = C.case(name).table
    m = int(t["parent"].shape[0]) - 1
    assert int(MR.masks(t, m)[1]) != 0
    assert gradient_miss(name, m, None, 5) <= 1.0                  # (the right copy passes the bar it is held to)
    assert forward_miss(name, m, None) <= 1.0
    for mistake in ("axis_kept", "mask_base", "point_too"):
        rf = forward_miss(name, m, mistake) if mistake != "mask_base" else float("nan")
        rg = gradient_miss(name, m, mistake, 5)
        print(f"[mounted] {name} mount {m} with {mistake}: joint_frames miss {rf:.3g} x the forward bar, offset gradient miss "
              f"{rg:.3g} x the gradient bar")
        assert rg >= 100.0
        if mistake != "mask_base":
            assert rf >= 100.0


# ---- 2. host kinematics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["xarm7", "franka"])
def test_host_kinematics_against_the_reference(robot):
    from easyhec_amd.robot import load_robot
    rb = load_robot(robot)
    base = rb.joint_table()
    again = rb.chain.joint_table(rb.use_links, mount=None)
    assert list(again) == list(base) == ["parent", "origin", "kind", "axis", "qidx", "use", "upstream"]
    assert all(np.array_equal(again[k], base[k]) and again[k].dtype == base[k].dtype for k in base)
    N = len(rb.chain.link_order)
    lim = rb.chain.limits()
    q = np.random.default_rng(3).uniform(lim[:, 0], lim[:, 1], size=(3, rb.chain.dof))
    for m in (0, 1, N // 2, N - 1):
        view = rb.mounted(m)
        t = view.joint_table()
        want = MR.mounted_table(base, m)
        assert t["mount"] == m and int(t["mount_upstream"]) == int(want["mount_upstream"])
        assert np.array_equal(t["upstream_base"], base["upstream"]) and np.array_equal(t["upstream"], want["upstream"])
        assert t["upstream"].dtype == np.uint32 and np.asarray(t["mount_upstream"]).dtype == np.uint32
        assert all(np.array_equal(t[k], base[k]) for k in ("parent", "origin", "kind", "axis", "qidx", "use"))
        lp = view.link_poses_batch(q)
        _, ref, _ = MR.fk_mounted(base, q, None, m)
        d = float(np.abs(lp - ref).max())
        print(f"[mounted] {robot} mount {m} ({rb.chain.link_order[m]}): host link poses - reference {d:.2e}")
        assert lp.dtype == np.float64 and d <= 1e-12
        assert np.abs(view.link_poses(q[1]) - lp[1]).max() <= 1e-15
        assert view.mount_link == rb.chain.link_order[m] and view.base is rb and view.meshes is rb.meshes
        assert rb.mounted(rb.chain.link_order[m]).mount == m                     # by name
    root = rb.mounted(0).link_poses_batch(q)
    assert np.array_equal(root, rb.link_poses_batch(q))                          # a mount at the root: the base-frame poses
    with pytest.raises(ValueError):
        rb.mounted(N)
    with pytest.raises(ValueError):
        rb.mounted("no_such_link")
    with pytest.raises(ValueError):
        rb.mounted(1).mounted(2)


# ---- 3. the gauge ------------------------------------------------------------------------------------------------------------------
def _gauge_residual(t, q, off, m, links):
    """|tangent of the mount's own joint - its projection on the six pose tangents| / |tangent|, over ``links`` (rows of the
    rendered links), at a general camera pose X.  Tangents of X @ P_l: d/d dof_i = J_i @ P_l, d/d offset_g = X @ D_lg."""
    g = MR.gauge_joint(t, m)
    _, lp, _ = MR.fk_mounted(t, q, off, m)
    D = MR.analytic_derivatives(t, q, off, m)
    X, Jac = R.exp_and_jac(np.array([0.3, -0.2, 0.5, 0.4, -0.3, 0.2], np.float32))
    X, Jac = np.asarray(X, np.float64), np.asarray(Jac, np.float64)
    A = np.stack([(Jac[i] @ lp[:, links]).reshape(-1) for i in range(6)], axis=1)
    y = (X @ D[:, links, g]).reshape(-1)
    res = y - A @ np.linalg.lstsq(A, y, rcond=None)[0]
    return float(np.linalg.norm(res) / np.linalg.norm(y)), g


@pytest.mark.parametrize("name", ["skew_serial", "prismatic_mid", "tree", "full"])
def test_the_mount_s_own_joint_is_a_gauge_with_the_camera_pose(name):
    """Over the links that do not ride with the mount, the tangent of the mount's own joint lies in the span of the six pose
    tangents (zero residual in exact arithmetic).  A rendered link that rides with the mount (the mount itself, or a link below
    it) has a zero joint tangent but a non-zero pose tangent, and breaks the gauge: from the mount a camera sees little of
    those, which is why the direction is weak, not always null, in the information report."""
    t = C.case(name).table
    q, off = C.qpos(name, 2), C.offsets(name).astype(np.float64)
    N = int(t["parent"].shape[0])
    seen = 0
    for m in sorted({N // 2, N - 1}):
        g = MR.gauge_joint(t, m)
        if g is None or JR.joint_kinds(t)[g] == 0:
            continue
        ul, um = MR.masks(t, m)
        apart = [l for l in range(len(ul)) if not (int(ul[l]) >> g) & 1]          # links the gauge joint does not carry
        riding = [l for l in range(len(ul)) if (int(ul[l]) >> g) & 1]
        if not apart:
            continue
        r, _ = _gauge_residual(t, q, off, m, apart)
        print(f"[mounted] {name} mount {m}: gauge joint {g}, {len(apart)} links apart: residual {r:.2e} of the tangent's norm")
        assert r <= 1e-9
        seen += 1
        if riding:
            r_all, _ = _gauge_residual(t, q, off, m, apart + riding)
            print(f"[mounted] {name} mount {m}: with the {len(riding)} links that ride with the mount: {r_all:.2e}")
            assert r_all > 1e-3
    assert seen >= 1


def test_default_free_joints_leave_out_the_gauge_joint_and_everything_below_the_mount():
    from easyhec_amd.joint_calib import default_free_joints, mount_gauge_joint
    from easyhec_amd.robot import load_robot
    rb = load_robot("xarm7")
    assert default_free_joints(rb.joint_table()) == [1, 2, 3, 4, 5, 6]           # the base-frame default is unchanged
    t = rb.mounted("link7").joint_table()
    assert mount_gauge_joint(t) == 6 == MR.gauge_joint(t, t["mount"])
    assert default_free_joints(t) == [0, 1, 2, 3, 4, 5]
    t4 = rb.mounted("link4").joint_table()
    assert mount_gauge_joint(t4) == 3 and default_free_joints(t4) == [0, 1, 2]   # joints 4..6 lie below the mount
    assert default_free_joints(rb.mounted("link_base").joint_table()) == []
    tt = C.case("tree").chain.joint_table(C.case("tree").use, mount="a4")
    g = mount_gauge_joint(tt)
    free = default_free_joints(tt)
    assert g == 7 and g not in free and all((int(tt["mount_upstream"]) >> j) & 1 for j in free)
    assert all(JR.joint_kinds(tt)[j] == 1 for j in free) and free == [0, 2]      # a1, a2; a3 is prismatic, a4 the gauge


# ---- 4. the end-to-end scene ---------------------------------------------------------------------------------------------------------
def test_scene_preconditions(oracle):
    rb, view, K, X, qp, lp = MS.scene()
    assert lp.shape == (MS.VIEWS, 8, 4, 4) and MS.H <= 120 and MS.W <= 160 and view.mount_link == "link7"
    # X is no half turn: there the rotation-vector coordinates of model.dof are singular (w and -w are one rotation), and a
    # solve that starts there is not what the end-to-end tests are about; 20 degrees off it, 10 times the start's 2 degrees
    turn = np.degrees(np.arccos(np.clip((np.trace(X[:3, :3]) - 1) / 2, -1, 1)))
    print(f"[mounted] scene: X turns the mount's frame by {turn:.1f} degrees")
    assert turn <= 160.0
    mask = MS.oracle_masks(oracle) > 0.5
    cover = mask.mean(axis=(1, 2))
    per = np.stack([(MS.oracle_masks(oracle, [l]) > 0.5).sum(axis=(1, 2)) for l in range(len(rb.meshes))], axis=1)
    shown = (per >= 20).sum(axis=1)
    print(f"[mounted] scene: coverage {np.round(cover, 3).tolist()}, links shown {shown.tolist()}, pixels per link {per.tolist()}")
    assert (cover >= 0.03).all() and (cover <= 0.70).all() and (shown >= 3).all() and mask.any(axis=(1, 2)).all()
