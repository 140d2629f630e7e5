"""Eye-in-hand on the device: ehr_joint_forward_mounted and ehr_joint_forward_multi_mounted (csrc/ehr_joint.hip) on the synthetic
kinematic trees of tests/joint_table_cases.py, the UNCHANGED ehr_joint_backward_adam and ehr_lm_linearize on their outputs, the
refusals, and the solves on xArm7 with the camera on its last arm link (tests/mounted_scene.py; its preconditions are checked
on the CPU in tests/test_mounted_reference.py).

No tolerance of its own.  link_poses, joint_frames and the offset gradient: the rules of
tests/test_gpu_joint_table_shapes.py against tests/mounted_reference.py; the tangents: ``lm_reference.tangent_ratio <= 1``; the
chain: the bars of test_chain_tracks_autograd_through_differentiable_kinematics.  Outputs are filled with NaN before each call
and finite after it.  Every figure is printed before it is asserted; the measured ones are in profiles/mounted.md."""
import numpy as np
import pytest
import torch

import joint_reference as JR
import joint_table_cases as C
import lm_reference as LR
import mounted_reference as MR
import mounted_scene as MS
import pose_reference as R
from test_gpu_joint_offsets import AutogradJointSolve, _Bwd, _bits, _dev, _dev_table, _forward, _stream
from test_gpu_joint_table_shapes import LM_FREE, _idle_joints, _ti, _upstream_i32
from test_gpu_lm_tangent_shapes import FAR, NEAR, dofs, linearize, pose_forward, t32

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U = R.U
DEV = torch.device("cuda:0")
NAMES = ("one", "tree", "prismatic_mid", "full", "serial64")


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib
    assert _lib.has_mounted() and _lib.has_joint_offsets() and _lib.has_lm() and _lib.has_lm_multi_calib()
    return _lib


def _mounts(t):
    N = int(t["parent"].shape[0])
    return sorted({0, N // 2, N - 1})


def _forward_mounted(t, m, q, off, multi=None, rc=False):
    """ehr_joint_forward_mounted (or, with multi = (P, Bv): q [Bv,J], off [P,J], the multi entry) -> (link_poses, joint_frames)
    device tensors, NaN before the call.  ``t``: the base table; the mask is walked by the reference."""
    from easyhec_amd import _lib
    d = _dev_table(t)
    tab = [_lib.ptr(d[k]) for k in ("parent", "origin", "kind", "axis", "qidx", "use")]
    um = int(MR.masks(t, max(0, min(m, t["parent"].shape[0] - 1)))[1])
    J = q.shape[1]
    N, L = t["parent"].shape[0], t["use"].shape[0]
    B = q.shape[0] if multi is None else multi[0] * multi[1]
    lp = torch.full((B, L, 4, 4), float("nan"), device=DEV)
    jf = torch.full((B, J, 6), float("nan"), device=DEV)
    qd, od = _dev(q.astype(np.float64)), _dev(off.astype(np.float32))
    if multi is None:
        code = _lib.lib().ehr_joint_forward_mounted(*tab, N, J, L, m, um, _lib.ptr(qd), _lib.ptr(od), B, _lib.ptr(lp),
                                                    _lib.ptr(jf), _stream())
    else:
        code = _lib.lib().ehr_joint_forward_multi_mounted(*tab, N, J, L, m, um, _lib.ptr(qd), _lib.ptr(od), multi[0], multi[1],
                                                          _lib.ptr(lp), _lib.ptr(jf), _stream())
    torch.cuda.synchronize()
    if rc:
        return code, lp, jf
    _lib.check(code, "ehr_joint_forward_mounted")
    return lp, jf


# ---- 1. forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_float64(env, name):
    t = C.case(name).table
    bad, negated = [], 0
    for m in _mounts(t):
        um = int(MR.masks(t, m)[1])
        for B in (1, 5):
            q, off = C.qpos(name, B), C.offsets(name)
            lp, jf = _forward_mounted(t, m, q, off)
            lp2, jf2 = _forward_mounted(t, m, q, off)
            assert torch.equal(lp, lp2) and torch.equal(jf, jf2), "two runs differ"
            lpb, jfb = _forward(t, q, off)
            if m == 0:      # the root's frame is the identity: the base kernel's values (the sign of a zero may differ)
                assert torch.equal(lp, lpb) and torch.equal(jf, jfb), "mount at the root differs from ehr_joint_forward"
            lp, jf = lp.cpu().numpy(), jf.cpu().numpy()
            lp64, jf64, _ = MR.folded(t, q, off, m)
            _, jf32, _ = MR.folded(t, q, off, m, dtype=F32)
            want = lp64.astype(np.float32)
            d_lp = float((np.abs(lp.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
            s = float(np.abs(jf64).max())
            e32, eh = R.rel_err(jf32, jf64, s), R.rel_err(jf, jf64, s)
            print(f"[mounted] {name} mount {m} B={B}: link_poses worst {d_lp / U:.2f} units | joint_frames e32 {e32:.2e} hip "
                  f"{eh:.2e} bound {R.bound(e32):.2e}")
            if not (d_lp <= U and eh <= R.bound(e32) and np.isfinite(lp).all() and np.isfinite(jf).all()):
                bad.append((m, B, d_lp, eh))
            if um:
                # the base kernel's axis (one float32 rounding of a unit vector: within U / 2 per component, so within U after
                # the rotation) turned into the mount's frame, against the mounted kernel's (its own rounding, U / 2): 2 U
                frames, _, _ = JR.fk(t, q, off)
                RmT = np.swapaxes(frames[:, m, :3, :3], 1, 2)
                turned = np.einsum("brc,bjc->bjr", RmT, jfb.cpu().numpy()[:, :, :3].astype(np.float64))
                neg = np.array([(um >> j) & 1 for j in range(jf.shape[1])], bool)
                assert np.abs(jf[:, neg, :3] + turned[:, neg]).max() <= 2 * U, "an axis upstream of the mount is not negated"
                if (~neg).any():
                    assert np.abs(jf[:, ~neg, :3] - turned[:, ~neg]).max() <= 2 * U
                negated += int(neg.sum())
    assert not bad, bad
    assert negated >= 1


@pytest.mark.parametrize("name", ["tree", "full"])
def test_multi_start_rows_are_the_solo_kernel_s(env, name):
    t = C.case(name).table
    P, Bv = 3, 2
    q = C.qpos(name, Bv)
    off = np.stack([C.offsets(name, seed=p) for p in range(P)])
    for m in _mounts(t)[1:]:
        lp, jf = _forward_mounted(t, m, q, off, multi=(P, Bv))
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(jf).all())
        for p in range(P):
            lp1, jf1 = _forward_mounted(t, m, q, off[p])
            for j in range(Bv):
                assert torch.equal(lp[p * Bv + j], lp1[j]), (m, p, j, "link_poses")
                assert torch.equal(jf[p * Bv + j], jf1[j]), (m, p, j, "joint_frames")
        assert not torch.equal(lp[:Bv], lp[Bv:2 * Bv]) and not torch.equal(lp[Bv:2 * Bv], lp[2 * Bv:])


# ---- 2. the offset gradient: the unchanged ehr_joint_backward_adam on the mounted outputs -----------------------------------------
GRAD_B = {name: (1, 5) for name in NAMES}
GRAD_B["full"] = (1, 5, 9)      # 9 views x 32 links = 288 pairs: one full tile of 256 and a partial one


@pytest.mark.parametrize("pattern", ["all", "frozen"])
@pytest.mark.parametrize("name", NAMES)
def test_offset_gradient_against_the_float64_reference(env, name, pattern):
    bad = []
    base = C.case(name).table
    m = int(base["parent"].shape[0]) - 1
    t = MR.mounted_table(base, m)
    assert int(t["mount_upstream"]) != 0
    for B in GRAD_B[name]:
        e32, eh = 0.0, 0.0
        for draw in range(2):
            c = C.bwd_case(name, B, draw, pattern)
            red = np.array([1, 2, 3, 4, 5, 6, 7, 1], np.float32)      # red[7] = 1: grad_out is the sum itself
            grads = []
            for _ in range(2):
                lp, jf = _forward_mounted(base, m, c["q"], c["off"])
                tc_jac = torch.full((7, 16), float("nan"), device=DEV)
                tc_jac[0] = _dev(c["Tc"].reshape(16))
                J = c["J"]
                b = _Bwd(t, c["off"], np.zeros(J), np.zeros(J), 0, c["free"])       # (reads t["upstream"]: the relative mask)
                b.grad.fill_(float("nan"))
                p, mm, v, step, grad = b.step(_dev(c["g"]), tc_jac, _dev(c["K"]), c["H"], c["W"], c["near"], c["far"], lp, jf,
                                              _dev(red), R.hyper32("default"))
                grads.append(grad)
            assert np.array_equal(_bits(grads[0]), _bits(grads[1])), "two runs differ"
            lp, jf = lp.cpu().numpy(), jf.cpu().numpy()
            args = (t, c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"], lp, jf)
            s64, scale = MR.offset_gradient(*args)
            s32, _ = MR.offset_gradient(*args, dtype=F32)
            fr = c["free"].astype(bool)
            assert step == 1 and np.isfinite(grad).all() and np.isfinite(lp).all() and np.isfinite(jf).all()
            assert (grad[~fr] == 0).all() and not np.signbit(grad[~fr]).any(), grad      # exactly +0 where not free
            idle = _idle_joints(t, c["J"])                                                # (of the relative mask)
            assert (scale[idle] == 0).all() and (grad[idle] == 0).all() and not np.signbit(grad[idle]).any()
            live = fr & (scale > 0)
            assert live.any() == (fr & ~idle).any() and (grad[fr & ~live] == 0).all()
            if live.any():
                assert (np.abs(s64[live]) > 0).any()
                e32 = max(e32, R.rel_err(s32[live], s64[live], scale[live]))
                eh = max(eh, R.rel_err(grad[live], s64[live], scale[live]))
        print(f"[mounted] {name} mount {m} {pattern} B={B}: offset gradient e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e}")
        if not eh <= R.bound(e32):
            bad.append((B, e32, eh))
    assert not bad, bad


# ---- 3. the tangents: the unchanged ehr_lm_linearize on the mounted frames ---------------------------------------------------------
@pytest.mark.parametrize("name", ["prismatic_mid", "tree", "full"])
def test_joint_tangents(env, name):
    _lib = env
    base = C.case(name).table
    m = int(base["parent"].shape[0]) - 1
    t = MR.mounted_table(base, m)
    L, B = base["use"].shape[0], 3
    kinds = JR.joint_kinds(base)
    free = LM_FREE[name]
    q, off = C.qpos(name, B), C.offsets(name)
    lp, jf = _forward_mounted(base, m, q, off)
    up = np.asarray(t["upstream"])
    joints = (jf, _upstream_i32(t), _ti(kinds), _ti(free))
    K, H, W = R.SMALL_K, 131, 97
    dof = dofs()["w0.3"]
    tdof, tK = t32(dof), t32(K)
    mvp, dmvp = linearize(_lib, tdof, tK, lp, H, W, joints=joints)
    assert torch.equal(mvp, pose_forward(_lib, tdof, tK, lp, H, W)), "mvp is not ehr_pose_forward's"
    lp64, jf64, _ = MR.folded(base, q, off, m)
    D, Dabs = MR.pose_derivatives(t, lp64, jf64), MR.pose_derivatives(t, lp64, jf64, absolute=True)
    assert np.abs(D - MR.analytic_derivatives(base, q, off.astype(np.float64), m)).max() <= 1e-12
    _, ref, Sabs = LR.tangents(dof, K, H, W, NEAR, FAR, lp.cpu().numpy(), D, Dabs, free)
    got = dmvp.cpu().numpy()
    assert got.shape == ref.shape == (6 + len(free), B, L, 4, 4) and np.isfinite(got).all() and bool(torch.isfinite(mvp).all())
    rp = LR.tangent_ratio(got[:6], ref[:6], Sabs[:6])
    rj = LR.tangent_ratio(got[6:], ref[6:], Sabs[6:], roundings=3)
    zero = [(l, j) for l in range(L) for j in free if not (int(up[l]) >> j) & 1]
    flipped = [(l, j) for l in range(L) for j in free if (int(up[l]) >> j) & 1 and (int(t["mount_upstream"]) >> j) & 1]
    print(f"[mounted] {name} mount {m} ({L} links, {len(free)} free joints): pose tangents worst |d - ref| / bar = {rp:.3f}, joint "
          f"tangents {rj:.3f}; {len(flipped)} (link, joint) blocks with the factor -1, {len(zero)} exactly zero")
    assert rp <= 1.0 and rj <= 1.0
    assert len(flipped) >= 1 and len(zero) >= 1
    row = lambda j: 6 + free.index(j)
    for l, j in zero:
        assert (got[row(j), :, l] == 0).all(), (l, j)
    for l, j in flipped:
        assert (got[row(j), :, l] != 0).any(), (l, j)


# ---- 4. refusals and existing behaviour --------------------------------------------------------------------------------------------
def test_a_mount_out_of_range_is_refused(env):
    t = C.case("tree").table
    N = int(t["parent"].shape[0])
    q, off = C.qpos("tree", 2), C.offsets("tree")
    for m in (-1, N, 64):
        code, lp, jf = _forward_mounted(t, m, q, off, rc=True)
        assert code == -1 and bool(torch.isnan(lp).all()) and bool(torch.isnan(jf).all()), m        # EHR_ERR_INVALID, nothing written
        code, lp, jf = _forward_mounted(t, m, q, np.stack([off, off]), multi=(2, 2), rc=True)
        assert code == -1 and bool(torch.isnan(lp).all()), m
    assert b"mount" in env.lib().ehr_last_error()


def _problem(offsets_true=None, views=MS.VIEWS):
    """The scene of tests/mounted_scene.py as a solve: (cfg, make, batch WITHOUT link_poses, view, qp, X).  The reference masks
    are the package's own render at the true X and the link poses at ``qpos + offsets_true``; ``make()`` starts 1 cm and
    2 degrees off in X."""
    from easyhec_amd import fused
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import perturb_pose
    rb, view, K, X, qp, _ = MS.scene()
    qp = qp[:views]
    B, H, W = qp.shape[0], MS.H, MS.W
    true = np.zeros(qp.shape[1]) if offsets_true is None else np.asarray(offsets_true, np.float64)
    lp = view.link_poses_batch(qp + true[None]).astype(np.float32)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(X, dt=(0.006, -0.006, 0.0053), drot_deg=(1.2, -1.2, 1.06)).tolist()

    def make():
        return RBSolver(cfg, meshes=rb.meshes).to(DEV)

    m0 = make()
    Kt = torch.tensor(K, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(X, dtype=torch.float32, device=DEV), torch.tensor(lp, device=DEV)),
            torch.zeros((B, H, W), device=DEV))
    batch = {"mask": (gt > 0.5).float(), "K": Kt[None].repeat(B, 1, 1)}
    return cfg, make, batch, view, qp, X


def test_rigs_and_the_feasibility_filter_refuse_a_mounted_view(env):
    from easyhec_amd.feasibility import FeasibilityFilter
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch, view, qp, X = _problem(views=2)
    with pytest.raises(ValueError, match="mounted on the arm.*one upstream mask"):
        RigJointStep([make(), make()], [batch, batch], view, [qp, qp])
    with pytest.raises(ValueError, match="base-frame question: pass the robot's .base"):
        FeasibilityFilter(view)


def test_a_plain_robot_still_runs_the_base_kernel(env, xarm7):
    """``JointPoseStep`` on a plain robot: the bits of ``corrected_link_poses()`` are ehr_joint_forward's."""
    from easyhec_amd.joint_calib import JointPoseStep
    from test_gpu_fast import problem
    from test_gpu_joint_offsets import _views_qpos
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    off = np.zeros(qp.shape[1], np.float32)
    off[[1, 3, 5]] = [0.01, -0.02, 0.015]
    js = JointPoseStep(make(), batch, xarm7, qp, init_offset=off)
    assert js.kinematics.mount is None and "mount" not in js.table
    lp, _ = _forward(xarm7.joint_table(), qp, off)
    assert torch.equal(js.corrected_link_poses(), lp)


# ---- 5. end to end: xArm7, the camera on link7 -----------------------------------------------------------------------------------------
def torch_fk_mounted(table, qpos, offsets):
    """Differentiable mounted kinematics in float64, composed with ``torch.linalg.inv``: qpos [B,J] float64 tensor, offsets [J]
    -> inv(F_mount) @ F_l as [B,L,4,4] float32."""
    dev = qpos.device
    q = qpos + offsets.double()[None]
    B = q.shape[0]
    frames = []
    for i in range(table["parent"].shape[0]):
        p, k, c = int(table["parent"][i]), int(table["kind"][i]), int(table["qidx"][i])
        T = torch.tensor(table["origin"][i].reshape(4, 4), dtype=F64, device=dev).expand(B, 4, 4)
        if p >= 0:
            T = frames[p] @ T
        if c >= 0 and k in (1, 2):
            a = torch.tensor(table["axis"][i], dtype=F64, device=dev)
            M = torch.eye(4, dtype=F64, device=dev).repeat(B, 1, 1)
            if k == 1:
                Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=F64, device=dev)
                ang = q[:, c, None, None]
                R3 = torch.eye(3, dtype=F64, device=dev) + torch.sin(ang) * Kx + (1 - torch.cos(ang)) * (Kx @ Kx)
                M = torch.cat([torch.cat([R3, torch.zeros((B, 3, 1), dtype=F64, device=dev)], 2), M[:, 3:]], 1)
            else:
                M = torch.cat([M[:, :, :3], torch.cat([a[None] * q[:, c, None], torch.ones((B, 1), dtype=F64, device=dev)],
                                                      1)[:, :, None]], 2)
            T = T @ M
        frames.append(T)
    inv = torch.linalg.inv(frames[int(table["mount"])])
    return torch.stack([inv @ frames[int(u)] for u in table["use"]], dim=1).float()


class AutogradMountedSolve(AutogradJointSolve):
    def step(self):
        self.opt.zero_grad(set_to_none=False)
        self.batch["link_poses"] = torch_fk_mounted(self.table, self.qpos, self.offsets * self.mask)
        _, ld = self.model(self.batch, with_outputs=False)
        loss = ld["mask_loss"]
        loss.backward()
        self.opt.step()
        return loss.detach()


def test_offsets_frozen_is_the_pose_only_step_bit_for_bit(env):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch, view, qp, X = _problem()
    mf, mj = make(), make()
    js = JointPoseStep(mj, batch, view, qp, offset_lr=0.0)
    assert js.kinematics.mount == (8, 127) and js.free_joints == [0, 1, 2, 3, 4, 5]
    fs = FusedPoseStep(mf, dict(batch, link_poses=js.corrected_link_poses()))
    for it in range(5):
        lf, lj = float(fs.step()), float(js.step())
        same = torch.equal(mf.dof.detach(), mj.dof.detach())
        print(f"[mounted] step {it}: loss {lf!r} / {lj!r}, dof {'equal' if same else 'DIFFER'}")
        assert lf == lj and same and np.isfinite(lf), it
    assert float(js.offsets.abs().max()) == 0.0 and float(js.offset_grad.abs().max()) > 0.0


def test_chain_tracks_autograd_through_differentiable_mounted_kinematics(env):
    """The bars of test_chain_tracks_autograd_through_differentiable_kinematics, unchanged: 5e-5 for steps 0..2, 1e-2 after,
    on the 4 views of the scene (measured: profiles/mounted.md)."""
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch, view, qp, X = _problem()
    table = view.joint_table()
    ma, mj = make(), make()
    js = JointPoseStep(mj, batch, view, qp)
    free = js.free_joints
    assert free == [0, 1, 2, 3, 4, 5]
    ref = AutogradMountedSolve(ma, batch, table, qp, free)
    moved = 0.0
    for it in range(12):
        la, lj = float(ref.step()), float(js.step())
        d_dof = float((ma.dof.detach() - mj.dof.detach()).abs().max())
        d_off = float((ref.offsets.detach() - js.offsets).abs().max())
        moved = max(moved, float(js.offsets.abs().max()))
        print(f"[mounted] step {it}: loss {la:.4f} / {lj:.4f} | max |d dof| {d_dof:.2e} | max |d offsets| {d_off:.2e}")
        bar = 5e-5 if it < 3 else 1e-2
        assert d_dof <= bar and d_off <= bar, (it, d_dof, d_off)
    assert moved > 1e-3 and float(js.offsets[6:].abs().max()) == 0.0
    assert int(js.offset_step_t) == 12 and int(js.step_t) == 12
    assert float(js.offset_grad[6]) == 0.0 and float(js.offset_grad[:6].abs().max()) > 0.0


def _pose_errors(model, X):
    """(translation error [m], rotation error [deg]) of the model's pose against X."""
    from easyhec_amd.se3 import se3_exp_map
    T = se3_exp_map(model.dof.detach()[None].cpu().double()).permute(0, 2, 1)[0].numpy()
    D = np.linalg.inv(np.asarray(X)) @ T
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(D[:3, 3])), float(ang)


INJECTED_JOINT, INJECTED_DEG = 3, 1.0


def test_solve_lm_recovers_the_pose(env):
    """1 cm and 2 degrees off in X, a zero error of 1 degree on joint 3.  The reached figures are printed, not asserted."""
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.lm import solve_lm
    true = np.zeros(9)
    true[INJECTED_JOINT] = np.radians(INJECTED_DEG)
    cfg, make, batch, view, qp, X = _problem(offsets_true=true)
    model = make()
    t0, r0 = _pose_errors(model, X)
    assert abs(t0 - 0.01) <= 5e-4 and abs(r0 - 2.0) <= 0.1, (t0, r0)
    js = JointPoseStep(model, batch, view, qp)
    assert INJECTED_JOINT in js.free_joints
    res = solve_lm(js, max_iters=40)
    traj = res.trajectory
    accepted = traj[traj[:, 1] > 0, 0]
    t1, r1 = _pose_errors(model, X)
    off = js.offsets.cpu().numpy()
    print(f"[mounted] solve_lm: loss {traj[0, 0]:.2f} -> {res.loss:.2f} in {res.iterations} iterations ({res.accepted} accepted, "
          f"{res.rejected} rejected, {res.reported} reported, {res.why}); X error {t0 * 1e3:.2f} mm / {r0:.3f} deg -> "
          f"{t1 * 1e3:.2f} mm / {r1:.3f} deg; offset[{INJECTED_JOINT}] {np.degrees(off[INJECTED_JOINT]):.3f} deg of "
          f"{INJECTED_DEG}; offsets [deg] {np.round(np.degrees(off[:7]), 3).tolist()}")
    assert res.reported == 0 and res.recoveries == []
    assert len(accepted) >= 1 and (np.diff(accepted) <= 0).all(), "the accepted losses are not monotone"
    assert res.loss < traj[0, 0]
    assert t1 < t0 and r1 < r0


def test_the_gauge_shows_in_the_information_report(env):
    from easyhec_amd.information import information_of
    from easyhec_amd.joint_calib import JointPoseStep, mount_gauge_joint
    cfg, make, batch, view, qp, X = _problem()
    reports = {}
    for key, free in (("default", None), ("gauge", [0, 1, 2, 3, 4, 5, 6])):
        js = JointPoseStep(make(), batch, view, qp, free=free)
        js.step()
        reports[key] = rep = information_of(js)
        print(f"[mounted] information, {key} free joints {js.free_joints}:\n{rep.summary()}")
    g = mount_gauge_joint(view.joint_table())
    assert g == 6
    top = [nm for nm, _ in reports["gauge"].direction(0)[:4]]
    assert f"offset[{g}]" in top and any(f"dof[{i}]" in top for i in (3, 4, 5)), top
    # without the gauge joint the direction is absent: the default system is a principal submatrix of the other (the scaling
    # is by the diagonal), so its smallest eigenvalue can only be larger (interlacing); strictly, where the direction is gone
    assert f"offset[{g}]" not in reports["default"].names
    w_def, w_g = float(reports["default"].eigenvalues[0]), float(reports["gauge"].eigenvalues[0])
    print(f"[mounted] smallest scaled eigenvalue: default {w_def:.3e}, gauge joint freed {w_g:.3e} (ratio {w_def / w_g:.1f})")
    assert w_def > w_g


def test_information_explorer_on_the_mounted_step(env):
    from easyhec_amd.info_explorer import InformationExplorer
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.synthetic import make_mounted_views
    cfg, make, batch, view, qp, X = _problem()
    js = JointPoseStep(make(), batch, view, qp)
    js.step()
    cand, _ = make_mounted_views(view, 8, MS.scene()[2], MS.H, MS.W, X, seed=1)
    out = InformationExplorer(js).forward(cand)
    gains = out["gains"].numpy()
    print(f"[mounted] exploration: gains {np.round(gains, 3).tolist()}, picked {int(out['qpos_idx'])}")
    assert gains.shape == (8,) and np.isfinite(float(out["gain"])) and 0 <= int(out["qpos_idx"]) < 8
