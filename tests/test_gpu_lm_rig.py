"""Levenberg-Marquardt over a camera rig on the GPU (csrc/ehr_lm.hip: lm_update_rig_kernel, easyhec_amd/lm_rig.py; DESIGN.md
section 6o) against the numpy restatement of tests/lm_rig_reference.py under tests/lm_reference.py's derived bars: the update
kernel alone on synthetic systems up to the limit N = 32, one camera against the solo solve (bit for bit), the composition of
one iteration, the loss the solve reports, monotone descent on a singular system, a reported iteration, non-interference with
the rig's Adam state, the refusals, and the solve end to end on the scene where two cameras pin the offsets that one camera
does not.  tests/test_lm_rig_reference.py pins the reference and the script on the CPU.  Every figure is printed before it is
asserted; the measured ones are in profiles/lm_rig.md."""
import ctypes
import types

import numpy as np
import pytest
import torch

import information_reference as IR
import lm_reference as LR
import lm_rig_reference as RR
from test_gpu_fast import problem
from test_gpu_joint_offsets import SOLVE_STEPS, _pose_errors, _solve_scene, _views_qpos
from test_gpu_lm import DEV, Upd, _stream, compare, ref_state, t32
from test_gpu_rig import CAMERA_B, _camera_b, _two_cameras

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm, lm_rig
    assert _lib.has_lm_rig()
    return _lib, fused, dr, lm, lm_rig


def _ns(_lib, state, N):
    return Upd.ns(types.SimpleNamespace(state=state, N=N, _lib=_lib))


def _rig_params(rig):
    """The rig's parameters in the system's order: every camera's dof, then the free joints' offsets (float32)."""
    out = [cam.model.dof.detach().cpu().numpy() for cam in rig.cameras]
    out.append(rig.offsets.cpu().numpy()[list(rig.free_joints)])
    return np.concatenate(out).astype(np.float32)


def _make_rig(xarm7, free, cams=None, **kw):
    from easyhec_amd.rig_calib import RigJointStep
    cams = _two_cameras(xarm7) if cams is None else cams
    models = [make() for _, make, _, _ in cams]
    return RigJointStep(models, [b for _, _, b, _ in cams], xarm7, [q for _, _, _, q in cams], free=free, **kw)


# ---- 1. the update kernel alone ----------------------------------------------------------------------------------------------
class RigUpd:
    """The tensors one ehr_lm_update_rig works on, without a renderer."""

    def __init__(self, _lib, C, F, Bs, seed=0, lambda0=1e-3):
        self._lib, self.C, self.F, self.Bs, self.N = _lib, C, F, Bs, 6 * C + F
        rng = np.random.default_rng(100 * C + F + seed)
        self.J = 32
        self.free = sorted(rng.permutation(self.J)[:F].tolist())
        self.free_list = torch.tensor(self.free, dtype=torch.int32, device=DEV) if F else None
        self.dofs = [t32(rng.uniform(-1, 1, 6)) for _ in range(C)]
        self.offset = t32(rng.uniform(-0.05, 0.05, self.J))
        self.offset0 = self.offset.clone()
        st = np.zeros(_lib.LM_STATE_DOUBLES)
        st[0], st[1] = lambda0, 2.0
        self.state = torch.from_numpy(st).to(DEV)
        self.log = torch.full((64, 4), float("nan"), dtype=torch.float64, device=DEV)

    def params(self):
        return np.concatenate([d.cpu().numpy() for d in self.dofs] + [self.offset.cpu().numpy()[self.free]]).astype(np.float32)

    def call(self, cams, ftol=RR.FTOL, lambda_max=1e6, finalize=0):
        _lib = self._lib
        dev = [(torch.tensor(np.ascontiguousarray(i, np.float64), device=DEV), torch.tensor(np.ascontiguousarray(g, np.float64), device=DEV),
                torch.tensor(np.ascontiguousarray(c, np.int64), device=DEV), t32(l)) for i, g, c, l in cams]
        arr = (_lib.LmRigCamera * self.C)(*[_lib.LmRigCamera(i.data_ptr(), g.data_ptr(), c.data_ptr(), l.data_ptr(), d.data_ptr(), B)
                                            for (i, g, c, l), d, B in zip(dev, self.dofs, self.Bs)])
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update_rig(
                arr, self.C, _lib.ptr(self.offset if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                ctypes.c_double(ftol), ctypes.c_double(lambda_max), finalize, _lib.ptr(self.state), _lib.ptr(self.log), 64,
                _stream()), "ehr_lm_update_rig")
            for i, g, c, l in dev:   # the call has read its inputs when the next one starts: garbage proves nothing is read later
                i.fill_(float("nan")), g.fill_(float("nan")), l.fill_(float("nan")), c.fill_(-7)
        torch.cuda.synchronize()
        return _ns(_lib, self.state, self.N)


def _rig_update_sequence(_lib, C, F, Bs, worst):
    u = RigUpd(_lib, C, F, Bs)
    accepted, z = None, RR.zeroed_parameter(C, F)
    for what, cams in RR.scripted_calls(C, F, Bs):
        before, now = ref_state(_ns(_lib, u.state, u.N)), u.params()
        fin = what == "finalize"
        raw = u.state.cpu().numpy().copy()
        ns = u.call(cams, finalize=int(fin))
        want = RR.update_rig(before, cams, now, RR.FTOL, 1e6, fin)
        compare(ns, before, u.params(), want, f"C={C} F={F} {what}", worst)
        if what in ("nan-loss", "bad-count", "finalize"):   # every camera's pose and the offsets: the accepted ones, bit for bit
            assert u.params().tobytes() == accepted.tobytes() == want.tobytes(), what
            assert fin or ns.last == -1
            assert ns.__dict__["lambda"] == before.lam
        if fin:
            assert ns.raw.tobytes() == raw.tobytes()
        if ns.last == 1 and not fin:
            accepted = ns.theta.astype(np.float32)
        if what == "reject":
            assert ns.rejected == 1 and ns.nu == 4.0 and (ns.H == before.H).all() and (u.params() != accepted).any()
        if what == "zero-diagonal":
            assert ns.H[z, z] == 0.0 and ns.delta[z] == 0.0 and u.params()[z] == accepted[z]
            assert (np.delete(ns.delta, z) != 0).all()
    assert (ns.accepted, ns.rejected, ns.reported, ns.iterations, ns.done) == (3, 1, 2, 6, 0)
    for a in range(C):           # the blocks between two different cameras' poses: exactly zero in H_acc
        for b in range(C):
            if a != b:
                assert (ns.H[6 * a:6 * a + 6, 6 * b:6 * b + 6] == 0).all()
    log = u.log.cpu().numpy()[:6]
    assert log[:, 1].tolist() == [1, 1, 0, -1, -1, 1] and np.isnan(log[3:5, 0]).all() and np.isnan(u.log.cpu().numpy()[6:]).all()
    keep = [j for j in range(u.J) if j not in u.free]        # the joints that are not free stay
    assert torch.equal(u.offset[keep], u.offset0[keep])
    return u


@pytest.mark.parametrize("C,F,Bs", RR.SHAPES)
def test_update_kernel_alone(env, C, F, Bs):
    _lib = env[0]
    worst = [0.0, 0.0]
    a = _rig_update_sequence(_lib, C, F, Bs, worst)
    print(f"[lm rig update] C={C} F={F} B={Bs} (N={6 * C + F}): worst |y - y_ref| / (32 2^-53 cond |y|) = {worst[0]:.4f}, "
          f"the same for pred = {worst[1]:.4f}")
    b = _rig_update_sequence(_lib, C, F, Bs, [0.0, 0.0])                           # two runs: identical bits
    for x, y in [(a.state, b.state), (a.offset, b.offset), (a.log, b.log)] + list(zip(a.dofs, b.dofs)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_update_entry_refuses_bad_arguments(env):
    """The cameras' array is a host array: the entry point judges every field before anything is launched."""
    _lib = env[0]
    u = RigUpd(_lib, 2, 1, [1, 2])
    untouched = u.state.clone()
    t = [torch.zeros(8, dtype=torch.float64, device=DEV) for _ in range(5)]
    for what, n, match in (("no camera", 0, "1 <= C"), ("B_1 = 0", 2, "camera 1 has B 0 < 1"), ("a NULL pointer", 2, "camera 1 has a NULL pointer"),
                           ("N = 37", 6, "N = 37")):
        arr = (_lib.LmRigCamera * max(n, 1))(*[_lib.LmRigCamera(*[x.data_ptr() for x in t], 1) for _ in range(max(n, 1))])
        if what == "B_1 = 0":
            arr[1].B = 0
        if what == "a NULL pointer":
            arr[1].loss = None
        rc = _lib.lib().ehr_lm_update_rig(arr, n, _lib.ptr(u.offset), _lib.ptr(u.free_list), 1, u.J, ctypes.c_double(1e-6),
                                          ctypes.c_double(1e6), 0, _lib.ptr(u.state), None, 0, _stream())
        msg = _lib.lib().ehr_last_error().decode()
        print(f"[lm rig update] refused ({what}): code {rc}: {msg}")
        assert rc != 0 and match in msg
    rc = _lib.lib().ehr_lm_update_rig(None, 1, _lib.ptr(u.offset), _lib.ptr(u.free_list), 1, u.J, ctypes.c_double(1e-6),
                                      ctypes.c_double(1e6), 0, _lib.ptr(u.state), None, 0, _stream())
    assert rc != 0 and "NULL" in _lib.lib().ehr_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(u.state, untouched)


# ---- 2. one camera is the solo solve -----------------------------------------------------------------------------------------
def test_one_camera_rig_is_the_solo_solve_bit_for_bit(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    mj, mr = make(), make()
    js = JointPoseStep(mj, batch, xarm7, qp, free=[1, 2, 3])
    rig = RigJointStep([mr], [batch], xarm7, [qp], free=[1, 2, 3])
    a = lm.LevenbergMarquardt(js).iterate(8).finalize()
    b = lm_rig.RigLM(rig).iterate(8).finalize()
    torch.cuda.synchronize()
    fused.check_status(js.glctx), fused.check_status(rig.cameras[0].glctx)
    sa, sb = a.state(), b.state()
    print(f"[lm rig C=1] solo: F_acc {sa.F_acc!r}, {sa.accepted} accepted of {sa.iterations}; rig: F_acc {sb.F_acc!r}, "
          f"{sb.accepted} accepted of {sb.iterations}")
    assert a.state_block.shape == b.state_block.shape == (_lib.LM_STATE_DOUBLES,) == (1136,)
    assert b.names == [f"cam0.dof[{i}]" for i in range(6)] + ["offset[1]", "offset[2]", "offset[3]"]
    for what, x, y in (("state block", a.state_block, b.state_block), ("log", a.log, b.log), ("dof", mj.dof.detach(), mr.dof.detach()),
                       ("offsets", js.offsets, rig.offsets), ("link_poses", js.link_poses, rig.cameras[0].link_poses)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), what
    assert sa.accepted >= 2 and sa.iterations == 8


# ---- 3. composition ----------------------------------------------------------------------------------------------------------
def test_iterate_is_its_pieces(env, xarm7):
    """Three consecutive iterations, each against: per camera ehr_joint_forward, ehr_lm_linearize into buffers of the test's
    own and mask_information on them; then the reference update from the GPU's own previous state."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd import information
    rig = _make_rig(xarm7, [1, 3])
    o = lm_rig.RigLM(rig)
    assert o.N == 14 and [u.B for u in o.units] == [2, 3] and [(u.H, u.W) for u in o.units] == [(120, 160), (96, 128)]
    worst = [0.0, 0.0]
    for it in range(3):
        before, now = ref_state(_ns(_lib, o.state_block, o.N)), _rig_params(rig)
        mine, own = [], []
        for u in o.units:
            keep = (u.mvp, u.dmvp)
            u.mvp, u.dmvp = torch.empty_like(keep[0]), torch.empty_like(keep[1])
            with torch.cuda.device(DEV):
                u._forward_kinematics(_stream())
                u._linearize(_stream())
            mine.append(information.mask_information(u.glctx, u.scene, u.mvp, u.dmvp, u.ref, want_loss=True))
            own.append((u.mvp, u.dmvp))
            u.mvp, u.dmvp = keep
        o.iterate(1)
        torch.cuda.synchronize()
        for c, (u, m, (own_mvp, own_dmvp)) in enumerate(zip(o.units, mine, own)):
            fused.check_status(u.glctx)
            assert torch.equal(own_mvp, u.mvp) and torch.equal(own_dmvp, u.dmvp), c
            for x, y in ((m.info, u.out.info), (m.grad, u.out.grad), (m.count, u.out.count), (m.loss, u.out.loss)):
                assert torch.equal(x, y), c
        cams = [(m.info.cpu().numpy(), m.grad.cpu().numpy(), m.count.cpu().numpy(), m.loss.cpu().numpy()) for m in mine]
        want = RR.update_rig(before, cams, now)
        compare(_ns(_lib, o.state_block, o.N), before, _rig_params(rig), want, f"rig iteration {it}", worst)
    s = o.state()
    print(f"[lm rig composition] worst delta / pred ratios {worst[0]:.4f}, {worst[1]:.4f}; F_acc {s.F_acc:.3f}, {s.accepted} accepted")
    assert s.accepted >= 1 and s.iterations == 3


# ---- 4. the loss is the solve's loss -----------------------------------------------------------------------------------------
def _loss_at_accepted(fused, dr, o, weighted=True):
    """sum_c (sum_b (double) loss) of render_mask_loss (another context) on the linearize kernel's mvp at the rig's parameters,
    in the update's order; and the per-camera sums."""
    F, per = 0.0, []
    for u in o.units:
        with torch.cuda.device(DEV):
            u._forward_kinematics(_stream())
            u._linearize(_stream())
        w = u.weight.clone() if (weighted and u.weight is not None) else None
        _, loss = fused.render_mask_loss(dr.RasterizeCudaContext(), u.scene, u.mvp.clone(), u.ref.clone(), want_mask=False, weight=w)
        torch.cuda.synchronize()
        Fc = 0.0
        for x in loss.detach().cpu().numpy():
            Fc += float(x)
        per.append(Fc)
        F += Fc
    return F, per


def test_accepted_loss_is_render_mask_loss(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    o = lm_rig.RigLM(_make_rig(xarm7, [1, 3]))
    o.iterate(6).finalize()
    s = o.state()
    F, per = _loss_at_accepted(fused, dr, o)
    print(f"[lm rig loss] F_acc {s.F_acc!r}, render_mask_loss at the accepted parameters {F!r} = {per}; {s.accepted} accepted of "
          f"{s.iterations}")
    assert F == s.F_acc and s.accepted >= 2


# ---- 5. monotone and deterministic -------------------------------------------------------------------------------------------
def test_monotone_and_deterministic_on_a_singular_system(env, xarm7):
    """The two-camera problem without the base link and free = [0]: joint 0's zero error is a camera rotation to each camera,
    H is singular, the damping carries it."""
    _lib, fused, dr, lm, lm_rig = env
    rb = IR.robot_without_base(xarm7)
    ends = []
    for _ in range(2):
        rig = _make_rig(rb, [0], cams=_two_cameras(rb))
        o = lm_rig.RigLM(rig)
        o.iterate(20).finalize()
        s, tr = o.state(), o.trajectory()
        for cam in rig.cameras:
            fused.check_status(cam.glctx)
        ends.append((o.state_block.cpu().numpy().tobytes(), o.log.cpu().numpy().tobytes(), _rig_params(rig).tobytes()))
    acc = tr[tr[:, 1] == 1, 0]
    print(f"[lm rig monotone] accepted losses {np.round(acc, 2).tolist()}; {s.accepted} accepted, {s.rejected} rejected, "
          f"{s.reported} reported, done {s.done} ({LR.WHY[s.why]}), lambda {s.__dict__['lambda']:.3g}, "
          f"condition of the scaled H_acc {o.report(s).condition:.3g}")
    assert (np.diff(acc) < 0).all() and len(acc) >= 2 and acc[-1] == s.F_acc       # (two: at least one real descent step)
    assert s.accepted + s.rejected + s.reported == s.iterations and (s.iterations == 20 or s.done)
    p = _rig_params(rig)
    assert np.isfinite(p).all() and (p == s.theta.astype(np.float32)).all()
    assert ends[0] == ends[1]


# ---- 6. a reported iteration -------------------------------------------------------------------------------------------------
def test_reported_iteration_is_rig_wide_and_recovered(env, xarm7, monkeypatch):
    """test_gpu_rig.py's close-up under a slot-limited plan on camera 0: the first iterations are reported for the whole rig,
    camera 0's plan is made again with every slot, and the solve ends on the bits of a solve that had every slot."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.rig_calib import RigJointStep
    from test_gpu_fused import workload
    H, W, B = 64, 96, 2
    K, lp, Tc, _ = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=DEV)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=DEV),
             "K": torch.tensor(K, dtype=torch.float32, device=DEV)[None].repeat(B, 1, 1)}
    qp = _views_qpos(xarm7, B, seed=3)
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    ends = []
    for slack in ([None, 0.0], [0.0, 0.0]):
        models = [RBSolver(cfg, meshes=xarm7.meshes).to(DEV) for _ in range(2)]
        rig = RigJointStep(models, [batch, batch], xarm7, [qp, qp], slack=slack)
        res = lm_rig.solve_lm_rig(rig, max_iters=6, check_every=2)
        if slack[0] is None:
            assert res.reported >= 1 and res.recoveries == ["camera 0: job slots"] and [c.slack for c in rig.cameras] == [0.0, 0.0]
        else:
            assert res.reported == 0 and res.recoveries == []
        assert res.iterations - res.reported >= 6 or res.done
        ends.append(([m.dof.detach().clone() for m in models], rig.offsets.clone(), res))
    a, b = ends[0][2], ends[1][2]
    print(f"[lm rig reported] limited plan: {a.reported} reported of {a.iterations}, F_acc {a.loss:.3f}, recoveries {a.recoveries}; "
          f"every slot: {b.iterations} iterations, F_acc {b.loss:.3f}")
    assert all(torch.equal(x, y) for x, y in zip(ends[0][0], ends[1][0])) and torch.equal(ends[0][1], ends[1][1])
    assert a.loss == b.loss and (a.state.theta == b.state.theta).all() and (a.state.H == b.state.H).all()
    assert a.state.__dict__["lambda"] == b.state.__dict__["lambda"] and a.accepted == b.accepted


# ---- 7. beside Adam ----------------------------------------------------------------------------------------------------------
def test_lm_leaves_the_rigs_adam_state_alone_and_honours_weights(env, xarm7):
    _lib, fused, dr, lm, lm_rig = env
    cams = _two_cameras(xarm7)
    cfg1, make1, batch1, qp1 = cams[1]
    w = torch.ones_like(batch1["mask"])
    w[:, :, :w.shape[2] // 2] = 0.0                                                # half of camera 1's pixels do not count
    cams[1] = (cfg1, make1, dict(batch1, weight=w), qp1)
    rig = _make_rig(xarm7, [1, 2, 3], cams=cams)
    for _ in range(5):
        rig.step()
    torch.cuda.synchronize()

    def snap():
        s = [rig.offset_exp_avg.clone(), rig.offset_exp_avg_sq.clone(), rig.offset_step_t.clone()]
        for cam in rig.cameras:
            s += [cam.exp_avg.clone(), cam.exp_avg_sq.clone(), cam.step_t.clone(), cam.hist_row.clone(), cam.model.history_ops.clone()]
        return s

    a = snap()
    res = lm_rig.solve_lm_rig(rig, max_iters=5)
    torch.cuda.synchronize()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y)
    Fw, per_w = _loss_at_accepted(fused, dr, res.lm)
    F1, per_1 = _loss_at_accepted(fused, dr, res.lm, weighted=False)
    print(f"[lm rig beside Adam] F_acc {res.loss!r}; weighted render_mask_loss {Fw!r} = {per_w}; unweighted {F1!r} = {per_1}; "
          f"{res.accepted} accepted of {res.iterations}")
    assert res.accepted >= 1 and int(rig.offset_step_t) == 5 and [int(cam.step_t) for cam in rig.cameras] == [5, 5]
    assert res.loss == Fw and per_w[0] == per_1[0] and per_w[1] < per_1[1]
    assert res.report.names == [f"cam{c}.dof[{i}]" for c in range(2) for i in range(6)] + [f"offset[{j}]" for j in (1, 2, 3)]
    assert res.report.loss == res.loss and res.report.count > 0 and (res.report.H == res.state.H).all()
    assert (_rig_params(rig) == res.state.theta.astype(np.float32)).all()
    losses = torch.stack([rig.step().clone() for _ in range(5)])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(losses).all()) and int(rig.offset_step_t) == 10 and [int(cam.step_t) for cam in rig.cameras] == [10, 10]


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(env, xarm7, monkeypatch):
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.rig_calib import RigJointStep
    cfg, make, batch = problem(xarm7, 1, 48, 64, 0.05)
    qp = _views_qpos(xarm7, 1)
    five = RigJointStep([make() for _ in range(5)], [batch] * 5, xarm7, [qp] * 5, free=[1, 2, 3, 4, 5, 6, 7])
    with pytest.raises(ValueError, match="37 parameters.*room for 4 cameras"):
        lm_rig.RigLM(five)
    with pytest.raises(TypeError, match="not a RigJointStep"):
        lm_rig.solve_lm_rig(FusedPoseStep(make(), batch))
    rig = _make_rig(xarm7, [1, 3])
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="being captured"):
        lm_rig.solve_lm_rig(rig)
    monkeypatch.undo()
    o = lm_rig.RigLM(rig)
    cam1 = rig.cameras[1]
    fused._ensure_plan(cam1.glctx, cam1.scene, 1, cam1.H, cam1.W)                # somebody else planned on camera 1's context
    with pytest.raises(RuntimeError, match="camera 1: its context holds another plan"):
        o.iterate(1)
    with pytest.raises(ValueError, match="one system over several contexts.*solve_lm_rig"):
        lm.LevenbergMarquardt(rig)
    with pytest.raises(ValueError, match="one system over several contexts"):
        lm.solve_lm(rig)
    import easyhec_amd
    assert easyhec_amd.solve_lm_rig is lm_rig.solve_lm_rig and easyhec_amd.RigLM is lm_rig.RigLM


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------
def test_end_to_end_from_the_start_and_after_adam(env, xarm7):
    """The scene of test_gpu_rig.py::test_two_cameras_pin_the_offsets_that_one_camera_does_not (camera A 320x240, camera B a
    quarter turn away at 256x192, 4 views each, injected zero errors on joints 1, 2, 3, 5, the default free set 1..6).
    (a) solve_lm_rig from the perturbed start, no Adam; (b) solve_lm_rig after solve_rig's SOLVE_STEPS Adam steps.  The accept
    rule is the contract: the loss falls and never rises.  The offset and pose errors are printed (profiles/lm_rig.md), not
    asserted: the silhouette model's H does not promise them."""
    _lib, fused, dr, lm, lm_rig = env
    from easyhec_amd.rig_calib import RigJointStep, solve_rig
    cfg, make_a, batch_a, qp_a, truth, Tc_a, _, _ = _solve_scene(xarm7)
    _, make_b, batch_b, qp_b, Tc_b = _camera_b(xarm7, truth, 4, **CAMERA_B)
    batches, qps, Tcs = [batch_a, batch_b], [qp_a, qp_b], [Tc_a, Tc_b]

    def errors(who, rig):
        off = float(np.abs(rig.offsets.cpu().numpy().astype(np.float64) - truth).max())
        pe = [_pose_errors(cam.model, Tc) for cam, Tc in zip(rig.cameras, Tcs)]
        print(f"[lm rig end to end] {who}: worst offset error {np.degrees(off):.3f} deg | "
              + " | ".join(f"camera {c}: trans {t * 1e3:.2f} mm rot {r:.3f} deg" for c, (t, r) in enumerate(pe)))

    def check(who, res, strict):
        tr = res.trajectory
        first, acc = tr[0, 0], tr[tr[:, 1] == 1, 0]
        print(f"[lm rig end to end] {who}: first evaluation {first:.2f} -> F_acc {res.loss:.2f} in {res.iterations} iterations "
              f"({res.accepted} accepted, {res.rejected} rejected, {res.reported} reported), stopped by {res.why}")
        assert (np.diff(acc) < 0).all() and acc[-1] == res.loss
        assert res.loss < first if strict else res.loss <= first

    # (a) from the perturbed start
    rig = RigJointStep([make_a(), make_b()], batches, xarm7, qps)
    assert rig.free_joints == [1, 2, 3, 4, 5, 6]
    errors("(a) start", rig)
    res = lm_rig.solve_lm_rig(rig, max_iters=30)
    errors("(a) after solve_lm_rig", rig)
    check("(a)", res, True)
    assert res.accepted >= 2
    # (b) the polish after Adam
    adam = solve_rig(cfg, [make_a(), make_b()], batches, xarm7, SOLVE_STEPS, qpos=qps)
    errors("(b) after solve_rig", adam.step)
    res = lm_rig.solve_lm_rig(adam.step)
    errors("(b) after solve_lm_rig", adam.step)
    check("(b)", res, False)
    assert res.done
