"""Joint-offset calibration on the GPU (csrc/ehr_joint.hip, easyhec_amd/joint_calib.py): the two kernels against the float64
reference of tests/joint_reference.py, the launch chain with them against torch autograd through a differentiable forward
kinematics, graph capture, checkpoints, reported steps, and a solve with injected joint zero errors.

Tolerances.  link_poses: one float32 unit of max(1, |x|) around the float64 reference rounded to float32 (the kernel works in
float64 and rounds once).  joint_frames, offset gradients and Adam: the pose head's rule (tests/test_gpu_pose_head.py),
|Xhip - X64| / s <= 4 e32 + 8 * 2^-23 with e32 from the same reference text run in float32.  Trajectories against autograd:
the bars of test_gpu_fast.py::test_fast_step_tracks_autograd_step.  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import joint_reference as JR
import pose_reference as R
from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U = R.U


def _f(x):
    return ctypes.c_float(float(x))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _robot(name):
    from easyhec_amd.robot import load_robot
    return load_robot(name)


@functools.lru_cache(maxsize=None)
def _table(name, every=False):
    rb = _robot(name)
    return rb.chain.joint_table(range(len(rb.chain.link_order))) if every else rb.joint_table()


TABLES = [("xarm7", False), ("franka", False), ("xarm7", True)]  # (the table of EVERY link reaches the prismatic fingers)


def _qpos(name, B, seed):
    rb = _robot(name)
    lim = rb.chain.limits()
    return np.random.default_rng(seed).uniform(lim[:, 0], lim[:, 1], size=(B, rb.chain.dof))


def _dev_table(t):
    return {k: _dev(np.asarray(t[k]).astype(dt)) for k, dt in (("parent", np.int32), ("origin", np.float64), ("kind", np.int32),
                                                               ("axis", np.float64), ("qidx", np.int32), ("use", np.int32))}


def _forward(t, q, off):
    from easyhec_amd import _lib
    d = _dev_table(t)
    B, J = q.shape
    N, L = t["parent"].shape[0], t["use"].shape[0]
    lp = torch.full((B, L, 4, 4), float("nan"), device="cuda:0")
    jf = torch.full((B, J, 6), float("nan"), device="cuda:0")
    qd, od = _dev(q.astype(np.float64)), _dev(off.astype(np.float32))
    _lib.check(_lib.lib().ehr_joint_forward(_lib.ptr(d["parent"]), _lib.ptr(d["origin"]), _lib.ptr(d["kind"]),
                                            _lib.ptr(d["axis"]), _lib.ptr(d["qidx"]), _lib.ptr(d["use"]), N, J, L,
                                            _lib.ptr(qd), _lib.ptr(od), B, _lib.ptr(lp), _lib.ptr(jf), _stream()), "fwd")
    torch.cuda.synchronize()
    return lp, jf


class _Bwd:
    """Device state of one offsets' Adam group and one call of ehr_joint_backward_adam on it."""

    def __init__(self, t, p, m, v, step, free):
        J = len(p)
        self.J = J
        self.p, self.m, self.v = (_dev(np.asarray(x, np.float32)) for x in (p, m, v))
        self.t = torch.tensor([int(step)], dtype=torch.int32, device="cuda:0")
        self.free = _dev(np.asarray(free, np.int32))
        self.up = _dev(np.asarray(t["upstream"]).astype(np.uint32).view(np.int32))
        self.jk = _dev(JR.joint_kinds(t))
        self.grad = torch.full((J,), 12345.0, device="cuda:0")

    def step(self, g, tc_jac, K, H, W, near, far, lp, jf, red, hyper, sync=True):
        from easyhec_amd import _lib
        B, L = lp.shape[:2]
        lr, b1, b2, eps, wd = hyper
        self.keep = (g, tc_jac, K, lp, jf, red)
        _lib.check(_lib.lib().ehr_joint_backward_adam(
            _lib.ptr(g), _lib.ptr(tc_jac), _lib.ptr(K), B, L, self.J, H, W, _f(near), _f(far), _lib.ptr(lp), _lib.ptr(jf),
            _lib.ptr(self.up), _lib.ptr(self.jk), _lib.ptr(red), _lib.ptr(self.free), _lib.ptr(self.p), _lib.ptr(self.m),
            _lib.ptr(self.v), _lib.ptr(self.t), _f(lr), _f(b1), _f(b2), _f(eps), _f(wd), _lib.ptr(self.grad), _stream()),
            "bwd")
        if sync:
            torch.cuda.synchronize()
            return self.state()

    def state(self):
        return (self.p.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(), int(self.t.item()), self.grad.cpu().numpy())


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


# ---- 1. forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,every", TABLES)
def test_forward_kinematics_and_joint_frames(name, every):
    t, rb = _table(name, every), _robot(name)
    J = rb.chain.dof
    rows, bad = [], []
    for B in (1, 3, 70):  # 70 views of 8 links: more than one chunk of the solver step, which this kernel does not care about
        q = _qpos(name, B, 10 + B)
        rng = np.random.default_rng(B)
        kinds = JR.joint_kinds(t)
        rnd = np.where(kinds == 2, rng.uniform(-0.005, 0.005, J), rng.uniform(-0.1, 0.1, J)).astype(np.float32)
        for what, off in (("zero", np.zeros(J, np.float32)), ("random", rnd)):
            lp, jf = _forward(t, q, off)
            lp, jf = lp.cpu().numpy(), jf.cpu().numpy()
            _, lp64, jf64 = JR.fk(t, q, off)
            _, _, jf32 = JR.fk(t, q, off, dtype=F32)
            if what == "zero":  # the host's own float64 kinematics, not only the table's
                links = list(range(len(rb.chain.link_order))) if every else rb.use_links
                assert np.abs(lp64 - rb.chain.link_poses_batch(q, links)).max() <= 1e-12
            want = lp64.astype(np.float32)
            d_lp = float((np.abs(lp.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max())
            s = float(np.abs(jf64).max())
            e32, eh = R.rel_err(jf32, jf64, s), R.rel_err(jf, jf64, s)
            same = float((lp.view(np.uint32) == want.view(np.uint32)).mean())
            print(f"{name} every={every} B={B} {what}: link_poses worst {d_lp / U:.2f} units ({same:.4f} bit-equal) | "
                  f"joint_frames e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e}")
            if not (d_lp <= U and eh <= R.bound(e32) and np.isfinite(lp).all() and np.isfinite(jf).all()):
                bad.append((B, what, d_lp, eh))
    assert not bad, bad


# ---- 2. backward -----------------------------------------------------------------------------------------------------------
def _bwd_case(name, every, B, draw):
    t = _table(name, every)
    J, L = _robot(name).chain.dof, t["use"].shape[0]
    rng = np.random.default_rng(7000 + 100 * B + draw + (50 if every else 0) + (25 if name == "franka" else 0))
    q = _qpos(name, B, 30 + B + draw)
    off = rng.uniform(-0.05, 0.05, J).astype(np.float32)
    g = rng.normal(size=(B, L, 4, 4))
    g *= np.where(rng.uniform(size=(B, L, 1, 1)) < 0.2, 1e6, 1.0)       # some pairs a million times the others
    K, H, W = R.CAMERAS[draw % 2]
    near, far = R.NEAR_FAR[(draw + B) % 2]
    Tc = R.random_rigid(rng, 1)[0]
    free = np.ones(J, np.int32)
    free[[0, J - 2]] = 0
    return dict(t=t, J=J, L=L, B=B, q=q, off=off, g=g.astype(np.float32), K=K, H=H, W=W, near=near, far=far, Tc=Tc, free=free)


def _run_bwd(c, red, state=None, hyper=None):
    lp, jf = _forward(c["t"], c["q"], c["off"])
    tc_jac = torch.full((7, 16), float("nan"), device="cuda:0")
    tc_jac[0] = _dev(c["Tc"].reshape(16))
    J = c["J"]
    p, m, v, step = state if state is not None else (c["off"], np.zeros(J), np.zeros(J), 0)
    b = _Bwd(c["t"], p, m, v, step, c["free"])
    out = b.step(_dev(c["g"]), tc_jac, _dev(c["K"]), c["H"], c["W"], c["near"], c["far"], lp, jf, _dev(red),
                 hyper or R.hyper32("default"))
    return out, lp.cpu().numpy(), jf.cpu().numpy()


@pytest.mark.parametrize("name,every", TABLES)
def test_offset_gradient_against_the_float64_reference(name, every):
    bad = []
    for B in (1, 5, 70):
        e32, eh = 0.0, 0.0
        for draw in range(2):
            c = _bwd_case(name, every, B, draw)
            red = np.array([1, 2, 3, 4, 5, 6, 7, 1], np.float32)      # red[7] = 1: grad_out is the sum itself
            (p, m, v, step, grad), lp, jf = _run_bwd(c, red)
            (_, _, _, _, grad2), _, _ = _run_bwd(c, red)
            assert np.array_equal(_bits(grad), _bits(grad2)), "two runs differ"
            args = (c["t"], c["g"], c["Tc"], c["K"], c["H"], c["W"], c["near"], c["far"], lp, jf)
            s64, scale = JR.offset_gradient(*args)
            s32, _ = JR.offset_gradient(*args, dtype=F32)
            fr = c["free"].astype(bool)
            assert step == 1 and np.isfinite(grad).all()
            assert (grad[~fr] == 0).all() and not np.signbit(grad[~fr]).any(), grad      # exactly 0 where not free
            assert (np.abs(s64[fr]) > 0).any()
            live = fr & (scale > 0)
            assert (grad[fr & ~live] == 0).all()
            e32 = max(e32, R.rel_err(s32[live], s64[live], scale[live]))
            eh = max(eh, R.rel_err(grad[live], s64[live], scale[live]))
        print(f"{name} every={every} B={B}: offset gradient e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e}")
        if not eh <= R.bound(e32):
            bad.append((B, e32, eh))
    assert not bad, bad


# ---- 3. Adam ---------------------------------------------------------------------------------------------------------------
QTY = ("p", "m", "v")


def _adam_errs(got, ref, e, free):
    for qi, q in enumerate(QTY):
        s = float(np.abs(ref[qi][free]).max())
        e[q] = max(e[q], R.rel_err(np.asarray(got[qi])[free], ref[qi][free], s))


def test_adam_one_step_from_a_given_state():
    """The update of the free joints from a state with 9 and with 999 steps behind it, for every hyper-parameter set of the
    pose head's sweep; the gradient the reference is given is the kernel's own grad_out (red[7] = 1: an exact quotient), so
    the update is judged alone."""
    bad = []
    for hname in R.ADAM_HYPER:
        h = R.hyper32(hname)
        for t0 in (0, 9, 999):
            e32, eh = dict.fromkeys(QTY, 0.0), dict.fromkeys(QTY, 0.0)
            for draw in range(2):
                c = _bwd_case("xarm7", False, 3, draw)
                rng = np.random.default_rng(100 * t0 + draw)
                J, fr = c["J"], c["free"].astype(bool)
                m0 = (rng.normal(size=J) * 10 * (t0 > 0)).astype(np.float32)
                v0 = (rng.uniform(1, 400, size=J) * (t0 > 0)).astype(np.float32)
                red = np.array([0, 0, 0, 0, 0, 0, 5, 1], np.float32)
                got, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, t0), hyper=h)
                assert got[3] == t0 + 1
                r64 = JR.adam_step(c["off"], m0, v0, t0, got[4], red, fr, *h)
                r32 = JR.adam_step(c["off"], m0, v0, t0, got[4], red, fr, *h, dtype=F32)
                assert np.array_equal(_bits(got[4][fr]), _bits(r64[4][fr]))
                for qi, x0 in enumerate((c["off"], m0, v0)):   # a joint that is not free keeps its bits
                    assert np.array_equal(_bits(got[qi][~fr]), _bits(x0[~fr]))
                _adam_errs(r32, r64, e32, fr)
                _adam_errs(got, r64, eh, fr)
            for q in QTY:
                ok = eh[q] <= R.bound(e32[q])
                print(f"adam one step {hname} t0={t0} {q}: e32 {e32[q]:.2e} hip {eh[q]:.2e} bound {R.bound(e32[q]):.2e} {'ok' if ok else 'FAIL'}")
                if not ok:
                    bad.append((hname, t0, q, e32[q], eh[q]))
    assert not bad, bad


def test_adam_trajectory_of_200_steps():
    """200 steps on a synthetic gradient: grad_mvp of step k is one random draw times +-2^e_k (exact scalings), the reference
    trajectory is fed the kernel's own grad_out of every step."""
    c = _bwd_case("franka", False, 5, 0)
    h = R.hyper32("default")
    J, fr = c["J"], c["free"].astype(bool)
    rng = np.random.default_rng(11)
    lp, jf = _forward(c["t"], c["q"], c["off"])
    tc_jac = torch.zeros((7, 16), device="cuda:0")
    tc_jac[0] = _dev(c["Tc"].reshape(16))
    b = _Bwd(c["t"], c["off"], np.zeros(J), np.zeros(J), 0, c["free"])
    red = _dev(np.array([0, 0, 0, 0, 0, 0, 5, 1], np.float32))
    g0, K = _dev(c["g"] * np.float32(1e-4)), _dev(c["K"])
    scal = (2.0 ** rng.integers(-3, 4, size=200)) * rng.choice([-1.0, 1.0], size=200)
    grads, snaps, keep = [], {}, []
    for k in range(200):  # no synchronisation inside
        gk = g0 * float(scal[k])
        keep.append(gk)
        b.step(gk, tc_jac, K, c["H"], c["W"], c["near"], c["far"], lp, jf, red, h, sync=False)
        grads.append(b.grad.clone())
        if k + 1 in (1, 10, 100, 200):
            snaps[k + 1] = (b.p.clone(), b.m.clone(), b.v.clone(), b.t.clone())
    torch.cuda.synchronize()
    grads = torch.stack(grads).cpu().numpy()
    assert np.isfinite(grads).all() and (np.abs(grads[:, fr]) > 0).any()
    st = {F64: (c["off"].astype(np.float64), np.zeros(J), np.zeros(J)), F32: (c["off"], np.zeros(J, np.float32), np.zeros(J, np.float32))}
    bad = []
    for k in range(200):
        for dt in (F64, F32):
            st[dt] = JR.adam_step(*st[dt], k, grads[k], [0, 0, 0, 0, 0, 0, 5, 1], fr, *h, dtype=dt)[:3]
        if k + 1 in snaps:
            got = [x.cpu().numpy() for x in snaps[k + 1][:3]]
            assert int(snaps[k + 1][3].item()) == k + 1
            e32, eh = dict.fromkeys(QTY, 0.0), dict.fromkeys(QTY, 0.0)
            _adam_errs(st[F32], st[F64], e32, fr)
            _adam_errs(got, st[F64], eh, fr)
            assert np.array_equal(_bits(got[0][~fr]), _bits(c["off"][~fr])) and (got[1][~fr] == 0).all() and (got[2][~fr] == 0).all()
            for q in QTY:
                ok = eh[q] <= R.bound(e32[q])
                print(f"adam trajectory step {k + 1} {q}: e32 {e32[q]:.2e} hip {eh[q]:.2e} bound {R.bound(e32[q]):.2e} {'ok' if ok else 'FAIL'}")
                if not ok:
                    bad.append((k + 1, q, e32[q], eh[q]))
    assert not bad, bad


@pytest.mark.parametrize("slot,value", [(0, float("nan")), (6, float("inf")), (2, float("-inf")), (7, float("nan")),
                                        (3, 3.1e38), (7, float("inf"))])
def test_non_finite_red_leaves_offsets_moments_and_counter_alone(slot, value):
    c = _bwd_case("xarm7", False, 3, 1)
    J, fr = c["J"], c["free"].astype(bool)
    rng = np.random.default_rng(5)
    m0, v0 = rng.normal(size=J).astype(np.float32), rng.uniform(1, 4, size=J).astype(np.float32)
    red = np.array([1, 2, 3, 4, 5, 6, 7, 3], np.float32)
    clean, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, 9))
    assert clean[3] == 10 and not np.array_equal(_bits(clean[0][fr]), _bits(c["off"][fr]))
    red[slot] = np.float32(value)
    got, _, _ = _run_bwd(c, red, state=(c["off"], m0, v0, 9))
    assert np.array_equal(_bits(got[0]), _bits(c["off"])) and np.array_equal(_bits(got[1]), _bits(m0))
    assert np.array_equal(_bits(got[2]), _bits(v0)) and got[3] == 9
    assert np.isnan(got[4][fr]).all() and (got[4][~fr] == 0).all()


# ---- the chain -------------------------------------------------------------------------------------------------------------
def torch_fk(table, qpos, offsets):
    """Differentiable forward kinematics from the flat table: qpos [B,J] float64 tensor, offsets [J] -> [B,L,4,4] float32."""
    dev = qpos.device
    q = qpos + offsets.double()[None]
    B = q.shape[0]
    eye = torch.eye(4, dtype=F64, device=dev).expand(B, 4, 4)
    frames = []
    for i in range(table["parent"].shape[0]):
        p, k, c = int(table["parent"][i]), int(table["kind"][i]), int(table["qidx"][i])
        T = (eye if p < 0 else frames[p]) @ torch.tensor(table["origin"][i].reshape(4, 4), dtype=F64, device=dev)
        if c >= 0 and k == 1:
            a = table["axis"][i]
            Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=F64, device=dev)
            ang = q[:, c, None, None]
            R3 = torch.eye(3, dtype=F64, device=dev) + torch.sin(ang) * Kx + (1 - torch.cos(ang)) * (Kx @ Kx)
            M = torch.cat([torch.cat([R3, torch.zeros((B, 3, 1), dtype=F64, device=dev)], 2),
                           torch.tensor([[[0, 0, 0, 1.0]]], dtype=F64, device=dev).expand(B, 1, 4)], 1)
            T = T @ M
        elif c >= 0 and k == 2:
            M = torch.eye(4, dtype=F64, device=dev).repeat(B, 1, 1)
            tr = torch.tensor(table["axis"][i], dtype=F64, device=dev)[None] * q[:, c, None]
            M = torch.cat([M[:, :, :3], torch.cat([tr, torch.ones((B, 1), dtype=F64, device=dev)], 1)[:, :, None]], 2)
            T = T @ M
        frames.append(T)
    return torch.stack([frames[int(u)] for u in table["use"]], dim=1).float()


class AutogradJointSolve:
    """The reference: RBSolver.forward (use_fused) on link poses from ``torch_fk``, loss.backward(), torch.optim.Adam over two
    parameter groups -- the pose and the offsets (the gradient of a joint that is not free is masked to zero)."""

    def __init__(self, model, batch, table, qpos, free, lr=0.003, wd=0.0005, offset_lr=None, offset_wd=None):
        dev = model.dof.device
        self.model, self.batch, self.table = model, dict(batch), table
        self.qpos = torch.tensor(np.asarray(qpos), dtype=F64, device=dev)
        J = self.qpos.shape[1]
        self.offsets = torch.zeros(J, device=dev, requires_grad=True)
        self.mask = torch.zeros(J, device=dev)
        self.mask[list(free)] = 1.0
        self.opt = torch.optim.Adam([{"params": [model.dof], "lr": lr, "weight_decay": wd},
                                     {"params": [self.offsets], "lr": lr if offset_lr is None else offset_lr,
                                      "weight_decay": wd if offset_wd is None else offset_wd}], lr)

    def step(self):
        self.opt.zero_grad(set_to_none=False)
        self.batch["link_poses"] = torch_fk(self.table, self.qpos, self.offsets * self.mask)
        _, ld = self.model(self.batch, with_outputs=False)
        loss = ld["mask_loss"]
        loss.backward()
        self.opt.step()
        return loss.detach()


def _views_qpos(xarm7, B, seed=0):
    from easyhec_amd.synthetic import make_views
    q, _ = make_views(xarm7, B, seed=seed)
    qp = np.zeros((B, xarm7.chain.dof))
    qp[:, :q.shape[1]] = q
    return qp


def test_chain_tracks_autograd_through_differentiable_kinematics(xarm7):
    from easyhec_amd.joint_calib import JointPoseStep, default_free_joints
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    table = xarm7.joint_table()
    free = default_free_joints(table)
    assert free == [1, 2, 3, 4, 5, 6]
    ma, mj = make(), make()
    ref = AutogradJointSolve(ma, batch, table, qp, free)
    js = JointPoseStep(mj, batch, xarm7, qp)
    moved = 0.0
    for it in range(12):
        la, lj = float(ref.step()), float(js.step())
        d_dof = float((ma.dof.detach() - mj.dof.detach()).abs().max())
        d_off = float((ref.offsets.detach() - js.offsets).abs().max())
        moved = max(moved, float(js.offsets.abs().max()))
        print(f"step {it}: loss {la:.4f} / {lj:.4f} | max |d dof| {d_dof:.2e} | max |d offsets| {d_off:.2e}")
        bar = 5e-5 if it < 3 else 1e-2
        assert d_dof <= bar and d_off <= bar, (it, d_dof, d_off)
    assert moved > 1e-3 and float(js.offsets[0]) == 0.0 and float(js.offsets[7:].abs().max()) == 0.0
    assert int(js.offset_step_t) == 12 and int(js.step_t) == 12
    assert float(js.offset_grad[0]) == 0.0 and float(js.offset_grad[1:7].abs().max()) > 0.0


def test_all_joints_frozen_reproduces_the_pose_only_step(xarm7):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    mf, mj = make(), make()
    fs = FusedPoseStep(mf, batch)
    js = JointPoseStep(mj, batch, xarm7, _views_qpos(xarm7, 2), free=[])
    torch.cuda.synchronize()
    same_lp = torch.equal(fs.link_poses, js.link_poses)
    units = float(((fs.link_poses - js.link_poses).abs() / fs.link_poses.abs().clamp(min=1)).max()) / U
    print(f"link_poses of the forward kernel {'EQUAL' if same_lp else 'DIFFER from'} the host's float32 cast (worst {units:.2f} units)")
    assert units <= 1.0
    equal = True
    for it in range(30):
        lf, lj = float(fs.step()), float(js.step())
        d = float((mf.dof.detach() - mj.dof.detach()).abs().max())
        equal = equal and d == 0.0 and lf == lj
        bar = 5e-5 if it < 3 else 1e-2
        assert d <= bar and abs(lf - lj) <= bar * max(1.0, abs(lf)), (it, d, lf, lj)
    print(f"trajectories bit-equal: {equal}")
    if same_lp:
        assert equal
    assert float(js.offsets.abs().max()) == 0.0 and float(js.offset_exp_avg.abs().max()) == 0.0


def _state(js, model):
    return [model.dof.detach().clone(), js.offsets.clone(), js.exp_avg.clone(), js.exp_avg_sq.clone(), js.offset_exp_avg.clone(),
            js.offset_exp_avg_sq.clone(), js.step_t.clone(), js.offset_step_t.clone(), js.loss.clone(), js.offset_grad.clone(),
            js.link_poses.clone()]


def test_graph_replay_and_checkpoint_resume_are_bit_equal(xarm7):
    from easyhec_amd import fused
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    ma, mb, mc = make(), make(), make()
    ja, jb, jc = JointPoseStep(ma, batch, xarm7, qp), JointPoseStep(mb, batch, xarm7, qp), JointPoseStep(mc, batch, xarm7, qp)
    jb.capture()
    for it in range(20):
        ja.step()
        jb.step()      # one ehr_graph_launch: forward kernel, chain, backward + Adam
        if it < 10:
            jc.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(ja, ma), _state(jb, mb)):
        assert torch.equal(x, y)
    assert int(jb.offset_step_t) == 20 and float(jb.offsets.abs().max()) > 0
    fused.check_status(jb.glctx)
    # checkpoint after 10 steps -> a new solver and a new JointPoseStep -> 10 more steps == the uninterrupted 20
    sd, msd = jc.state_dict(), {k: v.clone() for k, v in mc.state_dict().items()}
    assert set(sd["state"]) == {0, 1} and len(sd["param_groups"]) == 2 and sd["param_groups"][1]["params"] == [1]
    assert float(sd["state"][1]["step"]) == 10 and sd["state"][1]["exp_avg"].shape == (9,)
    md = make()
    md.load_state_dict(msd)
    jd = JointPoseStep(md, batch, xarm7, qp)
    jd.load_state_dict(sd)
    assert int(jd.hist_row) == 10 and torch.equal(jd.offsets, jc.offsets)
    for _ in range(10):
        jd.step()
    torch.cuda.synchronize()
    for x, y in zip(_state(ja, ma), _state(jd, md)):
        assert torch.equal(x, y)
    assert torch.equal(ma.history_ops[:21], md.history_ops[:21])
    # Adam moved the offsets after the step's own forward launch: the corrected poses are a fresh launch at the final offsets
    before = jd.link_poses.clone()
    fit = jd.corrected_link_poses()
    assert torch.equal(fit, ja.corrected_link_poses()) and not torch.equal(fit, before) and fit.data_ptr() != jd.link_poses.data_ptr()


def test_refuses_data_parallel_and_multi_start(xarm7):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    with pytest.raises(ValueError, match="data-parallel"):
        JointPoseStep(make(), batch, xarm7, qp, rccl=True)
    with pytest.raises(ValueError, match="multi-start"):
        JointPoseStep(make(), batch, xarm7, qp, starts=[np.eye(4)])
    with pytest.raises(ValueError, match="qpos"):
        JointPoseStep(make(), batch, xarm7)
    with pytest.raises(ValueError, match="free joints"):
        JointPoseStep(make(), batch, xarm7, qp, free=[9])
    with pytest.raises(ValueError, match="forward kinematics of qpos"):   # link poses and joint vectors of different views
        JointPoseStep(make(), batch, xarm7, qp[::-1].copy())
    js = JointPoseStep(make(), {k: v for k, v in batch.items() if k != "link_poses"}, xarm7, qp)   # link_poses are optional
    assert torch.equal(js.link_poses, batch["link_poses"])
    sd = js.state_dict()
    with pytest.raises(ValueError, match="free joints"):                  # a resumed solve keeps its free set
        JointPoseStep(make(), batch, xarm7, qp, free=[1, 2]).load_state_dict(sd)
    with pytest.raises(ValueError, match="offsets' group"):
        JointPoseStep(make(), batch, xarm7, qp, offset_lr=0.001).load_state_dict(sd)
    JointPoseStep(make(), batch, xarm7, qp).load_state_dict(FusedPoseStep(make(), batch).state_dict())   # pose-only: accepted


def test_reported_steps_freeze_the_offsets_and_the_run_recovers(xarm7, monkeypatch):
    """A close-up that a slot-limited plan (slack 1.0) reports: 48 unattended step() calls -- calls 1..32 are reported, the
    poll at call 32 plans again with every slot, calls 33..48 are 16 effective steps -- end bit-equal to 16 steps of a run
    planned with slack = 0 from the start."""
    from easyhec_amd.config import Cfg
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rb_solver import RBSolver
    from test_gpu_fused import workload
    dev = torch.device("cuda:0")
    H, W, B = 64, 96, 2
    K, lp, Tc, _ = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=dev)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(K, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    qp = _views_qpos(xarm7, B, seed=3)
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    init = np.zeros(9, np.float32)
    init[1:7] = [0.01, -0.02, 0.015, 0.0, -0.01, 0.02]
    m0 = make()
    j0 = JointPoseStep(m0, batch, xarm7, qp, slack=0.0, init_offset=init)
    for _ in range(16):
        j0.step()
    torch.cuda.synchronize()
    assert j0.recoveries == [] and int(j0.offset_step_t) == 16
    m1 = make()
    j1 = JointPoseStep(m1, batch, xarm7, qp, slack=1.0, init_offset=init)
    for i in range(48):
        loss = j1.step()
        if i in (0, 15, 31):
            torch.cuda.synchronize()
        if i in (0, 15):   # reported: NaN loss, nothing of the offsets' group has moved
            assert bool(torch.isnan(loss).all())
            assert np.array_equal(_bits(j1.offsets.cpu().numpy()), _bits(init)) and int(j1.offset_step_t) == 0
            assert float(j1.offset_exp_avg.abs().max()) == 0.0 and float(j1.offset_exp_avg_sq.abs().max()) == 0.0
    torch.cuda.synchronize()
    assert j1.recoveries == ["job slots"] and j1.slack == 0.0
    assert j1.steps_done == 16 and int(j1.offset_step_t) == 16
    for x, y in zip(_state(j0, m0), _state(j1, m1)):
        assert torch.equal(x, y)
    assert torch.equal(m0.history_ops[:17], m1.history_ops[:17])


# ---- 8. the solve ------------------------------------------------------------------------------------------------------------
SOLVE_STEPS = 600
SOLVE_VIEWS = 4
INJECTED = {1: 2.0, 2: -1.5, 3: 2.0, 5: -2.0}   # degrees, on four of the free joints
SOLVE_FREE = sorted(INJECTED)                   # the scene: see the test's docstring


def _pose_errors(model, Tc):
    from easyhec_amd.se3 import se3_exp_map
    T = se3_exp_map(model.dof.detach()[None].cpu().double()).permute(0, 2, 1)[0].numpy()
    D = np.linalg.inv(np.asarray(Tc)) @ T
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    return float(np.linalg.norm(D[:3, 3])), float(ang)   # metres, degrees


def _solve_scene(xarm7, B=None):
    """(cfg, make, batch, qpos, injected offsets, true Tc, true link poses, recorded link poses) of the solve test."""
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    B, H, W = B or SOLVE_VIEWS, 240, 320
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    qp = _views_qpos(xarm7, B, seed=0)
    truth = np.zeros(9)
    for j, deg in INJECTED.items():
        truth[j] = np.radians(deg)
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    m0 = make()
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lp_true = torch.tensor(xarm7.link_poses_batch(qp + truth[None]), dtype=torch.float32, device=dev)
    lp_rec = torch.tensor(xarm7.link_poses_batch(qp), dtype=torch.float32, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lp_true), torch.zeros((B, H, W), device=dev))
    batch = {"mask": (gt > 0.5).float(), "link_poses": lp_rec, "K": Kt[None].repeat(B, 1, 1)}
    return cfg, make, batch, qp, truth, Tc, lp_true, lp_rec


def test_solve_recovers_injected_joint_zero_errors(xarm7):
    """xArm7, 4 views at 320x240; the masks are rendered at the true camera pose with the arm's true joint angles = recorded
    qpos + injected zero errors (+2, -1.5, +2, -2 degrees on joints 1, 2, 3, 5); every solve starts at config 2's pose
    perturbation with zero offsets and takes SOLVE_STEPS steps.

    The scene.  With the default free set (joints 1..6) and 400 steps the REFERENCE missed the condition below: joint 2 came
    out at -1.92 degrees for -1.5 injected, while the two free joints without an injected error wandered (joint 4 to -0.43,
    the wrist roll 6 to +1.48 degrees): four views do not pin six offsets.  As the issue asks, the scene was changed, not
    the bar: the four joints that carry an error are free, the others are not, and the solves take 600 steps.

    Scene condition (reference alone): the autograd solve recovers every injected offset to within a quarter of its size.
    JointPoseStep: tail loss, worst offset error and pose errors at most twice the reference's (BASELINE row 2: HIP- and
    oracle-driven solves of one problem end up to that far apart once Adam has amplified rounding), and tail loss and pose
    errors below the pose-only FusedPoseStep solve's.  Measured figures: profiles/joint_offsets.md."""
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.joint_calib import solve_joint_offsets
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    cfg, make, batch, qp, truth, Tc, lp_true, lp_rec = _solve_scene(xarm7)
    table = xarm7.joint_table()
    tail = 20

    def figures(losses, offsets, model):
        off_err = float(np.abs(np.asarray(offsets, np.float64) - truth).max())
        et, er = _pose_errors(model, Tc)
        return float(np.mean(losses[-tail:])), off_err, et, er

    # the autograd reference
    ma = make()
    ref = AutogradJointSolve(ma, batch, table, qp, SOLVE_FREE, lr=cfg.solver.max_lr, wd=cfg.solver.weight_decay)
    la = torch.stack([ref.step() for _ in range(SOLVE_STEPS)]).cpu().numpy()
    ro = ref.offsets.detach().cpu().numpy()
    fr = figures(la, ro, ma)
    print(f"reference   : tail loss {fr[0]:.3f} | worst offset error {np.degrees(fr[1]):.3f} deg | trans {fr[2] * 1e3:.2f} mm | rot {fr[3]:.3f} deg")
    print("reference offsets (deg):", np.degrees(ro).round(3).tolist())
    for j, deg in INJECTED.items():
        assert abs(ro[j] - truth[j]) <= 0.25 * abs(truth[j]), ("scene condition", j, np.degrees(ro[j]), deg)
    # the launch chain with the joint kernels
    mj = make()
    res = solve_joint_offsets(cfg, mj, batch, xarm7, SOLVE_STEPS, qpos=qp, free=SOLVE_FREE)
    assert res.losses.shape == (SOLVE_STEPS,) and res.recoveries == []
    fj = figures(res.losses.numpy(), res.offsets.numpy(), mj)
    print(f"JointPoseStep: tail loss {fj[0]:.3f} | worst offset error {np.degrees(fj[1]):.3f} deg | trans {fj[2] * 1e3:.2f} mm | rot {fj[3]:.3f} deg")
    print("JointPoseStep offsets (deg):", np.degrees(res.offsets.numpy()).round(3).tolist())
    # the pose-only solve from the same start
    mf = make()
    fs = FusedPoseStep(mf, batch, lr=cfg.solver.max_lr, weight_decay=cfg.solver.weight_decay)
    lf = torch.stack([fs.step().clone() for _ in range(SOLVE_STEPS)]).cpu().numpy().reshape(-1)
    ff = figures(lf, np.zeros(9), mf)
    print(f"pose only   : tail loss {ff[0]:.3f} | trans {ff[2] * 1e3:.2f} mm | rot {ff[3]:.3f} deg")
    for k, name in enumerate(("tail loss", "offset error", "translation error", "rotation error")):
        assert fj[k] <= 2.0 * fr[k], (name, fj[k], fr[k])
    for k, name in ((0, "tail loss"), (2, "translation error"), (3, "rotation error")):
        assert fj[k] < ff[k], (name, fj[k], ff[k])
    # what comes after the solve sees the corrected kinematics
    lp_fit = res.step.corrected_link_poses()
    assert float((lp_fit - lp_true).abs().max()) < float((lp_rec - lp_true).abs().max())
