"""Intrinsics refinement on the GPU (csrc/ehr_intrinsics.hip, easyhec_amd/intrinsics_calib.py): the kernel against the float64
reference of tests/intrinsics_reference.py, the launch chain with it against torch autograd through the projection, graph
capture, checkpoints, reported steps, the composition with the joint offsets, and a solve with an injected focal error.

Tolerances.  Gradients and Adam: the pose head's rule (tests/test_gpu_pose_head.py), |Xhip - X64| / s <= 4 e32 + 8 * 2^-23
with e32 from the same reference text run in float32.  The written K: bit-equal to the float64 evaluation at the kernel's own
theta rounded once; one float32 unit where the device's exp (1 ulp of float64) moves the rounding.  Trajectories against
autograd: the bars of test_gpu_fast.py::test_fast_step_tracks_autograd_step.  Every figure is printed before it is asserted;
measured figures: profiles/intrinsics.md."""
import ctypes
import math

import numpy as np
import pytest
import torch

import intrinsics_reference as IR
import pose_reference as R
from test_gpu_fast import problem
from test_gpu_joint_offsets import _pose_errors, _views_qpos

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
U = R.U
ALL = ("fx", "fy", "cx", "cy")


def _f(x):
    return ctypes.c_float(float(x))


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _tc_jac(Tc):
    t = torch.full((7, 16), float("nan"), device="cuda:0")
    t[0] = _dev(np.asarray(Tc, np.float32).reshape(16))
    return t


class _Group:
    """Device state of one intrinsics group and one call of ehr_intrinsics_backward_adam on it."""

    def __init__(self, K0, H, W, p, m, v, step, free, tie):
        from easyhec_amd.intrinsics_calib import intrinsics_from_theta
        self.K0h, self.H, self.W, self.tie = np.asarray(K0, np.float32), H, W, int(tie)
        self.K0 = _dev(self.K0h)
        self.p, self.m, self.v = (_dev(np.asarray(x, np.float32)) for x in (p, m, v))
        self.t = torch.tensor([int(step)], dtype=torch.int32, device="cuda:0")
        self.free = _dev(np.asarray(free, np.int32))
        self.K = _dev(intrinsics_from_theta(K0, p, H, W))
        self.grad = torch.full((4,), 12345.0, device="cuda:0")

    def step(self, g, tc_jac, lp, red, hyper, sync=True):
        from easyhec_amd import _lib
        B, L = lp.shape[:2]
        lr, b1, b2, eps, wd = hyper
        self.keep = (g, tc_jac, lp, red)
        _lib.check(_lib.lib().ehr_intrinsics_backward_adam(
            _lib.ptr(g), _lib.ptr(tc_jac), _lib.ptr(lp), B, L, self.H, self.W, _lib.ptr(red), _lib.ptr(self.K0),
            _lib.ptr(self.free), self.tie, _lib.ptr(self.p), _lib.ptr(self.m), _lib.ptr(self.v), _lib.ptr(self.t), _f(lr),
            _f(b1), _f(b2), _f(eps), _f(wd), _lib.ptr(self.K), _lib.ptr(self.grad), _stream()), "intrinsics")
        if sync:
            torch.cuda.synchronize()
            return self.state()

    def state(self):
        return (self.p.cpu().numpy(), self.m.cpu().numpy(), self.v.cpu().numpy(), int(self.t.item()), self.grad.cpu().numpy(),
                self.K.cpu().numpy())


def _k_check(K0, H, W, theta_after, K_got):
    """(entries off by one float32 unit, entries off by more) of the written K against the float64 evaluation at theta_after."""
    want = IR.K_of_theta(K0, theta_after, H, W).astype(np.float32)
    one = more = 0
    for a, b in zip(K_got.reshape(-1), want.reshape(-1)):
        if _bits(a) != _bits(b):
            if abs(float(a) - float(b)) <= float(np.spacing(np.float32(abs(b)))):
                one += 1
            else:
                more += 1
    return one, more


# ---- 1. gradient -----------------------------------------------------------------------------------------------------------
def _grad_case(ci, BL, draw):
    rng = np.random.default_rng(9000 + 1000 * ci + 10 * BL + draw)
    K0, H, W = R.CAMERAS[ci]
    B, L = (BL // 8, 8) if BL % 8 == 0 else (BL, 1)
    g = rng.normal(size=(B, L, 4, 4))
    g *= np.where(rng.uniform(size=(B, L, 1, 1)) < 0.2, 1e6, 1.0)       # some pairs a million times the others
    lp = R.random_rigid(rng, BL).reshape(B, L, 4, 4)
    Tc = R.random_rigid(rng, 1)[0]
    theta = np.zeros(4, np.float32) if draw == 0 else (rng.normal(size=4) * 0.02).astype(np.float32)
    return dict(K0=K0, H=H, W=W, g=g.astype(np.float32), lp=lp, Tc=Tc, theta=theta)


def _run_grad(c, free, tie):
    b = _Group(c["K0"], c["H"], c["W"], c["theta"], np.zeros(4), np.zeros(4), 0, free, tie)
    red = _dev(np.array([1, 2, 3, 4, 5, 6, 7, 1], np.float32))      # red[7] = 1: grad_out is the sum itself
    return b.step(_dev(c["g"]), _tc_jac(c["Tc"]), _dev(c["lp"]), red, R.hyper32("default"))


@pytest.mark.parametrize("ci", [0, 1])
def test_theta_gradient_against_the_float64_reference(ci):
    bad = []
    for BL in R.PAIR_COUNTS:
        for draw in range(2):
            c = _grad_case(ci, BL, draw)
            args = (c["g"], c["Tc"], c["lp"], c["K0"], c["theta"], c["H"], c["W"])
            s64, scale = IR.theta_gradient(*args)
            s32, _ = IR.theta_gradient(*args, dtype=F32)
            # every element free
            got = _run_grad(c, [1, 1, 1, 1], 0)
            again = _run_grad(c, [1, 1, 1, 1], 0)
            assert np.array_equal(_bits(got[4]), _bits(again[4])), "two runs differ"
            assert got[3] == 1 and np.isfinite(got[4]).all() and (np.abs(s64) > 0).all()
            e32, eh = R.rel_err(s32, s64, scale), R.rel_err(got[4], s64, scale)
            # a partial free set: the others are exactly +0
            part = _run_grad(c, [1, 0, 0, 1], 0)
            assert np.array_equal(_bits(part[4][[0, 3]]), _bits(got[4][[0, 3]]))
            assert np.array_equal(_bits(part[4][[1, 2]]), _bits(np.zeros(2, np.float32))), part[4]
            # tied focal lengths: both report g0 + g1
            tied = _run_grad(c, [1, 1, 0, 1], 1)
            assert _bits(tied[4][0]) == _bits(tied[4][1]) and _bits(tied[4][3]) == _bits(got[4][3]) and _bits(tied[4][2]) == 0
            t64, ts = s64[0] + s64[1], scale[0] + scale[1]
            e32t, eht = R.rel_err(s32[0] + s32[1], t64, ts), R.rel_err(tied[4][0], t64, ts)
            zero = "zero" if draw == 0 else "random"
            print(f"camera {ci} pairs {BL} theta {zero}: gradient e32 {e32:.2e} hip {eh:.2e} bound {R.bound(e32):.2e} | "
                  f"tied e32 {e32t:.2e} hip {eht:.2e} bound {R.bound(e32t):.2e}")
            if not (eh <= R.bound(e32) and eht <= R.bound(e32t)):
                bad.append((BL, draw, e32, eh, e32t, eht))
    assert not bad, bad


# ---- 2. Adam ---------------------------------------------------------------------------------------------------------------
QTY = ("p", "m", "v")


def _adam_errs(got, ref, e, free):
    for qi, q in enumerate(QTY):
        s = float(np.abs(ref[qi][free]).max())
        e[q] = max(e[q], R.rel_err(np.asarray(got[qi])[free], ref[qi][free], s))


def test_adam_one_step_from_a_given_state():
    """The update of the free elements from a state with 0, 9 and 999 steps behind it, for every hyper-parameter set of the
    pose head's sweep; the gradient the reference is given is the kernel's own grad_out (red[7] = 1: an exact quotient), so
    the update is judged alone.  Draw 1 ties the focal lengths."""
    bad, k_one = [], 0
    for hname in R.ADAM_HYPER:
        h = R.hyper32(hname)
        for t0 in (0, 9, 999):
            e32, eh = dict.fromkeys(QTY, 0.0), dict.fromkeys(QTY, 0.0)
            for draw in range(2):
                c = _grad_case(draw, 8, 1)
                rng = np.random.default_rng(100 * t0 + draw)
                fr = np.array([1, 1, 0, 1], bool)
                p0 = c["theta"].copy()
                if draw == 1:
                    p0[1] = p0[0]
                m0 = (rng.normal(size=4) * 10 * (t0 > 0)).astype(np.float32)
                v0 = (rng.uniform(1, 400, size=4) * (t0 > 0)).astype(np.float32)
                if draw == 1:
                    m0[1], v0[1] = m0[0], v0[0]
                red = np.array([0, 0, 0, 0, 0, 0, 5, 1], np.float32)
                b = _Group(c["K0"], c["H"], c["W"], p0, m0, v0, t0, fr.astype(np.int32), draw)
                got = b.step(_dev(c["g"] * np.float32(1e-4)), _tc_jac(c["Tc"]), _dev(c["lp"]), _dev(red), h)
                assert got[3] == t0 + 1
                r64 = IR.adam_step(p0, m0, v0, t0, got[4], red, fr, 0, *h)        # (grad_out is tied already)
                r32 = IR.adam_step(p0, m0, v0, t0, got[4], red, fr, 0, *h, dtype=F32)
                assert np.array_equal(_bits(got[4][fr]), _bits(r64[4][fr])) and _bits(got[4][2]) == 0
                for qi, x0 in enumerate((p0, m0, v0)):   # an element that is not free keeps its bits
                    assert np.array_equal(_bits(got[qi][~fr]), _bits(x0[~fr]))
                if draw == 1:                            # tied: equal starts stay equal bit for bit
                    assert all(_bits(got[qi][0]) == _bits(got[qi][1]) for qi in range(3))
                _adam_errs(r32, r64, e32, fr)
                _adam_errs(got, r64, eh, fr)
                one, more = _k_check(c["K0"], c["H"], c["W"], got[0], got[5])
                k_one += one
                assert more == 0, (hname, t0, draw, got[5])
            for q in QTY:
                ok = eh[q] <= R.bound(e32[q])
                print(f"adam one step {hname} t0={t0} {q}: e32 {e32[q]:.2e} hip {eh[q]:.2e} bound {R.bound(e32[q]):.2e} {'ok' if ok else 'FAIL'}")
                if not ok:
                    bad.append((hname, t0, q, e32[q], eh[q]))
    print(f"written K: {k_one} entries one float32 unit from the float64 evaluation, the others bit-equal")
    assert not bad, bad


@pytest.mark.parametrize("kind", ["noisy1e3", "zero_moving", "mixed"])
def test_adam_trajectory_of_200_steps(kind):
    """200 steps on the gradients of pose_reference.adam_gradients: one pair with Tc = link pose = identity, whose grad_mvp
    entries [0,0], [1,1], [0,2], [1,2] carry the step's gradient (divided by the factor the kernel multiplies with, at theta
    = 0); the reference trajectory is fed the kernel's own grad_out of every step."""
    K0, H, W = R.CAMERAS[0]
    h = R.hyper32("default")
    fr = np.ones(4, bool)
    rng = np.random.default_rng(17)
    want = R.adam_gradients(kind, rng, 200)[:, :4] * 1e-3        # (theta is dimensionless: keep exp(theta) in range)
    g = np.zeros((200, 1, 1, 4, 4), np.float32)
    g[:, 0, 0, 0, 0] = want[:, 0] / (K0[0, 0] * 2 / W)
    g[:, 0, 0, 1, 1] = -want[:, 1] / (K0[1, 1] * 2 / H)
    g[:, 0, 0, 0, 2] = want[:, 2] / 2
    g[:, 0, 0, 1, 2] = -want[:, 3] / 2
    gd = _dev(g)
    eye = np.eye(4, dtype=np.float32)
    tc_jac, lp = _tc_jac(eye), _dev(eye.reshape(1, 1, 4, 4))
    p0 = np.array([0.01, -0.02, 0.005, 0.0], np.float32)
    b = _Group(K0, H, W, p0, np.zeros(4), np.zeros(4), 0, fr.astype(np.int32), 0)
    red = _dev(np.array([0, 0, 0, 0, 0, 0, 5, 1], np.float32))
    grads, snaps = [], {}
    for k in range(200):  # no synchronisation inside
        b.step(gd[k], tc_jac, lp, red, h, sync=False)
        grads.append(b.grad.clone())
        if k + 1 in (1, 10, 100, 200):
            snaps[k + 1] = (b.p.clone(), b.m.clone(), b.v.clone(), b.t.clone(), b.K.clone())
    torch.cuda.synchronize()
    grads = torch.stack(grads).cpu().numpy()
    assert np.isfinite(grads).all() and (np.abs(grads) > 0).any()
    # the gradients the kernel formed are the prescribed ones (cu, cv exactly up to rounding; fu, fv times exp(theta))
    assert np.allclose(grads[0, 2:], want[0, 2:].astype(np.float32), rtol=1e-6, atol=0)
    st = {F64: (p0.astype(np.float64), np.zeros(4), np.zeros(4)), F32: (p0, np.zeros(4, np.float32), np.zeros(4, np.float32))}
    bad, k_one = [], 0
    for k in range(200):
        for dt in (F64, F32):
            st[dt] = IR.adam_step(*st[dt], k, grads[k], [0, 0, 0, 0, 0, 0, 5, 1], fr, 0, *h, dtype=dt)[:3]
        if k + 1 in snaps:
            got = [x.cpu().numpy() for x in snaps[k + 1][:3]]
            assert int(snaps[k + 1][3].item()) == k + 1
            e32, eh = dict.fromkeys(QTY, 0.0), dict.fromkeys(QTY, 0.0)
            _adam_errs(st[F32], st[F64], e32, fr)
            _adam_errs(got, st[F64], eh, fr)
            one, more = _k_check(K0, H, W, got[0], snaps[k + 1][4].cpu().numpy())
            k_one += one
            assert more == 0
            for q in QTY:
                ok = eh[q] <= R.bound(e32[q])
                print(f"adam trajectory {kind} step {k + 1} {q}: e32 {e32[q]:.2e} hip {eh[q]:.2e} bound {R.bound(e32[q]):.2e} {'ok' if ok else 'FAIL'}")
                if not ok:
                    bad.append((k + 1, q, e32[q], eh[q]))
    print(f"written K ({kind}): {k_one} entries one float32 unit from the float64 evaluation, the others bit-equal")
    assert not bad, bad


# ---- 3. freeze rule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot,value", [(0, float("nan")), (6, float("inf")), (2, float("-inf")), (7, float("nan")),
                                        (3, 3.1e38), (7, float("inf"))])
def test_non_finite_red_leaves_theta_moments_counter_and_K_alone(slot, value):
    c = _grad_case(1, 8, 1)
    fr = np.array([1, 0, 1, 1], bool)
    rng = np.random.default_rng(5)
    m0, v0 = rng.normal(size=4).astype(np.float32), rng.uniform(1, 4, size=4).astype(np.float32)
    red = np.array([1, 2, 3, 4, 5, 6, 7, 3], np.float32)

    def run(red):
        b = _Group(c["K0"], c["H"], c["W"], c["theta"], m0, v0, 9, fr.astype(np.int32), 0)
        K_before = b.K.cpu().numpy()
        return b.step(_dev(c["g"]), _tc_jac(c["Tc"]), _dev(c["lp"]), _dev(red), R.hyper32("default")), K_before

    clean, K_before = run(red)
    assert clean[3] == 10 and not np.array_equal(_bits(clean[0][fr]), _bits(c["theta"][fr]))
    assert not np.array_equal(_bits(clean[5]), _bits(K_before))
    red[slot] = np.float32(value)
    got, K_before = run(red)
    assert np.array_equal(_bits(got[0]), _bits(c["theta"])) and np.array_equal(_bits(got[1]), _bits(m0))
    assert np.array_equal(_bits(got[2]), _bits(v0)) and got[3] == 9
    assert np.array_equal(_bits(got[5]), _bits(K_before))
    assert np.isnan(got[4][fr]).all() and _bits(got[4][1]) == 0


def test_argument_checks():
    from easyhec_amd import _lib
    assert _lib.has_intrinsics()
    c = _grad_case(0, 8, 0)
    b = _Group(c["K0"], c["H"], c["W"], c["theta"], np.zeros(4), np.zeros(4), 0, [1, 1, 1, 1], 0)
    g, tj, lp, red = _dev(c["g"]), _tc_jac(c["Tc"]), _dev(c["lp"]), _dev(np.ones(8, np.float32))
    lib, P, h = _lib.lib(), _lib.ptr, [_f(x) for x in R.hyper32("default")]
    call = lambda B, L, K: lib.ehr_intrinsics_backward_adam(P(g), P(tj), P(lp), B, L, 8, 8, P(red), P(b.K0), P(b.free), 0, P(b.p),
                                                            P(b.m), P(b.v), P(b.t), *h, K, None, _stream())
    assert call(1, 8, None) != 0 and call(0, 8, P(b.K)) != 0 and call(1 << 20, 1 << 8, P(b.K)) != 0
    assert call(1, 8, P(b.K)) == 0        # grad_out may be NULL
    torch.cuda.synchronize()


# ---- the chain -------------------------------------------------------------------------------------------------------------
def _snap(st, model):
    return [model.dof.detach().clone(), st.loss.clone(), st.loss_b.clone(), st.grad_mvp.clone(), st.exp_avg.clone(),
            st.exp_avg_sq.clone(), st.step_t.clone(), st.red.clone()]


def test_frozen_intrinsics_reproduce_the_pose_only_step(xarm7):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    mf, m1, m2 = make(), make(), make()
    fs = FusedPoseStep(mf, batch)
    i1 = IntrinsicsPoseStep(m1, batch, free=())
    i2 = IntrinsicsPoseStep(m2, batch, intrinsics_lr=0, intrinsics_weight_decay=0)
    assert i1.K.data_ptr() != batch["K"].data_ptr() and i1.K.data_ptr() != i1.K0.data_ptr()
    for it in range(30):
        fs.step(), i1.step(), i2.step()
        torch.cuda.synchronize()
        ref = _snap(fs, mf)
        for st, m in ((i1, m1), (i2, m2)):
            for k, (x, y) in enumerate(zip(ref, _snap(st, m))):
                assert torch.equal(x, y), (it, k)
            assert torch.equal(st.K, fs.K) and torch.equal(st.K, st.K0)
    assert torch.equal(mf.history_ops[:31], m1.history_ops[:31]) and torch.equal(mf.history_ops[:31], m2.history_ops[:31])
    assert int(i1.theta_step_t) == 30 and float(i1.theta.abs().max()) == 0.0 and float(i1.theta_grad.abs().max()) == 0.0
    assert float(i2.theta.abs().max()) == 0.0 and float(i2.theta_grad[:2].abs().max()) > 0.0
    assert _bits(i2.theta_grad[0].item()) == _bits(i2.theta_grad[1].item())          # tied by default


def test_chain_renders_the_K_that_was_written(xarm7):
    """Ten steps with all four elements free, then ONE more step next to a fresh FusedPoseStep that is given the written K as a
    constant: everything the chain leaves behind is bit-equal, i.e. nothing derived from K is cached across calls."""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    mi = make()
    ip = IntrinsicsPoseStep(mi, batch, free=ALL)
    for _ in range(10):
        ip.step()
    torch.cuda.synchronize()
    Kfit = ip.intrinsics()
    assert not torch.equal(Kfit, ip.K0.cpu()) and float((Kfit - ip.K0.cpu()).abs().max()) > 1e-3
    mf = make()
    mf.load_state_dict({k: v.clone() for k, v in mi.state_dict().items()})
    b2 = dict(batch)
    b2["K"] = Kfit.to(batch["K"].device)[None].repeat(2, 1, 1)
    fs = FusedPoseStep(mf, b2)
    fs.load_state_dict(ip.state_dict())
    assert int(fs.hist_row) == 10 and int(fs.step_t) == 10
    ip.step(), fs.step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_snap(ip, mi), _snap(fs, mf))):
        assert torch.equal(x, y), k
    assert torch.equal(mi.history_ops[:12], mf.history_ops[:12])
    assert not torch.equal(ip.intrinsics(), Kfit)                 # (and the eleventh step wrote the next K)


def torch_K(K0, theta, H, W, tie):
    """Differentiable float32 K(theta) on the device; with ``tie`` both focal lengths read theta[0]."""
    K = K0.clone()
    K[0, 0] = K0[0, 0] * torch.exp(theta[0])
    K[1, 1] = K0[1, 1] * torch.exp(theta[0] if tie else theta[1])
    K[0, 2] = K0[0, 2] + W * theta[2]
    K[1, 2] = K0[1, 2] + H * theta[3]
    return K


class AutogradIntrinsicsSolve:
    """The reference: RBSolver.forward (use_fused: K_to_projection, fused.mvp_matrices, the fused.render_mask_loss autograd
    op) with K(theta) built by torch from a leaf theta, loss.backward(), torch.optim.Adam over two parameter groups.  The
    gradient of an element that is not free is masked to zero; tied focal lengths are ONE leaf element (theta[0])."""

    def __init__(self, model, batch, free, lr=0.003, wd=0.0005, theta_lr=None, theta_wd=None):
        from easyhec_amd.intrinsics_calib import _parse_free
        dev = model.dof.device
        self.model, self.batch = model, dict(batch)
        mask, self.tie, _ = _parse_free(free)
        if self.tie:
            mask[1] = 0
        self.K0 = batch["K"][0].detach().clone().float()
        self.B = batch["K"].shape[0]
        self.theta = torch.zeros(4, device=dev, requires_grad=True)
        self.mask = torch.tensor(mask, dtype=torch.float32, device=dev)
        self.opt = torch.optim.Adam([{"params": [model.dof], "lr": lr, "weight_decay": wd},
                                     {"params": [self.theta], "lr": lr if theta_lr is None else theta_lr,
                                      "weight_decay": wd if theta_wd is None else theta_wd}], lr)

    def step(self):
        self.opt.zero_grad(set_to_none=False)
        K = torch_K(self.K0, self.theta * self.mask, self.model.H, self.model.W, self.tie)
        self.batch["K"] = K[None].expand(self.B, 3, 3)
        _, ld = self.model(self.batch, with_outputs=False)
        loss = ld["mask_loss"]
        loss.backward()
        self.opt.step()
        return loss.detach()

    def focal_theta(self):
        return float(self.theta.detach()[0])


def test_chain_tracks_autograd_through_the_projection(xarm7):
    """Bars: those of test_chain_tracks_autograd_through_differentiable_kinematics (5e-5 for the first three steps, 1e-2 once
    the discontinuous raster has amplified rounding) on dof and theta.  The gradient of step 0 is compared before any update:
    its bar is the 2e-4 relative (to the largest element) that test_fast_step_tracks_autograd_step grants float32 quantities of
    the first steps -- autograd carries it through float32 products of K, the projection and the pose, the kernel sums in
    float64."""
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    ma, mi = make(), make()
    ref = AutogradIntrinsicsSolve(ma, batch, ALL)
    ip = IntrinsicsPoseStep(mi, batch, free=ALL)
    moved = 0.0
    for it in range(12):
        la, li = float(ref.step()), float(ip.step())
        if it == 0:
            ga, gi = ref.theta.grad.detach().cpu().numpy(), ip.theta_grad.cpu().numpy()
            d_g = float(np.abs(ga - gi).max() / np.abs(ga).max())
            print(f"step 0 gradient: autograd {ga.tolist()} chain {gi.tolist()} | relative difference {d_g:.2e}")
            assert d_g <= 2e-4 and (np.abs(gi) > 0).all()
        d_dof = float((ma.dof.detach() - mi.dof.detach()).abs().max())
        d_th = float((ref.theta.detach() - ip.theta).abs().max())
        moved = max(moved, float(ip.theta.abs().max()))
        print(f"step {it}: loss {la:.4f} / {li:.4f} | max |d dof| {d_dof:.2e} | max |d theta| {d_th:.2e}")
        bar = 5e-5 if it < 3 else 1e-2
        assert d_dof <= bar and d_th <= bar, (it, d_dof, d_th)
    assert moved > 1e-3 and int(ip.theta_step_t) == 12 and int(ip.step_t) == 12
    # the tied default: one leaf element on the autograd side, two bit-equal elements on the chain's
    ma, mi = make(), make()
    ref, ip = AutogradIntrinsicsSolve(ma, batch, ("f",)), IntrinsicsPoseStep(mi, batch)
    for it in range(6):
        ref.step(), ip.step()
        if it == 0:
            ga, gi = float(ref.theta.grad[0]), ip.theta_grad.cpu().numpy()
            print(f"tied step 0 gradient: autograd {ga} chain {gi.tolist()}")
            assert abs(ga - gi[0]) <= 2e-4 * abs(ga) and _bits(gi[0]) == _bits(gi[1]) and (gi[2:] == 0).all()
        d_th = float((ref.theta.detach()[0] - ip.theta[:2]).abs().max())
        assert d_th <= (5e-5 if it < 3 else 1e-2), (it, d_th)
    assert _bits(float(ip.theta[0])) == _bits(float(ip.theta[1])) and float(ip.theta[2:].abs().max()) == 0.0


def _state(st, model):
    return [model.dof.detach().clone(), st.theta.clone(), st.K.clone(), st.exp_avg.clone(), st.exp_avg_sq.clone(),
            st.theta_exp_avg.clone(), st.theta_exp_avg_sq.clone(), st.step_t.clone(), st.theta_step_t.clone(), st.loss.clone(),
            st.theta_grad.clone()]


def test_graph_replay_and_checkpoint_resume_are_bit_equal(xarm7):
    from easyhec_amd import fused
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, intrinsics_from_theta
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    ma, mb, mc = make(), make(), make()
    ia, ib, ic = (IntrinsicsPoseStep(m, batch, free=("f", "cx")) for m in (ma, mb, mc))
    ib.capture()
    for it in range(20):
        ia.step()
        ib.step()      # one ehr_graph_launch: the chain and the intrinsics launch
        if it < 10:
            ic.step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_state(ia, ma), _state(ib, mb))):
        assert torch.equal(x, y), k
    assert int(ib.theta_step_t) == 20 and float(ib.theta.abs().max()) > 0
    fused.check_status(ib.glctx)
    # checkpoint after 10 steps -> a new solver and a new step -> 10 more steps == the uninterrupted 20
    sd, msd = ic.state_dict(), {k: v.clone() for k, v in mc.state_dict().items()}
    assert set(sd["state"]) == {0, 1} and len(sd["param_groups"]) == 2 and sd["param_groups"][1]["params"] == [1]
    assert float(sd["state"][1]["step"]) == 10 and sd["state"][1]["exp_avg"].shape == (4,)
    assert sd["intrinsics"]["free"] == ["f", "cx"] and torch.equal(sd["intrinsics"]["K0"], batch["K"][0].cpu())
    md = make()
    md.load_state_dict(msd)
    idd = IntrinsicsPoseStep(md, batch, free=("cx", "f"))
    idd.load_state_dict(sd)
    assert int(idd.hist_row) == 10 and torch.equal(idd.theta, ic.theta) and torch.equal(idd.K, ic.K)
    for _ in range(10):
        idd.step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_state(ia, ma), _state(idd, md))):
        assert torch.equal(x, y), k
    assert torch.equal(ma.history_ops[:21], md.history_ops[:21])
    # what comes after the solve: the host helper gives the K the device holds
    K = intrinsics_from_theta(ia.K0.cpu().numpy(), ia.theta.cpu().numpy(), ia.H, ia.W)
    d = np.abs(K.astype(np.float64) - ia.intrinsics().numpy()) / np.spacing(np.abs(K))
    assert d.max() <= 1.0 and ia.intrinsics().data_ptr() != ia.K.data_ptr()


def test_reported_steps_freeze_the_group_and_the_run_recovers(xarm7):
    """The close-up of test_reported_steps_freeze_the_offsets_and_the_run_recovers, which a slot-limited plan (slack 1.0)
    reports: 48 unattended step() calls -- calls 1..32 are reported, the poll at call 32 plans again with every slot, calls
    33..48 are 16 effective steps -- end bit-equal to 16 steps of a run planned with slack = 0 from the start; and
    effective_rounds takes exactly 16 effective steps to the same end."""
    from easyhec_amd.config import Cfg
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, intrinsics_from_theta
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
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    init = np.array([0.01, -0.02, 0.015, -0.01], np.float32)
    K_init = intrinsics_from_theta(batch["K"][0].cpu().numpy(), init, H, W)
    m0 = make()
    i0 = IntrinsicsPoseStep(m0, batch, free=ALL, slack=0.0, init_theta=init)
    for _ in range(16):
        i0.step()
    torch.cuda.synchronize()
    assert i0.recoveries == [] and int(i0.theta_step_t) == 16
    m1 = make()
    i1 = IntrinsicsPoseStep(m1, batch, free=ALL, slack=1.0, init_theta=init)
    for i in range(48):
        loss = i1.step()
        if i in (0, 15, 31):
            torch.cuda.synchronize()
        if i in (0, 15):   # reported: NaN loss, nothing of the intrinsics' group has moved, K is what was rendered
            assert bool(torch.isnan(loss).all())
            assert np.array_equal(_bits(i1.theta.cpu().numpy()), _bits(init)) and int(i1.theta_step_t) == 0
            assert np.array_equal(_bits(i1.K.cpu().numpy()), _bits(K_init))
            assert float(i1.theta_exp_avg.abs().max()) == 0.0 and float(i1.theta_exp_avg_sq.abs().max()) == 0.0
            assert bool(torch.isnan(i1.theta_grad).all())
    torch.cuda.synchronize()
    assert i1.recoveries == ["job slots"] and i1.slack == 0.0
    assert i1.steps_done == 16 and int(i1.theta_step_t) == 16
    for k, (x, y) in enumerate(zip(_state(i0, m0), _state(i1, m1))):
        assert torch.equal(x, y), k
    assert torch.equal(m0.history_ops[:17], m1.history_ops[:17])
    # the loop that takes an exact number of effective steps
    m2 = make()
    i2 = IntrinsicsPoseStep(m2, batch, free=ALL, slack=1.0, init_theta=init)
    for remaining, _ in i2.effective_rounds(16, "test"):
        for _ in range(remaining):
            i2.step()
    torch.cuda.synchronize()
    assert i2.recoveries == ["job slots"] and int(i2.theta_step_t) == 16
    for k, (x, y) in enumerate(zip(_state(i0, m0), _state(i2, m2))):
        assert torch.equal(x, y), k


def test_refusals(xarm7):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, JointIntrinsicsPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    with pytest.raises(ValueError, match="data-parallel"):
        IntrinsicsPoseStep(make(), batch, rccl=True)
    with pytest.raises(ValueError, match="data-parallel"):
        IntrinsicsPoseStep(make(), batch, p2p=True)
    with pytest.raises(ValueError, match="multi-start"):
        IntrinsicsPoseStep(make(), batch, starts=[np.eye(4)])
    with pytest.raises(ValueError, match="cannot be combined"):
        IntrinsicsPoseStep(make(), batch, free=("f", "fx"))
    with pytest.raises(ValueError, match="names are"):
        IntrinsicsPoseStep(make(), batch, free=("focal",))
    b2 = dict(batch)
    b2["K"] = batch["K"].clone()
    b2["K"][1, 0, 0] += 1.0
    with pytest.raises(ValueError, match="differs between views"):
        IntrinsicsPoseStep(make(), b2)
    with pytest.raises(ValueError, match="equal theta"):
        IntrinsicsPoseStep(make(), batch, init_theta=[0.01, 0.02, 0, 0])
    with pytest.raises(ValueError, match="data-parallel"):
        JointIntrinsicsPoseStep(make(), batch, xarm7, _views_qpos(xarm7, 2), rccl=True)
    st = IntrinsicsPoseStep(make(), batch)
    sd = st.state_dict()
    with pytest.raises(ValueError, match="free intrinsics"):          # a resumed solve keeps its free set ...
        IntrinsicsPoseStep(make(), batch, free=("f", "cx")).load_state_dict(sd)
    with pytest.raises(ValueError, match="free intrinsics"):          # ... and its tying
        IntrinsicsPoseStep(make(), batch, free=("fx", "fy")).load_state_dict(sd)
    with pytest.raises(ValueError, match="intrinsics' group"):
        IntrinsicsPoseStep(make(), batch, intrinsics_lr=0.001).load_state_dict(sd)
    IntrinsicsPoseStep(make(), batch).load_state_dict(sd)
    IntrinsicsPoseStep(make(), batch).load_state_dict(FusedPoseStep(make(), batch).state_dict())   # pose-only: accepted


# ---- 10. the solve ---------------------------------------------------------------------------------------------------------
SOLVE_STEPS = 600          # test_solve_recovers_injected_joint_zero_errors's
SOLVE_VIEWS = 4
FOCAL_ERROR = 1.02
TAIL = 20


def _focal_scene(xarm7, B=SOLVE_VIEWS, focal=FOCAL_ERROR, shift_px=(0.0, 0.0)):
    """(cfg, make, batch with the WRONG K0, true K, true Tc): masks rendered at the true pose with the true K."""
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    H, W = 240, 320
    K = np.asarray(scaled_K(XARM7_K_1280x720, 0.25, W, H, True), np.float64)
    _, lp = make_views(xarm7, B, seed=0)
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    m0 = make()
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lpt = torch.tensor(lp, dtype=torch.float32, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((B, H, W), device=dev))
    K0 = K.copy()
    K0[0, 0] *= focal
    K0[1, 1] *= focal
    K0[0, 2] += shift_px[0]
    K0[1, 2] += shift_px[1]
    batch = {"mask": (gt > 0.5).float(), "link_poses": lpt,
             "K": torch.tensor(K0, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    return cfg, make, batch, K, Tc


def _pose_only(cfg, make, batch, Tc, steps):
    from easyhec_amd.fast import FusedPoseStep
    mf = make()
    fs = FusedPoseStep(mf, batch, lr=cfg.solver.max_lr, weight_decay=cfg.solver.weight_decay)
    lf = torch.stack([fs.step().clone() for _ in range(steps)]).cpu().numpy().reshape(-1)
    return (float(np.mean(lf[-TAIL:])),) + _pose_errors(mf, Tc)


def test_solve_recovers_an_injected_focal_error(xarm7):
    """xArm7, 4 views at 320x240; the masks are rendered at the true camera pose with the true K; every solve starts at config
    2's pose perturbation with a K0 whose focal lengths are 2 % too long, free=("f",), SOLVE_STEPS steps.

    Scene condition (reference alone): the autograd solve brings |theta_f - log(1/1.02)| below a quarter of log 1.02.  The
    first scene tried (the one above) met it, 0.0023 against 0.0050: nothing had to be changed.
    solve_intrinsics: tail loss, focal error and pose errors at most twice the reference's (BASELINE row 2: HIP- and
    oracle-driven solves of one problem end up to that far apart once Adam has amplified rounding), and tail loss and pose
    errors strictly below the pose-only FusedPoseStep solve's from the same start and the same wrong K0.  Measured figures:
    profiles/intrinsics.md."""
    from easyhec_amd.intrinsics_calib import solve_intrinsics
    cfg, make, batch, Ktrue, Tc = _focal_scene(xarm7)
    target = math.log(1.0 / FOCAL_ERROR)

    ma = make()
    ref = AutogradIntrinsicsSolve(ma, batch, ("f",), lr=cfg.solver.max_lr, wd=cfg.solver.weight_decay)
    la = torch.stack([ref.step() for _ in range(SOLVE_STEPS)]).cpu().numpy()
    fr = (float(np.mean(la[-TAIL:])), abs(ref.focal_theta() - target)) + _pose_errors(ma, Tc)
    print(f"reference      : tail loss {fr[0]:.3f} | focal error {fr[1]:.5f} (theta_f {ref.focal_theta():.5f}, target {target:.5f}) | "
          f"trans {fr[2] * 1e3:.2f} mm | rot {fr[3]:.3f} deg")
    assert fr[1] <= 0.25 * math.log(FOCAL_ERROR), ("scene condition", ref.focal_theta(), target)

    mi = make()
    res = solve_intrinsics(cfg, mi, batch, SOLVE_STEPS, free=("f",))
    assert res.losses.shape == (SOLVE_STEPS,) and res.recoveries == []
    th = res.theta.numpy()
    assert _bits(th[0]) == _bits(th[1]) and (th[2:] == 0).all()
    fi = (float(np.mean(res.losses.numpy()[-TAIL:])), abs(float(th[0]) - target)) + _pose_errors(mi, Tc)
    print(f"solve_intrinsics: tail loss {fi[0]:.3f} | focal error {fi[1]:.5f} (theta_f {float(th[0]):.5f}) | "
          f"trans {fi[2] * 1e3:.2f} mm | rot {fi[3]:.3f} deg")
    print("fitted K:", res.K.numpy().round(3).tolist(), "true K:", Ktrue.round(3).tolist())
    ff = _pose_only(cfg, make, batch, Tc, SOLVE_STEPS)
    print(f"pose only      : tail loss {ff[0]:.3f} | trans {ff[1] * 1e3:.2f} mm | rot {ff[2]:.3f} deg")
    for k, name in enumerate(("tail loss", "focal error", "translation error", "rotation error")):
        assert fi[k] <= 2.0 * fr[k], (name, fi[k], fr[k])
    for a, b, name in ((fi[0], ff[0], "tail loss"), (fi[2], ff[1], "translation error"), (fi[3], ff[2], "rotation error")):
        assert a < b, (name, a, b)
    # what comes after the solve sees the fitted intrinsics
    assert torch.equal(res.K, res.step.intrinsics())
    assert abs(float(res.K[0, 0]) - Ktrue[0, 0]) < abs(float(batch["K"][0, 0, 0]) - Ktrue[0, 0])


def test_principal_point_trades_off_against_rotation(xarm7):
    """The shorter case: a 3-pixel principal-point error on top of the focal error, free=("f", "cx", "cy"), 300 steps.  Only
    the tail loss is a bar (below the pose-only solve's); how far cx, cy and the rotation trade off is printed: the figure
    documents the gauge (profiles/intrinsics.md)."""
    from easyhec_amd.intrinsics_calib import solve_intrinsics
    steps = 300
    cfg, make, batch, Ktrue, Tc = _focal_scene(xarm7, shift_px=(3.0, -3.0))
    mi = make()
    res = solve_intrinsics(cfg, mi, batch, steps, free=("f", "cx", "cy"))
    assert res.losses.shape == (steps,)
    tail = float(np.mean(res.losses.numpy()[-TAIL:]))
    et, er = _pose_errors(mi, Tc)
    K = res.K.numpy().astype(np.float64)
    ff = _pose_only(cfg, make, batch, Tc, steps)
    print(f"f, cx, cy free : tail loss {tail:.3f} | focal {K[0, 0] / Ktrue[0, 0] - 1:+.4%} | cx error {K[0, 2] - Ktrue[0, 2]:+.2f} px "
          f"(started +3.00) | cy error {K[1, 2] - Ktrue[1, 2]:+.2f} px (started -3.00) | trans {et * 1e3:.2f} mm | rot {er:.3f} deg")
    print(f"pose only      : tail loss {ff[0]:.3f} | trans {ff[1] * 1e3:.2f} mm | rot {ff[2]:.3f} deg")
    assert tail < ff[0], (tail, ff[0])


# ---- 11. composition with the joint offsets ----------------------------------------------------------------------------------
def _jstate(js, model):
    return [model.dof.detach().clone(), js.offsets.clone(), js.exp_avg.clone(), js.exp_avg_sq.clone(), js.offset_exp_avg.clone(),
            js.offset_exp_avg_sq.clone(), js.step_t.clone(), js.offset_step_t.clone(), js.loss.clone(), js.offset_grad.clone(),
            js.link_poses.clone(), js.grad_mvp.clone()]


def test_composition_with_joint_offsets(xarm7):
    from easyhec_amd import _lib
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    qp = _views_qpos(xarm7, 2)
    # everything frozen: the pose-only step; joints free, intrinsics frozen: the joint step -- bit for bit over 30 steps
    mf, m0, mj, m1 = make(), make(), make(), make()
    fs = FusedPoseStep(mf, batch)
    c0 = JointIntrinsicsPoseStep(m0, batch, xarm7, qp, free=[], free_intrinsics=())
    js = JointPoseStep(mj, batch, xarm7, qp)
    c1 = JointIntrinsicsPoseStep(m1, batch, xarm7, qp, free_intrinsics=())
    assert c0.state_dict()["intrinsics"]["group"] == 2 and set(c1.state_dict()["state"]) == {0, 1, 2}
    for it in range(30):
        fs.step(), c0.step(), js.step(), c1.step()
        torch.cuda.synchronize()
        for k, (x, y) in enumerate(zip(_snap(fs, mf), _snap(c0, m0))):
            assert torch.equal(x, y), ("frozen", it, k)
        for k, (x, y) in enumerate(zip(_jstate(js, mj), _jstate(c1, m1))):
            assert torch.equal(x, y), ("joints free", it, k)
        assert torch.equal(c0.K, fs.K) and torch.equal(c1.K, js.K)
    assert torch.equal(mf.history_ops[:31], m0.history_ops[:31]) and torch.equal(mj.history_ops[:31], m1.history_ops[:31])
    assert float(c1.offsets.abs().max()) > 0 and float(c0.offsets.abs().max()) == 0.0
    # both free: the joint launch saw the K that was RENDERED, i.e. the launch that rewrites K ran after it
    m2 = make()
    c2 = JointIntrinsicsPoseStep(m2, batch, xarm7, qp, free_intrinsics=ALL, init_theta=[0.01, -0.01, 0.01, -0.01])
    for _ in range(3):
        c2.step()
    torch.cuda.synchronize()
    K_rendered = c2.K.clone()
    before = [x.clone() for x in (c2.offsets, c2.offset_exp_avg, c2.offset_exp_avg_sq, c2.offset_step_t)]
    c2.step()
    torch.cuda.synchronize()
    assert not torch.equal(c2.K, K_rendered)

    def alone(K):
        off, m, v, t = (x.clone() for x in before)
        grad = torch.full_like(c2.offset_grad, 12345.0)
        b1, b2 = c2.betas
        _lib.check(_lib.lib().ehr_joint_backward_adam(
            _lib.ptr(c2.grad_mvp), _lib.ptr(c2.tc_jac), _lib.ptr(K), c2.B, c2.L, c2.J, c2.H, c2.W, _f(c2.near), _f(c2.far),
            _lib.ptr(c2.link_poses), _lib.ptr(c2.joint_frames), _lib.ptr(c2.kinematics.upstream), _lib.ptr(c2.kinematics.jkind), _lib.ptr(c2.red),
            _lib.ptr(c2.kinematics.free), _lib.ptr(off), _lib.ptr(m), _lib.ptr(v), _lib.ptr(t), _f(c2.offset_lr), _f(b1), _f(b2),
            _f(c2.eps), _f(c2.offset_wd), _lib.ptr(grad), _stream()), "ehr_joint_backward_adam")
        torch.cuda.synchronize()
        return grad, off

    grad, off = alone(K_rendered)
    assert torch.equal(grad, c2.offset_grad) and torch.equal(off, c2.offsets) and float(grad.abs().max()) > 0
    grad_new, _ = alone(c2.K)
    assert not torch.equal(grad_new, c2.offset_grad)              # (the rewritten K gives another gradient: the order shows)
    # a three-group checkpoint resumes
    sd, msd = c2.state_dict(), {k: v.clone() for k, v in m2.state_dict().items()}
    m3 = make()
    m3.load_state_dict(msd)
    c3 = JointIntrinsicsPoseStep(m3, batch, xarm7, qp, free_intrinsics=ALL, init_theta=[0.01, -0.01, 0.01, -0.01])
    c3.load_state_dict(sd)
    c2.step(), c3.step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(_jstate(c2, m2) + _state(c2, m2), _jstate(c3, m3) + _state(c3, m3))):
        assert torch.equal(x, y), k
