"""The Levenberg-Marquardt kernels (csrc/ehr_lm.hip) and easyhec_amd/lm.py on the GPU, against the float64 restatement of
tests/lm_reference.py under its derived bars: the linearisation (matrix bit for bit ehr_pose_forward's, tangents within one
float32 rounding), the update kernel alone on synthetic systems, the composition of one iteration, the loss the solve reports,
monotone descent on the gauge problems, the solve from the start pose against the CPU loop, the polish after Adam,
non-interference with a running solve, a reported iteration, the refusals and determinism.  tests/test_lm_reference.py pins the
reference on the CPU.  Every figure is printed before it is asserted."""
import ctypes
import types

import numpy as np
import pytest
import torch

import fused_loss_reference as R
import information_reference as IR
import joint_reference as JR
import lm_reference as LR
import weighted_loss_reference as WR
from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS53 = 2.0 ** -53


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm
    assert _lib.has_lm()
    return _lib, fused, dr, lm


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def t32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def gauge_model(p):
    from easyhec_amd.rb_solver import RBSolver
    cfg, batch, qp = IR.gauge_batch(p, DEV)
    return RBSolver(cfg, meshes=p.rb.meshes).to(DEV), batch, qp


def soft_problem(xarm7):
    """fused_loss_reference.SOFT_SHAPES[0] as a solve -- xArm7, 2 views (seed 2) at 120x160, zoom 2, the camera pose perturbed,
    binary masks rendered at the true pose -> (make, batch, qpos [B,J])."""
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    H, W, scale, B, zoom, seed = R.SOFT_SHAPES[0]
    K = np.array(scaled_K(XARM7_K_1280x720, scale, W, H, True), dtype=np.float64)
    K[:2, :2] *= zoom
    q, lp = make_views(xarm7, B, seed=seed)
    qp = np.zeros((B, xarm7.chain.dof))
    qp[:, :q.shape[1]] = q
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(DEV)
    m0 = make()
    Kt, lpt = torch.tensor(K, dtype=torch.float32, device=DEV), torch.tensor(lp, device=DEV)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=DEV), lpt), torch.zeros((B, H, W), device=DEV))
    return make, {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(B, 1, 1)}, qp


_GAUGE = {}


def gauge(oracle, xarm7, base):
    if base not in _GAUGE:
        _GAUGE[base] = IR.gauge_problem(oracle, xarm7, base=base)
    return _GAUGE[base]


# ---- 1. linearize ------------------------------------------------------------------------------------------------------------
def _check_linearize(_lib, lm_obj, robot, qp, what, zero_link=False):
    """mvp against ehr_pose_forward (bits); every tangent against lm_reference.tangents under its bar."""
    st = lm_obj.step
    with torch.cuda.device(DEV):
        lm_obj._forward_kinematics(_stream())
        lm_obj._linearize(_stream())
        mvp2, tcj = torch.empty_like(lm_obj.mvp), torch.empty((7, 16), device=DEV)
        _lib.check(_lib.lib().ehr_pose_forward(_lib.ptr(st.model.dof.data), _lib.ptr(st.K), _lib.ptr(st.link_poses), st.B, st.L,
                                               st.H, st.W, ctypes.c_float(st.near), ctypes.c_float(st.far), _lib.ptr(mvp2),
                                               _lib.ptr(tcj), None, None, 0, _stream()), "ehr_pose_forward")
    torch.cuda.synchronize()
    assert torch.equal(lm_obj.mvp, mvp2), f"{what}: mvp is not ehr_pose_forward's"
    dof, K = st.model.dof.detach().cpu().numpy(), st.K.cpu().numpy()
    lp32 = st.link_poses.cpu().numpy()
    free = list(st.free_joints) if lm_obj.F else []
    D = Dabs = None
    if free:
        table = robot.joint_table()
        _, lp64, jf64 = JR.fk(table, qp, st.offsets.cpu().numpy().astype(np.float64))
        D, Dabs = JR.pose_derivatives(table, lp64, jf64), JR.pose_derivatives(table, lp64, jf64, absolute=True)
    free4 = [(lm_obj.free4_mask >> i) & 1 for i in range(4)]
    _, ref, Sabs = LR.tangents(dof, K, st.H, st.W, st.near, st.far, lp32, D, Dabs, free, free4, bool(lm_obj.tie_focal))
    got = lm_obj.dmvp.cpu().numpy().reshape(ref.shape)
    assert ref.shape[0] == lm_obj.N
    nj = len(free)
    rp = LR.tangent_ratio(got[:6], ref[:6], Sabs[:6])
    print(f"[lm linearize] {what}: pose tangents worst |d - ref| / bar = {rp:.3f}")
    assert rp <= 1.0
    if nj:
        rj = LR.tangent_ratio(got[6:6 + nj], ref[6:6 + nj], Sabs[6:6 + nj], roundings=3)
        up = np.asarray(robot.joint_table()["upstream"])
        zero = [(l, j) for l in range(st.L) for j in free if not (int(up[l]) >> j) & 1]
        print(f"[lm linearize] {what}: joint tangents worst |d - ref| / bar = {rj:.3f}; {len(zero)} (link, joint) blocks exactly zero")
        assert rj <= 1.0
        for l, j in zero:
            assert (got[6 + free.index(j), :, l] == 0).all()
        if zero_link:   # a link with none of them upstream
            assert len(zero) > 0 and any(all(not (int(up[l]) >> j) & 1 for j in free) for l in range(st.L))
    if lm_obj.N > 6 + nj:
        ri = LR.tangent_ratio(got[6 + nj:], ref[6 + nj:], Sabs[6 + nj:])
        print(f"[lm linearize] {what}: intrinsics tangents worst |d - ref| / bar = {ri:.3f}")
        assert ri <= 1.0


def test_linearize_xarm7_120x160x2(env, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    make, batch, qp = soft_problem(xarm7)
    off = np.zeros(xarm7.chain.dof, np.float32)
    off[[0, 3, 6]] = [0.01, -0.02, 0.015]
    st = JointIntrinsicsPoseStep(make(), batch, xarm7, qp, free=[0, 3, 6], free_intrinsics=("f", "cx", "cy"), init_offset=off,
                                 init_theta=[0.01, 0.01, -0.02, 0.015])
    o = lm.LevenbergMarquardt(st)
    assert o.names == [f"dof[{i}]" for i in range(6)] + ["offset[0]", "offset[3]", "offset[6]", "theta[f]", "theta[cx]", "theta[cy]"]
    _check_linearize(_lib, o, xarm7, qp, "xarm7 120x160x2, joints [0,3,6], f cx cy", zero_link=True)


def test_linearize_gauge_problem(env, oracle, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    p = gauge(oracle, xarm7, False)
    model, batch, qp = gauge_model(p)
    _check_linearize(_lib, lm.LevenbergMarquardt(JointPoseStep(model, batch, p.rb, qp, free=[0])), p.rb, qp, "gauge, joint 0")
    p = gauge(oracle, xarm7, True)
    model, batch, qp = gauge_model(p)
    st = IntrinsicsPoseStep(model, batch, free=("fx", "fy", "cx", "cy"), init_theta=[0.01, -0.01, 0.02, 0.0])
    _check_linearize(_lib, lm.LevenbergMarquardt(st), p.rb, qp, "gauge with base, fx fy cx cy")


# ---- 2. the update kernel alone ----------------------------------------------------------------------------------------------
UH, UW = 120, 160
K0 = np.array([[226.7, 0, 81.3], [0, 226.6, 61.2], [0, 0, 1]], np.float32)
FTOL = 1e-12   # the synthetic systems' predicted reductions are small next to their losses: the default 1e-6 would stop them
UPDATE_SHAPES = {1: (0, 0, 0), 6: (0, 0, 0), 7: (1, 0, 0), 10: (1, 15, 1), 32: (22, 15, 0)}   # N: (F, free4 mask, tie)


class Upd:
    """The tensors one ehr_lm_update works on, without a renderer."""

    def __init__(self, _lib, N, seed, lambda0=1e-3, zero_theta=True):
        self._lib, self.N = _lib, N
        self.F, self.mask, self.tie = UPDATE_SHAPES[N]
        rng = np.random.default_rng(1000 * N + seed)
        self.J = 32
        self.free = sorted(rng.permutation(self.J)[:self.F].tolist())
        self.free_list = torch.tensor(self.free, dtype=torch.int32, device=DEV) if self.F else None
        self.dof = t32(rng.uniform(-1, 1, 6))
        self.offset = t32(rng.uniform(-0.05, 0.05, self.J))
        th = rng.uniform(-0.02, 0.02, 4).astype(np.float32)
        if self.tie:
            th[1] = th[0]
        if zero_theta:
            th[3] = 0.0                                                           # (an exactly zero theta: K0's bits)
        self.theta = t32(th)
        self.K0, self.K = t32(K0), t32(K0)
        st = np.zeros(_lib.LM_STATE_DOUBLES)
        st[0], st[1] = lambda0, 2.0
        self.state = torch.from_numpy(st).to(DEV)
        self.log = torch.full((64, 4), float("nan"), dtype=torch.float64, device=DEV)
        self.els = LR.intrinsics_elements([(self.mask >> i) & 1 for i in range(4)], bool(self.tie))
        self.offset0, self.theta0 = self.offset.clone(), self.theta.clone()

    def params(self):
        d, o, th = self.dof.cpu().numpy(), self.offset.cpu().numpy(), self.theta.cpu().numpy()
        return np.concatenate([d[:min(self.N, 6)], o[self.free], [th[e[0]] for e in self.els]]).astype(np.float32)

    def call(self, info, grad, count, loss, ftol=1e-6, lambda_max=1e6, finalize=0):
        _lib = self._lib
        ti = torch.tensor(np.ascontiguousarray(info, np.float64), device=DEV)
        tg = torch.tensor(np.ascontiguousarray(grad, np.float64), device=DEV)
        tc = torch.tensor(np.ascontiguousarray(count, np.int64), device=DEV)
        tl = t32(loss)
        intr = self.mask != 0
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update(
                _lib.ptr(ti), _lib.ptr(tg), _lib.ptr(tc), _lib.ptr(tl), info.shape[0], self.N, _lib.ptr(self.dof),
                _lib.ptr(self.offset if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                _lib.ptr(self.theta if intr else None), self.mask, self.tie, _lib.ptr(self.K0 if intr else None),
                _lib.ptr(self.K if intr else None), UH, UW, ctypes.c_double(ftol), ctypes.c_double(lambda_max), finalize,
                _lib.ptr(self.state), _lib.ptr(self.log), 64, _stream()), "ehr_lm_update")
            # the call has read its inputs when the next one starts: garbage proves nothing is read later
            ti.fill_(float("nan")), tg.fill_(float("nan")), tl.fill_(float("nan")), tc.fill_(-7)
        torch.cuda.synchronize()
        return self.ns()

    def ns(self):
        s, N, L = self.state.cpu().numpy(), self.N, self._lib
        ns = types.SimpleNamespace(**{k: s[i] for k, i in L.LM_STATE.items()})
        ns.theta, ns.delta, ns.g = s[L.LM_THETA:L.LM_THETA + N], s[L.LM_DELTA:L.LM_DELTA + N], s[L.LM_G:L.LM_G + N]
        ns.H = s[L.LM_H:L.LM_H + 1024].reshape(32, 32)[:N, :N]
        ns.raw = s.copy()
        return ns


def ref_state(ns):
    """lm_reference's state at the GPU's own previous state."""
    st = LR.new_state()
    st.lam, st.nu, st.F_acc, st.pred, st.rho, st.F_trial = ns.__dict__["lambda"], ns.nu, ns.F_acc, ns.pred, ns.rho, ns.F_trial
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        setattr(st, k, int(getattr(ns, k)))
    st.theta, st.delta, st.g, st.H = ns.theta.copy(), ns.delta.copy(), ns.g.copy(), ns.H.copy()
    return st


def compare(ns, st, got_params, want_params, what, worst):
    """Exact: lambda, nu, F_acc, counters, flags, the stored linearisation and parameters.  delta, pred: the derived bar."""
    assert ns.__dict__["lambda"] == st.lam and ns.nu == st.nu and ns.F_acc == st.F_acc, (what, ns.__dict__["lambda"], st.lam)
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        assert int(getattr(ns, k)) == int(getattr(st, k)), (what, k, getattr(ns, k), getattr(st, k))
    if st.accepted:
        assert (ns.theta == st.theta).all() and (ns.H == st.H).all() and (ns.g == st.g).all(), what
    if st.last != -1 and st.delta is not None and st.cond is not None:
        s = np.sqrt(np.where(np.diag(st.H) > 0, np.diag(st.H), 1.0))
        y, yr = ns.delta * s, st.delta * s
        bar = 32 * EPS53 * st.cond
        ry = float(np.abs(y - yr).max() / max(np.abs(yr).max(), 1e-300)) / bar
        rp = abs(ns.pred - st.pred) / max(abs(st.pred), 1e-300) / bar
        worst[0], worst[1] = max(worst[0], ry), max(worst[1], rp)
        assert ry <= 1.0 and rp <= 1.0, (what, ry, rp, st.cond)
        assert ((st.delta == 0) == (ns.delta == 0)).all(), what
    gp, wp = np.asarray(got_params, np.float32), np.asarray(want_params, np.float32)
    assert (np.abs(gp.astype(np.float64) - wp.astype(np.float64)) <= LR.spacing_f32(wp)).all(), (what, gp, wp)


def system(N, B, seed):
    """info [B,N,N] SPD, scaled condition number <= 1e6, parameters of different units; grad = 2 H x for a small x."""
    rng = np.random.default_rng(77 * N + seed)
    scale = 10.0 ** rng.uniform(-2, 2, N)
    info = np.zeros((B, N, N))
    for b in range(B):
        Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
        M = (Q * 10.0 ** rng.uniform(-5, 0, N)) @ Q.T
        info[b] = 0.5 * (M + M.T) * scale[:, None] * scale[None, :]
    x = rng.normal(size=N) * 1e-3 / scale
    grad = np.stack([2.0 * info[b] @ x for b in range(B)])
    return info, grad, rng.integers(10, 500, B), rng.uniform(10, 100, B).astype(np.float32)


def K_expected(u):
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    return intrinsics_from_theta(K0, u.theta.cpu().numpy(), UH, UW)


def step_and_compare(u, info, grad, count, loss, what, worst, **kw):
    kw.setdefault("ftol", FTOL)
    before, now = ref_state(u.ns()), u.params()
    ns = u.call(info, grad, count, loss, **kw)
    want = LR.update(before, info, grad, count, loss, now, kw["ftol"], kw.get("lambda_max", 1e6))
    compare(ns, before, u.params(), want, what, worst)
    if u.mask:
        assert K_expected(u).tobytes() == u.K.cpu().numpy().tobytes(), f"{what}: K is not intrinsics_from_theta(theta)"
        if u.tie:
            assert u.theta[0].item() == u.theta[1].item()
    return ns, before


def _update_sequence(_lib, N, worst):
    B = 3
    u = Upd(_lib, N, 0)
    info, grad, count, loss = system(N, B, 0)
    ns, st = step_and_compare(u, info, grad, count, loss, f"N={N} first call", worst)
    assert ns.accepted == 1 and ns.__dict__["lambda"] == 1e-3
    # an accept: a lower loss, another linearisation
    info2, grad2, count2, _ = system(N, B, 1)
    lo = (loss * np.float32(0.9)).astype(np.float32)                             # rho >> 1: the factor's floor, 1/3
    ns, st = step_and_compare(u, info2, grad2, count2, lo, f"N={N} accept", worst)
    assert ns.accepted == 2 and ns.nu == 2.0 and ns.__dict__["lambda"] == 1e-3 * (1.0 / 3.0)
    # a reject: the inputs are another system again, the solve must come from the stored H_acc (the reference's does)
    info3, grad3, count3, _ = system(N, B, 2)
    accepted = ns.theta.copy()
    ns, st = step_and_compare(u, info3, grad3, count3, lo * np.float32(1.5), f"N={N} reject", worst)
    assert ns.rejected == 1 and ns.nu == 4.0 and (ns.H == st.H).all() and (ns.theta == accepted).all()
    ns, st = step_and_compare(u, info3, grad3, count3, lo * np.float32(2.0), f"N={N} second reject", worst)
    assert ns.rejected == 2 and ns.nu == 8.0
    # a reported call, four ways: parameters restored, lambda untouched
    lam = ns.__dict__["lambda"]
    for k, bad in enumerate(("info", "grad", "loss", "count")):
        i4, g4, c4, l4 = info.copy(), grad.copy(), count.copy(), lo.copy()
        if bad == "info":
            i4[B - 1, N - 1, 0] = np.nan
        elif bad == "grad":
            g4[0, N - 1] = np.inf
        elif bad == "loss":
            l4[1] = np.nan
        else:
            c4[2] = -1
        ns, st = step_and_compare(u, i4, g4, c4, l4, f"N={N} reported ({bad})", worst)
        assert ns.reported == k + 1 and ns.__dict__["lambda"] == lam and (u.params() == accepted.astype(np.float32)).all()
    assert ns.accepted + ns.rejected + ns.reported == ns.iterations == 8
    # finalize after a trial: the accepted parameters; the state does not move
    ns, st = step_and_compare(u, info3, grad3, count3, lo * np.float32(3.0), f"N={N} third reject", worst)
    assert (u.params() != accepted.astype(np.float32)).any()
    raw = ns.raw
    ns = u.call(info, grad, count, loss, ftol=FTOL, finalize=1)
    assert (u.params() == accepted.astype(np.float32)).all() and ns.raw.tobytes() == raw.tobytes()
    log = u.log.cpu().numpy()[:9]
    assert log[:, 1].tolist() == [1, 1, 0, 0, -1, -1, -1, -1, 0] and np.isnan(log[4:8, 0]).all()
    # what a solve does not own stays: the joints that are not free, theta's elements that are not free
    keep = [j for j in range(u.J) if j not in u.free]
    assert torch.equal(u.offset[keep], u.offset0[keep])
    fixed = [i for i in range(4) if not (u.mask >> i) & 1]
    assert torch.equal(u.theta[fixed], u.theta0[fixed])
    return u


@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_update_kernel_alone(env, N):
    _lib = env[0]
    worst = [0.0, 0.0]
    a = _update_sequence(_lib, N, worst)
    print(f"[lm update] N={N}: worst |y - y_ref| / (32 2^-53 cond |y|) = {worst[0]:.4f}, the same for pred = {worst[1]:.4f}")
    b = _update_sequence(_lib, N, [0.0, 0.0])                                    # two runs: identical bits
    for x, y in ((a.state, b.state), (a.dof, b.dof), (a.offset, b.offset), (a.theta, b.theta), (a.K, b.K), (a.log, b.log)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("N", [1, 6, 7, 10, 32])
def test_update_kernel_zero_diagonal_and_stopping_rules(env, N):
    _lib = env[0]
    worst = [0.0, 0.0]
    info, grad, count, loss = system(N, 2, 5)
    # a parameter without information: delta exactly 0, the parameter stays
    z = max(N - 2, 0)
    iz, gz = info.copy(), grad.copy()
    iz[:, z, :], iz[:, :, z], gz[:, z] = 0.0, 0.0, 0.0
    u = Upd(_lib, N, 1)
    p0 = u.params()
    ns, st = step_and_compare(u, iz, gz, count, loss, f"N={N} zero diagonal", worst)
    assert ns.delta[z] == 0.0 and u.params()[z] == p0[z] and (ns.delta[[k for k in range(N) if k != z]] != 0).all()
    if N == 1:   # nothing is left to move: the predicted reduction is 0 and the ftol rule stops the solve
        assert (ns.done, ns.why, ns.pred) == (1, 1, 0.0)
    # the three rules, each from a fresh state; done: the accepted parameters stay, later calls only restore them
    for kw, why, scale in (({"ftol": 1e30}, 1, 1.0), ({"lambda_max": 1e-3, "ftol": 0.0}, 2, 1.0), ({"ftol": 0.0}, 3, 1e24)):
        u = Upd(_lib, N, 2, zero_theta=False)
        p0 = u.params()
        ns, st = step_and_compare(u, info * scale, grad, count, loss, f"N={N} stop {why}", worst, **kw)
        assert (ns.done, ns.why) == (1, why) and (u.params() == p0).all()
        raw = ns.raw
        u.dof.fill_(9.0)
        ns = u.call(info, grad, count, loss, ftol=FTOL)
        assert ns.raw.tobytes() == raw.tobytes() and (u.params() == p0).all()
    print(f"[lm update] N={N} zero diagonal / stops: worst ratios {worst[0]:.4f}, {worst[1]:.4f}")


# ---- 3. composition ----------------------------------------------------------------------------------------------------------
def _make_step(kind, xarm7):
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    make, batch, qp = soft_problem(xarm7)
    if kind == "pose":
        return FusedPoseStep(make(), batch)
    return JointIntrinsicsPoseStep(make(), batch, xarm7, qp, free=[1, 3], free_intrinsics=("f",))


def _params_of(o):
    st = o.step
    out = [st.model.dof.detach().cpu().numpy()]
    if o.F:
        out.append(st.offsets.cpu().numpy()[list(st.free_joints)])
    if o.free4_mask:
        th = st.theta.cpu().numpy()
        out.append(np.array([th[e[0]] for e in LR.intrinsics_elements([(o.free4_mask >> i) & 1 for i in range(4)], bool(o.tie_focal))]))
    return np.concatenate(out).astype(np.float32)


def _ns_of(_lib, o):
    u = types.SimpleNamespace(state=o.state_block, N=o.N, _lib=_lib)
    return Upd.ns(u)


@pytest.mark.parametrize("kind", ["pose", "joints+f"])
def test_iterate_is_linearize_information_update(env, xarm7, kind):
    """Three consecutive iterations, each against: ehr_lm_linearize into buffers of its own, mask_information on them, and the
    reference update from the GPU's own previous state."""
    _lib, fused, dr, lm = env
    from easyhec_amd import information
    st = _make_step(kind, xarm7)
    o = lm.LevenbergMarquardt(st)
    worst = [0.0, 0.0]
    for it in range(3):
        before, now = ref_state(_ns_of(_lib, o)), _params_of(o)
        keep = (o.mvp, o.dmvp)
        o.mvp, o.dmvp = torch.empty_like(keep[0]), torch.empty_like(keep[1])
        with torch.cuda.device(DEV):
            o._forward_kinematics(_stream())
            o._linearize(_stream())
        mine = information.mask_information(st.glctx, st.scene, o.mvp, o.dmvp, st.ref, want_loss=True)
        own_mvp, own_dmvp = o.mvp, o.dmvp
        o.mvp, o.dmvp = keep
        o.iterate(1)
        torch.cuda.synchronize()
        fused.check_status(st.glctx)
        assert torch.equal(own_mvp, o.mvp) and torch.equal(own_dmvp, o.dmvp)
        for a, b in ((mine.info, o.out.info), (mine.grad, o.out.grad), (mine.count, o.out.count), (mine.loss, o.out.loss)):
            assert torch.equal(a, b)
        want = LR.update(before, mine.info.cpu().numpy(), mine.grad.cpu().numpy(), mine.count.cpu().numpy(),
                         mine.loss.cpu().numpy(), now)
        compare(_ns_of(_lib, o), before, _params_of(o), want, f"{kind} iteration {it}", worst)
        if o.free4_mask:
            from easyhec_amd.intrinsics_calib import intrinsics_from_theta
            K = intrinsics_from_theta(st.K0.cpu().numpy(), st.theta.cpu().numpy(), st.H, st.W)
            assert K.tobytes() == st.K.cpu().numpy().tobytes()
    print(f"[lm composition] {kind}: worst delta / pred ratios {worst[0]:.4f}, {worst[1]:.4f}; state {o.state().__dict__['F_acc']:.3f}")
    assert o.state().accepted >= 1


# ---- 4. the loss is the solve's loss -----------------------------------------------------------------------------------------
def _loss_at_accepted(fused, dr, o, weight=None):
    """float64 sum, in view order, of render_mask_loss (another context) on the linearize kernel's mvp at the step's parameters."""
    st = o.step
    with torch.cuda.device(DEV):
        o._forward_kinematics(_stream())
        o._linearize(_stream())
    _, loss = fused.render_mask_loss(dr.RasterizeCudaContext(), st.scene, o.mvp.clone(), st.ref.clone(), want_mask=False, weight=weight)
    torch.cuda.synchronize()
    F = 0.0
    for x in loss.detach().cpu().numpy():
        F += float(x)
    return F


def test_accepted_loss_is_render_mask_loss(env, xarm7):
    _lib, fused, dr, lm = env
    o = lm.LevenbergMarquardt(_make_step("joints+f", xarm7))
    o.iterate(6).finalize()
    s = o.state()
    F = _loss_at_accepted(fused, dr, o)
    print(f"[lm loss] F_acc {s.F_acc!r}, render_mask_loss at the accepted parameters {F!r}; {s.accepted} accepted of {s.iterations}")
    assert F == s.F_acc and s.accepted >= 2


# ---- 5. monotone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pose", "offset0-gauge", "f-cx-cy"])
def test_monotone_on_the_gauge_problem(env, oracle, xarm7, kind):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    p = gauge(oracle, xarm7, kind != "offset0-gauge")
    model, batch, qp = gauge_model(p)
    if kind == "pose":
        st = FusedPoseStep(model, batch)
    elif kind == "offset0-gauge":
        st = JointPoseStep(model, batch, p.rb, qp, free=[0])     # no base link: H is singular, the damping carries it
    else:
        st = IntrinsicsPoseStep(model, batch, free=("f", "cx", "cy"))
    o = lm.LevenbergMarquardt(st)
    o.iterate(20).finalize()
    s, tr = o.state(), o.trajectory()
    fused.check_status(st.glctx)
    acc = tr[tr[:, 1] == 1, 0]
    print(f"[lm monotone] {kind}: accepted losses {np.round(acc, 2).tolist()}; {s.accepted} accepted, {s.rejected} rejected, "
          f"{s.reported} reported, done {s.done} ({LR.WHY[s.why]}), lambda {s.__dict__['lambda']:.3g}")
    assert (np.diff(acc) < 0).all() and len(acc) >= 3 and acc[-1] == s.F_acc
    assert s.accepted + s.rejected + s.reported == s.iterations and (s.iterations == 20 or s.done)
    assert np.isfinite(_params_of(o)).all() and np.isfinite(st.K.cpu().numpy()).all()
    assert (_params_of(o) == s.theta.astype(np.float32)).all()


# ---- 6. end to end from the start pose --------------------------------------------------------------------------------------
def test_solve_from_the_start_pose_against_the_cpu_loop(env, oracle, xarm7):
    """GPU accepted loss after at most 12 iterations <= 1.5 x the CPU loop's loss after its 7th evaluation (the factor: the GPU
    trajectory differs by flipped razor-edge pixels; one accepted-then-rejected cycle of the reference loop moves the loss by
    less)."""
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    p = gauge(oracle, xarm7, True)
    _, traj, _ = LR.cpu_lm_loop(oracle, p, 7)
    F7 = [F for F, a in traj if a][-1]
    assert len(traj) == 8 and np.isclose(F7, LR.MEASURED["F7"], rtol=1e-6)
    model, batch, _ = gauge_model(p)
    o = lm.LevenbergMarquardt(FusedPoseStep(model, batch))
    o.iterate(12).finalize()
    s, tr = o.state(), o.trajectory()
    first = int(np.argmax((tr[:, 1] == 1) & (tr[:, 0] <= 1.5 * F7))) if ((tr[:, 1] == 1) & (tr[:, 0] <= 1.5 * F7)).any() else -1
    print(f"[lm end to end] CPU loop F7 = {F7:.2f}; GPU losses per iteration {np.round(tr[:, 0], 2).tolist()}, accepted "
          f"{tr[:, 1].astype(int).tolist()}; F_acc after {s.iterations} iterations {s.F_acc:.2f}; first <= 1.5 F7 at iteration {first}")
    assert s.F_acc <= 1.5 * F7


# ---- 7. polish after Adam ----------------------------------------------------------------------------------------------------
def test_polish_after_adam(env, oracle, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    p = gauge(oracle, xarm7, True)
    model, batch, _ = gauge_model(p)
    st = FusedPoseStep(model, batch)
    st.capture()
    adam = st.take_effective_steps(400, "test")[:400, 0].numpy().astype(np.float64) * st.B      # summed, like F
    res = lm.solve_lm(st, max_iters=25)
    first = res.trajectory[0, 0]
    print(f"[lm polish] Adam 400 steps: last {adam[-1]:.2f}, best {adam.min():.2f}; LM first evaluation {first:.2f} -> {res.loss:.2f} "
          f"in {res.iterations} iterations ({res.accepted} accepted), stopped by {res.why}")
    assert res.loss <= first
    assert res.done or res.iterations - res.reported >= 25
    assert res.report.names == [f"dof[{i}]" for i in range(6)] and res.report.loss == res.loss and res.report.count > 0
    assert (res.report.H == res.state.H).all()
    st.release_graph()


# ---- 8. non-interference -----------------------------------------------------------------------------------------------------
def test_lm_does_not_disturb_the_adam_state_or_a_captured_chain(env, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 120, 160, 0.125)
    model = make()
    st = FusedPoseStep(model, batch)
    st.capture()
    for _ in range(10):
        st.step()
    torch.cuda.synchronize()
    snap = lambda: [st.exp_avg.clone(), st.exp_avg_sq.clone(), st.step_t.clone(), st.hist_row.clone(), model.history_ops.clone()]
    a = snap()
    res = lm.solve_lm(st, max_iters=5)
    torch.cuda.synchronize()
    for x, y in zip(a, snap()):
        assert torch.equal(x, y)
    assert res.accepted >= 1 and int(st.step_t) == 10 and st._graph
    # the captured chain replays and gives the bits of an uncaptured step from the same state
    model2 = make()
    st2 = FusedPoseStep(model2, batch)
    model2.dof.data.copy_(model.dof.data)
    model2.history_ops.copy_(model.history_ops)
    for x, y in ((st2.exp_avg, st.exp_avg), (st2.exp_avg_sq, st.exp_avg_sq), (st2.step_t, st.step_t), (st2.hist_row, st.hist_row)):
        x.copy_(y)
    st.step()
    st2.step()
    torch.cuda.synchronize()
    for x, y in ((model.dof.data, model2.dof.data), (st.exp_avg, st2.exp_avg), (st.exp_avg_sq, st2.exp_avg_sq), (st.loss, st2.loss),
                 (st.step_t, st2.step_t), (model.history_ops, model2.history_ops), (st.grad_mvp, st2.grad_mvp)):
        assert torch.equal(x, y)
    assert int(st.step_t) == 11 and bool(torch.isfinite(st.loss).all())
    st.release_graph()


def test_bound_weights_are_honoured(env, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    w = WR.binary_weight("tiles", batch["mask"].cpu().numpy())
    batch = dict(batch, weight=torch.tensor(w, device=DEV))
    st = FusedPoseStep(make(), batch)
    o = lm.LevenbergMarquardt(st)
    o.iterate(4).finalize()
    s = o.state()
    Fw, F1 = _loss_at_accepted(fused, dr, o, weight=st.weight.clone()), _loss_at_accepted(fused, dr, o)
    print(f"[lm weights] F_acc {s.F_acc!r}; weighted render_mask_loss {Fw!r}; unweighted {F1!r}")
    assert s.F_acc == Fw and Fw < F1
    other = torch.ones_like(st.weight)
    fused.bind_weight(st.glctx, st.scene, other, views=st.B)                     # somebody else used the context
    with pytest.raises(RuntimeError, match="weights bound"):
        o.iterate(1)


# ---- 9. a reported iteration -------------------------------------------------------------------------------------------------
def test_reported_iteration_is_recovered(env, xarm7, monkeypatch):
    """The slot-limited plan of test_gpu_fused.py::test_default_launch_chain_recovers_from_a_slot_overflow, through solve_lm: the
    first iteration is reported, the plan is made again with every slot, and the solve ends on the bits of a solve that had
    every slot from the start."""
    _lib, fused, dr, lm = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.rb_solver import RBSolver
    from test_gpu_fused import workload
    H, W, B = 64, 96, 2
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=DEV)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=DEV),
             "K": torch.tensor(K, dtype=torch.float32, device=DEV)[None].repeat(B, 1, 1)}
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    ends = []
    for slack in (None, 0.0):
        model = RBSolver(cfg, meshes=xarm7.meshes).to(DEV)
        st = FusedPoseStep(model, batch, slack=slack)
        res = lm.solve_lm(st, max_iters=6, check_every=2)
        if slack is None:
            assert res.reported >= 1 and res.recoveries == ["job slots"] and st.slack == 0.0
        else:
            assert res.reported == 0 and res.recoveries == []
        assert res.iterations - res.reported >= 6 or res.done
        ends.append((model.dof.detach().clone(), res))
    a, b = ends[0][1], ends[1][1]
    print(f"[lm reported] limited plan: {a.reported} reported of {a.iterations}, F_acc {a.loss:.3f}; every slot: {b.iterations} iterations, F_acc {b.loss:.3f}")
    assert torch.equal(ends[0][0], ends[1][0]) and a.loss == b.loss and (a.state.theta == b.state.theta).all()
    assert (a.state.H == b.state.H).all() and a.state.__dict__["lambda"] == b.state.__dict__["lambda"] and a.accepted == b.accepted


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(env, xarm7, monkeypatch):
    _lib, fused, dr, lm = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    from easyhec_amd.rig_calib import RigJointStep
    from easyhec_amd.synthetic import camera_Tc_c2b
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    ms = MultiStartPoseStep(make(), batch, sample_starts(camera_Tc_c2b(), 2, 0.002, 0.3, seed=2))
    with pytest.raises(ValueError, match="multi-start"):
        lm.solve_lm(ms)
    with pytest.raises(ValueError, match="one system over several contexts"):
        lm.LevenbergMarquardt(RigJointStep.__new__(RigJointStep))
    st = FusedPoseStep(make(), batch)
    st.distributed = True
    with pytest.raises(ValueError, match="data-parallel"):
        lm.solve_lm(st)
    st.distributed = False
    with pytest.raises(TypeError, match="not a launch-chain step"):
        lm.solve_lm(object())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="being captured"):
        lm.solve_lm(st)
    monkeypatch.undo()
    o = lm.LevenbergMarquardt(st)
    fused._ensure_plan(st.glctx, st.scene, 1, st.H, st.W)                        # somebody else planned on the context
    with pytest.raises(RuntimeError, match="another plan"):
        o.iterate(1)
    import easyhec_amd
    assert easyhec_amd.solve_lm is lm.solve_lm and easyhec_amd.LevenbergMarquardt is lm.LevenbergMarquardt


# ---- 11. determinism ---------------------------------------------------------------------------------------------------------
def test_two_solves_end_on_identical_bits(env, oracle, xarm7):
    _lib, fused, dr, lm = env
    from easyhec_amd.joint_calib import JointPoseStep
    p = gauge(oracle, xarm7, True)
    ends = []
    for _ in range(2):
        model, batch, qp = gauge_model(p)
        st = JointPoseStep(model, batch, p.rb, qp, free=[1, 2, 3])
        res = lm.solve_lm(st, max_iters=8, check_every=3)
        ends.append((res.lm.state_block.cpu().numpy().tobytes(), model.dof.detach().cpu().numpy().tobytes(),
                     st.offsets.cpu().numpy().tobytes(), res.trajectory.tobytes(), st.link_poses.cpu().numpy().tobytes()))
    assert ends[0] == ends[1]
