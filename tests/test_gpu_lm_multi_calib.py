"""Multi-start Levenberg-Marquardt with joint offsets, intrinsics and priors per hypothesis on the GPU
(``ehr_joint_forward_multi`` / ``ehr_lm_linearize_multi_calib`` / ``ehr_lm_update_multi_calib``, easyhec_amd/lm_multi.py; DESIGN.md
section 6q).  The anchor is SOLO EQUALITY, as for tests/test_gpu_lm_multi.py: hypothesis p holds, bit for bit, what the solo
kernels and the solo ``solve_lm`` on a ``JointPoseStep`` / ``IntrinsicsPoseStep`` / ``JointIntrinsicsPoseStep`` built on start p
hold.  No tolerance anywhere: ``torch.equal``, or byte equality (``same``) where NaN may be held.  xArm7 at 120x160 throughout."""
import ctypes

import numpy as np
import pytest
import torch

import lm_multi_reference as MR
from test_gpu_joint_offsets import _dev_table, _qpos, _table, _views_qpos
from test_gpu_lm import soft_problem
from test_gpu_lm_multi import DEV, H, W, _stream, same, setup, t32, t64

pytestmark = pytest.mark.gpu

FREE = [1, 3]
K0 = np.array([[230.0, 0.0, 81.5], [0.0, 228.0, 58.25], [0.0, 0.0, 1.0]], dtype=np.float32)
# N -> (F, J, free4_mask, tie_focal): 7 = pose + tied focal; 12 = pose + 2 joints + fx fy cx cy; 32 = pose + 22 joints + fx fy cx cy
LAYOUTS = {7: (0, 0, 3, 1), 12: (2, 9, 15, 0), 32: (22, 32, 15, 0)}
ROWS = 16


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm, lm_multi
    assert _lib.has_lm_multi_calib()
    return _lib, fused, dr, lm, lm_multi


def _ti(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)


# ---- 1. kinematics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,every", [("xarm7", False), ("xarm7", True)])   # (the table of EVERY link: the prismatic fingers)
@pytest.mark.parametrize("P,Bv", [(1, 2), (3, 2), (5, 1)])
def test_kinematics_blocks_are_the_solo_kernel_s(env, name, every, P, Bv):
    _lib = env[0]
    t = _table(name, every)
    d = _dev_table(t)
    tab = [_lib.ptr(d[k]) for k in ("parent", "origin", "kind", "axis", "qidx", "use")]
    q = _qpos(name, Bv, 11)
    J, N, L = q.shape[1], t["parent"].shape[0], t["use"].shape[0]
    assert not every or 2 in np.asarray(t["kind"])[np.asarray(t["qidx"]) >= 0]
    off = np.random.default_rng(3).uniform(-0.03, 0.03, (P, J)).astype(np.float32)
    off[P // 2] = 0.0                                                            # one row all zero
    qd, od = t64(q), t32(off)
    lp = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    jf = torch.full((P * Bv, J, 6), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_joint_forward_multi(*tab, N, J, L, _lib.ptr(qd), _lib.ptr(od), P, Bv, _lib.ptr(lp), _lib.ptr(jf),
                                                      _stream()), "ehr_joint_forward_multi")
        for p in range(P):
            lp1 = torch.full((Bv, L, 4, 4), float("nan"), device=DEV)
            jf1 = torch.full((Bv, J, 6), float("nan"), device=DEV)
            op = od[p].contiguous()
            _lib.check(_lib.lib().ehr_joint_forward(*tab, N, J, L, _lib.ptr(qd), _lib.ptr(op), Bv, _lib.ptr(lp1), _lib.ptr(jf1),
                                                    _stream()), "ehr_joint_forward")
            torch.cuda.synchronize()
            v = slice(p * Bv, (p + 1) * Bv)
            assert same(lp[v], lp1), (p, "link_poses")
            assert same(jf[v], jf1), (p, "joint_frames")
    assert bool(torch.isfinite(lp).all())
    assert P == 1 or not same(lp[:Bv], lp[Bv:2 * Bv])


# ---- 2. linearize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("free,intr", [([1, 3], None), ([], ("f",)), ([], ("fx", "fy", "cx", "cy")), ([1, 3], ("f",))])
@pytest.mark.parametrize("P,Bv", [(3, 2), (5, 1)])
def test_linearize_blocks_are_the_solo_kernel_s(env, xarm7, free, intr, P, Bv):
    _lib = env[0]
    from easyhec_amd.intrinsics_calib import _parse_free
    from easyhec_amd.joint_calib import joint_kinds
    from easyhec_amd.multistart import _starts_to_dof
    make, batch, starts, _ = setup(xarm7, Bv, P)
    t = xarm7.joint_table()
    d = _dev_table(t)
    tab = [_lib.ptr(d[k]) for k in ("parent", "origin", "kind", "axis", "qidx", "use")]
    qp = _views_qpos(xarm7, Bv)
    J, NL, L = qp.shape[1], t["parent"].shape[0], t["use"].shape[0]
    rng = np.random.default_rng(17)
    off = t32(rng.uniform(-0.02, 0.02, (P, J)))
    lp, jf = torch.empty((P * Bv, L, 4, 4), device=DEV), torch.empty((P * Bv, J, 6), device=DEV)
    dof = _starts_to_dof(starts).to(DEV)
    Kp = batch["K"][0].cpu().numpy()[None].repeat(P, 0).copy()
    Kp[:, 0, 0] *= 1.0 + 0.01 * np.arange(P)                                     # a different K row per hypothesis
    Kp[:, 1, 1] *= 1.0 - 0.01 * np.arange(P)
    Kp[:, 0, 2] += np.arange(P)
    Kp = t32(Kp)
    F = len(free)
    mask, tie = 0, 0
    if intr is not None:
        m4, tie, _ = _parse_free(intr)
        mask = sum(1 << i for i in range(4) if m4[i])
    N = 6 + F + (0 if intr is None else len(intr))
    fl = _ti(free) if F else None
    up = _ti(np.asarray(t["upstream"]).astype(np.uint32).view(np.int32))
    jk = _ti(joint_kinds(t))
    near, far = ctypes.c_float(0.001), ctypes.c_float(10.0)
    mvp = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    dmvp = torch.full((N, P * Bv, L, 4, 4), float("nan"), device=DEV)
    qd = t64(qp)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_joint_forward_multi(*tab, NL, J, L, _lib.ptr(qd), _lib.ptr(off), P, Bv, _lib.ptr(lp),
                                                      _lib.ptr(jf), _stream()), "ehr_joint_forward_multi")
        _lib.check(_lib.lib().ehr_lm_linearize_multi_calib(
            _lib.ptr(dof), _lib.ptr(Kp), _lib.ptr(lp), P, Bv, L, H, W, near, far, _lib.ptr(jf if F else None),
            _lib.ptr(up if F else None), _lib.ptr(jk if F else None), _lib.ptr(fl), F, J if F else 0, mask, tie, N, _lib.ptr(mvp),
            _lib.ptr(dmvp), _stream()), "ehr_lm_linearize_multi_calib")
        for p in range(P):
            v = slice(p * Bv, (p + 1) * Bv)
            m1, d1 = torch.empty((Bv, L, 4, 4), device=DEV), torch.empty((N, Bv, L, 4, 4), device=DEV)
            lpp, jfp = lp[v].contiguous(), jf[v].contiguous()
            _lib.check(_lib.lib().ehr_lm_linearize(
                _lib.ptr(dof[p].contiguous()), _lib.ptr(Kp[p].contiguous()), _lib.ptr(lpp), Bv, L, H, W, near, far,
                _lib.ptr(jfp if F else None), _lib.ptr(up if F else None), _lib.ptr(jk if F else None), _lib.ptr(fl), F,
                J if F else 0, mask, tie, N, _lib.ptr(m1), _lib.ptr(d1), _stream()), "ehr_lm_linearize")
            torch.cuda.synchronize()
            assert torch.equal(mvp[v], m1), (p, "mvp")
            assert torch.equal(dmvp[:, v], d1), (p, "dmvp")
    assert bool(torch.isfinite(mvp).all()) and bool(torch.isfinite(dmvp).all())
    assert not torch.equal(mvp[:Bv], mvp[Bv:2 * Bv]) and bool((dmvp[6:].abs().amax(dim=(1, 2, 3, 4)) > 0).all())


# ---- 3. the update kernel alone ----------------------------------------------------------------------------------------------
class Calib:
    """The tensors one ehr_lm_update_multi_calib works on, and per hypothesis those of the solo ehr_lm_update[_prior]."""

    def __init__(self, _lib, N, P, Bv, prior, layout=None):
        self._lib, self.N, self.P, self.Bv = _lib, N, P, Bv
        self.F, self.J, self.mask, self.tie = LAYOUTS[N] if layout is None else layout
        rng = np.random.default_rng(900 + N)
        self.free = sorted(rng.permutation(self.J)[:self.F].tolist())
        self.fl = _ti(self.free) if self.F else None
        st = np.zeros((P, _lib.LM_STATE_DOUBLES))
        st[:, 0], st[:, 1] = 1e-3, 2.0
        th = rng.uniform(-0.02, 0.02, (P, 4)).astype(np.float32)
        if self.tie:
            th[:, 1] = th[:, 0]
        th[0, 3] = 0.0                                                           # (an exactly zero theta: K0's bits)
        self.dof, self.state = t32(MR.start_dof(P)), t64(st)
        self.offset = t32(rng.uniform(-0.05, 0.05, (P, max(self.J, 1))))
        self.theta, self.K0, self.K = t32(th), t32(K0), t32(K0[None].repeat(P, 0))
        self.log = torch.full((P, ROWS, 4), float("nan"), dtype=torch.float64, device=DEV)
        self.pw = self.pm = None
        if prior:                                                                # a row per hypothesis; some parameters without
            w = rng.uniform(0.5, 4.0, (P, N))
            w[:, ::3] = 0.0
            self.pw, self.pm = t64(w), t64(rng.uniform(-0.01, 0.01, (P, N)))
        self.names = ("dof", "offset", "theta", "K", "state", "log")
        self.solo = [{k: getattr(self, k)[p].clone() for k in self.names} for p in range(P)]

    def call(self, info, grad, count, loss, finalize=0):
        _lib, N, P, Bv = self._lib, self.N, self.P, self.Bv
        ti, tg, tl = t64(info), t64(grad), t32(loss)
        tc = torch.tensor(np.ascontiguousarray(count, np.int64), device=DEV)
        ftol, lmax = ctypes.c_double(MR.FTOL), ctypes.c_double(1e6)
        intr = self.mask != 0
        lay = lambda off, th, K: (_lib.ptr(off if self.F else None), _lib.ptr(self.fl), self.F, self.J, _lib.ptr(th if intr else None),
                                  self.mask, self.tie, _lib.ptr(self.K0 if intr else None), _lib.ptr(K if intr else None), H, W,
                                  ftol, lmax, finalize)
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update_multi_calib(
                _lib.ptr(ti), _lib.ptr(tg), _lib.ptr(tc), _lib.ptr(tl), P, Bv, N, _lib.ptr(self.dof),
                *lay(self.offset, self.theta, self.K), _lib.ptr(self.state), _lib.ptr(self.log), ROWS, _lib.ptr(self.pw),
                _lib.ptr(self.pm), _stream()), "ehr_lm_update_multi_calib")
            for p, s in enumerate(self.solo):
                v = slice(p * Bv, (p + 1) * Bv)
                si, sg, sc, sl = ti[v].contiguous(), tg[v].contiguous(), tc[v].contiguous(), tl[v].contiguous()
                args = (_lib.ptr(si), _lib.ptr(sg), _lib.ptr(sc), _lib.ptr(sl), Bv, N, _lib.ptr(s["dof"]),
                        *lay(s["offset"], s["theta"], s["K"]), _lib.ptr(s["state"]), _lib.ptr(s["log"]), ROWS)
                if self.pw is None:
                    _lib.check(_lib.lib().ehr_lm_update(*args, _stream()), "ehr_lm_update")
                else:
                    pw, pm = self.pw[p].contiguous(), self.pm[p].contiguous()
                    _lib.check(_lib.lib().ehr_lm_update_prior(*args, _lib.ptr(pw), _lib.ptr(pm), _stream()), "ehr_lm_update_prior")
                torch.cuda.synchronize()

    def assert_equal_solo(self, what):
        for p, s in enumerate(self.solo):
            for k in self.names:
                assert same(getattr(self, k)[p], s[k]), (what, p, k)

    def flags(self, block):
        s = block.cpu().numpy()
        L = self._lib.LM_STATE
        return {k: int(s[L[k]]) for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last")}


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("N", [7, 12, 32])
def test_update_kernel_alone(env, N, prior):
    """The scripted calls of tests/lm_multi_reference.py (accepts, rejects, a NaN in hypothesis 1's grad, hypothesis 0 stopped by
    call 4 while the others move), each compared with the solo kernel -- ``ehr_lm_update``, or ``ehr_lm_update_prior`` on
    hypothesis p's prior rows -- driven by the same inputs; then finalize.  The script's flags are asserted without a prior (its
    losses are scripted for the data's objective alone)."""
    _lib = env[0]
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    P, Bv = 3, 2
    u = Calib(_lib, N, P, Bv, prior)
    th0, off0 = u.theta.clone(), u.offset.clone()
    calls = MR.scripted_calls(N, P, Bv)
    for c, (info, grad, count, loss) in enumerate(calls):
        before_state, before_dof = u.state.clone(), u.dof.clone()
        u.call(info, grad, count, loss)
        u.assert_equal_solo(f"N={N} call {c}")
        for p in range(P):
            f = u.flags(u.solo[p]["state"])
            if not prior:
                assert (f["last"], f["done"]) == MR.expected_flags(p, c), (p, c, f)
            assert u.K[p].cpu().numpy().tobytes() == intrinsics_from_theta(K0, u.theta[p].cpu().numpy(), H, W).tobytes(), (p, c)
            assert not u.tie or u.theta[p, 0].item() == u.theta[p, 1].item()
        if not prior and c >= 5:   # hypothesis 0 is done: its block's bytes stay; hypothesis 1 moves
            assert same(u.state[0], before_state[0]) and same(u.dof[0], before_dof[0])
            assert not same(u.state[1], before_state[1])
        if not prior and c == 5:   # the NaN in hypothesis 1's grad: one reported call, nobody else's
            assert u.flags(u.state[1])["reported"] == 1 and u.flags(u.state[2])["reported"] == 0
            assert not same(u.dof[2], before_dof[2])
    assert not torch.equal(u.theta, th0) and (u.F == 0 or not torch.equal(u.offset, off0))
    if u.tie:
        assert not torch.equal(u.theta[:, 0], th0[:, 0]) and torch.equal(u.theta[:, 2:], th0[:, 2:])
    if u.F:                                                                      # the offsets of joints that are not free stay
        rest = [j for j in range(u.J) if j not in u.free]
        assert torch.equal(u.offset[:, rest], off0[:, rest])
    raw, log = u.state.clone(), u.log.clone()
    u.call(*calls[0], finalize=1)
    u.assert_equal_solo(f"N={N} finalize")
    assert same(u.state, raw) and same(u.log, log)
    TH = _lib.LM_THETA
    for p in range(P):
        assert torch.equal(u.dof[p], u.state[p, TH:TH + 6].float()), p


def test_update_kernel_zero_diagonal(env):
    """A parameter without information in hypothesis 1 alone (a free joint's offset): its delta is exactly 0 there."""
    _lib = env[0]
    N, P, Bv, z = 12, 3, 2, 7
    parts = [MR.system(N, Bv, 300 + p) for p in range(P)]
    parts[1][0][:, z, :], parts[1][0][:, :, z], parts[1][1][:, z] = 0.0, 0.0, 0.0
    u = Calib(_lib, N, P, Bv, False)
    o0 = u.offset.clone()
    u.call(*(np.concatenate([x[i] for x in parts]) for i in range(4)))
    u.assert_equal_solo("zero diagonal")
    D = _lib.LM_DELTA
    delta = u.state[:, D:D + N].cpu().numpy()
    j = u.free[z - 6]
    assert delta[1, z] == 0.0 and (np.delete(delta[1], z) != 0).all() and (delta[[0, 2]] != 0).all()
    assert u.offset[1, j] == o0[1, j] and bool((u.offset[[0, 2], j] != o0[[0, 2], j]).all())


@pytest.mark.parametrize("N", [1, 6])
def test_update_kernel_pose_only_is_ehr_lm_update_multi(env, N):
    """At F = 0 and mask 0 the new entry gives ``ehr_lm_update_multi``'s bytes."""
    _lib = env[0]
    P, Bv = 3, 2
    u = Calib(_lib, N, P, Bv, False, layout=(0, 0, 0, 0))
    dof, state, log = u.dof.clone(), u.state.clone(), u.log.clone()
    for c, (info, grad, count, loss) in enumerate(MR.scripted_calls(N, P, Bv)):
        u.call(info, grad, count, loss)
        ti, tg, tl = t64(info), t64(grad), t32(loss)                             # (held: the call reads them after it returns)
        tc = torch.tensor(np.ascontiguousarray(count, np.int64), device=DEV)
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update_multi(
                _lib.ptr(ti), _lib.ptr(tg), _lib.ptr(tc), _lib.ptr(tl), P, Bv, N, _lib.ptr(dof), ctypes.c_double(MR.FTOL),
                ctypes.c_double(1e6), 0, _lib.ptr(state), _lib.ptr(log), ROWS, _stream()), "ehr_lm_update_multi")
            torch.cuda.synchronize()
        assert same(u.dof, dof) and same(u.state, state) and same(u.log, log), c


# ---- 4. composition ----------------------------------------------------------------------------------------------------------
def _solo_step(xarm7, model, batch, qp, free=FREE, intr=("f",)):
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, JointIntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    if free is None:
        return IntrinsicsPoseStep(model, batch, free=intr)
    if intr is None:
        return JointPoseStep(model, batch, xarm7, qp, free=free)
    return JointIntrinsicsPoseStep(model, batch, xarm7, qp, free=free, free_intrinsics=intr)


def assert_hypothesis_is_step(ms, p, st, what=""):
    """Hypothesis p's parameters and buffers against a solo step's."""
    Bv = ms.Bv
    v = slice(p * Bv, (p + 1) * Bv)
    assert torch.equal(ms.dof[p], st.model.dof.detach()), (what, p, "dof")
    if ms.kin is not None:
        assert torch.equal(ms.offsets[p], st.offsets), (what, p, "offsets")
        assert same(ms.link_poses[v], st.link_poses) and same(ms.joint_frames[v], st.joint_frames), (what, p, "kinematics")
    if ms.free4_mask:
        assert torch.equal(ms.theta[p], st.theta) and torch.equal(ms.K[p], st.K), (what, p, "theta / K")


@pytest.mark.parametrize("P,Bv", [(1, 2), (3, 2), (70, 1)])
def test_iterate_equals_the_solo_iteration(env, xarm7, P, Bv):
    """(70, 1): two chunks of the chain; hypotheses on both sides of the boundary are compared."""
    _lib, fused, dr, lm, lm_multi = env
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    qp = _views_qpos(xarm7, Bv)
    model = make()
    dof0, plan0 = model.dof.detach().clone(), getattr(model._ensure_renderer().glctx, "_plan", None)
    ms = lm_multi.MultiStartLM(model, batch, starts, robot=xarm7, qpos=qp, free=FREE, free_intrinsics=("f",))
    assert ms.names == [f"dof[{i}]" for i in range(6)] + ["offset[1]", "offset[3]", "theta[f]"] and ms.N == 9
    assert ms.P == P and ms.B == P * Bv and ms.offsets.shape == (P, xarm7.chain.dof) and ms.K.shape == (P, 3, 3)
    ms.iterate(3)
    torch.cuda.synchronize()
    fused.check_status(ms.glctx)
    S = ms.state()
    assert [s.reported for s in S] == [0] * P and all(s.iterations == 3 or s.done for s in S)
    for p in ([0, 63, 64, 69] if P == 70 else range(P)):
        st = _solo_step(xarm7, solo_model(p), batch, qp)
        o = lm.LevenbergMarquardt(st).iterate(3)
        torch.cuda.synchronize()
        fused.check_status(st.glctx)
        assert o.names == ms.names
        assert same(ms.state_block[p], o.state_block), (p, "state")
        assert same(ms.log[p], o.log), (p, "log")
        assert_hypothesis_is_step(ms, p, st)
        v = slice(p * Bv, (p + 1) * Bv)
        assert same(ms.mvp[v], o.mvp) and same(ms.dmvp[:, v], o.dmvp), (p, "mvp / dmvp")
        assert ms.report(p).H.tobytes() == o.report().H.tobytes() and S[p].accepted >= 1
    assert P == 1 or not same(ms.state_block[0], ms.state_block[1])
    assert bool((ms.offsets[:, FREE] != 0).any()) and bool((ms.theta[:, :2] != 0).any()) and bool((ms.theta[:, 2:] == 0).all())
    assert torch.equal(model.dof.detach(), dof0) and getattr(model._ensure_renderer().glctx, "_plan", None) is plan0


@pytest.mark.parametrize("free,intr", [(FREE, None), (None, ("fx", "fy", "cx", "cy"))])
def test_iterate_joints_only_and_intrinsics_only(env, xarm7, free, intr):
    _lib, fused, dr, lm, lm_multi = env
    P, Bv = 3, 2
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    qp = _views_qpos(xarm7, Bv)
    kw = dict(robot=xarm7, qpos=qp, free=free) if free is not None else {}
    ms = lm_multi.MultiStartLM(make(), batch, starts, free_intrinsics=intr, **kw).iterate(3).finalize()
    torch.cuda.synchronize()
    if free is None:                                                             # the batch's link poses, repeated P times
        assert ms.kin is None and torch.equal(ms.link_poses, batch["link_poses"].repeat(P, 1, 1, 1))
    for p in range(P):
        st = _solo_step(xarm7, solo_model(p), batch, qp, free, intr)
        o = lm.LevenbergMarquardt(st).iterate(3).finalize()
        torch.cuda.synchronize()
        assert o.names == ms.names and same(ms.state_block[p], o.state_block) and same(ms.log[p], o.log), p
        assert_hypothesis_is_step(ms, p, st)


# ---- 5. the whole solve ------------------------------------------------------------------------------------------------------
def assert_result_is_solo(res, p, solo, st):
    assert res.losses[p] == solo.loss and same(res.lm.state_block[p], solo.lm.state_block), p
    assert (res.iterations[p], res.accepted[p], res.rejected[p], res.reported[p], res.done[p], res.why[p]) == \
           (solo.iterations, solo.accepted, solo.rejected, solo.reported, solo.done, solo.why), p
    assert res.trajectories[p].tobytes() == solo.trajectory.tobytes(), p
    assert torch.equal(res.dofs[p], st.model.dof.detach().cpu()), p
    assert torch.equal(res.offsets[p], st.offsets.cpu()) and torch.equal(res.thetas[p], st.theta.cpu()), p
    assert torch.equal(res.Ks[p], st.K.cpu()), p
    assert_hypothesis_is_step(res.lm, p, st, "solve")


@pytest.mark.parametrize("weighted", [False, True])
def test_solve_lm_multi(env, xarm7, weighted):
    _lib, fused, dr, lm, lm_multi = env
    P, Bv = 3, 2
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    qp = _views_qpos(xarm7, Bv)
    if weighted:
        w = torch.ones((Bv, H, W), device=DEV)
        w[:, :, :W // 3] = 0.25
        batch = dict(batch, weight=w)
    model = make()
    dof0, hist0 = model.dof.detach().clone(), model.history_ops.clone()
    plan0 = getattr(model._ensure_renderer().glctx, "_plan", None)
    res = lm_multi.solve_lm_multi(model, batch, starts, max_iters=10, check_every=5, robot=xarm7, qpos=qp, free=FREE,
                                  free_intrinsics=("f",))
    print(f"[lm multi calib solve] weighted {weighted}: losses {res.losses.tolist()}, iterations {res.iterations}, why {res.why}, "
          f"offsets {res.offsets[:, FREE].tolist()}, theta f {res.thetas[:, 0].tolist()}")
    assert res.names == res.lm.names and res.report.names == res.names and res.prior is None and res.posterior is None
    assert same(res.data_losses, res.losses) and (res.prior_losses == 0).all()
    for p in range(P):
        st = _solo_step(xarm7, solo_model(p), batch, qp)
        solo = lm.solve_lm(st, max_iters=10, check_every=5)
        assert_result_is_solo(res, p, solo, st)
    assert res.recoveries == [] and res.winner == res.ranking[0]
    assert torch.equal(model.dof.detach(), dof0) and torch.equal(model.history_ops, hist0)
    assert getattr(model._ensure_renderer().glctx, "_plan", None) is plan0


def test_reported_iterations_are_recovered(env, xarm7, monkeypatch):
    """tests/test_gpu_lm_multi.py's slot-limited close-up with offsets and focal length free: the first iterations are reported,
    the plan is made again with every slot, and every hypothesis ends on the bits of a solve that had them all."""
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.rb_solver import RBSolver
    from test_gpu_fused import workload
    h, w, B, P = 64, 96, 2, 2
    K, lp, Tc, mvp = workload(xarm7, h, w, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = h, w
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, h, w), device=DEV)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=DEV),
             "K": torch.tensor(K, dtype=torch.float32, device=DEV)[None].repeat(B, 1, 1)}
    starts = sample_starts(np.asarray(Tc, dtype=np.float64), P, 0.002, 0.3, seed=2)
    qp = _views_qpos(xarm7, B, seed=3)
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    ends = []
    for slack in (None, 0.0):
        res = lm_multi.solve_lm_multi(RBSolver(cfg, meshes=xarm7.meshes).to(DEV), batch, starts, max_iters=6, check_every=2,
                                      slack=slack, robot=xarm7, qpos=qp, free=FREE, free_intrinsics=("f",))
        if slack is None:
            assert sum(res.reported) >= 1 and res.recoveries == ["job slots"] and res.lm.slack == 0.0
        else:
            assert res.reported == [0] * P and res.recoveries == []
        assert all(res.iterations[p] - res.reported[p] >= 6 or res.done[p] for p in range(P))
        ends.append(res)
    a, b = ends
    print(f"[lm multi calib reported] limited plan: {a.reported} reported of {a.iterations}, F_acc {a.losses.tolist()}; every slot: "
          f"{b.iterations} iterations, F_acc {b.losses.tolist()}")
    for p in range(P):
        sa, sb = a.states[p], b.states[p]
        assert (sa.theta == sb.theta).all() and (sa.H == sb.H).all() and sa.__dict__["lambda"] == sb.__dict__["lambda"]
        assert sa.F_acc == sb.F_acc and sa.accepted == sb.accepted and torch.equal(a.dofs[p], b.dofs[p])
        assert torch.equal(a.offsets[p], b.offsets[p]) and torch.equal(a.Ks[p], b.Ks[p])


# ---- 6. the prior ------------------------------------------------------------------------------------------------------------
def test_prior_with_a_given_sigma2(env, xarm7):
    _lib, fused, dr, lm, lm_multi = env
    P, Bv, s2 = 3, 2, 0.05
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    qp = _views_qpos(xarm7, Bv)
    res = lm_multi.solve_lm_multi(make(), batch, starts, max_iters=10, check_every=5, robot=xarm7, qpos=qp, free=FREE,
                                  free_intrinsics=("f",), prior_sigma="default", sigma2=s2)
    print(f"[lm multi calib prior] losses {res.losses.tolist()} = data {res.data_losses.tolist()} + prior {res.prior_losses.tolist()}")
    pw = res.prior.weight.cpu().numpy()
    assert res.prior.sigma2 == s2 and pw.shape == (P, 9) and (pw == pw[0]).all() and (pw[0, :6] == 0).all() and (pw[0, 6:] > 0).all()
    assert (res.prior.mean.cpu().numpy()[:, 6:] == 0).all()
    assert same(res.data_losses + res.prior_losses, res.losses) and (res.prior_losses > 0).all()
    for p in range(P):
        st = _solo_step(xarm7, solo_model(p), batch, qp)
        solo = lm.solve_lm(st, max_iters=10, check_every=5, prior_sigma="default", sigma2=s2)
        assert_result_is_solo(res, p, solo, st)
        assert res.prior_losses[p] == solo.prior_loss
        assert same(res.prior.weight[p], solo.prior.weight) and same(res.prior.mean[p], solo.prior.mean)
    w = res.winner
    post = res.posterior
    assert post is not None and post.names == res.names and (post.H_views[0] == res.states[w].H).all()
    assert (np.diag(post.H_views[1]) == pw[w]).all() and post.sigma2() == s2


def test_prior_default_sigma2_and_pose_means(env, xarm7):
    """``sigma2=None``: the minimum over the hypotheses of loss / max(count - N, 1), recomputed here from each solo driver's
    ``evaluate()``; a solo solve given that value reproduces its hypothesis.  A user-given pose sigma takes each hypothesis's
    own start as its mean."""
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.multistart import _starts_to_dof
    P, Bv = 3, 2
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    qp = _views_qpos(xarm7, Bv)
    sig = {"translation": 0.05, "revolute": 0.02, "focal": 0.03}
    res = lm_multi.solve_lm_multi(make(), batch, starts, max_iters=8, check_every=4, robot=xarm7, qpos=qp, free=FREE,
                                  free_intrinsics=("f",), prior_sigma=sig)
    each = []
    for p in range(P):
        loss, count = lm.LevenbergMarquardt(_solo_step(xarm7, solo_model(p), batch, qp)).evaluate()
        each.append(loss / max(count - 9, 1))
    print(f"[lm multi calib prior] sigma2 per hypothesis {each}; recorded {res.prior.sigma2!r}")
    assert res.prior.sigma2 == min(each)
    mean = res.prior.mean.cpu().numpy()
    assert np.array_equal(mean[:, :3], _starts_to_dof(starts).numpy()[:, :3].astype(np.float64))
    assert (mean[:, 3:] == 0).all() and (res.prior.weight.cpu().numpy()[:, 3:6] == 0).all()
    assert not np.array_equal(mean[0, :3], mean[1, :3])
    for p in range(P):
        st = _solo_step(xarm7, solo_model(p), batch, qp)
        solo = lm.solve_lm(st, max_iters=8, check_every=4, prior_sigma=sig, sigma2=res.prior.sigma2)
        assert_result_is_solo(res, p, solo, st)
        assert same(res.prior.mean[p], solo.prior.mean)


# ---- 7. the global solve -----------------------------------------------------------------------------------------------------
def test_solve_global_lm_with_a_planted_offset_and_focal_error(env, xarm7):
    """``soft_problem`` seen through encoders whose joint 1 reads one degree low and a focal length given 2 % short: Q = 16
    candidates, P = 3 starts, offsets of joints 1 and 3 and the tied focal length free under the default prior."""
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose
    make, batch, qp = soft_problem(xarm7)
    Q, P, s2 = 16, 3, 0.05
    qbad = qp.copy()
    qbad[:, 1] -= np.radians(1.0)
    Kbad = batch["K"].clone()
    Kbad[:, 0, 0] /= 1.02
    Kbad[:, 1, 1] /= 1.02
    seen = dict(batch, K=Kbad, link_poses=torch.from_numpy(xarm7.link_poses_batch(qbad)).float().to(DEV))
    Tc_true = camera_Tc_c2b()
    Tc_init = perturb_pose(Tc_true)
    kw = dict(robot=xarm7, qpos=qbad, free=FREE, free_intrinsics=("f",), prior_sigma="default", sigma2=s2)
    model = make()
    hist0 = model.history_ops.clone()
    search, res = lm_multi.solve_global_lm(model, seen, Tc_init, Q, P, max_iters=12, **kw)
    assert np.array_equal(search.starts[0], Tc_init) and search.starts.shape == (P, 4, 4)
    st = _solo_step(xarm7, make(), seen, qbad)
    solo = lm.solve_lm(st, max_iters=12, prior_sigma="default", sigma2=s2)
    assert_result_is_solo(res, 0, solo, st)                                      # hypothesis 0 IS the plain full solve
    w = res.winner
    assert np.isfinite(res.losses).all() and res.losses[w] <= res.losses[0]
    assert torch.equal(model.dof.detach().cpu(), res.dofs[w]) and torch.equal(model.history_ops, hist0)
    step = _solo_step(xarm7, make(), seen, qbad)
    assert res.write_into(step) is step
    loss, _ = lm.LevenbergMarquardt(step).evaluate()
    print(f"[lm multi calib global] losses {res.losses.tolist()}, winner {w}, basins {res.basins}; data loss {res.data_losses[w]!r}, "
          f"evaluate() of the written step {loss!r}")
    assert loss == res.data_losses[w] and torch.equal(step.K.cpu(), res.Ks[w]) and torch.equal(step.offsets.cpu(), res.offsets[w])
    from easyhec_amd.se3 import se3_exp_map
    Tc = se3_exp_map(res.dofs[w].double()[None]).permute(0, 2, 1)[0].numpy()
    D = np.linalg.inv(Tc_true) @ Tc
    rot = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
    f_true, f_got, f_given = batch["K"][0, 0, 0].item(), res.Ks[w][0, 0].item(), Kbad[0, 0, 0].item()
    print(f"[lm multi calib global] recovered: offset[1] {np.degrees(res.offsets[w][1].item()):+.3f} deg (planted +1.000), offset[3] "
          f"{np.degrees(res.offsets[w][3].item()):+.3f} deg (planted 0); focal {f_got:.3f} (true {f_true:.3f}, given {f_given:.3f}: "
          f"error {100 * (f_got / f_true - 1):+.3f} %); pose error {1e3 * np.linalg.norm(D[:3, 3]):.2f} mm, {rot:.3f} deg "
          f"(start: {1e3 * np.linalg.norm((np.linalg.inv(Tc_true) @ Tc_init)[:3, 3]):.2f} mm)")
    other = _solo_step(xarm7, make(), seen, qbad, free=[2])
    with pytest.raises(ValueError, match=r"free joints \[1, 3\], the step has \[2\]"):
        res.write_into(other)
    with pytest.raises(ValueError, match="free intrinsics"):
        res.write_into(_solo_step(xarm7, make(), seen, qbad, intr=("fx", "fy")))


# ---- 8. determinism and refusals ---------------------------------------------------------------------------------------------
def test_two_runs_on_two_contexts_end_on_identical_bytes(env, xarm7):
    _lib, fused, dr, lm, lm_multi = env
    make, batch, starts, _ = setup(xarm7, 2, 3)
    qp = _views_qpos(xarm7, 2)
    ends = []
    for _ in range(2):
        res = lm_multi.solve_lm_multi(make(), batch, starts, max_iters=7, check_every=3, robot=xarm7, qpos=qp, free=FREE,
                                      free_intrinsics=("f",), prior_sigma="default", sigma2=0.05)
        o = res.lm
        ends.append(tuple(x.cpu().numpy().tobytes() for x in (o.state_block, o.dof, o.offsets, o.theta, o.K, o.log, o.link_poses))
                    + (res.losses.tobytes(), res.data_losses.tobytes(), o.glctx))
    assert ends[0][:-1] == ends[1][:-1] and ends[0][-1] is not ends[1][-1]


def test_refusals(env, xarm7, monkeypatch):
    _lib, fused, dr, lm, lm_multi = env
    make, batch, starts, _ = setup(xarm7, 2, 2)
    qp = _views_qpos(xarm7, 2)
    model = make()
    kw = dict(robot=xarm7, qpos=qp, free=FREE, free_intrinsics=("f",))
    with pytest.raises(ValueError, match="needs the recorded joint vectors"):
        lm_multi.MultiStartLM(model, batch, starts, robot=xarm7)
    with pytest.raises(ValueError, match="need robot="):
        lm_multi.MultiStartLM(model, batch, starts, free=FREE)
    assert _lib.LM_MAX_PARAMS == 32
    monkeypatch.setattr(_lib, "LM_MAX_PARAMS", 8)                                # (no arm here has the 23 joints N > 32 takes)
    with pytest.raises(ValueError, match="optimises 9 parameters; the kernels take 8"):
        lm_multi.MultiStartLM(model, batch, starts, **kw)
    monkeypatch.undo()
    with pytest.raises(RuntimeError, match="must be a tensor on the HIP device"):
        lm_multi.MultiStartLM(model, dict(batch, mask=batch["mask"].cpu()), starts, **kw)
    with pytest.raises(RuntimeError, match="must be a tensor on the HIP device"):
        lm_multi.solve_lm_multi(model, dict(batch, K=batch["K"].cpu()), starts, **kw)
    with pytest.raises(ValueError, match="multi-start solve: it is pose-only"):  # a prior in the pose-only form: refused first
        lm_multi.solve_lm_multi(None, None, None, prior_sigma="default")
    with pytest.raises(ValueError, match="multi-start solve: it is pose-only"):  # ... and with a robot whose joints are all fixed
        lm_multi.solve_lm_multi(model, batch, starts, robot=xarm7, qpos=qp, free=[], prior_sigma="default", sigma2=1.0)
    with pytest.raises(ValueError, match="pass prior_sigma as well"):
        lm_multi.solve_lm_multi(model, batch, starts, sigma2=1.0, **kw)
    monkeypatch.setattr(_lib, "has_lm_multi_calib", lambda: False)
    with pytest.raises(RuntimeError, match="rebuild it"):
        lm_multi.MultiStartLM(model, batch, starts, **kw)
    lm_multi.MultiStartLM(model, batch, starts)                                  # (the pose-only form does not need them)
    monkeypatch.undo()
    ms = lm_multi.MultiStartLM(model, batch, starts, **kw)
    solo_prior = lm.make_prior(_solo_step(xarm7, make(), batch, qp), "default", sigma2=1.0)
    with pytest.raises(ValueError, match="a row per hypothesis"):
        ms.set_prior(solo_prior)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="being captured"):
        ms.iterate(1)
    with pytest.raises(RuntimeError, match="being captured"):
        lm_multi.MultiStartLM(model, batch, starts, **kw)
    monkeypatch.undo()
    assert _lib.has_lm_multi_calib()


def test_invalid_c_arguments(env):
    """EHR_ERR_INVALID, with the entry's name in ``ehr_last_error()``: a NULL, P = 0, an N that is not the layout's, prior arrays
    given singly, sizes that overflow."""
    _lib = env[0]
    lib = _lib.lib()
    z = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    zp, f, dbl = _lib.ptr(z), ctypes.c_float, ctypes.c_double

    def forward(P=2, Bv=2, qpos=zp, L=8):
        return lib.ehr_joint_forward_multi(zp, zp, zp, zp, zp, zp, 8, 7, L, qpos, zp, P, Bv, zp, zp, _stream())

    def linearize(P=2, Bv=2, N=9, dof=zp, mask=3, tie=1):
        return lib.ehr_lm_linearize_multi_calib(dof, zp, zp, P, Bv, 8, H, W, f(0.001), f(10.0), zp, zp, zp, zp, 2, 7, mask, tie, N,
                                                zp, zp, _stream())

    def update(P=2, Bv=2, N=9, state=zp, pw=None, pm=None, mask=3, tie=1):
        return lib.ehr_lm_update_multi_calib(zp, zp, zp, zp, P, Bv, N, zp, zp, zp, 2, 7, zp, mask, tie, zp, zp, H, W, dbl(1e-6),
                                             dbl(1e6), 0, state, None, 0, pw, pm, _stream())

    for name, fn, bad in (
            (b"ehr_joint_forward_multi", forward, (dict(P=0), dict(Bv=0), dict(qpos=None), dict(P=1 << 20, Bv=1 << 10))),
            (b"ehr_lm_linearize_multi_calib", linearize, (dict(P=0), dict(Bv=0), dict(dof=None), dict(N=8), dict(N=10),
                                                          dict(mask=1, tie=1), dict(P=1 << 20, Bv=1 << 10))),
            (b"ehr_lm_update_multi_calib", update, (dict(P=0), dict(Bv=0), dict(state=None), dict(N=8), dict(N=6), dict(pw=zp),
                                                    dict(pm=zp), dict(mask=16, tie=0), dict(P=1 << 20, Bv=1 << 10)))):
        for kw in bad:
            assert fn(**kw) == -1, (name, kw)                                    # EHR_ERR_INVALID
            assert name in lib.ehr_last_error(), (name, kw, lib.ehr_last_error())
    torch.cuda.synchronize()


def test_package_names(env):
    import easyhec_amd
    lm_multi = env[4]
    for name in ("MultiStartLM", "MultiLmResult", "solve_lm_multi", "solve_global_lm", "group_basins"):
        assert getattr(easyhec_amd, name) is getattr(lm_multi, name)
    assert "pose-based" in lm_multi.group_basins.__doc__.lower() and hasattr(lm_multi.MultiLmResult, "write_into")
