"""Multi-start Levenberg-Marquardt on the GPU (``ehr_lm_linearize_multi`` / ``ehr_lm_update_multi``, easyhec_amd/lm_multi.py).
The anchor is SOLO EQUALITY, as for tests/test_gpu_multistart.py: hypothesis p holds, bit for bit, what the solo kernels and the
solo ``LevenbergMarquardt`` on a ``FusedPoseStep`` built on start p hold -- the solve tests/test_gpu_lm.py anchors against the
float64 reference.  No tolerance anywhere: ``torch.equal``, or byte equality of state blocks (they hold NaN).

The starts are ``sample_starts(Tc, P, 0.002, 0.3, seed=2)`` (the scale of test_gpu_lm.py::test_refusals) around the problem's
start pose, so that start 0 is the plain solve's."""
import ctypes

import numpy as np
import pytest
import torch

import lm_multi_reference as MR
from test_gpu_fast import problem
from test_gpu_lm import soft_problem, system as solo_system

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
H, W = 120, 160


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused, lm, lm_multi
    assert _lib.has_lm_multi()
    return _lib, fused, dr, lm, lm_multi


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same(a, b):
    """Byte equality of two tensors or arrays (NaN included)."""
    a, b = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def t32(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def t64(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


_SETUPS = {}


def setup(xarm7, Bv, P):
    """``problem(xarm7, Bv, 120, 160, 0.125)``, P starts around its start pose, and ``solo_model(p)``: a solver built on start p."""
    from easyhec_amd.multistart import sample_starts
    if Bv not in _SETUPS:
        _SETUPS[Bv] = problem(xarm7, Bv, H, W, 0.125)
    cfg, make, batch = _SETUPS[Bv]
    Tc_init = np.asarray(_SETUPS.setdefault(("Tc", Bv), cfg.model.rbsolver.init_Tc_c2b), dtype=np.float64)
    starts = sample_starts(Tc_init, P, 0.002, 0.3, seed=2)

    def solo_model(p):
        cfg.model.rbsolver.init_Tc_c2b = np.asarray(starts[p]).tolist()
        try:
            return make()
        finally:
            cfg.model.rbsolver.init_Tc_c2b = Tc_init.tolist()

    return make, batch, starts, solo_model


# ---- 1. linearize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Bv", [(1, 2), (3, 2), (5, 1)])
def test_linearize_blocks_are_the_solo_kernel_s(env, xarm7, P, Bv):
    _lib = env[0]
    from easyhec_amd.multistart import _starts_to_dof
    make, batch, starts, _ = setup(xarm7, Bv, P)
    dof = _starts_to_dof(starts).to(DEV)
    K, lp = batch["K"][0].contiguous(), batch["link_poses"].contiguous()
    L = lp.shape[1]
    near, far = ctypes.c_float(0.001), ctypes.c_float(10.0)
    mvp = torch.full((P * Bv, L, 4, 4), float("nan"), device=DEV)
    dmvp = torch.full((6, P * Bv, L, 4, 4), float("nan"), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_lm_linearize_multi(_lib.ptr(dof), _lib.ptr(K), _lib.ptr(lp), P, Bv, L, H, W, near, far,
                                                     _lib.ptr(mvp), _lib.ptr(dmvp), _stream()), "ehr_lm_linearize_multi")
        for p in range(P):
            m1, d1 = torch.empty((Bv, L, 4, 4), device=DEV), torch.empty((6, Bv, L, 4, 4), device=DEV)
            _lib.check(_lib.lib().ehr_lm_linearize(_lib.ptr(dof[p].contiguous()), _lib.ptr(K), _lib.ptr(lp), Bv, L, H, W, near, far,
                                                   None, None, None, None, 0, 0, 0, 0, 6, _lib.ptr(m1), _lib.ptr(d1), _stream()),
                       "ehr_lm_linearize")
            torch.cuda.synchronize()
            v = slice(p * Bv, (p + 1) * Bv)
            assert torch.equal(mvp[v], m1), (p, "mvp")
            assert torch.equal(dmvp[:, v], d1), (p, "dmvp")
    assert bool(torch.isfinite(mvp).all()) and bool(torch.isfinite(dmvp).all())
    assert P == 1 or not torch.equal(mvp[:Bv], mvp[Bv:2 * Bv])


# ---- 2. the update kernel alone ----------------------------------------------------------------------------------------------
ROWS = 16


class Multi:
    """The tensors one ehr_lm_update_multi works on, and per hypothesis those of the solo ehr_lm_update, without a renderer."""

    def __init__(self, _lib, N, P, Bv):
        self._lib, self.N, self.P, self.Bv = _lib, N, P, Bv
        st = np.zeros((P, _lib.LM_STATE_DOUBLES))
        st[:, 0], st[:, 1] = 1e-3, 2.0
        self.dof, self.state = t32(MR.start_dof(P)), t64(st)
        self.log = torch.full((P, ROWS, 4), float("nan"), dtype=torch.float64, device=DEV)
        self.sdof = [self.dof[p].clone() for p in range(P)]
        self.sstate = [self.state[p].clone() for p in range(P)]
        self.slog = [self.log[p].clone() for p in range(P)]

    def call(self, info, grad, count, loss, finalize=0, solo=True):
        _lib, N, P, Bv = self._lib, self.N, self.P, self.Bv
        ti, tg, tl = t64(info), t64(grad), t32(loss)
        tc = torch.tensor(np.ascontiguousarray(count, np.int64), device=DEV)
        ftol, lmax = ctypes.c_double(MR.FTOL), ctypes.c_double(1e6)
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().ehr_lm_update_multi(
                _lib.ptr(ti), _lib.ptr(tg), _lib.ptr(tc), _lib.ptr(tl), P, Bv, N, _lib.ptr(self.dof), ftol, lmax, finalize,
                _lib.ptr(self.state), _lib.ptr(self.log), ROWS, _stream()), "ehr_lm_update_multi")
            for p in range(P if solo else 0):
                v = slice(p * Bv, (p + 1) * Bv)
                si, sg, sc, sl = ti[v].contiguous(), tg[v].contiguous(), tc[v].contiguous(), tl[v].contiguous()
                _lib.check(_lib.lib().ehr_lm_update(
                    _lib.ptr(si), _lib.ptr(sg), _lib.ptr(sc), _lib.ptr(sl), Bv, N, _lib.ptr(self.sdof[p]), None, None, 0, 0,
                    None, 0, 0, None, None, H, W, ftol, lmax, finalize, _lib.ptr(self.sstate[p]), _lib.ptr(self.slog[p]), ROWS,
                    _stream()), "ehr_lm_update")
            torch.cuda.synchronize()

    def assert_equal_solo(self, what):
        for p in range(self.P):
            assert same(self.state[p], self.sstate[p]), (what, p, "state")
            assert same(self.dof[p], self.sdof[p]), (what, p, "dof")
            assert same(self.log[p], self.slog[p]), (what, p, "log")

    def flags(self, block):
        s = block.cpu().numpy()
        L = self._lib.LM_STATE
        return {k: int(s[L[k]]) for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last")}


@pytest.mark.parametrize("N", [1, 6])
@pytest.mark.parametrize("P,Bv", [(1, 1), (3, 2)])
def test_update_kernel_alone(env, N, P, Bv):
    """Seven scripted calls (tests/lm_multi_reference.py: accepts, rejects, a NaN in hypothesis 1's grad, hypothesis 0 stopped by
    call 4), each compared with the solo kernel driven by the same inputs; then finalize."""
    _lib = env[0]
    i0, g0, c0, l0 = MR.system(N, Bv, 5)
    for a, b in zip((i0, g0, c0, l0), solo_system(N, Bv, 5)):                   # the generator is test_gpu_lm.py's
        assert np.array_equal(a, b)
    u = Multi(_lib, N, P, Bv)
    TH = _lib.LM_THETA
    for c, (info, grad, count, loss) in enumerate(MR.scripted_calls(N, P, Bv)):
        before_state, before_dof = u.state.clone(), u.dof.clone()
        u.call(info, grad, count, loss)
        u.assert_equal_solo(f"N={N} call {c}")
        for p in range(P):                                                       # asserted on the SOLO states
            f = u.flags(u.sstate[p])
            assert (f["last"], f["done"]) == MR.expected_flags(p, c), (p, c, f)
        if P > 1 and c >= 5:   # hypothesis 0 is done: its block's bytes stay, its pose is the accepted one; hypothesis 1 moves
            assert same(u.state[0], before_state[0]) and same(u.dof[0], before_dof[0])
            assert not same(u.state[1], before_state[1])
        if P > 1 and c == 5:   # the NaN in hypothesis 1's grad: one reported call, its trial discarded, nobody else's
            f1 = u.flags(u.state[1])
            assert f1["reported"] == 1 and f1["last"] == -1
            acc = u.state[1, TH:TH + N].float()
            assert torch.equal(u.dof[1, :N], acc) and not torch.equal(before_dof[1, :N], acc)
            assert u.flags(u.state[2])["reported"] == 0 and not same(u.dof[2], before_dof[2])
    f0 = u.flags(u.sstate[0])
    assert f0["accepted"] >= 2 and f0["rejected"] >= 1 and f0["done"] == 1 and f0["why"] == 1 and f0["iterations"] == 5
    if P > 1:
        f1, f2 = u.flags(u.sstate[1]), u.flags(u.sstate[2])
        assert f1["iterations"] == f2["iterations"] == 7 and f1["done"] == f2["done"] == 0 and f2["reported"] == 0
        assert not torch.equal(u.dof[1, :N], u.state[1, TH:TH + N].float())     # a trial is in hypothesis 1's pose
    # finalize restores all P poses and changes nothing else
    raw, log = u.state.clone(), u.log.clone()
    u.call(*MR.scripted_calls(N, P, Bv)[0], finalize=1)
    u.assert_equal_solo(f"N={N} finalize")
    assert same(u.state, raw) and same(u.log, log)
    for p in range(P):
        assert torch.equal(u.dof[p, :N], u.state[p, TH:TH + N].float()), p
    assert torch.equal(u.dof[:, N:], t32(MR.start_dof(P))[:, N:])               # the coordinates behind N are nobody's


def test_update_kernel_zero_diagonal(env):
    """A parameter without information in hypothesis 1 alone: its delta is exactly 0 there, and every block is the solo kernel's."""
    _lib = env[0]
    N, P, Bv, z = 6, 3, 2, 4
    parts = [MR.system(N, Bv, 300 + p) for p in range(P)]
    parts[1][0][:, z, :], parts[1][0][:, :, z], parts[1][1][:, z] = 0.0, 0.0, 0.0
    u = Multi(_lib, N, P, Bv)
    p0 = u.dof.clone()
    u.call(*(np.concatenate([x[i] for x in parts]) for i in range(4)))
    u.assert_equal_solo("zero diagonal")
    D = _lib.LM_DELTA
    delta = u.state[:, D:D + N].cpu().numpy()
    assert delta[1, z] == 0.0 and (np.delete(delta[1], z) != 0).all() and (delta[[0, 2]] != 0).all()
    assert u.dof[1, z] == p0[1, z] and bool((u.dof[[0, 2]] != p0[[0, 2]]).all())


# ---- 3. composition ----------------------------------------------------------------------------------------------------------
def _solo_iterate(lm, solo_model, batch, p, n):
    from easyhec_amd.fast import FusedPoseStep
    model = solo_model(p)
    o = lm.LevenbergMarquardt(FusedPoseStep(model, batch))
    o.iterate(n)
    torch.cuda.synchronize()
    return o, model


@pytest.mark.parametrize("P,Bv", [(1, 2), (3, 2), (70, 1)])
def test_iterate_equals_the_solo_iteration(env, xarm7, P, Bv):
    """(70, 1): 70 x 8 (view, link) units are more than one pass of the chain takes -- two chunks; hypotheses on both sides of
    the boundary are compared."""
    _lib, fused, dr, lm, lm_multi = env
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    model = make()
    dof0, plan0 = model.dof.detach().clone(), getattr(model._ensure_renderer().glctx, "_plan", None)
    ms = lm_multi.MultiStartLM(model, batch, starts)
    assert ms.P == P and ms.B == P * Bv and ms.ref.shape == (P * Bv, H, W)
    if P == 70:
        assert ms.L == 8 and ms.B * ms.L > 512
    ms.iterate(3)
    torch.cuda.synchronize()
    fused.check_status(ms.glctx)
    S = ms.state()
    assert [s.reported for s in S] == [0] * P and all(s.iterations == 3 or s.done for s in S)
    for p in ([0, 63, 64, 69] if P == 70 else range(P)):
        o, m = _solo_iterate(lm, solo_model, batch, p, 3)
        fused.check_status(o.step.glctx)
        assert same(ms.state_block[p], o.state_block), (p, "state")
        assert torch.equal(ms.dof[p], m.dof.detach()), (p, "dof")
        assert same(ms.log[p], o.log), (p, "log")
        assert same(ms.trajectory(p), o.trajectory()) and S[p].accepted >= 1
        assert ms.report(p).H.tobytes() == o.report().H.tobytes() and ms.report(p).names == o.names
    assert P == 1 or not same(ms.state_block[0], ms.state_block[1])
    # the model is read, never written: its pose, and its context's plan
    assert torch.equal(model.dof.detach(), dof0) and getattr(model._ensure_renderer().glctx, "_plan", None) is plan0
    print(f"[lm multi] P={P} Bv={Bv}: F_acc {[round(s.F_acc, 3) for s in S[:4]]}; context + tiled reference {ms.memory_bytes() / 1e6:.1f} MB")


def test_iterate_on_soft_problem_equals_the_solo_iteration(env, xarm7):
    """``soft_problem`` (zoom 2, seed-2 views) with P = 3: the solo solvers get start p's dof through ``_starts_to_dof``."""
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import _starts_to_dof, sample_starts
    from easyhec_amd.se3 import se3_exp_map
    make, batch, _ = soft_problem(xarm7)
    m0 = make()
    Tc = se3_exp_map(m0.dof.detach().cpu().double()[None]).permute(0, 2, 1)[0].numpy()
    starts = sample_starts(Tc, 3, 0.002, 0.3, seed=2)
    dof = _starts_to_dof(starts)
    ms = lm_multi.MultiStartLM(m0, batch, dof).iterate(3)
    torch.cuda.synchronize()
    fused.check_status(ms.glctx)
    for p in range(3):
        m = make()
        m.dof.data.copy_(dof[p])
        o = lm.LevenbergMarquardt(FusedPoseStep(m, batch)).iterate(3)
        torch.cuda.synchronize()
        assert same(ms.state_block[p], o.state_block) and torch.equal(ms.dof[p], m.dof.detach()) and same(ms.log[p], o.log), p
    assert all(s.reported == 0 and s.accepted >= 1 for s in ms.state())


# ---- 4. the whole solve ------------------------------------------------------------------------------------------------------
def _loss_at(_lib, fused, dr, scene, batch, dof):
    """float64 sum, in view order, of render_mask_loss (another context) on the solo linearize kernel's mvp at ``dof``
    (test_gpu_lm.py::test_accepted_loss_is_render_mask_loss's recipe)."""
    K, lp = batch["K"][0].contiguous(), batch["link_poses"].contiguous()
    Bv, L = lp.shape[0], lp.shape[1]
    mvp, dmvp = torch.empty((Bv, L, 4, 4), device=DEV), torch.empty((6, Bv, L, 4, 4), device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().ehr_lm_linearize(_lib.ptr(dof.to(DEV).contiguous()), _lib.ptr(K), _lib.ptr(lp), Bv, L, H, W,
                                               ctypes.c_float(0.001), ctypes.c_float(10.0), None, None, None, None, 0, 0, 0, 0,
                                               6, _lib.ptr(mvp), _lib.ptr(dmvp), _stream()), "ehr_lm_linearize")
    _, loss = fused.render_mask_loss(dr.RasterizeCudaContext(), scene, mvp, batch["mask"].clone(), want_mask=False,
                                     weight=batch.get("weight"))
    torch.cuda.synchronize()
    F = 0.0
    for x in loss.detach().cpu().numpy():
        F += float(x)
    return F


def test_solve_lm_multi(env, xarm7):
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import rank_losses
    P, Bv = 3, 2
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    model = make()
    dof0, hist0 = model.dof.detach().clone(), model.history_ops.clone()
    res = lm_multi.solve_lm_multi(model, batch, starts, max_iters=12, check_every=5)
    m = solo_model(0)
    solo = lm.solve_lm(FusedPoseStep(m, batch), max_iters=12, check_every=5)
    print(f"[lm multi solve] losses {res.losses.tolist()}, iterations {res.iterations}, accepted {res.accepted}, why {res.why}, "
          f"basins {res.basins}; solo {solo.loss!r} in {solo.iterations} ({solo.why})")
    assert res.losses[0] == solo.loss and torch.equal(res.dofs[0], m.dof.detach().cpu())
    assert same(res.lm.state_block[0], solo.lm.state_block) and res.trajectories[0].tobytes() == solo.trajectory.tobytes()
    assert (res.iterations[0], res.accepted[0], res.rejected[0], res.done[0], res.why[0]) == \
           (solo.iterations, solo.accepted, solo.rejected, solo.done, solo.why)
    assert res.reported == [0] * P and res.recoveries == []
    for p in range(P):
        F = _loss_at(_lib, fused, dr, model._ensure_scene(), batch, res.dofs[p])
        print(f"[lm multi solve] hypothesis {p}: F_acc {res.losses[p]!r}, render_mask_loss at its accepted pose {F!r}")
        assert res.losses[p] == F and res.accepted[p] >= 1
        assert torch.equal(res.dofs[p], torch.from_numpy(res.states[p].theta.astype(np.float32)))
        assert res.done[p] or res.iterations[p] >= 12
    assert res.winner == rank_losses(res.losses)[0] == res.ranking[0] and res.losses.dtype == np.float64
    assert res.report.loss == res.losses[res.winner] and (res.report.H == res.states[res.winner].H).all()
    assert sorted(i for b in res.basins for i in b) == list(range(P)) and res.basins[0][0] == res.winner
    assert torch.equal(model.dof.detach(), dof0) and torch.equal(model.history_ops, hist0)


# ---- 5. weights --------------------------------------------------------------------------------------------------------------
def test_shared_weights(env, xarm7):
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.fast import FusedPoseStep
    P, Bv = 2, 2
    make, batch, starts, solo_model = setup(xarm7, Bv, P)
    w = torch.ones((Bv, H, W), device=DEV)
    ys, xs = torch.nonzero(batch["mask"].amax(dim=0) > 0.5, as_tuple=True)
    y0, y1, x0, x1 = int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())
    w[:, y0:y1 + 1, x0:(x0 + x1) // 2 + 1] = 0.0                                 # a zeroed rectangle: the silhouettes' left half
    assert 0 < float((batch["mask"] * (1 - w)).sum()) < float(batch["mask"].sum())
    wb = dict(batch, weight=w)
    ms = lm_multi.MultiStartLM(make(), wb, starts).iterate(4).finalize()
    plain = lm_multi.MultiStartLM(make(), batch, starts).iterate(4).finalize()
    torch.cuda.synchronize()
    fused.check_status(ms.glctx)
    for p in range(P):
        m = solo_model(p)
        o = lm.LevenbergMarquardt(FusedPoseStep(m, wb)).iterate(4).finalize()
        torch.cuda.synchronize()
        assert same(ms.state_block[p], o.state_block) and torch.equal(ms.dof[p], m.dof.detach()) and same(ms.log[p], o.log), p
        s = ms.state()[p]
        Fw, F1 = _loss_at(_lib, fused, dr, ms.scene, wb, ms.dof[p]), _loss_at(_lib, fused, dr, ms.scene, batch, ms.dof[p])
        print(f"[lm multi weights] hypothesis {p}: F_acc {s.F_acc!r}; weighted render_mask_loss {Fw!r}; unweighted {F1!r}")
        assert s.F_acc == Fw and Fw < F1 and not same(ms.state_block[p], plain.state_block[p])
    other = torch.ones_like(w)
    fused.bind_weight(ms.glctx, ms.scene, other, views=ms.B)                     # somebody else used the context
    with pytest.raises(RuntimeError, match="weights bound"):
        ms.iterate(1)


# ---- 6. recovery -------------------------------------------------------------------------------------------------------------
def test_reported_iterations_are_recovered(env, xarm7, monkeypatch):
    """The slot-limited close-up of test_gpu_lm.py::test_reported_iteration_is_recovered with P = 2: the first iterations are
    reported, the plan is made again with every slot, and every hypothesis ends on the bits of a solve that had them all."""
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
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    ends = []
    for slack in (None, 0.0):
        res = lm_multi.solve_lm_multi(RBSolver(cfg, meshes=xarm7.meshes).to(DEV), batch, starts, max_iters=6, check_every=2,
                                      slack=slack)
        if slack is None:
            assert sum(res.reported) >= 1 and res.recoveries == ["job slots"] and res.lm.slack == 0.0
        else:
            assert res.reported == [0] * P and res.recoveries == []
        assert all(res.iterations[p] - res.reported[p] >= 6 or res.done[p] for p in range(P))
        ends.append(res)
    a, b = ends
    print(f"[lm multi reported] limited plan: {a.reported} reported of {a.iterations}, F_acc {a.losses.tolist()}; every slot: "
          f"{b.iterations} iterations, F_acc {b.losses.tolist()}")
    for p in range(P):
        sa, sb = a.states[p], b.states[p]
        assert (sa.theta == sb.theta).all() and (sa.H == sb.H).all() and sa.__dict__["lambda"] == sb.__dict__["lambda"]
        assert sa.F_acc == sb.F_acc and sa.accepted == sb.accepted and torch.equal(a.dofs[p], b.dofs[p])


# ---- 7. determinism ----------------------------------------------------------------------------------------------------------
def test_two_runs_on_two_contexts_end_on_identical_bytes(env, xarm7):
    _lib, fused, dr, lm, lm_multi = env
    make, batch, starts, _ = setup(xarm7, 2, 3)
    ends = []
    for _ in range(2):
        res = lm_multi.solve_lm_multi(make(), batch, starts, max_iters=7, check_every=3)
        ends.append((res.lm.state_block.cpu().numpy().tobytes(), res.lm.dof.cpu().numpy().tobytes(),
                     res.lm.log.cpu().numpy().tobytes(), res.losses.tobytes(), res.lm.glctx))
    assert ends[0][:4] == ends[1][:4] and ends[0][4] is not ends[1][4]


# ---- 8. the global solve -----------------------------------------------------------------------------------------------------
def test_solve_global_lm_is_never_worse_than_the_plain_solve(env, xarm7):
    """The problem of test_gpu_pose_search.py's solve_global test (4 views at 120x160), Q = 16 candidates, P = 3 starts."""
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.fast import FusedPoseStep
    Bv, Q, P = 4, 16, 3
    make, batch, _, _ = setup(xarm7, Bv, 1)
    model = make()
    Tc_init = np.asarray(_SETUPS[("Tc", Bv)], dtype=np.float64)
    hist0 = model.history_ops.clone()
    search, res = lm_multi.solve_global_lm(model, batch, Tc_init, Q, P, max_iters=12)
    assert np.array_equal(search.starts[0], Tc_init) and search.starts.shape == (P, 4, 4)
    m = make()
    solo = lm.solve_lm(FusedPoseStep(m, batch), max_iters=12)
    print(f"[lm multi global] losses {res.losses.tolist()}, winner {res.winner}, basins {res.basins}, why {res.why}; plain {solo.loss!r}")
    assert res.losses[0] == solo.loss and torch.equal(res.dofs[0], m.dof.detach().cpu())   # hypothesis 0 IS the plain solve
    assert np.isfinite(res.losses).all() and res.losses[res.winner] <= res.losses[0]
    assert torch.equal(model.dof.detach().cpu(), res.dofs[res.winner]) and torch.equal(model.history_ops, hist0)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(env, xarm7, monkeypatch):
    _lib, fused, dr, lm, lm_multi = env
    from easyhec_amd.multistart import MultiStartPoseStep
    make, batch, starts, _ = setup(xarm7, 2, 2)
    model = make()
    with pytest.raises(RuntimeError, match="must be a tensor on the HIP device"):
        lm_multi.MultiStartLM(model, dict(batch, mask=batch["mask"].cpu()), starts)
    with pytest.raises(RuntimeError, match="must be a tensor on the HIP device"):
        lm_multi.solve_lm_multi(model, dict(batch, link_poses=batch["link_poses"].cpu()), starts)
    u = Multi(_lib, 6, 2, 2)
    z = torch.zeros(8 * 49, dtype=torch.float64, device=DEV)
    args = lambda P, Bv, N: (_lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), P, Bv, N, _lib.ptr(u.dof), ctypes.c_double(1e-6),
                             ctypes.c_double(1e6), 0, _lib.ptr(u.state), None, 0, _stream())
    for P, Bv, N in ((2, 2, 7), (2, 2, 0), (0, 2, 6), (2, 0, 6)):
        assert _lib.lib().ehr_lm_update_multi(*args(P, Bv, N)) == -1             # EHR_ERR_INVALID
    assert b"ehr_lm_update_multi" in _lib.lib().ehr_last_error()
    assert _lib.lib().ehr_lm_update_multi(None, *args(2, 2, 6)[1:]) == -1
    f = ctypes.c_float
    assert _lib.lib().ehr_lm_linearize_multi(_lib.ptr(u.dof), None, _lib.ptr(z), 2, 2, 8, H, W, f(0.001), f(10.0), _lib.ptr(z),
                                             _lib.ptr(z), _stream()) == -1
    assert _lib.lib().ehr_lm_linearize_multi(_lib.ptr(u.dof), _lib.ptr(z), _lib.ptr(z), 1 << 20, 1 << 10, 8, H, W, f(0.001),
                                             f(10.0), _lib.ptr(z), _lib.ptr(z), _stream()) == -1   # the matrix count overflows
    torch.cuda.synchronize()
    ms = lm_multi.MultiStartLM(model, batch, starts)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="being captured"):
        ms.iterate(1)
    with pytest.raises(RuntimeError, match="being captured"):
        lm_multi.MultiStartLM(model, batch, starts)
    monkeypatch.undo()
    fused._ensure_plan(ms.glctx, ms.scene, 1, ms.H, ms.W)                        # somebody else planned on its context
    with pytest.raises(RuntimeError, match="another plan"):
        ms.iterate(1)
    with pytest.raises(ValueError, match="multi-start"):                         # the solo entry still turns the Adam step away
        lm.solve_lm(MultiStartPoseStep(model, batch, starts))
    import easyhec_amd
    for name in ("MultiStartLM", "MultiLmResult", "solve_lm_multi", "solve_global_lm", "group_basins"):
        assert getattr(easyhec_amd, name) is getattr(lm_multi, name)
