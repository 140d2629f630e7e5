"""Multi-start solve on the GPU (easyhec_amd.multistart / ehr_solver_step_multi).  The anchor is SOLO EQUALITY: hypothesis p
of a P-start solve holds, bit for bit, the state of a FusedPoseStep solve from start p -- the chain the oracle and the
float64 pose reference already anchor.  No tolerance anywhere: ``torch.equal``."""
import numpy as np
import pytest
import torch

from test_gpu_fast import problem

pytestmark = pytest.mark.gpu

STEPS = 6


def starts_for(cfg, P, seed=3, ts=0.01, rs=1.5):
    from easyhec_amd.multistart import sample_starts
    return sample_starts(np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64), P, ts, rs, seed=seed)


def solo_states(cfg, make, batch, starts, steps=STEPS, want_mask=False, recover=False, slack=None):
    """One FusedPoseStep solve per start (each on a solver built on that start, one context for all of them); per start the
    compared state after `steps` effective steps and the loss of every effective step."""
    from easyhec_amd.fast import FusedPoseStep
    out = []
    model = None
    for T in starts:
        cfg.model.rbsolver.init_Tc_c2b = np.asarray(T).tolist()
        fresh = make()
        if model is None:
            model = fresh
        else:  # the same context again: a new solve from the next start
            with torch.no_grad():
                model.dof.copy_(fresh.dof)
                model.history_ops.zero_()
            model._hist_n = 0
        f = FusedPoseStep(model, batch, slack=slack)
        dof0 = model.dof.detach().clone()
        losses = []
        while len(losses) < steps:
            last = len(losses) == steps - 1
            l = float(f.step(want_mask=want_mask and last))
            if l != l and recover:
                assert f.recover_from_overflow()
                continue
            losses.append(l)
        torch.cuda.synchronize()
        s = {k: getattr(f, k).clone() for k in ("exp_avg", "exp_avg_sq", "loss", "grad", "red", "loss_b", "grad_mvp", "mvp",
                                               "tc_jac")}
        s.update(dof=model.dof.detach().clone(), dof0=dof0, step=int(f.step_t), hist_row=int(f.hist_row),
                 history=model.history_ops[:steps + 2].clone(), losses=losses)
        if want_mask:
            s["mask"] = f.mask.clone()
        out.append(s)
    return out


def assert_hypotheses_equal_solo(ms, solo, steps=STEPS, losses=None, skip=()):
    Bv = ms.Bv
    for p, s in enumerate(solo):
        if p in skip:
            continue
        v = slice(p * Bv, (p + 1) * Bv)
        for name, mine in [("dof", ms.dof[p]), ("exp_avg", ms.exp_avg[p]), ("exp_avg_sq", ms.exp_avg_sq[p]),
                           ("loss", ms.loss[p:p + 1]), ("grad", ms.grad[p]), ("red", ms.red[p]), ("loss_b", ms.loss_b[v]),
                           ("grad_mvp", ms.grad_mvp[v]), ("mvp", ms.mvp[v]), ("tc_jac", ms.tc_jac[p]),
                           ("history", ms.history[p, :steps + 2])]:
            assert torch.equal(mine, s[name]), (p, name)
        assert int(ms.step_t[p]) == s["step"] == steps and int(ms.hist_row[p]) == s["hist_row"], p
        if losses is not None:
            assert [float(x[p]) for x in losses] == s["losses"], p
        if "mask" in s and ms.mask is not None:
            assert torch.equal(ms.mask[v], s["mask"]), (p, "mask")


def run_multi(make, batch, starts, steps=STEPS, want_mask=False, **kw):
    from easyhec_amd.multistart import MultiStartPoseStep
    ms = MultiStartPoseStep(make(), batch, starts, **kw)
    losses = [ms.step(want_mask=want_mask and it == steps - 1).clone() for it in range(steps)]
    torch.cuda.synchronize()
    return ms, losses


@pytest.mark.parametrize("P,Bv", [(1, 1), (3, 1), (16, 1), (4, 4), (70, 1)])
def test_every_hypothesis_equals_its_solo_solve(xarm7, P, Bv):
    """(70, 1): 70 x 8 (view, link) units are more than one pass of the chain takes -- two chunks."""
    from easyhec_amd import fused
    cfg, make, batch = problem(xarm7, Bv, 240, 320, 0.25)
    starts = starts_for(cfg, P)
    ms, losses = run_multi(make, batch, starts)
    fused.check_status(ms.glctx)
    if P == 70:
        assert ms.L == 8 and ms.B * ms.L > 512
    assert ms.P == P
    solo = solo_states(cfg, make, batch, starts)
    for p in range(P):  # the starts really are the solo solvers' starts, and they differ
        assert torch.equal(ms.history[p, 0], solo[p]["dof0"])
    assert P == 1 or not torch.equal(ms.dof[0], ms.dof[1])
    assert_hypotheses_equal_solo(ms, solo, losses=losses)
    assert all(np.isfinite(s["losses"]).all() for s in solo)


def test_solo_equality_with_clip_space_vertices_on_demand(xarm7, monkeypatch):
    monkeypatch.setenv("EHR_VB_LAZY", "1")  # (read by ehr_fused_plan: everything below plans afresh)
    cfg, make, batch = problem(xarm7, 2, 240, 320, 0.25)
    starts = starts_for(cfg, 3)
    ms, losses = run_multi(make, batch, starts)
    solo = solo_states(cfg, make, batch, starts)
    monkeypatch.delenv("EHR_VB_LAZY")
    assert_hypotheses_equal_solo(ms, solo, losses=losses)


def test_solo_equality_with_the_mask_output(xarm7):
    cfg, make, batch = problem(xarm7, 2, 240, 320, 0.25)
    starts = starts_for(cfg, 3)
    ms, losses = run_multi(make, batch, starts, want_mask=True)
    solo = solo_states(cfg, make, batch, starts, want_mask=True)
    assert ms.mask is not None and float(ms.mask.sum()) > 100.0
    assert_hypotheses_equal_solo(ms, solo, losses=losses)
    assert not torch.equal(ms.mask[0:2], ms.mask[2:4])


def test_graph_replay_and_a_second_context_give_the_same_bits(xarm7):
    from easyhec_amd.multistart import MultiStartPoseStep
    cfg, make, batch = problem(xarm7, 2, 240, 320, 0.25)
    starts = starts_for(cfg, 5)
    a, b, c = (MultiStartPoseStep(make(), batch, starts) for _ in range(3))
    b.capture()
    for it in range(STEPS):
        la, lb, lc = a.step().clone(), b.step().clone(), c.step().clone()
        assert torch.equal(la, lb) and torch.equal(la, lc), it
    torch.cuda.synchronize()
    for name in ("dof", "exp_avg", "exp_avg_sq", "step_t", "hist_row", "history", "red", "grad", "loss_b", "grad_mvp", "mvp",
                 "tc_jac"):
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name)), name
    assert a.steps_done == STEPS


def test_a_start_with_the_robot_out_of_frame(xarm7):
    """Hypothesis 1 starts 5 m to the side: no jobs, zero gradient, the constant loss sum(ref^2); it stays finite and
    ranks last, and its empty slice of views does not disturb the others."""
    from easyhec_amd.multistart import rank_losses
    cfg, make, batch = problem(xarm7, 2, 240, 320, 0.25)
    starts = starts_for(cfg, 4)
    side = np.eye(4)
    side[0, 3] = 5.0  # along the camera's x axis: the depth stays what it was, nothing comes near the near plane
    starts[1] = side @ starts[0]
    ms, losses = run_multi(make, batch, starts)
    const = float(batch["mask"].double().pow(2).sum(dim=(1, 2)).mean())
    for l in losses:
        assert float(l[1]) == float(losses[0][1]) and abs(float(l[1]) - const) <= 1e-6 * const
    assert torch.equal(ms.grad[1], torch.zeros(6, device=ms.dev)) and torch.isfinite(ms.dof).all()
    assert torch.equal(ms.grad_mvp[2:4], torch.zeros_like(ms.grad_mvp[2:4]))
    assert rank_losses(ms.loss.cpu().numpy())[-1] == 1
    solo = solo_states(cfg, make, batch, starts)
    assert_hypotheses_equal_solo(ms, solo, losses=losses)


def test_a_start_that_needs_the_general_triangle_pass(xarm7):
    """The near-camera scene of test_solver_step_switches_the_general_triangle_pass_on_when_a_step_needs_it: the first step
    is reported for ALL hypotheses, recover_from_overflow switches the pass on, and every hypothesis ends bit-equal to its
    solo solve with one history row per effective step."""
    from easyhec_amd import _lib
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, scaled_K
    dev = torch.device("cuda:0")
    H, W, B = 240, 320, 2
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    K[:2, :2] *= 12.0
    _, lp = make_views(xarm7, B, seed=4)
    Tc = camera_Tc_c2b(radius=0.45, lift=0.2)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=dev)
    ref[:, 8:200, 10:300] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(np.array(K), dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    make = lambda: RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    starts = sample_starts(Tc, 3, 0.002, 0.3, seed=2)
    for graph in (False, True):
        ms = MultiStartPoseStep(make(), batch, starts, slack=0.0)  # (every job slot: this test is about the other report)
        if graph:
            ms.capture()
        dof0 = ms.dof.clone()
        l = ms.step()
        torch.cuda.synchronize()
        assert torch.isnan(l).all() and torch.equal(ms.dof, dof0) and int(ms.step_t.max()) == 0
        assert _lib.lib().ehr_fused_status(ms.glctx.handle) == _lib.EHR_ERR_RETRY
        assert ms.recover_from_overflow() == "general-triangle pass"
        losses = [ms.step().clone() for _ in range(5)]
        torch.cuda.synchronize()
        assert all(torch.isfinite(x).all() for x in losses)
        assert ms.hist_row.tolist() == [5, 5, 5] and ms.step_t.tolist() == [5, 5, 5]
        assert (ms.history[:, :5].abs().sum(dim=2) > 0).all() and float(ms.history[:, 5:].abs().sum()) == 0.0
        assert torch.equal(ms.history[:, 0], dof0)
        if not graph:
            solo = solo_states(cfg, make, batch, starts, steps=5, recover=True, slack=0.0)
        assert_hypotheses_equal_solo(ms, solo, steps=5, losses=losses)


def test_checkpoint_round_trip(xarm7):
    from easyhec_amd.multistart import MultiStartPoseStep
    cfg, make, batch = problem(xarm7, 2, 240, 320, 0.25)
    starts = starts_for(cfg, 4)
    whole, _ = run_multi(make, batch, starts, steps=6)
    first, _ = run_multi(make, batch, starts, steps=3)
    sd = first.state_dict()
    assert sd["history"].shape == (4, 3, 6)
    second = MultiStartPoseStep(make(), batch, starts_for(cfg, 4, seed=9))  # other starts: the state must come from `sd`
    second.load_state_dict(sd)
    for _ in range(3):
        second.step()
    torch.cuda.synchronize()
    for name in ("dof", "exp_avg", "exp_avg_sq", "step_t", "hist_row", "history", "red", "loss", "grad", "loss_b", "grad_mvp"):
        assert torch.equal(getattr(whole, name), getattr(second, name)), name


def test_solve_multistart_end_to_end(xarm7):
    """Start 0 = perturb_pose(Tc) on the 4-view problem: hypothesis 0 ends where the existing fast solve ends; the winner is
    the argmin of the tail-mean losses and the model holds its pose and history."""
    from easyhec_amd.multistart import solve_multistart
    from easyhec_amd.trainer import RBSolverTrainer
    cfg, make, batch = problem(xarm7, 4, 240, 320, 0.25)
    n, tail = 30, 10
    starts = starts_for(cfg, 4, seed=1)
    model = make()
    res = solve_multistart(cfg, model, batch, starts, n, tail=tail)
    ref_model = make()
    tr = RBSolverTrainer(cfg, ref_model, batch, fast=True, graph=True)
    tr.fit(num_steps=n)
    torch.cuda.synchronize()
    assert res.steps == n and res.loss_history.shape == (n, 4) and torch.isfinite(res.loss_history).all()
    assert torch.equal(res.dofs[0], ref_model.dof.detach().cpu())
    want = res.loss_history[-tail:].double().mean(dim=0)
    assert torch.equal(res.losses, want)
    assert res.winner == int(torch.argmin(want)) == res.ranking[0] and sorted(res.ranking) == [0, 1, 2, 3]
    assert torch.equal(model.dof.detach().cpu(), res.dofs[res.winner])
    assert model.history_cursor() == n and float(model.history_ops[n:].abs().sum()) == 0.0
    from easyhec_amd.multistart import _starts_to_dof
    assert torch.equal(model.history_ops[0].cpu(), _starts_to_dof(starts)[res.winner])
    if res.winner == 0:
        assert torch.equal(model.history_ops[:n], ref_model.history_ops[:n])


@pytest.fixture(scope="module")
def closeup(xarm7):
    """The close-up of test_gpu_fused.py::test_an_unattended_stepping_loop_recovers_by_itself (64 x 96, two views, zoomed
    2.5 x: under EHR_VB_SLACK=1.0 its steps are reported for want of job slots), two starts around its pose, and per start
    the solo solve that has every slot from the beginning: 16 steps, computed once."""
    from easyhec_amd.config import Cfg
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
    starts = starts_for(cfg, 2)
    solo = solo_states(cfg, make, batch, starts, steps=16, slack=0.0)
    return cfg, make, batch, starts, solo


def test_an_unattended_multi_start_loop_recovers_job_slots_by_itself(closeup, monkeypatch):
    """48 step() calls and nobody looks: calls 1..32 are reported (the poll at call 16 starts the look, the one at call 32
    sees it and plans again with every slot), calls 33..48 are the 16 steps of the solo solves."""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import MultiStartPoseStep
    cfg, make, batch, starts, solo = closeup
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(starts[0]).tolist()
    f = FusedPoseStep(make(), batch)  # the precondition: alone, start 0 is reported for want of job slots
    assert f.slack == 1.0 and bool(torch.isnan(f.step()).all())
    assert f.recover_from_overflow() == "job slots"
    ms = MultiStartPoseStep(make(), batch, starts)
    assert ms.slack == 1.0 and ms.check_every == 16 and (ms.P, ms.Bv) == (2, 2)
    for i in range(48):
        ms.step()
        if i in (15, 31):
            torch.cuda.synchronize()   # (so that the look started at call 16 has certainly arrived by call 32)
    torch.cuda.synchronize()
    assert ms.recoveries == ["job slots"] and ms.slack == 0.0
    assert ms.steps_done == 16
    assert_hypotheses_equal_solo(ms, solo, steps=16)


def test_solve_multistart_takes_a_reported_step_again(closeup, monkeypatch):
    """Five EFFECTIVE steps on the same close-up: the first round's steps are all reported, the loop recovers and runs them
    again.  (Row r of a solo solve's history is its pose after r steps.)"""
    from easyhec_amd.multistart import solve_multistart
    cfg, make, batch, starts, solo = closeup
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    model = make()
    res = solve_multistart(cfg, model, batch, starts, num_steps=5)
    assert res.steps == 5 and res.recoveries == ["job slots"]
    assert torch.isfinite(res.loss_history).all()
    for p in range(2):
        assert torch.equal(res.dofs[p], solo[p]["history"][5].cpu()), p
    assert torch.equal(model.dof.detach(), solo[res.winner]["history"][5])
    assert torch.equal(model.history_ops[:5], solo[res.winner]["history"][:5])
