"""The fixed-launch-chain step (FusedPoseStep: pose kernels + fused render + Adam kernel) is the autograd step of
RBSolverTrainer, number for number: same loss, same dof trajectory, same history rows; and it is bit-reproducible."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def problem(xarm7, B, H, W, scale, links=None):
    """links: build the scene from the first `links` links of the robot only (default: all of them)."""
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    K = scaled_K(XARM7_K_1280x720, scale, W, H, True)
    _, lp = make_views(xarm7, B, seed=0)
    meshes = xarm7.meshes
    if links is not None:
        lp, meshes = np.ascontiguousarray(lp[:, :links]), xarm7.meshes[:links]
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()

    def make():
        return RBSolver(cfg, meshes=meshes).to(dev)

    m0 = make()
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lpt = torch.tensor(lp, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((B, H, W), device=dev))
    batch = {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(B, 1, 1)}
    return cfg, make, batch


def test_pose_kernels_match_torch_math(xarm7):
    """ehr_pose_forward's MVP and ehr_pose_backward's dof gradient against torch autograd on the same tensors."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 240, 320, 0.25)
    model = make()
    fs = FusedPoseStep(model, batch)
    dof0 = model.dof.detach().clone()
    fs.step()
    torch.cuda.synchronize()
    d = dof0.clone().requires_grad_(True)
    from easyhec_amd.se3 import se3_exp_map
    Tc = se3_exp_map(d[None]).permute(0, 2, 1)[0]
    mvp = fused.mvp_matrices(batch["K"][0], 240, 320, Tc, batch["link_poses"])
    assert (mvp - fs.mvp).abs().max() <= 2e-6 * mvp.abs().max()
    (mvp * fs.grad_mvp).sum().backward()
    g = d.grad / 3.0
    assert (g - fs.grad).abs().max() <= 1e-4 * g.abs().max()
    assert abs(float(fs.loss) - float(fs.loss_b.mean())) <= 1e-6 * float(fs.loss)
    assert (model.history_ops[0] == dof0).all() and int(fs.step_t) == 1


def test_fast_step_tracks_autograd_step(xarm7):
    from easyhec_amd.trainer import RBSolverTrainer
    cfg, make, batch = problem(xarm7, 4, 240, 320, 0.25)
    ma, mf, mg = make(), make(), make()
    ta = RBSolverTrainer(cfg, ma, batch)
    tf = RBSolverTrainer(cfg, mf, batch, fast=True)
    tg = RBSolverTrainer(cfg, mg, batch, fast=True)
    la, lf = [], []
    for it in range(12):
        la.append(float(ta.step()[1]))
        lf.append(float(tf.step()[1]))
        # identical arithmetic up to rounding; rounding differences are amplified by the (discontinuous) raster after
        # a few steps, exactly as between two nvdiffrast runs (tests/test_gpu_solver.py docstring)
        d = float((ma.dof.detach() - mf.dof.detach()).abs().max())
        assert d <= (5e-5 if it < 3 else 1e-2), (it, d)
    assert np.allclose(la[:3], lf[:3], rtol=2e-4)
    assert la[-1] < la[0]
    # two independent contexts run the same chain bit for bit from the same state (no float atomics anywhere)
    mg.dof.data.copy_(mf.dof.data)
    tg.fast.exp_avg.copy_(tf.fast.exp_avg)
    tg.fast.exp_avg_sq.copy_(tf.fast.exp_avg_sq)
    tg.fast.step_t.copy_(tf.fast.step_t)
    for _ in range(5):
        l1 = float(tf.step()[1])
        l2 = float(tg.step()[1])
        assert l1 == l2
    assert (mf.dof.detach() == mg.dof.detach()).all()
    # Adam state is torch.optim.Adam-shaped
    sd = tf.fast.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 17


@pytest.mark.parametrize("B,H,W,scale", [(3, 240, 320, 0.25), (8, 720, 1280, 1.0)])
def test_merged_step_equals_the_separate_kernels(xarm7, B, H, W, scale):
    """ehr_solver_step (what bench.py times) against ehr_pose_forward -> ehr_render_mask_loss -> ehr_pose_backward ->
    ehr_pose_adam called one by one from the same state: identical bits -- also at BASELINE configs[2]'s full size
    (8 views 1280x720), where ehr_render_mask_loss is the entry point tests/test_gpu_fused.py checks against the
    oracle, which closes the chain  oracle == ehr_render_mask_loss == timed step."""
    import ctypes
    from easyhec_amd import _lib, fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, B, H, W, scale)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    lib = _lib.lib()
    f = lambda x: ctypes.c_float(float(x))
    for it in range(4):
        fa.step()
        # the same step, piece by piece, on model b
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dof, hist = mb.dof.data, mb.history_ops
        _lib.check(lib.ehr_pose_forward(_lib.ptr(dof), _lib.ptr(fb.K), _lib.ptr(fb.link_poses), fb.B, fb.L, fb.H, fb.W,
                                        f(fb.near), f(fb.far), _lib.ptr(fb.mvp), _lib.ptr(fb.tc_jac),
                                        _lib.ptr(fb.hist_row), _lib.ptr(hist), hist.shape[0], stream), "fwd")
        fb.hist_row += 1  # ehr_solver_step advances the history row itself, the stand-alone kernel only reads it
        fused._launch(fb.glctx, fb.scene, fb.mvp, fb.ref, None, fb.loss_b, fb.grad_mvp)
        _lib.check(lib.ehr_pose_backward(_lib.ptr(fb.grad_mvp), _lib.ptr(fb.loss_b), _lib.ptr(fb.K),
                                         _lib.ptr(fb.link_poses), _lib.ptr(fb.tc_jac), fb.B, fb.L, fb.H, fb.W,
                                         f(fb.near), f(fb.far), _lib.ptr(fb.red), stream), "bwd")
        _lib.check(lib.ehr_pose_adam(_lib.ptr(dof), _lib.ptr(fb.exp_avg), _lib.ptr(fb.exp_avg_sq), _lib.ptr(fb.step_t),
                                     _lib.ptr(fb.red), f(fb.lr), f(fb.betas[0]), f(fb.betas[1]), f(fb.eps), f(fb.wd),
                                     _lib.ptr(fb.loss), _lib.ptr(fb.grad), stream), "adam")
        torch.cuda.synchronize()
        for name in ["mvp", "tc_jac", "loss_b", "grad_mvp", "red", "loss", "grad", "exp_avg", "exp_avg_sq", "step_t",
                     "hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data) and torch.equal(ma.history_ops[:8], mb.history_ops[:8])
    fused.check_status(fa.glctx)


def test_graph_replay_equals_eager_launches(xarm7):
    """The step captured as a hipGraph by the library (ehr_graph_begin / _end / _launch: main-stream chain + the
    side-stream kernels and their fork/join events) replays to the same bits as eager launches, with several
    rasterizer contexts alive in the process and interleaved with eager work on another context."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 240, 320, 0.25)
    ma, mb, mc = make(), make(), make()
    fa, fb, fc = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch), FusedPoseStep(mc, batch)
    fb.capture()
    for it in range(25):
        fa.step()
        fb.step()                      # one ehr_graph_launch
        if it % 5 == 0:
            fc.step()                  # unrelated eager work on a third context in between
    torch.cuda.synchronize()
    for name in ["mvp", "tc_jac", "loss_b", "grad_mvp", "red", "loss", "grad", "exp_avg", "exp_avg_sq", "step_t"]:
        assert torch.equal(getattr(fa, name), getattr(fb, name)), name
    assert torch.equal(ma.dof.data, mb.dof.data) and torch.equal(ma.history_ops[:30], mb.history_ops[:30])
    assert int(fb.step_t.item()) == 25
    fused.check_status(fb.glctx)
    # a step that wants the mask falls back to eager launches and keeps the trajectory
    fa.step(want_mask=True)
    fb.step(want_mask=True)
    torch.cuda.synchronize()
    assert torch.equal(ma.dof.data, mb.dof.data) and torch.equal(fa.mask, fb.mask)
    fb.release_graph()
    fa.step()
    fb.step()
    torch.cuda.synchronize()
    assert torch.equal(ma.dof.data, mb.dof.data)


def test_outputs_step_shares_the_optimiser_state(xarm7):
    """RBSolverTrainer(fast=True).step(with_outputs=True) is the SAME launch chain with the mask written (it used to
    fall through to torch autograd with a second Adam state): a run that asks for outputs every third step is bit
    identical to one that never does, and the outputs describe the pose the step started from."""
    from easyhec_amd.trainer import RBSolverTrainer
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    from easyhec_amd.synthetic import camera_Tc_c2b
    batch = dict(batch)
    batch["Tc_c2b"] = torch.tensor(camera_Tc_c2b(), dtype=torch.float32, device="cuda:0")[None].repeat(2, 1, 1)
    ma, mb = make(), make()
    ta, tb = RBSolverTrainer(cfg, ma, batch, fast=True), RBSolverTrainer(cfg, mb, batch, fast=True)
    for it in range(9):
        ta.step()
        out, loss = tb.step(with_outputs=(it % 3 == 0))
        if it % 3 == 0:
            assert set(out) >= {"rendered_masks", "ref_masks", "error_maps", "metrics", "tsfm"}
            assert out["rendered_masks"].shape == batch["mask"].shape and float(out["rendered_masks"].max()) <= 1.0
            sse = ((out["rendered_masks"] - batch["mask"]) ** 2).sum(dim=(1, 2)).mean()
            assert abs(float(sse) - float(loss)) <= 1e-4 * float(loss)       # the loss of exactly these masks
            assert torch.equal(mb.history_ops[it], ma.history_ops[it])
    torch.cuda.synchronize()
    assert torch.equal(ma.dof.data, mb.dof.data) and torch.equal(ta.fast.exp_avg, tb.fast.exp_avg)
    assert ta.global_steps == tb.global_steps == 9 and int(tb.fast.step_t) == 9


def test_fresh_optimiser_on_a_loaded_model_is_adam_step_one(xarm7, tmp_path):
    """A solver built on a model that already holds N history rows (the reference's load_model path, or a checkpoint
    without an optimiser) starts a FRESH Adam: step count 0, zero moments -- the first update is lr * sign(g), exactly
    what torch.optim.Adam does on the same gradient -- while the pose history keeps appending at row N.  (The launch
    chain used to take N as Adam's step count: bias corrections of step N + 1 on zero moments, a 2.5-3x lr first update.)"""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.trainer import RBSolverTrainer
    cfg, make, batch = problem(xarm7, 2, 120, 160, 0.125)
    t0 = RBSolverTrainer(cfg, make(), batch, fast=True)
    for _ in range(40):
        t0.step()
    path = str(tmp_path / "m.pth")
    t0.save(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    del ck["optimizer"]                                  # what the reference's load_model path sees
    torch.save(ck, path)
    hist40 = t0.model.history_ops[:40].clone()
    # (a) FusedPoseStep on a loaded model
    m = make()
    m.load_state_dict(ck["model"])
    fs = FusedPoseStep(m, batch)
    assert int(fs.step_t) == 0 and int(fs.hist_row) == 40
    dof0 = m.dof.detach().clone()
    fs.step()
    torch.cuda.synchronize()
    g = fs.grad.clone()                                  # gradient of the mean loss at dof0 (before weight decay)
    p = dof0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=fs.lr, betas=fs.betas, eps=fs.eps, weight_decay=fs.wd)
    p.grad = g.clone()
    opt.step()
    assert (m.dof.detach() - p.detach()).abs().max() <= 1e-7
    assert float((m.dof.detach() - dof0).abs().max()) <= fs.lr * 1.0001   # |first update| = lr, not 2.5-3 lr
    assert int(fs.step_t) == 1 and int(fs.hist_row) == 41
    assert torch.equal(m.history_ops[:40], hist40) and torch.equal(m.history_ops[40], dof0)
    # (b) trainer.resume() on the optimiser-less checkpoint: same semantics
    tr = RBSolverTrainer(cfg, make(), batch, fast=True)
    tr.resume(path)
    assert int(tr.fast.step_t) == 0 and int(tr.fast.hist_row) == 40 and float(tr.fast.exp_avg.abs().max()) == 0
    tr.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.model.dof.detach(), m.dof.detach())
    # (c) a loaded optimiser whose step count is smaller than the history cursor never overwrites history rows
    ck2 = torch.load(path, map_location="cpu", weights_only=False)
    ck2["optimizer"] = {"state": {0: {"step": torch.tensor(5.0), "exp_avg": torch.zeros(6), "exp_avg_sq": torch.zeros(6)}},
                        "param_groups": []}
    torch.save(ck2, path)
    tr2 = RBSolverTrainer(cfg, make(), batch, fast=True)
    tr2.resume(path)
    assert int(tr2.fast.step_t) == 5 and int(tr2.fast.hist_row) == 40
    tr2.step()
    torch.cuda.synchronize()
    assert torch.equal(tr2.model.history_ops[:40], hist40)


def test_default_solver_context_stays_under_100_mb_at_8_views_720p(xarm7):
    """8 views x 8 links at 1280x720 used to reserve 0.8 GB of job slots (one per (view, link, tile))
    for 17 MB touched; the launch chain now plans half as many slots as a view has tiles (a robot's links touch ~5 % of them)."""
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 8, 720, 1280, 1.0)
    m = make()
    f = FusedPoseStep(m, batch)
    for _ in range(3):
        f.step()
    torch.cuda.synchronize()
    from easyhec_amd import fused
    fused.check_status(f.glctx)
    mb = f.glctx.scratch_bytes() / 1048576.0
    assert f.slack == 0.5 and mb <= 100.0, mb   # 50 MB of slots + records, clip-space vertices, hint tables, spill pool (16 MB)


def test_clip_space_vertices_on_demand_equal_the_kept_ones(xarm7, monkeypatch):
    """Round 6: a plan either keeps every vertex's clip-space position per view (posc, written by the vertex kernel) or lets
    the depth tests, the silhouette analysis and the backward pass transform the few vertices they look up themselves
    (VbLazy in csrc/ehr_vbuf.hip: the choice for meshes with unshared vertices, V > 1.5 T).  Same fma chain on the same matrix:
    the launch chain's losses, gradients and pose trajectory must be bit-identical either way, and so must the stateless
    render (mask included)."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = problem(xarm7, 3, 240, 320, 0.25)
    res = {}
    for lazy in ("0", "1"):
        monkeypatch.setenv("EHR_VB_LAZY", lazy)     # (read by ehr_fused_plan: every FusedPoseStep below plans afresh)
        m = make()
        f = FusedPoseStep(m, batch)
        losses = [float(f.step()) for _ in range(6)]
        f.step(want_mask=True)
        torch.cuda.synchronize()
        fused.check_status(f.glctx)
        res[lazy] = (losses, m.dof.detach().clone(), f.grad_mvp.clone(), f.mask.clone(), f.loss_b.clone())
    monkeypatch.delenv("EHR_VB_LAZY")
    a, b = res["0"], res["1"]
    assert a[0] == b[0] and a[0][-1] < a[0][0]
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    assert float(a[3].sum()) > 100.0
