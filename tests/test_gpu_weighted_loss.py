"""Per-pixel weights of the fused mask loss (ehr_fused_bind_weight) on the GPU: loss = sum w (m - r)^2 in
the stateless op, under a bound reference, in the solver step, the multi-start step and their captured graphs.  Anchors: an
all-ones weight is no weight, bit for bit; binary weights against the CPU oracle on the reference with the hidden pixels
replaced by the oracle's own mask; real weights against the float64 reference of tests/weighted_loss_reference.py with the
per-block bars of tests/fused_loss_reference.py; tests/test_weighted_loss_reference.py pins the references on the CPU."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import helpers
import weighted_loss_reference as WR
from test_gpu_fast import problem
from test_gpu_finisher import STATE, _piecewise_step
from test_gpu_fused_loss import XARM7_KEYS, link_scene, soft_problem, unaligned

pytestmark = pytest.mark.gpu

STEPS = 30
SOLVE_STATE = ["exp_avg", "exp_avg_sq", "step_t", "loss", "loss_b", "grad_mvp"]


@pytest.fixture(scope="module")
def env(xarm7):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr, fused
    assert _lib.has_weighted_loss(), "libehr_hip.so has no ehr_fused_bind_weight"
    dev = torch.device("cuda:0")
    scene = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    return fused, dr, scene, dev


def call(fused, ctx, scene, mvp, ref, w, dev, bind=False, want_mask=True):
    """One fused call on device tensors ``ref`` / ``w`` (None: no weights): weights first, then (bind) the reference.
    -> mask, loss, grad as numpy."""
    B, H, W = ref.shape
    tm = torch.as_tensor(mvp, device=dev)
    fused._ensure_plan(ctx, scene, B, H, W)
    fused.bind_weight(ctx, scene, w, views=B)
    if bind:
        fused.bind_ref(ctx, scene, ref)
    mask = torch.full((B, H, W), float("nan"), device=dev) if want_mask else None
    loss, grad = torch.empty((B,), device=dev), torch.empty((B, scene.num_links, 4, 4), device=dev)
    fused._launch(ctx, scene, tm, ref, mask, loss, grad)
    torch.cuda.synchronize()
    return None if mask is None else mask.cpu().numpy(), loss.cpu().numpy(), grad.cpu().numpy()


def same(a, b):
    return all(x is None or y is None or (x == y).all() for x, y in zip(a, b))


# ---- 1. ones are nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", XARM7_KEYS + [("ties",)], ids=lambda k: "x".join(str(v) for v in k[1:3]) or "ties")
def test_unit_weights_change_no_bit(env, oracle, xarm7, key):
    fused, dr, scene, dev = env
    e = R.expected_for(oracle, xarm7, key, "uniform")
    sc = scene if key[0] == "xarm7" else link_scene(fused, e.s, dev)
    ref = torch.tensor(e.ref, device=dev)
    ones = torch.ones_like(ref)
    ctx = dr.RasterizeCudaContext()
    base = call(fused, ctx, sc, e.s.mvp, ref, None, dev)
    R.check_against_oracle(*base, e, "no weights")
    assert same(base, call(fused, ctx, sc, e.s.mvp, ref, ones, dev))
    assert same(base, call(fused, ctx, sc, e.s.mvp, ref, ones[:1].contiguous(), dev))      # one image shared by every view
    for want_mask in (False, True):
        assert same(base, call(fused, ctx, sc, e.s.mvp, ref, ones, dev, bind=True, want_mask=want_mask))
    if e.s.W % 4 == 0:  # weights that are not 16-byte aligned: the scalar path, stateless and bound
        assert same(base, call(fused, ctx, sc, e.s.mvp, ref, unaligned(ones), dev))
        assert same(base, call(fused, ctx, sc, e.s.mvp, ref, unaligned(ones), dev, bind=True))
    fused.check_status(ctx)
    # the autograd entry point: weight= binds, weight=None unbinds
    tm = torch.tensor(e.s.mvp, device=dev, requires_grad=True)
    mask, loss = fused.render_mask_loss(ctx, sc, tm, ref, weight=ones)
    assert ctx._bound_weight is ones
    loss.sum().backward()
    assert same(base, (mask.cpu().numpy(), loss.detach().cpu().numpy(), tm.grad.cpu().numpy()))
    fused.render_mask_loss(ctx, sc, tm.detach(), ref)
    assert ctx._bound_weight is None


def solo_solve(xarm7, batch_of, steps=STEPS, graph=False, B=2):
    """A FusedPoseStep solve of `steps` steps on soft_problem with batch_of(batch) -> dof trajectory [steps,6] and end state."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = soft_problem(xarm7, B, 120, 160, 0.125)
    model = make()
    fs = FusedPoseStep(model, batch_of(batch))
    if graph:
        fs.capture()
    traj = []
    for _ in range(steps):
        fs.step()
        traj.append(model.dof.detach().clone())
    torch.cuda.synchronize()
    fused.check_status(fs.glctx)
    assert int(fs.step_t.item()) == steps
    return torch.stack(traj), {k: getattr(fs, k).clone() for k in SOLVE_STATE}


def multi_solve(xarm7, batch_of, steps=STEPS, graph=False, P=3, Bv=2):
    from easyhec_amd import fused
    from easyhec_amd.multistart import MultiStartPoseStep
    from test_gpu_multistart import starts_for
    cfg, make, batch = soft_problem(xarm7, Bv, 120, 160, 0.125)
    ms = MultiStartPoseStep(make(), batch_of(batch), starts_for(cfg, P))
    if graph:
        ms.capture()
    traj = []
    for _ in range(steps):
        ms.step()
        traj.append(ms.dof.clone())
    torch.cuda.synchronize()
    fused.check_status(ms.glctx)
    assert int(ms.step_t.min()) == steps
    return torch.stack(traj), {k: getattr(ms, k).clone() for k in SOLVE_STATE}


def assert_same_solve(a, b):
    assert torch.equal(a[0], b[0])
    for k in SOLVE_STATE:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("solve", [solo_solve, multi_solve], ids=["solo", "multi"])
def test_a_solve_with_unit_weights_is_the_unweighted_solve(xarm7, solve):
    plain = solve(xarm7, lambda b: b)
    ones = solve(xarm7, lambda b: dict(b, weight=torch.ones_like(b["mask"])))
    assert_same_solve(plain, ones)
    assert not torch.equal(plain[0][0], plain[0][-1])


# ---- 2. binary weights against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", WR.BINARY_PATTERNS)
@pytest.mark.parametrize("key", XARM7_KEYS, ids=lambda k: "%dx%d" % (k[1], k[2]))
def test_binary_weights_match_the_oracle_on_the_hidden_reference(env, oracle, xarm7, key, pattern):
    """The GPU on (ref, w) against oracle.render_mask_loss on ref' = where(w, ref, oracle mask): a pixel with e == 0
    contributes exactly what a pixel with w == 0 does, so the bars of check_against_oracle apply unchanged.  Stateless and
    bound, which are bit-equal."""
    fused, dr, scene, dev = env
    e = R.expected_for(oracle, xarm7, key, "uniform")
    w, eh = WR.expected_binary(oracle, xarm7, key, "uniform", pattern)
    ref, wt = torch.tensor(e.ref, device=dev), torch.tensor(w, device=dev)
    ctx = dr.RasterizeCudaContext()
    got = call(fused, ctx, scene, e.s.mvp, ref, wt, dev)
    fused.check_status(ctx)
    what = f"binary {key[1]}x{key[2]} {pattern}"
    R.check_against_oracle(*got, eh, what)
    sse = WR.weighted_sse(got[0], e.ref, w)
    assert (np.abs(got[1] - sse) <= 1e-6 * np.abs(sse)).all(), what
    assert same(got, call(fused, ctx, scene, e.s.mvp, ref, wt, dev, bind=True, want_mask=False))
    fused.check_status(ctx)


# ---- 3. real weights against the float64 reference -----------------------------------------------------------------------
REAL_CASES = [(k, kind) for k in XARM7_KEYS for kind in ("uniform", "own_aa")] + [(("ties",), "uniform")]


@pytest.mark.parametrize("key,kind", REAL_CASES, ids=["%s-%s" % ("x".join(str(v) for v in k[1:3]) or "ties", kind) for k, kind in REAL_CASES])
def test_real_weights_match_the_float64_reference(env, oracle, xarm7, key, kind):
    """w uniform in [0, 2]: masks bit-exact (they do not depend on w), loss within 1e-6 of the float64 weighted SSE of the
    GPU's own mask, the suite's global 1e-5 bar and every (view, link) block within its own bar."""
    fused, dr, scene, dev = env
    w, e, c = WR.expected_real(oracle, xarm7, key, kind)
    sc = scene if key[0] == "xarm7" else link_scene(fused, e.s, dev)
    ref, wt = torch.tensor(e.ref, device=dev), torch.tensor(w, device=dev)
    ctx = dr.RasterizeCudaContext()
    what = f"weighted {e.s.name} {kind}"
    mask, loss, grad = call(fused, ctx, sc, e.s.mvp, ref, wt, dev)
    fused.check_status(ctx)
    assert (mask == e.m_ref).all(), what
    sse = WR.weighted_sse(mask, e.ref, w)
    assert (np.abs(loss - sse) <= 1e-6 * np.abs(sse)).all(), what
    assert (np.abs(loss - c.loss) <= 1e-6 * np.abs(c.loss)).all(), what
    assert np.abs(grad - c.G).max() <= 1e-5 * np.abs(c.G).max(), what
    assert (grad[:, :, 2, :] == 0).all(), what
    R.check_blocks(grad, c, what)
    assert same((mask, loss, grad), call(fused, ctx, sc, e.s.mvp, ref, wt, dev, bind=True))


# ---- 4. zero weight hides the reference -------------------------------------------------------------------------------------
def hide(batch, seed):
    """batch with a speckle of zero weights and a reference that is arbitrary (finite) under them"""
    rng = np.random.default_rng(5)
    w = torch.tensor((rng.uniform(size=tuple(batch["mask"].shape)) > 0.4).astype(np.float32), device=batch["mask"].device)
    junk = torch.tensor(np.random.default_rng(seed).uniform(-50, 50, size=tuple(w.shape)).astype(np.float32), device=w.device)
    return dict(batch, weight=w, mask=torch.where(w > 0, batch["mask"], junk))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("solve", [solo_solve, multi_solve], ids=["solo", "multi"])
def test_the_reference_under_a_zero_weight_is_never_seen(xarm7, solve, graph):
    a = solve(xarm7, lambda b: hide(b, 1), graph=graph)
    b = solve(xarm7, lambda b: hide(b, 2), graph=graph)
    assert_same_solve(a, b)
    assert bool(torch.isfinite(a[1]["loss"]).all()) and not torch.equal(a[0][0], a[0][-1])


# ---- 5. bound equals unbound; the binding protocol ------------------------------------------------------------------------
def test_binding_protocol(env, oracle, xarm7):
    fused, dr, scene, dev = env
    w, e, c = WR.expected_real(oracle, xarm7, XARM7_KEYS[0], "uniform")
    ref, wt = torch.tensor(e.ref, device=dev), torch.tensor(w, device=dev)
    ctx = dr.RasterizeCudaContext()
    plain = call(fused, ctx, scene, e.s.mvp, ref, None, dev)
    weighted = call(fused, ctx, scene, e.s.mvp, ref, wt, dev)
    assert not (plain[1] == weighted[1]).any()
    for want_mask in (False, True):
        assert same(weighted, call(fused, ctx, scene, e.s.mvp, ref, wt, dev, bind=True, want_mask=want_mask))

    def launch():
        loss, grad = torch.empty((e.s.B,), device=dev), torch.empty((e.s.B, scene.num_links, 4, 4), device=dev)
        fused._launch(ctx, scene, torch.tensor(e.s.mvp, device=dev), ref, None, loss, grad)
        torch.cuda.synchronize()
        return None, loss.cpu().numpy(), grad.cpu().numpy()

    # bind_weight after bind_ref leaves the reference unbound: right results, by the unbound path
    fused.bind_ref(ctx, scene, ref)
    assert ctx._bound_ref is ref
    fused.bind_weight(ctx, scene, wt)
    assert ctx._bound_ref is None and ctx._bound_weight is wt
    assert same(weighted, launch())
    # ... observed on the library, not on the Python mirror: the unbound path streams every tile, so it sees a pixel written
    # into a tile no link touches; the bound path adds that tile's CACHED sum and cannot
    assert e.m_ref[1, :8, :32].max() == 0 and float(wt[1, 3, 5]) > 0
    keep = float(ref[1, 3, 5])
    ref[1, 3, 5] = keep + 3.0
    moved = call(fused, dr.RasterizeCudaContext(), scene, e.s.mvp, ref.clone(), wt, dev)   # the truth for the edited reference
    assert moved[1][1] != weighted[1][1] and moved[1][0] == weighted[1][0]
    assert same(moved, launch())                         # unbound: the edit is seen
    ref[1, 3, 5] = keep
    fused.bind_ref(ctx, scene, ref)
    ref[1, 3, 5] = keep + 3.0
    assert same(weighted, launch())                      # bound (what a caller must not do): the cached sum answers
    ref[1, 3, 5] = keep
    fused.bind_ref(ctx, scene, ref)                      # the sparse path again, on sum(w r^2)
    assert same(weighted, launch())
    w2 = (2.0 - wt).contiguous()                         # other weights: new sums
    want2 = call(fused, dr.RasterizeCudaContext(), scene, e.s.mvp, ref, w2, dev)
    fused.bind_weight(ctx, scene, w2)
    fused.bind_ref(ctx, scene, ref)
    assert same(want2, launch()) and not (want2[1] == weighted[1]).any()
    sse2 = WR.weighted_sse(want2[0], e.ref, w2.cpu().numpy())
    assert (np.abs(want2[1] - sse2) <= 1e-6 * sse2).all()
    fused.bind_weight(ctx, scene, None)                  # back to the unweighted bits, unbound and bound
    assert ctx._bound_weight is None and ctx._bound_ref is None
    assert same(plain, launch())
    fused.bind_ref(ctx, scene, ref)
    assert same(plain, launch())
    fused.check_status(ctx)
    # a new plan forgets the weights
    fused.bind_weight(ctx, scene, wt)
    fused._ensure_plan(ctx, scene, e.s.B, e.s.H, e.s.W, slack=float(scene.num_links))   # (another budget, as roomy: a slot per link)
    assert ctx._bound_weight is None
    assert same(plain, launch())
    with pytest.raises(RuntimeError, match="multiple"):
        fused.bind_weight(ctx, scene, torch.ones((3, e.s.H, e.s.W), device=dev), views=7)


# ---- 6. the solver step equals its pieces ------------------------------------------------------------------------------------
def weighted_batch(batch, seed=0):
    return dict(batch, weight=torch.tensor(WR.real_weight(tuple(batch["mask"].shape), seed), device=batch["mask"].device))


@pytest.mark.parametrize("bound", [True, False], ids=["bound", "unbound"])
def test_weighted_solver_step_equals_the_stateless_pieces(xarm7, bound):
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = soft_problem(xarm7, 3, 120, 160, 0.125)
    batch = weighted_batch(batch)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    assert fa.weight is not batch["weight"] and torch.equal(fa.weight, batch["weight"]) and fa.glctx._bound_weight is fa.weight
    fused.bind_ref(fb.glctx, fb.scene, None)
    if not bound:
        fused.bind_ref(fa.glctx, fa.scene, None)
    for it in range(4):
        fa.step()
        _piecewise_step(fb, mb)             # (fused._launch on fb's context: its bound weights apply)
        torch.cuda.synchronize()
        for name in STATE + ["hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
    sse = WR.weighted_sse(fa_mask(fa), batch["mask"].cpu().numpy(), batch["weight"].cpu().numpy())
    assert (np.abs(fa.loss_b.cpu().numpy() - sse) <= 1e-6 * sse).all()
    fused.check_status(fa.glctx)


def fa_mask(fa):
    """the mask of the step just taken: one more step with a mask output renders the NEXT pose, so render fa.mvp statelessly"""
    from easyhec_amd import dr, fused
    ctx = dr.RasterizeCudaContext()
    with torch.no_grad():
        mask, _ = fused.render_mask_loss(ctx, fa.scene, fa.mvp.clone(), fa.ref)
    return mask.cpu().numpy()


def test_weighted_multi_start_hypotheses_equal_their_solo_solves(xarm7):
    """Shared weights [Bv] read by P x Bv virtual views: hypothesis p is the solo weighted solve from start p, bit for bit."""
    from test_gpu_multistart import assert_hypotheses_equal_solo, run_multi, solo_states, starts_for
    cfg, make, batch = soft_problem(xarm7, 2, 120, 160, 0.125)
    batch = weighted_batch(batch, seed=3)
    starts = starts_for(cfg, 3)
    ms, losses = run_multi(make, batch, starts)
    assert ms.weight.shape[0] == ms.Bv and ms.B == 3 * ms.Bv
    solo = solo_states(cfg, make, batch, starts)
    assert_hypotheses_equal_solo(ms, solo, losses=losses)
    plain = solo_states(cfg, make, {k: v for k, v in batch.items() if k != "weight"}, starts[:1])
    assert not torch.equal(plain[0]["dof"], solo[0]["dof"])


# ---- 7. chunks -----------------------------------------------------------------------------------------------------------------
def test_seventy_weighted_views_go_through_in_two_chunks(env, xarm7):
    fused, dr, scene, dev = env
    from test_gpu_fused import workload
    B, H, W, scale = 70, 120, 160, 0.125                # 70 views x 8 links = 560 units -> 2 chunks (64 + 6)
    assert scene.num_links == 8
    _, _, _, mvp = workload(xarm7, H, W, scale, B, seed=11)
    rng = np.random.default_rng(12)
    ref = torch.tensor(rng.uniform(size=(B, H, W)).astype(np.float32), device=dev)
    wt = torch.tensor(rng.uniform(0, 2, size=(B, H, W)).astype(np.float32), device=dev)   # a different image per view
    big, small = dr.RasterizeCudaContext(), dr.RasterizeCudaContext()
    all_ = call(fused, big, scene, mvp, ref, wt, dev)
    assert same(all_, call(fused, big, scene, mvp, ref, wt, dev, bind=True, want_mask=False))
    fused.check_status(big)
    for lo in (0, 31, 62, 67):                           # 3-view calls, one of them across the chunk border
        sl = slice(lo, lo + 3)
        got = call(fused, small, scene, mvp[sl], ref[sl].contiguous(), wt[sl].contiguous(), dev)
        assert same(tuple(x[sl] for x in all_), got), lo
    sse = WR.weighted_sse(all_[0], ref.cpu().numpy(), wt.cpu().numpy())
    assert (np.abs(all_[1] - sse) <= 1e-6 * sse).all()


# ---- 8. graph ------------------------------------------------------------------------------------------------------------------
def test_a_captured_weighted_chain_replays_the_eager_bits_and_rebinding_drops_it(xarm7):
    from easyhec_amd import _lib, fused
    eager = solo_solve(xarm7, weighted_batch, steps=8)
    graph = solo_solve(xarm7, weighted_batch, steps=8, graph=True)
    assert_same_solve(eager, graph)
    from easyhec_amd.fast import FusedPoseStep
    cfg, make, batch = soft_problem(xarm7, 2, 120, 160, 0.125)
    fs = FusedPoseStep(make(), weighted_batch(batch))
    fs.capture()
    fs.step()
    fused.bind_weight(fs.glctx, fs.scene, fs.weight, views=fs.B)     # the old exec is gone, as after bind_ref
    with pytest.raises(RuntimeError, match="no instantiated graph"):
        _lib.check(_lib.lib().ehr_graph_launch(fs.glctx.handle, None), "ehr_graph_launch")


def test_a_chain_step_takes_its_own_weights_back(xarm7):
    """The weights are state of the CONTEXT, which the solver's forward shares with the launch chain: a render_mask_loss with
    other weights, or none, between two steps must not change what the chain minimises.  step() binds its own again (and
    captures again where it was replaying): the trajectory equals the undisturbed one bit for bit, eager and captured."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    want = solo_solve(xarm7, weighted_batch, steps=8)
    for graph in (False, True):
        cfg, make, batch = soft_problem(xarm7, 2, 120, 160, 0.125)
        model = make()
        fs = FusedPoseStep(model, weighted_batch(batch))
        if graph:
            fs.capture()
        traj = []
        for it in range(8):
            if it == 3:    # the forward of a caller without weights: unbinds them on the shared context
                with torch.no_grad():
                    fused.render_mask_loss(fs.glctx, fs.scene, fs.mvp.clone(), batch["mask"])
                assert fs.glctx._bound_weight is None
            if it == 5:    # ... and one with other weights
                with torch.no_grad():
                    fused.render_mask_loss(fs.glctx, fs.scene, fs.mvp.clone(), batch["mask"], weight=torch.ones_like(batch["mask"]))
                assert fs.glctx._bound_weight is not fs.weight
            fs.step()
            assert fs.glctx._bound_weight is fs.weight and fs.glctx._bound_ref is fs.ref and bool(fs._graph) == graph
            traj.append(model.dof.detach().clone())
        torch.cuda.synchronize()
        fused.check_status(fs.glctx)
        assert torch.equal(torch.stack(traj), want[0]), graph
        for k in SOLVE_STATE:
            assert torch.equal(getattr(fs, k), want[1][k]), (graph, k)


# ---- 9. reported, not silent ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,where", [(float("nan"), "covered_tile"), (float("nan"), "empty_tile"), (1e20, "covered_tile")],
                         ids=["nan-job", "nan-empty", "1e20"])
def test_bad_weights_are_reported(env, oracle, xarm7, bad, where):
    fused, dr, scene, dev = env
    from easyhec_amd.fast import FusedPoseStep
    e = R.expected_for(oracle, xarm7, XARM7_KEYS[0], "uniform")
    ref = torch.tensor(e.ref, device=dev)
    if where == "empty_tile":
        y, x = 3, 5
        assert e.m_ref[1, :8, :32].max() == 0
    else:
        inside = np.argwhere(e.m_ref[1] == 1)
        y, x = (int(v) for v in inside[len(inside) // 2])
    assert e.ref[1, y, x] != e.m_ref[1, y, x]             # e != 0 there: the addend is w e^2
    wt = torch.ones_like(ref)
    wt[1, y, x] = bad
    for bind in (False, True):
        ctx = dr.RasterizeCudaContext()
        _, loss, grad = call(fused, ctx, scene, e.s.mvp, ref, wt, dev, bind=bind, want_mask=False)
        assert np.isnan(loss).all() and np.isnan(grad).all(), bind
        with pytest.raises(RuntimeError, match="overflow"):
            fused.check_status(ctx)
    cfg, make, batch = soft_problem(xarm7, 2, 120, 160, 0.125)
    if where == "covered_tile":
        inside = (batch["mask"][1] > 0.9).nonzero()
        y, x = (int(v) for v in inside[len(inside) // 2])
    batch = dict(batch, weight=torch.ones_like(batch["mask"]))
    batch["weight"][1, y, x] = bad
    for unbind in (False, True):
        model = make()
        fs = FusedPoseStep(model, batch)
        if unbind:
            fused.bind_ref(fs.glctx, fs.scene, None)
        dof0 = model.dof.detach().clone()
        fs.step()
        torch.cuda.synchronize()
        assert torch.isnan(fs.loss).all() and torch.isnan(fs.loss_b).all()
        assert torch.equal(model.dof.detach(), dof0)
        assert float(fs.exp_avg.abs().sum()) == 0 and float(fs.exp_avg_sq.abs().sum()) == 0 and int(fs.step_t.item()) == 0
        with pytest.raises(RuntimeError, match="overflow"):
            fused.check_status(fs.glctx)


# ---- 10. an occluder, end to end -----------------------------------------------------------------------------------------------
def test_zero_weights_on_an_occluder_bring_the_solve_back(xarm7):
    """4 views at 160x120, references rendered at the true camera pose, then a rectangle per view set to 0 (something in front
    of the arm's far end segmented as background).  Three 300-step solves from the same perturbed start: clean, occluded, occluded with
    w = 0 on the rectangle.  The weighted solve ends strictly closer to the truth than the occluded unweighted one, in
    translation and in rotation.  The rectangle hides one END of the silhouette: that shortens it, which pulls the pose (a
    rectangle that leaves both ends in place removes as many pixels and hardly moves the optimum).  Figures:
    profiles/weighted_loss.md."""
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.se3 import se3_log_map
    from easyhec_amd.synthetic import camera_Tc_c2b
    B, H, W = 4, 120, 160
    cfg, make, batch = problem(xarm7, B, H, W, 0.125)
    clean = batch["mask"]
    m = clean.cpu().numpy()
    occ, wt = m.copy(), np.ones_like(m)
    for b in range(B):
        # the far end of the arm (what a payload in the gripper hides): the top rows of the foreground's box, as many as
        # hold 30 % of the foreground
        ys, xs = np.nonzero(m[b] > 0)
        rows = np.cumsum(m[b].sum(axis=1)) / m[b].sum()
        z = int(np.searchsorted(rows, 0.30)) + 1
        occ[b, ys.min():z, xs.min():xs.max() + 1] = 0
        wt[b, ys.min():z, xs.min():xs.max() + 1] = 0
        frac = 1.0 - occ[b].sum() / m[b].sum()
        assert 0.15 <= frac <= 0.40, (b, frac)
    dev = clean.device
    gt = se3_log_map(torch.tensor(camera_Tc_c2b(), dtype=torch.float32)[None].permute(0, 2, 1), eps=1e-5, backend="opencv")[0]

    def solve(bt):
        model = make()
        fs = FusedPoseStep(model, bt)
        for _ in range(300):
            fs.step()
        torch.cuda.synchronize()
        d = model.dof.detach().cpu()
        return float((d[:3] - gt[:3]).norm() * 100), float((d[3:] - gt[3:]).norm() * 180 / np.pi)

    e_clean = solve(batch)
    e_occ = solve(dict(batch, mask=torch.tensor(occ, device=dev)))
    e_w = solve(dict(batch, mask=torch.tensor(occ, device=dev), weight=torch.tensor(wt, device=dev)))
    print(f"[occluder] translation cm / rotation deg: clean {e_clean[0]:.4f} / {e_clean[1]:.4f}, occluded {e_occ[0]:.4f} / "
          f"{e_occ[1]:.4f}, occluded + weights {e_w[0]:.4f} / {e_w[1]:.4f}")
    assert e_w[0] < e_occ[0] and e_w[1] < e_occ[1]


# ---- 11. pose search ---------------------------------------------------------------------------------------------------------
def test_pose_search_ranks_on_the_valid_pixels(oracle, xarm7):
    from easyhec_amd import pose_search, space_explorer
    from easyhec_amd.synthetic import camera_Tc_c2b
    from test_gpu_pose_search import oracle_masks
    H, W, Bv, Q, P = 120, 160, 3, 12, 3
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    model = make()
    dev = batch["mask"].device
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    glctx, scene = model._ensure_renderer().glctx, model._ensure_scene()
    cands = np.concatenate([pose_search.sample_starts(Tc_init, Q, 0.03, 4.0, seed=2), Tc_gt[None]])
    mvp = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(cands, dtype=torch.float32, device=dev), batch["link_poses"])
    _, _, counts = space_explorer.mask_variance(glctx, scene, mvp[Q][:, None].contiguous(), H, W, return_counts=True)
    own = counts.float()                                    # the planted pose's own non-antialiased render
    wt = torch.ones_like(own)
    occ = own.clone()
    for b in range(Bv):
        ys = own[b].nonzero()[:, 0]
        a = int(ys.min()) + (int(ys.max()) - int(ys.min())) // 3
        occ[b, a:a + 12] = 0                                # an occluder over the arm ...
        wt[b, a:a + 12] = 0                                 # ... known to the weights
    bt = dict(batch, mask=occ, weight=wt)
    res = pose_search.search_starts(model, bt, Tc_init, Q, P, seed=2, extra=Tc_gt[None])
    masks = oracle_masks(oracle, xarm7, mvp.cpu().numpy(), H, W)
    valid, fg = wt.cpu().numpy() > 0, occ.cpu().numpy() > 0.5
    area = (masks & valid[None]).sum(axis=(2, 3))
    inter = (masks & fg[None] & valid[None]).sum(axis=(2, 3))
    ra = (fg & valid).sum(axis=(1, 2))
    assert (res.area.numpy() == area).all() and (res.inter.numpy() == inter).all() and (res.ref_area.numpy() == ra).all()
    assert (res.xor.numpy() == (area + ra[None] - 2 * inter).sum(axis=1)).all()
    assert int(res.xor[Q]) == 0 and res.ranking[0] == Q and float(res.iou[Q]) == 1.0 and int(res.xor[:Q].min()) > 0
    plain = pose_search.search_starts(model, dict(batch, mask=occ), Tc_init, Q, P, seed=2, extra=Tc_gt[None])
    assert int(plain.xor[Q]) > 0                            # without the weights the occluder counts against the true pose


def test_solve_global_with_weights_is_never_worse_than_the_weighted_solve(xarm7):
    from easyhec_amd import pose_search
    from test_gpu_multistart import solo_states
    H, W, Bv, Q, P, n, tail = 120, 160, 2, 16, 3, 30, 10
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    wt = torch.ones_like(batch["mask"])
    wt[:, 40:60] = 0
    batch = dict(batch, weight=wt)
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    search, res = pose_search.solve_global(cfg, make(), batch, Tc_init, Q, P, n, tail=tail)
    solo = solo_states(cfg, make, batch, [Tc_init], steps=n, recover=True)[0]
    assert torch.equal(res.dofs[0], solo["dof"].cpu())     # hypothesis 0 IS the plain weighted solve
    assert res.loss_history[:, 0].tolist() == solo["losses"]
    solo_tail = res.loss_history[-tail:].double().mean(dim=0)[0]
    assert torch.isfinite(res.losses).all() and float(res.losses[res.winner]) <= float(solo_tail)
