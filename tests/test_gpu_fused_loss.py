"""The last stage of the fused mask-loss path (vb_composite_kernel, the same stage inside ehr_solver_step) against the CPU
oracle on what the binary-reference cases of tests/test_gpu_fused.py leave out: real-valued and out-of-range reference
masks, clamp ties between links, images that are not 16-byte aligned, and references that the accumulators' guard has to
report.  Every comparison with the oracle also holds each (view, link) gradient block to its own bar
(tests/fused_loss_reference.py); tests/test_fused_loss_reference.py pins the oracle and the scenes on the CPU."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import helpers
from test_gpu_finisher import STATE, _piecewise_step
from test_gpu_fused import run

pytestmark = pytest.mark.gpu

XARM7_KEYS = [("xarm7",) + shape for shape in R.SOFT_SHAPES]


@pytest.fixture(scope="module")
def env(xarm7):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused
    dev = torch.device("cuda:0")
    ctx = dr.RasterizeCudaContext()
    scene = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    return fused, ctx, scene, dev


def link_scene(fused, s, dev):
    return fused.LinkScene([v for v, _ in s.meshes], [f for _, f in s.meshes], dev)


def stateless(fused, ctx, scene, mvp, ref, dev):
    """test_gpu_fused.run; a DEVICE tensor is passed on as it is (run() would copy it, and its address is the point)."""
    if not torch.is_tensor(ref):
        return run(fused, ctx, scene, mvp, ref, dev)
    tm = torch.tensor(mvp, device=dev, requires_grad=True)
    mask, loss = fused.render_mask_loss(ctx, scene, tm, ref)
    loss.sum().backward()
    torch.cuda.synchronize()
    fused.check_status(ctx)
    return mask.cpu().numpy(), loss.detach().cpu().numpy(), tm.grad.cpu().numpy()


def bound(fused, ctx, scene, mvp, ref, dev, want_mask=False):
    """bind_ref followed by fused._launch; ``ref``: a device tensor (bound as it is)."""
    B, H, W = ref.shape
    tm = torch.tensor(mvp, device=dev)
    fused._ensure_plan(ctx, scene, B, H, W)
    fused.bind_ref(ctx, scene, ref)
    mask = torch.full((B, H, W), float("nan"), device=dev) if want_mask else None
    loss, grad = torch.empty((B,), device=dev), torch.empty((B, scene.num_links, 4, 4), device=dev)
    fused._launch(ctx, scene, tm, ref, mask, loss, grad)
    torch.cuda.synchronize()
    fused.check_status(ctx)
    fused.bind_ref(ctx, scene, None)
    return None if mask is None else mask.cpu().numpy(), loss.cpu().numpy(), grad.cpu().numpy()


def both_forms_against_oracle(fused, scene, e, dev, what):
    from easyhec_amd import dr
    ctx = dr.RasterizeCudaContext()
    mask, loss, grad = stateless(fused, ctx, scene, e.s.mvp, e.ref, dev)
    R.check_against_oracle(mask, loss, grad, e, what + " stateless")
    _, loss_b, grad_b = bound(fused, ctx, scene, e.s.mvp, torch.tensor(e.ref, device=dev), dev)
    assert (loss_b == loss).all() and (grad_b == grad).all(), what            # (ii) bit-equal to (i)
    R.check_against_oracle(mask, loss_b, grad_b, e, what + " bound")


@pytest.mark.parametrize("kind", R.SOFT_REFS)
@pytest.mark.parametrize("key", XARM7_KEYS, ids=lambda k: "%dx%d" % (k[1], k[2]))
def test_soft_reference_masks_match_the_oracle(env, oracle, xarm7, key, kind):
    """Real-valued references (uniform in [0, 1); the oracle's own antialiased mask of the unperturbed pose; values in
    [-0.5, 2]) on the vector path (120 x 160) and the ragged one (100 x 150): e = mask - ref is non-zero on nearly every
    pixel, so nearly every blended pair reaches aa_pos_grad.  Stateless and bound form, each against the oracle."""
    fused, _, scene, dev = env
    both_forms_against_oracle(fused, scene, R.expected_for(oracle, xarm7, key, kind), dev, f"soft {key[1]}x{key[2]} {kind}")


@pytest.mark.parametrize("kind", R.TIE_REFS)
def test_clamp_ties_match_the_oracle(env, oracle, xarm7, kind):
    """Synthetic links whose antialiased fractions meet on one pixel: float32 sums of exactly 1.0f and an ulp or two either
    side (acc > 1 picks the mask value, acc <= 1 the gate), 1 + fraction under a fully covering link, three links in one
    sum (counts asserted in tests/test_fused_loss_reference.py)."""
    fused, _, _, dev = env
    e = R.expected_for(oracle, xarm7, ("ties",), kind)
    both_forms_against_oracle(fused, link_scene(fused, e.s, dev), e, dev, f"clamp ties {kind}")


def soft_problem(xarm7, B, H, W, scale):
    """test_gpu_fast.problem with a soft reference mask: the rendered one blended with uniform noise."""
    from test_gpu_fast import problem
    cfg, make, batch = problem(xarm7, B, H, W, scale)
    rng = np.random.default_rng(B * H + W)
    noise = torch.tensor(rng.uniform(size=(B, H, W)).astype(np.float32), device=batch["mask"].device)
    soft = (0.7 * batch["mask"] + 0.3 * noise).contiguous()
    return cfg, make, dict(batch, mask=soft)


def test_solver_step_on_a_soft_reference(oracle, xarm7):
    """FusedPoseStep (bound reference, default plan) on a soft batch["mask"]: four steps bit-equal to the piecewise step
    around the stateless op, and at step 1 loss_b and grad_mvp against the oracle on the mvp the step wrote."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    B, H, W = 3, 120, 160
    cfg, make, batch = soft_problem(xarm7, B, H, W, 0.125)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    fused.bind_ref(fb.glctx, fb.scene, None)
    ref = batch["mask"].cpu().numpy()
    assert ((ref > 0) & (ref < 1)).mean() > 0.9
    for it in range(4):
        fa.step()
        _piecewise_step(fb, mb)
        torch.cuda.synchronize()
        for name in STATE + ["hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
        if it == 0:
            mvp = fa.mvp.cpu().numpy()
            verts, tris, toff, voff = helpers.scene_arrays(xarm7)
            m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
            loss, grad = fa.loss_b.cpu().numpy(), fa.grad_mvp.cpu().numpy()
            sse = ((m_ref.astype(np.float64) - ref) ** 2).sum(axis=(1, 2))
            assert (np.abs(loss - sse) <= 1e-6 * sse).all()
            assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
            R.check_blocks(grad, R.block_reference(oracle, xarm7.meshes, mvp, ref), "solver step soft 120x160")
    assert int(fa.step_t.item()) == 4
    fused.check_status(fa.glctx)


def unaligned(t):
    """A contiguous copy of ``t`` that starts one element into a fresh buffer: 4-byte aligned only."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    u = buf[1:1 + t.numel()].view(t.shape)
    u.copy_(t)
    assert u.is_contiguous() and u.data_ptr() % 16 == 4
    return u


def test_unaligned_images_take_the_scalar_path_to_the_same_bits(env, oracle, xarm7):
    """W % 4 == 0 with a reference (or a mask output) that is not 16-byte aligned: the composite stage and the bind-time
    pass each decide their own vec_ok.  Stateless and bound, and the solver step with an unaligned mask output over an
    aligned reference: mask, loss and gradient equal the aligned call bit for bit."""
    fused, _, scene, dev = env
    from easyhec_amd import dr
    from easyhec_amd.fast import FusedPoseStep
    key = XARM7_KEYS[0]
    e = R.expected_for(oracle, xarm7, key, "uniform")
    assert e.s.W % 4 == 0
    ctx = dr.RasterizeCudaContext()
    ref_a = torch.tensor(e.ref, device=dev)
    ref_u = unaligned(ref_a)
    base = stateless(fused, ctx, scene, e.s.mvp, ref_a, dev)
    R.check_against_oracle(*base, e, "aligned")
    got = stateless(fused, ctx, scene, e.s.mvp, ref_u, dev)
    assert all((x == y).all() for x, y in zip(base, got))
    for want_mask in (False, True):
        a = bound(fused, ctx, scene, e.s.mvp, ref_a, dev, want_mask)
        u = bound(fused, ctx, scene, e.s.mvp, ref_u, dev, want_mask)
        for x, y, z in zip(a, u, base):
            if x is not None:
                assert (x == y).all() and (x == z).all()
    # solver step: unaligned mask output, aligned reference
    B, H, W = 2, 120, 160
    cfg, make, batch = soft_problem(xarm7, B, H, W, 0.125)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    fb.mask = unaligned(fb.mask)
    assert fb.ref.data_ptr() % 16 == 0
    for it in range(2):
        fa.mask.fill_(float("nan"))
        fb.mask.fill_(float("nan"))
        fa.step(want_mask=True)
        fb.step(want_mask=True)
        torch.cuda.synchronize()
        assert torch.equal(fa.mask, fb.mask) and float(fa.mask.sum()) > 0
        for name in STATE:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
    fused.check_status(fa.glctx)
    fused.check_status(fb.glctx)


BAD = [float("nan"), float("inf"), 1e20, 4e4]   # 4e4: one tile's sum of squares is 1.6e9, above the per-addend guard of 1e9


@pytest.mark.parametrize("where", ["empty_tile", "covered_tile"])
@pytest.mark.parametrize("bad", BAD, ids=["nan", "inf", "1e20", "4e4"])
def test_non_finite_and_huge_references_are_reported(env, oracle, xarm7, bad, where):
    """One pixel of one view that the accumulators cannot hold, in a corner tile no link touches or in a tile under the
    robot: the guard of fix_add (stateless), vb_refsum_kernel (at bind time) and fix_add_delta (a tile with a job under a
    bound reference) reports the step -- every loss and gradient NaN, raised status; in the solver step pose and optimiser
    untouched -- and the next clean call is right again."""
    fused, _, scene, dev = env
    from easyhec_amd import dr
    from easyhec_amd.fast import FusedPoseStep
    e = R.expected_for(oracle, xarm7, XARM7_KEYS[0], "uniform")
    s = e.s
    ref = torch.tensor(e.ref, device=dev)
    if where == "empty_tile":
        y, x = 3, 5
        assert e.m_ref[1, :8, :32].max() == 0
    else:
        inside = np.argwhere(e.m_ref[1] == 1)
        y, x = (int(v) for v in inside[len(inside) // 2])
    dirty = ref.clone()
    dirty[1, y, x] = bad
    ctx = dr.RasterizeCudaContext()
    tm = torch.tensor(s.mvp, device=dev, requires_grad=True)
    _, loss = fused.render_mask_loss(ctx, scene, tm, dirty)
    loss.sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(tm.grad).all()
    with pytest.raises(RuntimeError, match="overflow"):
        fused.check_status(ctx)
    clean = stateless(fused, ctx, scene, s.mvp, ref, dev)           # (check_status inside: the flag is per call)
    fresh = stateless(fused, dr.RasterizeCudaContext(), scene, s.mvp, ref, dev)
    assert all((x_ == y_).all() for x_, y_ in zip(clean, fresh))
    R.check_against_oracle(*clean, e, "clean call after a reported one")

    def launch(r):
        loss_b, grad_b = torch.zeros((s.B,), device=dev), torch.zeros((s.B, scene.num_links, 4, 4), device=dev)
        fused._launch(ctx, scene, tm.detach(), r, None, loss_b, grad_b)
        torch.cuda.synchronize()
        return loss_b, grad_b

    # bound: the bind-time pass raises its flag (kept beside the cached sums, seen by every launch on this binding)
    fused._ensure_plan(ctx, scene, s.B, s.H, s.W)
    fused.bind_ref(ctx, scene, dirty)
    for _ in range(2):
        loss_b, grad_b = launch(dirty)
        assert torch.isnan(loss_b).all() and torch.isnan(grad_b).all()
        with pytest.raises(RuntimeError, match="overflow"):
            fused.check_status(ctx)
    if where == "covered_tile":
        # fix_add_delta alone: the clean tensor is bound (no flag, clean cached sums), then the pixel is written into it --
        # which a caller must not do, and here is the only way to a bad addend that the bind-time pass has not seen
        work = ref.clone()
        fused.bind_ref(ctx, scene, work)
        loss_b, grad_b = launch(work)
        assert (loss_b.cpu().numpy() == clean[1]).all() and (grad_b.cpu().numpy() == clean[2]).all()
        fused.check_status(ctx)
        work[1, y, x] = bad
        loss_b, grad_b = launch(work)
        assert torch.isnan(loss_b).all() and torch.isnan(grad_b).all()
        with pytest.raises(RuntimeError, match="overflow"):
            fused.check_status(ctx)
    fused.bind_ref(ctx, scene, None)
    # solver step, bound (as constructed) and unbound: reported, nothing moves
    B, H, W = 2, 120, 160
    cfg, make, batch = soft_problem(xarm7, B, H, W, 0.125)
    if where == "covered_tile":
        inside = (batch["mask"][1] > 0.9).nonzero()
        y, x = (int(v) for v in inside[len(inside) // 2])
    batch["mask"][1, y, x] = bad
    for unbind in (False, True):
        model = make()
        fs = FusedPoseStep(model, batch)
        if unbind:
            fused.bind_ref(fs.glctx, fs.scene, None)
        dof0 = model.dof.detach().clone()
        for _ in range(2):
            fs.step()
            torch.cuda.synchronize()
            assert torch.isnan(fs.loss).all() and torch.isnan(fs.loss_b).all() and torch.isnan(fs.grad_mvp).all()
            assert torch.equal(model.dof.detach(), dof0)
            assert float(fs.exp_avg.abs().sum()) == 0 and float(fs.exp_avg_sq.abs().sum()) == 0 and int(fs.step_t.item()) == 0
            with pytest.raises(RuntimeError, match="overflow"):
                fused.check_status(fs.glctx)
