"""The composite stage's finisher after profiles/atomic_spread.md: it no longer resets the XCDs' arrival counters (only
the vertex kernel does, at the start of every step and chunk), and the four lanes of a quad share out the reads of a
(view, link)'s gradient sums, a column each.  The scenes are the smallest at which that can go wrong: fewer tiles than
arrival counters (most counters expect no arrival), three views of three unequal links on an image that is no multiple of
the tile (view stride, odd link count, no XCD split), 32 links, the multi-start finish, a link whose silhouette crosses
two dozen tiles, and consecutive steps eager and replayed from a graph (the counters must be zero again without the
finisher's reset).  Copies of the gradient sums and several counters per XCD were measured and left out of the code, so
there is no case for the coverage of every copy or for shards.

Every step is held against the CPU oracle and the float64 references at the bars of the fused-chain parity tests
(tests/test_gpu_link_scenes.py::test_solver_step_at_many_links): the mvp the head wrote and the pose backward's sums at
pose_reference's bar, loss per view 1e-6, grad_mvp 1e-5 globally and per block (fused_loss_reference.check_blocks), and
the pose and moments after Adam at pose_reference's bar against adam_step on the step's own sums."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import link_scenes as S
import pose_reference as P

pytestmark = pytest.mark.gpu

SCENES = {
    # 2 x 2 tiles: fewer tiles than arrival counters
    "one_link_64x16": dict(counts=[65], H=16, W=64, B=1, seed=41, cols=1, pitch=0.2, size=0.5, f=60.0),
    # B = 3 (no multiple of the XCDs), L = 3, 40 rows = 5 tiles, 96 columns = 3 tiles
    "three_by_three_96x40": dict(counts=[129, 3, 31], H=40, W=96, B=3, seed=42, cols=3, pitch=0.3, size=0.35, f=60.0),
    # the widest block of accumulators: 32 links of one triangle
    "L32_one_view": dict(counts=[1] * 32, H=72, W=104, B=1, seed=43, cols=8, pitch=0.22, size=0.25, f=55.0),
    # the multi-start step's two real views
    "multi_2view": dict(counts=[65, 3, 129], H=40, W=96, B=2, seed=44, cols=3, pitch=0.3, size=0.35, f=60.0),
    # one link of about 90 x 90 pixels, all four edges inside the image: its silhouette crosses 3 tiles a row, 11 a column
    "edges_128x104": dict(counts=[257], H=104, W=128, B=1, seed=45, cols=1, pitch=0.2, size=0.6, f=150.0),
}
_CACHE = {}


def scene_and_ref(oracle, name):
    """The scene and its seeded soft reference mask, made once and never written to."""
    if name not in _CACHE:
        s = S.scene(name=name, **SCENES[name])
        _CACHE[name] = (s, R.reference_mask(oracle, s, "uniform"))
    return _CACHE[name]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def problem(s, ref, dev):
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import perturb_pose
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = s.H, s.W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(np.eye(4)).tolist()   # (off the identity: the exponential's clamp is not the subject)
    batch = {"mask": torch.tensor(ref, device=dev), "link_poses": torch.tensor(s.link_poses.astype(np.float32), device=dev),
             "K": torch.tensor(s.K.astype(np.float32), device=dev)[None].repeat(s.B, 1, 1)}
    return cfg, (lambda: RBSolver(cfg, meshes=s.meshes).to(dev)), batch


def _np(x):
    return x.detach().cpu().numpy().copy()


def _rel(x, x64, s):
    return float(P.rel_err(x, x64, s))


def check_step(oracle, s, ref, f, before, after, what):
    """One step of one pose against the references.  f: the stepper (K, link_poses, near, far, Adam's constants);
    before = (dof, m, v, t) ahead of the step; after: what the step wrote for this pose -- mvp, loss_b, grad_mvp [B,...], red,
    tc_jac, dof, m, v."""
    dof0, m0, v0, t0 = before
    assert P.clamp_margin(dof0) >= 0.01
    K, lp = _np(f.K), _np(f.link_poses)
    near, far = P.f32(f.near), P.f32(f.far)
    mvp, loss, grad, red = after["mvp"], after["loss_b"], after["grad_mvp"], after["red"]
    # the head's mvp
    M64 = P.mvp(P.exp_and_jac(dof0)[0], K, s.H, s.W, near, far, lp)
    M32 = P.mvp(P.exp_and_jac(dof0, dtype=torch.float32)[0], K, s.H, s.W, near, far, lp, dtype=torch.float32)
    scale = float(np.abs(M64).max())
    e32, ehip = _rel(M32, M64, scale), _rel(mvp, M64, scale)
    print(f"[atomic spread] {what} mvp: e32 {e32:.3e} hip {ehip:.3e} bound {P.bound(e32):.3e}")
    assert ehip <= P.bound(e32), what
    # loss per view and grad_mvp against the oracle and the block reference on that mvp
    verts, tris, toff, voff = s.arrays
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
    sse = ((m_ref.astype(np.float64) - ref) ** 2).sum(axis=(1, 2))
    print(f"[atomic spread] {what} loss: worst {float((np.abs(loss - sse) / sse).max()):.3e} of 1e-6; grad: "
          f"{float(np.abs(grad - g_ref).max() / np.abs(g_ref).max()):.3e} of 1e-5")
    assert np.isfinite(loss).all() and (np.abs(loss - sse) <= 1e-6 * sse).all(), what
    assert np.abs(g_ref).max() > 0 and np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max(), what
    assert (grad[:, :, 2, :] == 0).all(), what
    R.check_blocks(grad, R.block_reference(oracle, s.meshes, mvp, ref), f"atomic spread {what}")
    # the pose backward's sums over all B x L blocks
    jac = after["tc_jac"].reshape(7, 4, 4)[1:]
    args = (grad, loss, K, s.H, s.W, near, far, lp, jac)
    r64, sc = P.backward(*args)
    r32, _ = P.backward(*args, dtype=torch.float32)
    assert red[7] == s.B and np.isfinite(red).all(), what
    for name, sl in (("red[0:6]", slice(0, 6)), ("red[6]", slice(6, 7))):
        e32, ehip = _rel(r32[sl], r64[sl], sc[sl]), _rel(red[sl], r64[sl], sc[sl])
        print(f"[atomic spread] {what} {name}: e32 {e32:.3e} hip {ehip:.3e} bound {P.bound(e32):.3e}")
        assert ehip <= P.bound(e32), (what, name)
    # the pose after Adam, from the step's own sums
    h = tuple(np.float32(x) for x in (f.lr, f.betas[0], f.betas[1], f.eps, f.wd))
    a64 = P.adam_step(dof0, m0, v0, t0, red, *h)
    a32 = P.adam_step(dof0, m0, v0, t0, red, *h, dtype=torch.float32)
    for qi, q in ((0, "dof"), (1, "m"), (2, "v")):
        sc_q = float(np.abs(a64[qi]).max())
        e32, ehip = _rel(a32[qi], a64[qi], sc_q), _rel(after[q], a64[qi], sc_q)
        print(f"[atomic spread] {what} adam {q}: e32 {e32:.3e} hip {ehip:.3e} bound {P.bound(e32):.3e}")
        assert ehip <= P.bound(e32), (what, q)
    assert not np.array_equal(after["dof"], dof0), what


def solo_before(f, model):
    return _np(model.dof.data), _np(f.exp_avg), _np(f.exp_avg_sq), int(f.step_t.item())


def solo_after(f, model):
    torch.cuda.synchronize()
    return dict(mvp=_np(f.mvp), loss_b=_np(f.loss_b), grad_mvp=_np(f.grad_mvp), red=_np(f.red), tc_jac=_np(f.tc_jac),
                dof=_np(model.dof.data), m=_np(f.exp_avg), v=_np(f.exp_avg_sq))


def solo_stepper(oracle, name, dev):
    from easyhec_amd.fast import FusedPoseStep
    s, ref = scene_and_ref(oracle, name)
    _, make, batch = problem(s, ref, dev)
    model = make()
    f = FusedPoseStep(model, batch, slack=0.0)   # (a job slot for every (link, tile): no step is reported)
    assert f.B == s.B and f.L == len(s.counts)
    return s, ref, f, model


@pytest.mark.parametrize("name", ["one_link_64x16", "three_by_three_96x40", "L32_one_view"])
def test_first_step_matches_the_references(dev, oracle, name):
    from easyhec_amd import fused
    s, ref, f, model = solo_stepper(oracle, name, dev)
    if name == "one_link_64x16":
        assert S.n_tiles(s) == 4
    before = solo_before(f, model)
    f.step()
    check_step(oracle, s, ref, f, before, solo_after(f, model), name)
    fused.check_status(f.glctx)


def test_many_tiles_add_to_one_link(dev, oracle):
    """edges_128x104: the tiles in which the link has antialiased pixels -- blended pairs, hence a 12-lane add to the link's
    sums -- number at least two dozen and lie in every tile row but the first, so the sums of one (view, link) come from
    many workgroups of several XCDs and the finish must not start before the last of them has arrived."""
    from easyhec_amd import fused
    s, ref, f, model = solo_stepper(oracle, "edges_128x104", dev)
    before = solo_before(f, model)
    f.step()
    after = solo_after(f, model)
    verts, tris, toff, voff = s.arrays
    m = oracle.render_mask_loss(verts, tris, toff, voff, after["mvp"], ref, want_grad=False)[0][0]
    soft = (m > 0) & (m < 1)
    ty, tx = np.nonzero(soft.reshape(s.H // 8, 8, s.W // 32, 32).any(axis=(1, 3)))
    assert len(tx) >= 24 and len(set(ty.tolist())) >= s.H // 8 - 1, sorted(zip(tx.tolist(), ty.tolist()))
    check_step(oracle, s, ref, f, before, after, "edges_128x104")
    fused.check_status(f.glctx)


def test_multi_start_step_matches_the_references(dev, oracle):
    """P = 2 hypotheses x 2 views through vb_finish_multi_kernel: every hypothesis is held to the references like a solo
    step on its own pose."""
    from easyhec_amd import fused
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    s, ref = scene_and_ref(oracle, "multi_2view")
    cfg, make, batch = problem(s, ref, dev)
    starts = sample_starts(np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64), 2, 0.01, 1.5, seed=3)
    ms = MultiStartPoseStep(make(), batch, starts, slack=0.0)
    assert ms.P == 2 and ms.Bv == 2 and ms.L == 3
    dof0 = _np(ms.dof)
    assert not np.array_equal(dof0[0], dof0[1])
    ms.step()
    torch.cuda.synchronize()
    for p in range(2):
        v = slice(p * ms.Bv, (p + 1) * ms.Bv)
        after = dict(mvp=_np(ms.mvp[v]), loss_b=_np(ms.loss_b[v]), grad_mvp=_np(ms.grad_mvp[v]), red=_np(ms.red[p]),
                     tc_jac=_np(ms.tc_jac[p]), dof=_np(ms.dof[p]), m=_np(ms.exp_avg[p]), v=_np(ms.exp_avg_sq[p]))
        check_step(oracle, s, ref, ms, (dof0[p], np.zeros(6, np.float32), np.zeros(6, np.float32), 0), after, f"multi_2view p{p}")
    assert ms.step_t.tolist() == [1, 1]
    fused.check_status(ms.glctx)


def test_two_steps_eager_and_replayed(dev, oracle):
    """The arrival counters are zero again when the second step's composite stage starts, although the finisher does not
    reset them: both eager steps match the references, and two replays of the captured step give the eager steps' bits."""
    from easyhec_amd import fused
    from easyhec_amd.fast import FusedPoseStep
    s, ref, fa, ma = solo_stepper(oracle, "three_by_three_96x40", dev)
    _, make, batch = problem(s, ref, dev)
    mb = make()
    fb = FusedPoseStep(mb, batch, slack=0.0)
    fb.capture()
    for it in range(2):
        before = solo_before(fa, ma)
        fa.step()
        fb.step()
        after = solo_after(fa, ma)
        check_step(oracle, s, ref, fa, before, after, f"three_by_three_96x40 step {it}")
        for name in ("mvp", "tc_jac", "loss_b", "grad_mvp", "red", "loss", "grad", "exp_avg", "exp_avg_sq", "step_t"):
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data), it
    assert int(fa.step_t.item()) == 2 and int(fb.step_t.item()) == 2
    fused.check_status(fa.glctx)
    fused.check_status(fb.glctx)
    fb.release_graph()
