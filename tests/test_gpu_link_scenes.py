"""The fused mask-loss chain (ehr_render_mask_loss, ehr_solver_step) and the scoring chain on the scenes of
tests/link_scenes.py: 1 .. 32 links, prime link counts, views x links at and above the 512 units one pass plans for, links
of 0, 1 and 63 .. 4161 triangles, the lazy vertex form on a small scene, images smaller than a 32 x 8 tile.  Every
comparison is with the CPU oracle and the float64 block reference at the project's own bars
(tests/fused_loss_reference.py); tests/test_link_scenes.py pins the scenes on the CPU."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import helpers
import link_scenes as S
import pose_reference as P
import weighted_loss_reference as WR
from test_gpu_finisher import STATE, _piecewise_step
from test_gpu_fused_loss import both_forms_against_oracle, link_scene, stateless
from test_gpu_pose_search import expected as overlap_expected
from test_gpu_weighted_loss import call as weighted_call, same

pytestmark = pytest.mark.gpu

_SCENES = {}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused
    return fused, dr, torch.device("cuda:0")


def device_scene(fused, case, dev):
    if case not in _SCENES:
        _SCENES[case] = link_scene(fused, S.scene_of(case), dev)
    return _SCENES[case]


# ---- a. stateless and bound form against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("case,kind", S.RUNS, ids=S.RUN_IDS)
def test_both_forms_match_the_oracle(env, oracle, case, kind):
    """Masks bit-exact, loss 1e-6 per view, gradient 1e-5 globally, row 2 of every block zero, every (view, link) block
    within K_ROUNDINGS * 2^-24 * A, the blocks of empty links (A == 0) exactly zero; the bound form bit-equal to the
    stateless one."""
    fused, _, dev = env
    e = S.expected_of(oracle, case, kind)
    assert (e.c.A[:, S.empty_links(e.s)] == 0).all()
    both_forms_against_oracle(fused, device_scene(fused, case, dev), e, dev, f"link scene {case} {kind}")


# ---- b. chunks are invisible ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,slices", [("units513", [(0, 3), (7, 10), (14, 17)]), ("prime7", [(0, 10), (30, 40), (64, 74)])])
def test_views_in_chunks_equal_single_chunk_calls(env, oracle, case, slices):
    """units513: 17 views x 32 links go through in chunks of 16 + 1 views; prime7: 74 x 7 in chunks of 73 + 1.  Every view of
    the chunked call equals, bit for bit, the same view in a small single-chunk call on a second context -- the last slice
    lies across the chunk border -- stateless and bound; the mask-output form gives the same losses and the oracle's masks."""
    fused, dr, dev = env
    e = S.expected_of(oracle, case)
    s, scene = e.s, device_scene(fused, case, dev)
    B, H, W = s.B, s.H, s.W
    bc = 512 // s.L
    assert bc < B <= 2 * bc and slices[-1][0] < bc < slices[-1][1] and B - bc == 1
    ref, tm = torch.tensor(e.ref, device=dev), torch.tensor(s.mvp, device=dev)

    def call(ctx, lo, hi, bound):
        n = hi - lo
        r, m = ref[lo:hi].contiguous(), tm[lo:hi].contiguous()
        fused._ensure_plan(ctx, scene, n, H, W)
        fused.bind_ref(ctx, scene, r if bound else None)
        loss, grad = torch.empty((n,), device=dev), torch.empty((n, s.L, 4, 4), device=dev)
        fused._launch(ctx, scene, m, r, None, loss, grad)
        torch.cuda.synchronize()
        fused.check_status(ctx)
        return loss, grad

    big, small = dr.RasterizeCudaContext(), dr.RasterizeCudaContext()
    l_all, g_all = call(big, 0, B, False)
    l_bnd, g_bnd = call(big, 0, B, True)
    assert torch.equal(l_all, l_bnd) and torch.equal(g_all, g_bnd)
    for lo, hi in slices:
        for bound in (False, True):
            l_s, g_s = call(small, lo, hi, bound)
            assert torch.equal(l_all[lo:hi], l_s) and torch.equal(g_all[lo:hi], g_s), (lo, hi, bound)
    mask, loss_m = torch.full((B, H, W), float("nan"), device=dev), torch.empty((B,), device=dev)
    fused._ensure_plan(big, scene, B, H, W)
    fused.bind_ref(big, scene, None)
    fused._launch(big, scene, tm, ref, mask, loss_m, None)
    torch.cuda.synchronize()
    fused.check_status(big)
    assert torch.equal(loss_m, l_all)
    assert (mask.cpu().numpy() == e.m_ref).all()


# ---- c. weights --------------------------------------------------------------------------------------------------------------
def test_unit_weights_change_no_bit_at_32_links(env, oracle):
    fused, dr, dev = env
    e = S.expected_of(oracle, "full32")
    scene = device_scene(fused, "full32", dev)
    ref = torch.tensor(e.ref, device=dev)
    ones = torch.ones_like(ref)
    ctx = dr.RasterizeCudaContext()
    base = weighted_call(fused, ctx, scene, e.s.mvp, ref, None, dev)
    R.check_against_oracle(*base, e, "full32 no weights")
    assert same(base, weighted_call(fused, ctx, scene, e.s.mvp, ref, ones, dev))
    assert same(base, weighted_call(fused, ctx, scene, e.s.mvp, ref, ones[:1].contiguous(), dev))
    for want_mask in (False, True):
        assert same(base, weighted_call(fused, ctx, scene, e.s.mvp, ref, ones, dev, bind=True, want_mask=want_mask))
    fused.check_status(ctx)


@pytest.mark.parametrize("pattern", ["speckle", "tiles"])
def test_binary_weights_match_the_oracle_on_the_hidden_reference_at_32_links(env, oracle, pattern):
    """The GPU on (ref, w) against the oracle on ref' = where(w, ref, oracle mask), as tests/test_gpu_weighted_loss.py holds
    the xArm7: a pixel with e == 0 contributes exactly what a pixel with w == 0 does, so every bar applies unchanged."""
    fused, dr, dev = env
    e = S.expected_of(oracle, "full32")
    scene = device_scene(fused, "full32", dev)
    w = WR.binary_weight(pattern, e.m_ref, seed=32)
    assert 0.2 < w.mean() < 0.8
    eh = R.expected(oracle, e.s, WR.hidden_reference(e.ref, w, e.m_ref))
    ref, wt = torch.tensor(e.ref, device=dev), torch.tensor(w, device=dev)
    ctx = dr.RasterizeCudaContext()
    got = weighted_call(fused, ctx, scene, e.s.mvp, ref, wt, dev)
    fused.check_status(ctx)
    what = f"link scene full32 weights {pattern}"
    R.check_against_oracle(*got, eh, what)
    sse = WR.weighted_sse(got[0], e.ref, w)
    assert (np.abs(got[1] - sse) <= 1e-6 * np.abs(sse)).all(), what
    assert same(got, weighted_call(fused, ctx, scene, e.s.mvp, ref, wt, dev, bind=True, want_mask=False))
    fused.check_status(ctx)


# ---- d. lazy against eager -------------------------------------------------------------------------------------------------
def test_lazy_and_eager_form_each_draw_their_oracle_masks(env, oracle):
    """full32 with shared vertices and full32_lazy, the same triangles with three vertices of their own each.  The form a plan
    picks is not observable from Python: what is asserted is the plan's own criterion, V > 1.5 T, on the two scenes -- no
    environment variable is set.  Each scene's masks equal the oracle's for that scene, on one context that plans the lazy
    scene after the eager one and the eager one again.  (The two scenes' masks differ from each other, in the oracle too:
    without shared vertices every interior edge is an open edge to the antialiasing.)"""
    fused, dr, dev = env
    ee, el = S.expected_of(oracle, "full32"), S.expected_of(oracle, "full32_lazy")
    for e, lazy in ((ee, False), (el, True)):
        V, T = e.s.arrays[0].shape[0], e.s.arrays[1].shape[0]
        assert (V > 1.5 * T) == lazy
    assert (ee.m_ref != el.m_ref).any()
    ctx = dr.RasterizeCudaContext()
    first = None
    for case, e in (("full32", ee), ("full32_lazy", el), ("full32", ee)):
        got = stateless(fused, ctx, device_scene(fused, case, dev), e.s.mvp, e.ref, dev)
        R.check_against_oracle(*got, e, f"link scene {case} on a context shared by both forms")
        if case == "full32":
            assert first is None or all((x == y).all() for x, y in zip(first, got))
            first = got


# ---- e. the launch chain -----------------------------------------------------------------------------------------------------
def chain_problem(oracle, case, dev):
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import perturb_pose
    e = S.expected_of(oracle, case)
    s = e.s
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = s.H, s.W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(np.eye(4)).tolist()   # (off the identity: the exponential's clamp is not the subject)
    batch = {"mask": torch.tensor(e.ref, device=dev), "link_poses": torch.tensor(s.link_poses.astype(np.float32), device=dev),
             "K": torch.tensor(s.K.astype(np.float32), device=dev)[None].repeat(s.B, 1, 1)}
    return e, (lambda: RBSolver(cfg, meshes=s.meshes).to(dev)), batch


def _rel(x, x64, s):
    return float(P.rel_err(x, x64, s))


@pytest.mark.parametrize("case", ["full32", "L13"])
def test_solver_step_at_many_links(env, oracle, case):
    """FusedPoseStep on a soft reference at 32 links x 2 views and 13 links x 3 views: four steps bit-equal to the piecewise
    step around the stateless op.  A first step that the slot-limited default plan reports (NaN, nothing moves) is recovered
    from on both solvers before the four.  At the first of the four: the mvp the head wrote against pose_reference in
    float64 at the pose-head test's bar (4 e32 + 8 u), loss_b and grad_mvp against the oracle and the block reference on that
    mvp, and the pose backward's sums over all B x L blocks against pose_reference.backward of that grad_mvp at the same bar."""
    fused, _, dev = env
    from easyhec_amd.fast import FusedPoseStep
    e, make, batch = chain_problem(oracle, case, dev)
    s = e.s
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch), FusedPoseStep(mb, batch)
    assert fa.B * fa.L == s.B * s.L and fa.scene.num_links == s.L
    for _ in range(3):     # a reported step changes nothing but the plan; both solvers see the same thing
        fa.step()
        fb.step()
        torch.cuda.synchronize()
        if not bool(torch.isnan(fa.loss).any()):
            break
        what = fa.recover_from_overflow(), fb.recover_from_overflow()
        print(f"[link scene] {case}: first step reported, recovered by {what}")
        assert what[0] and what[0] == what[1]
    assert int(fa.step_t.item()) == 1 and int(fb.step_t.item()) == 1 and torch.equal(ma.dof.data, mb.dof.data)
    fused.bind_ref(fb.glctx, fb.scene, None)
    ref = batch["mask"].cpu().numpy()
    for it in range(4):
        dof0 = ma.dof.detach().cpu().numpy().copy()
        fa.step()
        _piecewise_step(fb, mb)
        torch.cuda.synchronize()
        for name in STATE + ["hist_row"]:
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data)
        assert bool(torch.isfinite(fa.loss).all())
        if it == 0:
            assert P.clamp_margin(dof0) >= 0.01
            K, lp = fa.K.cpu().numpy(), fa.link_poses.cpu().numpy()
            near, far = P.f32(fa.near), P.f32(fa.far)
            mvp = fa.mvp.cpu().numpy()
            M64 = P.mvp(P.exp_and_jac(dof0)[0], K, s.H, s.W, near, far, lp)
            M32 = P.mvp(P.exp_and_jac(dof0, dtype=torch.float32)[0], K, s.H, s.W, near, far, lp, dtype=torch.float32)
            scale = float(np.abs(M64).max())
            e32, ehip = _rel(M32, M64, scale), _rel(mvp, M64, scale)
            print(f"[link scene] {case} mvp: e32 {e32:.3e} hip {ehip:.3e} bound {P.bound(e32):.3e}")
            assert ehip <= P.bound(e32)
            verts, tris, toff, voff = s.arrays
            m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
            loss, grad = fa.loss_b.cpu().numpy(), fa.grad_mvp.cpu().numpy()
            sse = ((m_ref.astype(np.float64) - ref) ** 2).sum(axis=(1, 2))
            assert (np.abs(loss - sse) <= 1e-6 * sse).all()
            assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
            assert (grad[:, :, 2, :] == 0).all() and (grad[:, S.empty_links(s)] == 0).all()
            R.check_blocks(grad, R.block_reference(oracle, s.meshes, mvp, ref), f"solver step link scene {case}")
            red = fa.red.cpu().numpy()
            jac = fa.tc_jac.cpu().numpy().reshape(7, 4, 4)[1:]
            args = (grad, loss, K, s.H, s.W, near, far, lp, jac)
            r64, sc = P.backward(*args)
            r32, _ = P.backward(*args, dtype=torch.float32)
            assert red[7] == s.B and np.isfinite(red).all()
            for name, sl in (("red[0:6]", slice(0, 6)), ("red[6]", slice(6, 7))):
                e32, ehip = _rel(r32[sl], r64[sl], sc[sl]), _rel(red[sl], r64[sl], sc[sl])
                print(f"[link scene] {case} {name}: e32 {e32:.3e} hip {ehip:.3e} bound {P.bound(e32):.3e}")
                assert ehip <= P.bound(e32), name
    assert int(fa.step_t.item()) == 5
    fused.check_status(fa.glctx)


# ---- f. the scoring chain ------------------------------------------------------------------------------------------------------
def score_inputs(s, S_poses):
    from easyhec_amd.synthetic import perturb_pose
    rng = np.random.default_rng(320)
    cams = [perturb_pose(np.eye(4), dt=rng.normal(0, 0.02, 3), drot_deg=rng.normal(0, 2.0, 3)) for _ in range(S_poses)]
    mvp = np.ascontiguousarray(np.stack([helpers.mvp_numpy(s.K, s.H, s.W, Tc, s.link_poses) for Tc in cams], axis=1))
    vl = np.concatenate([np.full(v.shape[0], l, np.int32) for l, (v, _) in enumerate(s.meshes)])
    return mvp, vl


@pytest.mark.parametrize("path", ["chain", None], ids=["chain", "default"])
def test_mask_variance_and_overlap_at_32_links(env, oracle, monkeypatch, path):
    """ehr_mask_variance on full32 (vert_link of the scene, three empty links among the 32), two candidates x three perturbed
    cameras: counts and scores equal the oracle's bit for bit; ehr_mask_overlap on the same matrices equals the popcounts
    of the oracle's masks.  path "chain": an error if the coverage chain cannot take the call."""
    fused, dr, dev = env
    from easyhec_amd import pose_search, space_explorer
    if path:
        monkeypatch.setenv("EHR_SCORE_PATH", path)
    else:
        monkeypatch.delenv("EHR_SCORE_PATH", raising=False)
    s = S.scene_of("full32")
    scene = device_scene(fused, "full32", dev)
    mvp, vl = score_inputs(s, 3)
    Q, Sp = mvp.shape[:2]
    verts, tris, _, _ = s.arrays
    assert (vl == scene.vert_link.cpu().numpy()).all()
    s_ref, c_ref = oracle.mask_variance(verts, tris, vl, mvp, s.H, s.W, return_counts=True)
    assert s_ref.min() > 0 and c_ref.max() == Sp
    ctx = dr.RasterizeCudaContext()
    _, score, counts = space_explorer.mask_variance(ctx, scene, torch.tensor(mvp, device=dev), s.H, s.W, return_counts=True)
    assert (counts.cpu().numpy() == c_ref).all() and (score.cpu().numpy() == s_ref).all()
    _, c1 = oracle.mask_variance(verts, tris, vl, np.ascontiguousarray(mvp.reshape(Q * Sp, 1, s.L, 4, 4)), s.H, s.W,
                                 return_counts=True)
    masks = c1.reshape(Q, Sp, s.H, s.W) > 0
    ref = np.random.default_rng(321).uniform(size=(Sp, s.H, s.W)).astype(np.float32)
    i_ref, a_ref, r_ref = overlap_expected(masks, ref)
    assert i_ref.min() > 0 and (i_ref < a_ref).all()
    inter, area, ref_area = pose_search.mask_overlap(ctx, scene, torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev))
    assert (ref_area.cpu().numpy() == r_ref).all() and (area.cpu().numpy() == a_ref).all() and (inter.cpu().numpy() == i_ref).all()


# ---- g. refusals that must stay refusals ------------------------------------------------------------------------------------
def tiny_scene(L):
    return S.scene([2] * L, 40, 56, 1, seed=33, cols=7, pitch=0.15, size=0.2, f=45.0, name=f"tiny{L}")


def test_refusals_leave_the_context_usable(env, oracle, monkeypatch):
    """33 links and an unsorted tri_link are refused by the plan, 33 links and 16 x 33 units by the scoring chain: argument
    checks on the host that return an error with its message before anything is launched.  After each, the good call that
    went before gives the same bits on the same context."""
    fused, dr, dev = env
    from easyhec_amd import space_explorer
    e = S.expected_of(oracle, "first_empty")
    good = device_scene(fused, "first_empty", dev)
    ctx = dr.RasterizeCudaContext()
    base = stateless(fused, ctx, good, e.s.mvp, e.ref, dev)
    R.check_against_oracle(*base, e, "before the refusals")

    def still_good():
        fused.check_status(ctx)
        got = stateless(fused, ctx, good, e.s.mvp, e.ref, dev)
        assert all((x == y).all() for x, y in zip(base, got))

    s33 = tiny_scene(33)
    sc33 = link_scene(fused, s33, dev)
    ref33 = torch.zeros((1, s33.H, s33.W), device=dev)
    with pytest.raises(RuntimeError, match=r"ehr_fused_plan: bad sizes \(1 <= L <= 32\)"):
        fused.render_mask_loss(ctx, sc33, torch.tensor(s33.mvp, device=dev), ref33)
    still_good()
    s2 = tiny_scene(2)
    sc2 = link_scene(fused, s2, dev)
    sc2.tri_link = sc2.tri_link.flip(0).contiguous()
    assert sc2.tri_link.tolist() == [1, 1, 0, 0]
    with pytest.raises(RuntimeError, match="ehr_fused_plan: tri_link must be sorted by link"):
        fused.render_mask_loss(ctx, sc2, torch.tensor(s2.mvp, device=dev), torch.zeros((1, s2.H, s2.W), device=dev))
    still_good()
    # the scoring chain: asked for by name, it must say that it cannot take the call
    monkeypatch.setenv("EHR_SCORE_PATH", "chain")
    for S_poses in (1, 16):
        mvp = torch.tensor(np.repeat(s33.mvp[:, None], S_poses, axis=1), device=dev)
        with pytest.raises(RuntimeError, match="ehr_mask_variance: EHR_SCORE_PATH=chain, but the call's sizes do not allow it"):
            space_explorer.mask_variance(ctx, sc33, mvp, s33.H, s33.W, return_counts=True)
    monkeypatch.delenv("EHR_SCORE_PATH")
    still_good()
