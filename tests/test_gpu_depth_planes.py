"""The fused chain and the scoring chains at the depth planes and at the 512-pixel bar (scenes: tests/depth_plane_scenes.py,
pinned on the CPU by tests/test_depth_plane_scenes.py) against the CPU oracle.  What is under test is the contract of
``vb_depth_safe`` in csrc/ehr_vbuf.hip -- "safe" is never said wrongly, so classifying a triangle draws the same pixels as
testing every pixel -- and the paths only unsafe (flagged) units take: partial flushes of a full deferred list, flagged
boxes under the interior skip and the span walker, the heavy-job hint on a tile of flagged units, and the hand-over from the
32-bit records to the general-triangle pass at VB_FAST_EXTENT.  The bars are the suite's: masks bit-exact, loss 1e-6,
gradient 1e-5 and every (view, link) block to its own bar (tests/fused_loss_reference.py), scoring integers equal."""
import numpy as np
import pytest
import torch

import depth_plane_scenes as D
import fused_loss_reference as R
import helpers
from test_gpu_fused_loss import both_forms_against_oracle, link_scene, stateless
from test_gpu_pose_search import expected as overlap_expected
from test_gpu_pose_search import oracle_masks
from test_gpu_score import vert_link_of

pytestmark = pytest.mark.gpu

SCENES = ["far_soup", "far_slivers", "far_perspective", "stack_base", "stack_wide", "stack_heavy", "robot_120", "robot_100"]
_CACHE = {}


def scene(xarm7, name):
    if name not in _CACHE:
        if name.startswith("stack_"):
            parts = D.flagged_stack(name[6:])
        elif name.startswith("robot_"):
            H, W, scale = [s for s in D.ROBOT_SHAPES if s[0] == int(name[6:])][0]
            parts = D.robot_cut_by_far(xarm7, H, W, scale)
        elif name.startswith("extent_"):
            _, axis, which = name.split("_")
            parts = D.extent_bar(axis, D.EXTENTS if which == "all" else (int(which),))
        else:
            parts = getattr(D, name)()
        _CACHE[name] = R._scene(name, *parts)
    return _CACHE[name]


def expected(oracle, xarm7, name):
    """The oracle's result on the scene with a uniform-random reference (every pixel carries a gradient); computed once."""
    key = (name, "expected")
    if key not in _CACHE:
        s = scene(xarm7, name)
        _CACHE[key] = R.expected(oracle, s, R.reference_mask(oracle, s, "uniform"))
    return _CACHE[key]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import fused
    return fused, torch.device("cuda:0")


@pytest.mark.parametrize("name", SCENES)
def test_depth_plane_scenes_match_the_oracle(env, oracle, xarm7, name):
    """Stateless and with a bound reference (bit-identical to each other), each against the oracle."""
    fused, dev = env
    e = expected(oracle, xarm7, name)
    both_forms_against_oracle(fused, link_scene(fused, e.s, dev), e, dev, name)


@pytest.mark.parametrize("name", ["far_soup", "stack_base", "robot_120"])
def test_eager_and_lazy_plans_draw_the_same_pixels(env, oracle, xarm7, monkeypatch, name):
    """EHR_VB_LAZY=0 keeps every clip-space vertex, =1 transforms the vertices of the depth-tested units on demand: the
    per-pixel depth test of the unsafe triangles reads either; same bits, and the oracle's mask."""
    fused, dev = env
    from easyhec_amd import dr
    e = expected(oracle, xarm7, name)
    sc = link_scene(fused, e.s, dev)
    res = []
    for lazy in ("0", "1"):
        monkeypatch.setenv("EHR_VB_LAZY", lazy)          # (read by ehr_fused_plan: a fresh context plans afresh)
        res.append(stateless(fused, dr.RasterizeCudaContext(), sc, e.s.mvp, e.ref, dev))
    monkeypatch.delenv("EHR_VB_LAZY")
    for a, b in zip(*res):
        assert (a == b).all(), name
    assert (res[0][0] == e.m_ref).all(), name


@pytest.mark.parametrize("name", ["stack_heavy", "stack_base"])
def test_flagged_stack_twice_on_one_context(env, oracle, xarm7, name):
    """The first call records the stack's tile as a heavy job (its cost is asserted on the CPU), the second hands it to a
    whole workgroup whose four waves share the flagged units; a third for good measure.  Same bits, the oracle's mask."""
    fused, dev = env
    from easyhec_amd import dr
    e = expected(oracle, xarm7, name)
    sc = link_scene(fused, e.s, dev)
    ctx = dr.RasterizeCudaContext()
    first = stateless(fused, ctx, sc, e.s.mvp, e.ref, dev)
    for _ in range(2):
        again = stateless(fused, ctx, sc, e.s.mvp, e.ref, dev)
        for a, b in zip(first, again):
            assert (a == b).all(), name
    R.check_against_oracle(*first, e, name + " warm hint")


@pytest.mark.parametrize("H,W,scale", D.ROBOT_SHAPES)
def test_robot_cut_by_far_through_one_solver_step(env, oracle, xarm7, H, W, scale):
    """FusedPoseStep (ehr_solver_step: default slack, bound reference) with ``far`` inside the arm: mask, loss_b and grad_mvp
    bit-equal to the stateless call on the matrices the step wrote, the oracle's mask, a clean status -- the chain does
    not launch the general-triangle pass, and unsafe triangles must not ask for it."""
    fused, dev = env
    from easyhec_amd import _lib, dr
    from easyhec_amd.config import Cfg
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.rb_solver import RBSolver
    B, far = 2, D.ROBOT_FAR[H]
    K, lp, _, Tc = D.robot_camera(xarm7, H, W, scale, B)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    ref = np.random.default_rng(H).uniform(size=(B, H, W)).astype(np.float32)
    batch = {"mask": torch.tensor(ref, device=dev), "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(np.asarray(K), dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    fs = FusedPoseStep(model, batch, far=far)
    fs.step(want_mask=True)
    torch.cuda.synchronize()
    assert _lib.lib().ehr_fused_status(fs.glctx.handle) == 0          # neither an overflow nor EHR_ERR_RETRY
    assert int(fs.step_t) == 1 and bool(torch.isfinite(fs.loss_b).all())
    mvp = fs.mvp.cpu().numpy()
    mask, loss, grad = stateless(fused, dr.RasterizeCudaContext(), fs.scene, mvp, ref, dev)
    assert (fs.mask.cpu().numpy() == mask).all() and (fs.loss_b.cpu().numpy() == loss).all()
    assert (fs.grad_mvp.cpu().numpy() == grad).all()
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
    assert (mask == m_ref).all()
    assert (np.abs(loss - l_ref) <= 1e-6 * np.abs(l_ref)).all() and np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    whole = oracle.render_mask_loss(verts, tris, toff, voff, D.robot_cut_by_far(xarm7, H, W, scale, far=10.0)[1], ref,
                                    want_grad=False)[0]
    assert ((m_ref > 0).sum(axis=(1, 2)) < 0.85 * (whole > 0).sum(axis=(1, 2))).all()     # the step's far plane did cut the arm


@pytest.mark.parametrize("which", ["all"] + [str(e) for e in D.EXTENTS])
@pytest.mark.parametrize("axis", ["x", "y"])
def test_extent_bar(env, oracle, xarm7, axis, which):
    """Snapped extents of 8191 and 8192 sixteenth-pixels take the 32-bit records, 8193 the general-triangle pass: together,
    and one at a time so that a failure names its side of the bar."""
    fused, dev = env
    from easyhec_amd import dr
    name = f"extent_{axis}_{which}"
    e = expected(oracle, xarm7, name)
    assert 0.02 < (e.m_ref > 0).mean() < 0.98
    mask, loss, grad = stateless(fused, dr.RasterizeCudaContext(), link_scene(fused, e.s, dev), e.s.mvp, e.ref, dev)
    R.check_against_oracle(mask, loss, grad, e, name)


@pytest.mark.parametrize("H,W,scale", D.ROBOT_SHAPES)
@pytest.mark.parametrize("cut", [True, False], ids=["zero_plane_through_the_robot", "zero_plane_in_front"])
def test_scoring_at_the_zero_plane(oracle, xarm7, monkeypatch, H, W, scale, cut):
    """mask_variance and mask_overlap (mask = z/w of the nearest fragment > 0) with the near plane pushed out.  z/w = 0
    through the robot: coverage cannot decide, the chain says so (an error where it is demanded) and the default call falls
    back.  z/w = 0 in front of the whole robot: its unsafe slivers all pass with a positive depth, and the chain must take
    the call.  The tile path, the default and -- where it runs -- the chain give the oracle's integers."""
    from easyhec_amd import dr, fused, pose_search, space_explorer
    dev = torch.device("cuda:0")
    ctx = dr.RasterizeCudaContext()
    sc = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    mvp = D.robot_scoring(xarm7, H, W, scale, near=None if cut else D.SCORE_NEAR_FRONT)
    Q, S = mvp.shape[:2]
    verts, tris, _, _ = helpers.scene_arrays(xarm7)
    s_ref, c_ref = oracle.mask_variance(verts, tris, vert_link_of(xarm7), mvp, H, W, return_counts=True)
    masks = oracle_masks(oracle, xarm7, mvp, H, W)
    ref = masks[1].astype(np.float32)
    want = overlap_expected(masks, ref)
    assert s_ref.min() > 0 and want[0].min() > 0 and (want[0][0] < want[1][0]).any()
    mvp_t, ref_t = torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev)

    def both_ops():
        _, s, c = space_explorer.mask_variance(ctx, sc, mvp_t, H, W, return_counts=True)
        got = pose_search.mask_overlap(ctx, sc, mvp_t, ref_t)
        return [s.cpu().numpy(), c.cpu().numpy()] + [g.cpu().numpy() for g in got]

    for path in ("tile", None, "chain"):
        if path is None:
            monkeypatch.delenv("EHR_SCORE_PATH")
        else:
            monkeypatch.setenv("EHR_SCORE_PATH", path)
        if path == "chain" and cut:
            with pytest.raises(RuntimeError, match="ehr_mask_variance"):
                space_explorer.mask_variance(ctx, sc, mvp_t, H, W, return_counts=True)
            with pytest.raises(RuntimeError, match="ehr_mask_overlap"):
                pose_search.mask_overlap(ctx, sc, mvp_t, ref_t)
            continue
        got = both_ops()          # (chain, zero plane in front: an error here is the chain falling back)
        for g, w in zip(got, (s_ref, c_ref) + tuple(want)):
            assert (g == w).all(), (path, H, W)
