"""GPU parity of the pose search (ehr_mask_overlap through easyhec_amd.pose_search) against the CPU oracle: the op returns
integers, so the bar is exact equality everywhere.  The oracle side is ``oracle.mask_variance`` on the Q x S matrices
viewed as single-pose candidates: its count images are the binary masks, and the expected integers are numpy popcounts
of those masks against ``ref > 0.5``."""
import numpy as np
import pytest
import torch

import helpers
from test_gpu_score import candidate_mvps, vert_link_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(xarm7):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused, pose_search
    dev = torch.device("cuda:0")
    ctx = dr.RasterizeCudaContext()
    scene = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    return pose_search, ctx, scene, dev


def oracle_masks(oracle, xarm7, mvp, H, W):
    """bool [Q,S,H,W] (row 0 = top): the oracle's non-antialiased masks of mvp [Q,S,L,4,4]."""
    Q, S, L = mvp.shape[:3]
    verts, tris, _, _ = helpers.scene_arrays(xarm7)
    _, c = oracle.mask_variance(verts, tris, vert_link_of(xarm7), np.ascontiguousarray(mvp.reshape(Q * S, 1, L, 4, 4)), H, W,
                                return_counts=True)
    assert c.max() <= 1
    return c.reshape(Q, S, H, W) > 0


def expected(masks, ref):
    """(inter [Q,S], area [Q,S], ref_area [S]) int64 from bool masks [Q,S,H,W] and a float reference [S,H,W]."""
    with np.errstate(invalid="ignore"):
        fg = ref > np.float32(0.5)          # NaN compares false: background
    return (masks & fg[None]).sum(axis=(2, 3)).astype(np.int64), masks.sum(axis=(2, 3)).astype(np.int64), \
        fg.sum(axis=(1, 2)).astype(np.int64)


_CASES = {}


def parity_case(oracle, xarm7, H, W, scale, Q, S):
    """Inputs and the oracle's masks of one shape, computed once: Q candidates plus one more, differently posed, whose
    masks are the reference; where there are views to spare, view 1's reference is all zero and view 2's all ones."""
    key = (H, W, Q, S)
    if key not in _CASES:
        mvp_all = candidate_mvps(xarm7, H, W, scale, Q + 1, S, seed=H + S)
        masks_all = oracle_masks(oracle, xarm7, mvp_all, H, W)
        ref = masks_all[Q].astype(np.float32)
        plain = np.ones(S, bool)                    # views whose reference is an ordinary silhouette
        if S >= 4:
            ref[1], ref[2] = 0.0, 1.0
            plain[[1, 2]] = False
        _CASES[key] = (np.ascontiguousarray(mvp_all[:Q]), masks_all[:Q], ref, plain)
    return _CASES[key]


def run(env, mvp, ref, **kw):
    ps, ctx, scene, dev = env
    inter, area, ref_area = ps.mask_overlap(ctx, scene, torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev), **kw)
    assert inter.dtype == area.dtype == ref_area.dtype == torch.int64 and inter.is_cuda
    return inter.cpu().numpy(), area.cpu().numpy(), ref_area.cpu().numpy()


@pytest.mark.parametrize("H,W,scale,Q,S", [(120, 160, 0.125, 5, 4), (64, 96, 0.07, 4, 1), (100, 150, 0.12, 14, 10),
                                           (100, 150, 0.12, 4, 17)])
def test_mask_overlap_matches_oracle(env, oracle, xarm7, H, W, scale, Q, S):
    """100x150: a ragged right and top tile.  Q=14, S=10 at 8 links: chunks of 6, 6 and 2 candidates; S=17: two 16-view
    round trips of the count kernel, chunks of 3 and 1.  The case is only worth something if every ordinary view of every
    candidate overlaps its reference and some render sticks out of it (the all-zero view has inter = 0 by construction, so
    the first condition is asserted over the ordinary views)."""
    mvp, masks, ref, plain = parity_case(oracle, xarm7, H, W, scale, Q, S)
    i_ref, a_ref, r_ref = expected(masks, ref)
    assert i_ref[:, plain].min() > 0 and (i_ref < a_ref).any()
    if S >= 4:
        assert r_ref[1] == 0 and r_ref[2] == H * W and (i_ref[:, 1] == 0).all() and (i_ref[:, 2] == a_ref[:, 2]).all()
    inter, area, ref_area = run(env, mvp, ref)
    assert (ref_area == r_ref).all()
    assert (area == a_ref).all()
    assert (inter == i_ref).all()


def test_reference_threshold_is_above_one_half_and_nan_is_background(env, oracle, xarm7):
    H, W, Q, S = 120, 160, 5, 4
    mvp, masks, _, _ = parity_case(oracle, xarm7, H, W, 0.125, Q, S)
    rng = np.random.default_rng(7)
    ref = np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], np.float32)[rng.integers(0, 6, (S, H, W))]
    i_ref, a_ref, r_ref = expected(masks, ref)
    assert (r_ref == np.isin(ref, [0.75, 1.0]).sum(axis=(1, 2))).all()          # 0.5 itself and NaN are background
    assert i_ref.min() > 0 and (i_ref < a_ref).all()
    inter, area, ref_area = run(env, mvp, ref)
    assert (ref_area == r_ref).all() and (area == a_ref).all() and (inter == i_ref).all()


def near_camera_mvps(xarm7):
    """The cameras of test_gpu_score.py::test_mask_variance_slow_tiles_match_oracle: a few centimetres from the robot and a
    12x zoom, so triangles cross the near plane or span hundreds of pixels and coverage alone cannot decide."""
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, scaled_K
    H, W, Q = 240, 320, 2
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    Kz = K.copy()
    Kz[:2, :2] *= 12.0
    _, lp = make_views(xarm7, Q, seed=4)
    cams = [(K, camera_Tc_c2b(radius=0.12, lift=0.15)), (Kz, camera_Tc_c2b(radius=0.45, lift=0.2)),
            (K, camera_Tc_c2b(radius=0.9))]
    return np.stack([helpers.mvp_numpy(k, H, W, tc, lp) for k, tc in cams], axis=1), H, W


def test_fall_back_near_the_camera_matches_oracle(env, oracle, xarm7, monkeypatch):
    """The chain reports that it cannot decide (an error when it is demanded); the default call redoes everything on the
    exact path, in one pass and in passes of two views, with the oracle's integers."""
    ps, ctx, scene, dev = env
    mvp, H, W = near_camera_mvps(xarm7)
    masks = oracle_masks(oracle, xarm7, mvp, H, W)
    ref = masks[1].astype(np.float32)               # candidate 1's own masks
    i_ref, a_ref, r_ref = expected(masks, ref)
    assert masks.mean() > 0.2 and (i_ref[1] == a_ref[1]).all() and (a_ref[1] == r_ref).all() and (i_ref[0] < a_ref[0]).any()
    for chunk in (0, 2):
        inter, area, ref_area = run(env, mvp, ref, chunk_views=chunk)
        assert (inter == i_ref).all() and (area == a_ref).all() and (ref_area == r_ref).all(), chunk
    monkeypatch.setenv("EHR_SCORE_PATH", "chain")
    with pytest.raises(RuntimeError, match="ehr_mask_overlap"):
        run(env, mvp, ref)


def test_tile_and_chain_paths_agree(env, oracle, xarm7, monkeypatch):
    mvp, masks, ref, _ = parity_case(oracle, xarm7, 120, 160, 0.125, 5, 4)
    want = expected(masks, ref)
    monkeypatch.setenv("EHR_SCORE_PATH", "chain")      # an error if the chain cannot take the call
    chain = run(env, mvp, ref)
    monkeypatch.setenv("EHR_SCORE_PATH", "tile")
    tile = run(env, mvp, ref, chunk_views=7)            # 20 views in passes of 7, 7 and 6
    for a, b, c in zip(chain, tile, want):
        assert (a == b).all() and (a == c).all()


def test_properties_at_full_size(env, xarm7, monkeypatch):
    """1280x720, 16 candidates x 8 views: size-independent identities, no oracle."""
    ps, ctx, scene, dev = env
    from easyhec_amd import space_explorer
    H, W, Q, S, gen = 720, 1280, 16, 8, 5
    mvp = torch.tensor(candidate_mvps(xarm7, H, W, 1.0, Q, S, seed=5), device=dev)
    # the library's own masks of candidate `gen`, one view each
    _, _, counts = space_explorer.mask_variance(ctx, scene, mvp[gen][:, None].contiguous(), H, W, return_counts=True)
    assert int(counts.max()) == 1
    ref = counts.float()
    inter, area, ref_area = ps.mask_overlap(ctx, scene, mvp, ref)
    xor, iou = ps.overlap_scores(inter, area, ref_area)
    assert float((ref > 0).float().mean()) > 0.02 and int(inter.min()) > 0
    assert torch.equal(inter[gen], area[gen]) and torch.equal(area[gen], ref_area) and int(xor[gen]) == 0
    assert float(iou[gen]) == 1.0
    others = torch.arange(Q, device=dev) != gen
    assert (xor[others] > 0).all() and (inter <= area).all() and (inter <= ref_area[None]).all()
    # permuting the views permutes the columns
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(0)).to(dev)
    i_p, a_p, r_p = ps.mask_overlap(ctx, scene, mvp[:, perm].contiguous(), ref[perm].contiguous())
    assert torch.equal(i_p, inter[:, perm]) and torch.equal(a_p, area[:, perm]) and torch.equal(r_p, ref_area[perm])
    # reversing the candidates reverses the rows; chunk_views changes nothing
    i_r, a_r, r_r = ps.mask_overlap(ctx, scene, mvp.flip(0).contiguous(), ref, chunk_views=3)
    assert torch.equal(i_r, inter.flip(0)) and torch.equal(a_r, area.flip(0)) and torch.equal(r_r, ref_area)
    # ... nor on the exact path, where it sets the passes (128 views in passes of 40, 40, 40 and 8)
    monkeypatch.setenv("EHR_SCORE_PATH", "tile")
    i_t, a_t, r_t = ps.mask_overlap(ctx, scene, mvp, ref, chunk_views=40)
    assert torch.equal(i_t, inter) and torch.equal(a_t, area) and torch.equal(r_t, ref_area)


def test_search_starts_ranks_like_the_oracle_and_finds_a_planted_pose(oracle, xarm7):
    from easyhec_amd import pose_search, space_explorer
    from easyhec_amd.multistart import rank_losses
    from easyhec_amd.synthetic import camera_Tc_c2b
    from test_gpu_fast import problem
    H, W, Bv, Q, P = 120, 160, 3, 24, 4
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    model = make()
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    res = pose_search.search_starts(model, batch, Tc_init, Q, P, seed=2)
    assert res.starts.shape == (P, 4, 4) and res.starts.dtype == np.float64
    assert np.array_equal(res.starts[0], Tc_init) and np.array_equal(res.candidates[0], Tc_init)
    # the same matrices through the oracle
    dev = batch["mask"].device
    mvp = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(res.candidates, dtype=torch.float32, device=dev),
                                     batch["link_poses"])
    masks = oracle_masks(oracle, xarm7, mvp.cpu().numpy(), H, W)
    i_ref, a_ref, r_ref = expected(masks, batch["mask"].cpu().numpy())
    assert (res.inter.numpy() == i_ref).all() and (res.area.numpy() == a_ref).all() and (res.ref_area.numpy() == r_ref).all()
    xor_ref = (a_ref + r_ref[None] - 2 * i_ref).sum(axis=1)
    assert (res.xor.numpy() == xor_ref).all() and len(set(xor_ref.tolist())) > Q // 2
    assert res.ranking == rank_losses(xor_ref) and sorted(res.ranking) == list(range(Q))
    rest = [i for i in res.ranking if i != 0][:P - 1]
    assert np.array_equal(res.starts[1:], res.candidates[rest])
    # a ground-truth pose planted behind the draw, the references its own renders: first, with nothing left over
    Tc_gt = camera_Tc_c2b()
    glctx, scene = model._ensure_renderer().glctx, model._ensure_scene()
    cands = np.concatenate([res.candidates, Tc_gt[None]])    # (the very matrices the search will form, batch size included)
    mvp_gt = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(cands, dtype=torch.float32, device=dev),
                                        batch["link_poses"])[Q]                                # [Bv,L,4,4]
    _, _, counts = space_explorer.mask_variance(glctx, scene, mvp_gt[:, None].contiguous(), H, W, return_counts=True)
    planted = dict(batch, mask=counts.float())
    res2 = pose_search.search_starts(model, planted, Tc_init, Q, P, seed=2, extra=Tc_gt[None])
    assert np.array_equal(res2.candidates, cands)
    assert res2.ranking[0] == Q and int(res2.xor[Q]) == 0 and float(res2.iou[Q]) == 1.0 and int(res2.xor[:Q].min()) > 0
    assert np.array_equal(res2.starts[0], Tc_init) and np.array_equal(res2.starts[1], Tc_gt)


def test_solve_global_is_never_worse_than_the_plain_solve(xarm7):
    from easyhec_amd import pose_search
    from test_gpu_fast import problem
    from test_gpu_multistart import solo_states
    H, W, Bv, Q, P, n, tail = 120, 160, 4, 64, 4, 30, 10
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    model = make()
    search, res = pose_search.solve_global(cfg, model, batch, Tc_init, Q, P, n, tail=tail)
    assert np.array_equal(search.starts[0], Tc_init) and search.starts.shape == (P, 4, 4) and res.steps == n
    solo = solo_states(cfg, make, batch, [Tc_init], steps=n, recover=True)[0]
    assert torch.equal(res.dofs[0], solo["dof"].cpu())                       # hypothesis 0 IS the plain solve
    assert res.loss_history[:, 0].tolist() == solo["losses"]
    solo_tail = res.loss_history[-tail:].double().mean(dim=0)[0]
    assert torch.isfinite(res.losses).all() and float(res.losses[res.winner]) <= float(solo_tail)
    assert torch.equal(model.dof.detach().cpu(), res.dofs[res.winner])
