"""GPU parity of the pose search's soft score (ehr_mask_distance and ehr_mask_cost through easyhec_amd.pose_search)
against the numpy reference of soft_search_reference.py and the CPU oracle's masks.  Both ops return integers, so the bar
is exact equality; the soft IoU is one float64 quotient of those integers per (candidate, view) and is held to 1e-12."""
import numpy as np
import pytest
import torch

import soft_search_reference as ssr
from test_gpu_pose_search import near_camera_mvps, oracle_masks, parity_case

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def env(xarm7):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused, pose_search
    dev = torch.device("cuda:0")
    ctx = dr.RasterizeCudaContext()
    scene = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    return pose_search, ctx, scene, dev


def six_valued(rng, fg):
    """float32 image with the foreground `fg`: {0.75, 1} on it, {0, 0.25, 0.5, NaN} off it (0.5 and NaN are background)."""
    on = np.array([0.75, 1.0], np.float32)[rng.integers(0, 2, fg.shape)]
    off = np.array([0.0, 0.25, 0.5, np.nan], np.float32)[rng.integers(0, 4, fg.shape)]
    return np.where(fg, on, off).astype(np.float32)


def distance_bank(oracle, xarm7, H, W, S, rng):
    """The images of one case: S six-valued ones (the ladder's real silhouettes at 120x160, random foreground elsewhere:
    dense, sparse, ...), then all background, all foreground and a single foreground pixel in a corner."""
    if (H, W) == (120, 160):
        sil = ssr.ladder(oracle, xarm7)["masks"][1][:S]
    else:
        sil = np.stack([rng.random((H, W)) < (0.5, 0.03, 0.2)[s % 3] for s in range(S)])
    corner = np.zeros((H, W), np.float32)
    corner[H - 1, 0] = 1.0
    return [six_valued(rng, m) for m in sil] + [np.zeros((H, W), np.float32), np.ones((H, W), np.float32), corner]


@pytest.mark.parametrize("H,W,S,cap", [(1, 1, 1, 1), (5, 7, 2, 1), (5, 7, 2, 3), (9, 33, 3, 5), (40, 70, 3, 16), (40, 70, 3, 300),
                                       (120, 160, 3, 64)])
def test_mask_distance_matches_reference(env, oracle, xarm7, H, W, S, cap):
    """9x33: a ragged tile column and row; 40x70 at cap 300: the cap lies beyond the diagonal, so nothing is capped but
    the empty view; 120x160: real silhouettes.  Every case: six-valued images, then all background (cap^2 everywhere), all
    foreground (0 everywhere) and a single foreground pixel in a corner."""
    ps, ctx, _, dev = env
    bank = distance_bank(oracle, xarm7, H, W, S, np.random.default_rng(H * W + cap))
    while len(bank) % S:
        bank.append(bank[0])
    for i in range(0, len(bank), S):
        ref = np.stack(bank[i:i + S])
        d2 = ps.mask_distance(ctx, torch.tensor(ref, device=dev), cap)
        assert d2.dtype == torch.int32 and d2.is_cuda and d2.shape == (S, H, W)
        want = ssr.edt(ref, cap)
        assert (d2.cpu().numpy() == want).all(), i
        fg = ssr.foreground(ref)
        for s in range(S):
            if not fg[s].any():
                assert (want[s] == cap * cap).all()
            if fg[s].all():
                assert (want[s] == 0).all()


@pytest.mark.parametrize("cap", [3, 40, 300])
def test_mask_distance_across_row_segments(env, cap):
    """8x600: three 256-pixel row segments, the last one ragged; the staged windows overlap at cap 40 and cover the whole
    row at cap 300.  Sparse foreground, so that nearest pixels lie across the seams."""
    ps, ctx, _, dev = env
    rng = np.random.default_rng(cap)
    ref = (rng.random((2, 8, 600)) < 0.004).astype(np.float32)
    ref[1, :, 100:] = 0.0                                   # everything right of column 100 looks left across the seams
    d2 = ps.mask_distance(ctx, torch.tensor(ref, device=dev), cap)
    assert (d2.cpu().numpy() == ssr.edt(ref, cap)).all()


def test_mask_distance_cap_out_of_range_raises(env):
    ps, ctx, _, dev = env
    ref = torch.zeros((1, 5, 7), device=dev)
    for cap in (0, 4097):
        with pytest.raises(RuntimeError, match="cap_px"):
            ps.mask_distance(ctx, ref, cap)
    assert int(ps.mask_distance(ctx, ref, 4096).min()) == 4096 * 4096


_COSTS = {}


def cost_case(oracle, xarm7, H, W, scale, Q, S, C):
    """parity_case's inputs and masks with C cost images: random in +-2^20, INT32_MIN and INT32_MAX planted under covered
    pixels of every (channel, view)."""
    key = (H, W, Q, S, C)
    if key not in _COSTS:
        mvp, masks, ref, _ = parity_case(oracle, xarm7, H, W, scale, Q, S)
        rng = np.random.default_rng(H + 7 * S + C)
        cost = rng.integers(-2 ** 20, 2 ** 20 + 1, (C, S, H, W)).astype(np.int32)
        covered = masks.any(axis=0)
        for c in range(C):
            for s in range(S):
                ys, xs = np.nonzero(covered[s])
                assert len(ys) > 4
                pick = rng.choice(len(ys), 4, replace=False)
                for n, val in zip(pick, (I32_MIN, I32_MAX, I32_MAX, I32_MAX)):
                    cost[c, s, ys[n], xs[n]] = val
        _COSTS[key] = (mvp, masks, ref, cost, ssr.cost_sums(masks, cost))
    return _COSTS[key]


def run_cost(env, mvp, cost, **kw):
    ps, ctx, scene, dev = env
    area, sums = ps.mask_cost(ctx, scene, torch.tensor(mvp, device=dev), torch.tensor(cost, device=dev), **kw)
    assert area.dtype == sums.dtype == torch.int64 and area.is_cuda and sums.is_cuda
    return area.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("C", [1, 2, 4])
@pytest.mark.parametrize("H,W,scale,Q,S", [(120, 160, 0.125, 5, 4), (64, 96, 0.07, 4, 1), (100, 150, 0.12, 14, 10),
                                           (100, 150, 0.12, 4, 17)])
def test_mask_cost_matches_numpy_sums_over_oracle_masks(env, oracle, xarm7, H, W, scale, Q, S, C):
    """The shapes of test_mask_overlap_matches_oracle (ragged tiles, three chunks, two 16-view round trips)."""
    mvp, masks, _, cost, (a_ref, s_ref) = cost_case(oracle, xarm7, H, W, scale, Q, S, C)
    assert s_ref.shape == (Q, S, C) and (np.abs(s_ref) > 2 ** 30).any()
    area, sums = run_cost(env, mvp, cost)
    assert (area == a_ref).all()
    assert (sums == s_ref).all()


def test_mask_cost_three_channels_and_a_single_image(env, oracle, xarm7):
    mvp, masks, _, cost, (a_ref, s_ref) = cost_case(oracle, xarm7, 120, 160, 0.125, 5, 4, 4)
    area, sums = run_cost(env, mvp, cost[:3])
    assert (area == a_ref).all() and (sums == s_ref[..., :3]).all()
    area, sums = run_cost(env, mvp, cost[3])                 # [S,H,W]: one channel
    assert sums.shape == (5, 4, 1) and (area == a_ref).all() and (sums[..., 0] == s_ref[..., 3]).all()


def test_mask_cost_identities_with_mask_overlap(env, oracle, xarm7):
    ps, ctx, scene, dev = env
    mvp, masks, ref, _ = parity_case(oracle, xarm7, 120, 160, 0.125, 5, 4)
    tm, tr = torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev)
    inter, area, _ = ps.mask_overlap(ctx, scene, tm, tr)
    fg = (tr > 0.5).to(torch.int32)
    a, s = ps.mask_cost(ctx, scene, tm, torch.stack([torch.ones_like(fg), fg]))
    assert torch.equal(a, area) and torch.equal(s[..., 0], area) and torch.equal(s[..., 1], inter)
    assert int(inter.sum()) > 0 and not torch.equal(inter, area)


def test_fall_back_near_the_camera_matches_oracle(env, oracle, xarm7, monkeypatch):
    """The chain reports that it cannot decide (an error when it is demanded); the default call redoes everything on the
    exact path, in one pass and in passes of two views, with the oracle's sums."""
    mvp, H, W = near_camera_mvps(xarm7)
    masks = oracle_masks(oracle, xarm7, mvp, H, W)
    Q, S = masks.shape[:2]
    rng = np.random.default_rng(11)
    cost = rng.integers(-2 ** 20, 2 ** 20 + 1, (2, S, H, W)).astype(np.int32)
    for s in range(S):
        ys, xs = np.nonzero(masks[:, s].any(axis=0))
        cost[0, s, ys[0], xs[0]], cost[1, s, ys[-1], xs[-1]] = I32_MIN, I32_MAX
    a_ref, s_ref = ssr.cost_sums(masks, cost)
    assert masks.mean() > 0.2
    for chunk in (0, 2):
        area, sums = run_cost(env, mvp, cost, chunk_views=chunk)
        assert (area == a_ref).all() and (sums == s_ref).all(), chunk
    monkeypatch.setenv("EHR_SCORE_PATH", "chain")
    with pytest.raises(RuntimeError, match="ehr_mask_cost"):
        run_cost(env, mvp, cost)


def test_tile_and_chain_paths_agree(env, oracle, xarm7, monkeypatch):
    mvp, masks, _, cost, want = cost_case(oracle, xarm7, 120, 160, 0.125, 5, 4, 2)
    monkeypatch.setenv("EHR_SCORE_PATH", "chain")      # an error if the chain cannot take the call
    chain = run_cost(env, mvp, cost)
    monkeypatch.setenv("EHR_SCORE_PATH", "tile")
    tile = run_cost(env, mvp, cost, chunk_views=7)      # 20 views in passes of 7, 7 and 6
    for a, b, c in zip(chain, tile, want):
        assert (a == b).all() and (a == c).all()


def test_views_permute_columns_and_candidates_reverse_rows(env, oracle, xarm7):
    ps, ctx, scene, dev = env
    mvp, masks, _, cost, _ = cost_case(oracle, xarm7, 120, 160, 0.125, 5, 4, 2)
    tm, tc = torch.tensor(mvp, device=dev), torch.tensor(cost, device=dev)
    area, sums = ps.mask_cost(ctx, scene, tm, tc)
    perm = torch.tensor([2, 0, 3, 1], device=dev)
    a_p, s_p = ps.mask_cost(ctx, scene, tm[:, perm].contiguous(), tc[:, perm].contiguous())
    assert torch.equal(a_p, area[:, perm]) and torch.equal(s_p, sums[:, perm])
    a_r, s_r = ps.mask_cost(ctx, scene, tm.flip(0).contiguous(), tc, chunk_views=3)
    assert torch.equal(a_r, area.flip(0)) and torch.equal(s_r, sums.flip(0))


def ladder_problem(oracle, xarm7, dev):
    """(model, batch, ladder): the ladder's scene as a solver model and a batch whose masks are rung 0's."""
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    lad = ssr.ladder(oracle, xarm7)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = lad["H"], lad["W"]
    cfg.model.rbsolver.init_Tc_c2b = lad["poses"][0].tolist()
    model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    batch = {"mask": torch.tensor(lad["ref"], device=dev), "link_poses": torch.tensor(lad["link_poses"], device=dev),
             "K": torch.tensor(lad["K"], dtype=torch.float32, device=dev)[None].repeat(3, 1, 1)}
    return model, batch, lad


def reference_of_search(oracle, xarm7, res, batch, H, W, cap, valid=None):
    """The reference's integers and soft IoU for the very matrices the search formed from res.candidates."""
    from easyhec_amd import pose_search
    dev = batch["mask"].device
    mvp = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(res.candidates, dtype=torch.float32, device=dev),
                                     batch["link_poses"])
    masks = oracle_masks(oracle, xarm7, mvp.cpu().numpy(), H, W)
    return masks, ssr.soft_scores(masks, batch["mask"].cpu().numpy(), cap, valid)


@pytest.mark.parametrize("cap", [16, 64, None])
def test_ladder_on_the_device_ranks_by_displacement(env, oracle, xarm7, cap):
    from easyhec_amd import pose_search
    from easyhec_amd.multistart import rank_losses
    dev = env[3]
    model, batch, lad = ladder_problem(oracle, xarm7, dev)
    res = pose_search.search_starts(model, batch, lad["poses"][0], 1, 1, score="soft", cap_px=cap, extra=lad["poses"])
    assert res.score == "soft" and res.soft.dtype == torch.float64 and res.soft.shape == (11,)
    assert np.array_equal(res.candidates[0], lad["poses"][0]) and np.array_equal(res.candidates[1:], lad["poses"])
    _, want = reference_of_search(oracle, xarm7, res, batch, lad["H"], lad["W"], 40 if cap is None else cap)
    for k in ("area", "inter", "ref_area"):
        assert (getattr(res, k).numpy() == want[k]).all(), k
    assert (res.xor.numpy() == want["xor"]).all()
    assert np.abs(res.soft.numpy() - want["soft"]).max() <= 1e-12
    # candidate 0 is rung 0 again; then the rungs in order of displacement (the two that left the image tie at 0: by index)
    assert res.ranking == list(range(11)) and res.ranking == rank_losses(-want["soft"])
    soft = res.soft.numpy()
    assert (np.diff(soft[1:10]) < 0).all() and soft[9] == 0.0 and soft[10] == 0.0
    assert np.array_equal(res.starts, lad["poses"][:1])


def test_planted_ground_truth_is_found_from_a_wide_draw(xarm7):
    from easyhec_amd import pose_search, space_explorer
    from easyhec_amd.synthetic import camera_Tc_c2b
    from test_gpu_fast import problem
    H, W, Bv, Q, P = 120, 160, 3, 24, 4
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    model = make()
    dev = batch["mask"].device
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    wide = dict(trans_sigma_m=0.3, rot_sigma_deg=20, score="soft", extra=Tc_gt[None])
    res = pose_search.search_starts(model, batch, Tc_init, Q, P, seed=2, **wide)
    # the references: the planted pose's own renders, of the very matrices the search forms (batch size included)
    mvp_gt = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(res.candidates, dtype=torch.float32, device=dev),
                                        batch["link_poses"])[Q]
    glctx, scene = model._ensure_renderer().glctx, model._ensure_scene()
    _, _, counts = space_explorer.mask_variance(glctx, scene, mvp_gt[:, None].contiguous(), H, W, return_counts=True)
    planted = dict(batch, mask=counts.float())
    res2 = pose_search.search_starts(model, planted, Tc_init, Q, P, seed=2, **wide)
    assert np.array_equal(res2.candidates, res.candidates) and np.array_equal(res2.candidates[Q], Tc_gt)
    assert res2.ranking[0] == Q and float(res2.soft[Q]) == 1.0 and int(res2.xor[Q]) == 0 and float(res2.iou[Q]) == 1.0
    assert float(res2.soft[:Q].max()) < 1.0 and float(res2.soft.min()) >= 0.0
    assert np.array_equal(res2.starts[0], Tc_init) and np.array_equal(res2.starts[1], Tc_gt)
    assert res2.starts.shape == (P, 4, 4)


def test_weights_restrict_every_sum_to_the_valid_pixels(env, oracle, xarm7):
    from easyhec_amd import pose_search
    ps, ctx, scene, dev = env
    model, batch, lad = ladder_problem(oracle, xarm7, dev)
    H, W, cap = lad["H"], lad["W"], 16
    fg = lad["ref"] > 0.5
    ys, xs = np.nonzero(fg[0])
    y0, y1, x0, x1 = int(ys.min()), int((ys.min() + ys.max()) // 2), int(xs.min()), int(xs.max()) + 1
    weight = np.ones((3, H, W), np.float32)
    weight[:, y0:y1, x0:x1] = 0.0                     # the upper half of view 0's silhouette, the same rectangle in every view
    weight[2, :5] = -1.0                              # a negative weight is not valid either
    valid = weight > 0
    assert (fg & ~valid).any(axis=(1, 2))[0] and (fg & valid).any(axis=(1, 2)).all()
    wbatch = dict(batch, weight=torch.tensor(weight, device=dev))
    res = pose_search.search_starts(model, wbatch, lad["poses"][0], 1, 1, score="soft", cap_px=cap, extra=lad["poses"][:6])
    masks, want = reference_of_search(oracle, xarm7, res, batch, H, W, cap, valid)
    for k in ("area", "inter", "ref_area"):
        assert (getattr(res, k).numpy() == want[k]).all(), k
    assert np.abs(res.soft.numpy() - want["soft"]).max() <= 1e-12 and (res.xor.numpy() == want["xor"]).all()
    free = ssr.soft_scores(masks, lad["ref"], cap)
    assert (want["inter"] < free["inter"]).any() and (want["area"] < free["area"]).any()
    # the cost images hold nothing inside the rectangle, although the renders cover reference pixels there (k = cap:
    # the dearest pixels there are), and a cost planted there by hand reaches no sum either
    d2 = ps.mask_distance(ctx, batch["mask"], cap)
    tv = torch.tensor(valid, device=dev)
    cost = ps.soft_costs(d2, cap, tv)
    assert int(cost[:, :, y0:y1, x0:x1].abs().sum()) == 0 and (masks[:, 0] & fg[0] & ~valid[0]).any()
    mvp = ps.candidate_mvps(batch["K"][0], H, W, torch.tensor(res.candidates, dtype=torch.float32, device=dev), batch["link_poses"])
    area, sums = ps.mask_cost(ctx, scene, mvp, cost)
    assert (sums[..., 0].cpu().numpy() == want["inter"]).all() and (sums[..., 1].cpu().numpy() == want["ksum"]).all()
    assert (sums[..., 2].cpu().numpy() == want["area"]).all()
    planted = torch.ones((1, 3, H, W), dtype=torch.int32, device=dev)
    planted[0, :, y0 + 1, x0 + 1] = I32_MAX
    _, s_pl = ps.mask_cost(ctx, scene, mvp, planted * tv.to(torch.int32))
    assert (s_pl[..., 0].cpu().numpy() == want["area"]).all()


def test_solve_global_soft_is_never_worse_than_the_plain_solve(xarm7):
    from easyhec_amd import pose_search
    from test_gpu_fast import problem
    from test_gpu_multistart import solo_states
    H, W, Bv, Q, P, n, tail = 120, 160, 4, 64, 4, 30, 10
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    model = make()
    search, res = pose_search.solve_global(cfg, model, batch, Tc_init, Q, P, n, tail=tail, score="soft")
    assert search.score == "soft" and search.soft is not None and search.ranking == sorted(
        range(Q), key=lambda i: (-float(search.soft[i]), i))
    assert np.array_equal(search.starts[0], Tc_init) and search.starts.shape == (P, 4, 4) and res.steps == n
    solo = solo_states(cfg, make, batch, [Tc_init], steps=n, recover=True)[0]
    assert torch.equal(res.dofs[0], solo["dof"].cpu())                       # hypothesis 0 IS the plain solve
    assert res.loss_history[:, 0].tolist() == solo["losses"]
    solo_tail = res.loss_history[-tail:].double().mean(dim=0)[0]
    assert torch.isfinite(res.losses).all() and float(res.losses[res.winner]) <= float(solo_tail)
    assert torch.equal(model.dof.detach().cpu(), res.dofs[res.winner])


def test_search_starts_default_is_unchanged(xarm7):
    """No new argument: every field is what mask_overlap + overlap_scores + rank_losses give directly."""
    from easyhec_amd import pose_search
    from easyhec_amd.multistart import rank_losses, sample_starts
    from test_gpu_fast import problem
    H, W, Bv, Q, P = 120, 160, 3, 24, 4
    cfg, make, batch = problem(xarm7, Bv, H, W, 0.125)
    model = make()
    dev = batch["mask"].device
    Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
    res = pose_search.search_starts(model, batch, Tc_init, Q, P, seed=2)
    cands = sample_starts(Tc_init, Q, 0.03, 4.0, seed=2)
    mvp = pose_search.candidate_mvps(batch["K"][0], H, W, torch.tensor(cands, dtype=torch.float32, device=dev), batch["link_poses"])
    inter, area, ref_area = pose_search.mask_overlap(model._ensure_renderer().glctx, model._ensure_scene(), mvp, batch["mask"])
    xor, iou = pose_search.overlap_scores(inter, area, ref_area)
    ranking = rank_losses(xor.cpu().numpy())
    assert res.score == "xor" and res.soft is None
    assert np.array_equal(res.candidates, cands) and res.ranking == ranking
    assert np.array_equal(res.starts, cands[[0] + [i for i in ranking if i != 0][:P - 1]])
    assert torch.equal(res.xor, xor.cpu()) and torch.equal(res.iou, iou.cpu())
    assert torch.equal(res.inter, inter.cpu()) and torch.equal(res.area, area.cpu()) and torch.equal(res.ref_area, ref_area.cpu())


def test_mask_distance_is_capturable_once_its_scratch_is_reserved(env):
    """The call only launches: after one call of the same size it records into a stream capture, and the replays follow
    the masks' contents."""
    ps, ctx, _, dev = env
    rng = np.random.default_rng(5)
    sparse = (rng.random((2, 40, 70)) < 0.02).astype(np.float32)
    dense = (rng.random((2, 40, 70)) < 0.3).astype(np.float32)
    ref = torch.tensor(sparse, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ps.mask_distance(ctx, ref, 16)                      # warm-up: reserves the scratch
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d2 = ps.mask_distance(ctx, ref, 16)
    for img in (dense, sparse):
        ref.copy_(torch.tensor(img, device=dev))
        g.replay()
        torch.cuda.synchronize()
        assert (d2.cpu().numpy() == ssr.edt(img, 16)).all()
