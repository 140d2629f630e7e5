"""GPU parity of the fused mask-loss path (ehr_render_mask_loss through the C ABI) against the CPU oracle, the
committed fixtures, the three-op composition, and size-independent properties at BASELINE's full sizes."""
import os

import numpy as np
import pytest
import torch

import fused_loss_reference
import helpers

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def env(xarm7):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused
    dev = torch.device("cuda:0")
    ctx = dr.RasterizeCudaContext()
    scene = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    return fused, ctx, scene, dev


def run(fused, ctx, scene, mvp, ref, dev):
    tm = torch.tensor(mvp, device=dev, requires_grad=True)
    tr = torch.tensor(ref, device=dev)
    mask, loss = fused.render_mask_loss(ctx, scene, tm, tr)
    loss.sum().backward()
    torch.cuda.synchronize()
    fused.check_status(ctx)
    return mask.cpu().numpy(), loss.detach().cpu().numpy(), tm.grad.cpu().numpy()


def workload(xarm7, H, W, scale, B, seed, perturb=True):
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    K = scaled_K(XARM7_K_1280x720, scale, W, H, scale != 1.0)
    _, lp = make_views(xarm7, B, seed=seed)
    Tc = camera_Tc_c2b()
    return K, lp, Tc, helpers.mvp_numpy(K, H, W, perturb_pose(Tc) if perturb else Tc, lp)


@pytest.mark.parametrize("H,W,scale,B", [(120, 160, 0.125, 2), (480, 640, 0.5, 1), (720, 1280, 1.0, 8),
                                         (100, 150, 0.12, 3)])
def test_fused_matches_oracle(env, oracle, xarm7, H, W, scale, B):
    fused, ctx, scene, dev = env
    K, lp, Tc, mvp = workload(xarm7, H, W, scale, B, seed=H)
    rng = np.random.default_rng(H)
    ref = (rng.uniform(size=(B, H, W)) > 0.85).astype(np.float32)
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
    mask, loss, grad = run(fused, ctx, scene, mvp, ref, dev)
    assert (mask == m_ref).all()                                   # rendered masks: bit-exact (<= 1e-4 L-inf bar)
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max()  # float vs double accumulation
    assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    assert (grad[:, :, 2, :] == 0).all()
    if H < 720:   # every (view, link) block against its own bar (the 720p case: oracle time for no new coverage)
        blocks = fused_loss_reference.block_reference(oracle, xarm7.meshes, mvp, ref)
        fused_loss_reference.check_blocks(grad, blocks, f"test_fused_matches_oracle {H}x{W}")


def test_fused_slow_tiles_match_oracle(env, oracle, xarm7):
    """Camera almost inside the robot: triangles cross the near plane and span hundreds of pixels, so their tiles take
    the 64-bit / clipping instantiation of the tile kernel.  Same bit-exact bar."""
    fused, ctx, scene, dev = env
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, scaled_K
    H, W, B = 240, 320, 2
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    _, lp = make_views(xarm7, B, seed=4)
    Tc = camera_Tc_c2b(radius=0.12, lift=0.15)          # eye a few centimetres from link geometry
    Tc2 = camera_Tc_c2b(radius=0.45, lift=0.2)
    Kz = K.copy()
    Kz[:2, :2] *= 12.0                                  # and a 12x zoom: triangles of several hundred pixels
    mvp = np.concatenate([helpers.mvp_numpy(K, H, W, Tc, lp[:1]), helpers.mvp_numpy(Kz, H, W, Tc2, lp[1:])])
    rng = np.random.default_rng(3)
    ref = (rng.uniform(size=(B, H, W)) > 0.5).astype(np.float32)
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp, ref)
    assert (m_ref > 0).mean() > 0.2
    mask, loss, grad = run(fused, ctx, scene, mvp, ref, dev)
    assert (mask == m_ref).all()
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max()
    assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()


def test_span_walker_on_slivers_and_axis_aligned_edges(env, oracle):
    """Synthetic long thin triangles (boxes of 4+ units per row: the job kernel's span walker, which solves every row's
    covered span from the edge functions) at random slopes and sub-pixel offsets, plus exactly horizontal / vertical /
    45-degree edges through pixel centres (zero edge steps, quotients that are exact integers: the tie cases of the
    solver's integer correction) and tiny triangles the vertex kernel's exact small-box test has to judge -- masks,
    losses and gradients against the oracle, bit-exact on the masks."""
    fused, ctx, _, dev = env
    H, W = 96, 160
    rng = np.random.default_rng(12)
    verts, tris = [], []

    def add(a, b, c):
        i = len(verts)
        verts.extend([a, b, c])
        tris.append([i, i + 1, i + 2])

    def px(x, y, z=0.0):   # pixel coordinates (centre of pixel (ix, iy) = (ix + 0.5, iy + 0.5)) -> object space of an identity MVP
        return [2.0 * x / W - 1.0, 2.0 * y / H - 1.0, z]

    for _ in range(160):   # slivers: two far-apart points and a third one 0.2-2 pixels off the line, random winding
        p = rng.uniform([5, 5], [W - 5, H - 5])
        ang = rng.uniform(0, 2 * np.pi)
        ln = rng.uniform(20, 90)
        q = np.clip(p + ln * np.array([np.cos(ang), np.sin(ang)]), 2, [W - 2, H - 2])
        m = 0.5 * (p + q) + rng.uniform(0.2, 2.0) * np.array([-np.sin(ang), np.cos(ang)])
        z = rng.uniform(-0.5, 0.5)
        pts = [px(*p, z), px(*q, z), px(*m, z)]
        if rng.uniform() < 0.5:
            pts = pts[::-1]
        add(*pts)
    for k in range(12):    # axis-aligned and diagonal edges exactly through pixel centres, widths of 4+ units
        y0 = 6.5 + 7 * k
        add(px(10.5, y0), px(70.5, y0), px(40.5, y0 + 3.0))          # horizontal edge on a row of centres
        add(px(90.5 + k, 4.5), px(90.5 + k, 60.5), px(93.5 + k, 30.5))  # vertical edge on a column of centres
        add(px(100.5, 10.5 + k), px(150.5, 60.5 + k), px(150.5, 10.5 + k))  # 45 degrees through centres
    for _ in range(300):   # tiny triangles around pixel centres and between them
        c = rng.uniform([3, 3], [W - 3, H - 3])
        d = rng.uniform(-1.2, 1.2, (3, 2))
        add(*[px(c[0] + d[i, 0], c[1] + d[i, 1]) for i in range(3)])
    v = np.asarray(verts, np.float32)
    f = np.asarray(tris, np.int32)
    scene = fused.LinkScene([v], [f], dev)
    mvp = np.eye(4, dtype=np.float32)[None, None].repeat(2, axis=0)
    mvp[1, 0, 0, 3] = 0.37 / W                     # second view: everything shifted by a fraction of a pixel
    mvp[1, 0, 1, 3] = -0.61 / H
    ref = (rng.uniform(size=(2, H, W)) > 0.5).astype(np.float32)
    toff, voff = np.array([0, f.shape[0]], np.int32), np.array([0, v.shape[0]], np.int32)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(v, f, toff, voff, mvp, ref)
    assert 0.05 < (m_ref > 0).mean() < 0.9
    mask, loss, grad = run(fused, ctx, scene, mvp, ref, dev)
    assert (mask == m_ref).all()
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max()
    assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    fused_loss_reference.check_blocks(grad, fused_loss_reference.block_reference(oracle, [(v, f)], mvp, ref), "span walker")


def test_fused_golden_fixtures(env, xarm7):
    fused, ctx, scene, dev = env
    g = np.load(os.path.join(GOLD, "fused_xarm7_160x120.npz"))
    H, W = int(g["H"]), int(g["W"])
    ref = np.unpackbits(g["ref"])[:2 * H * W].reshape(2, H, W).astype(np.float32)
    mask, loss, grad = run(fused, ctx, scene, g["mvp"], ref, dev)
    assert (mask == g["mask"]).all()
    assert np.allclose(loss, g["loss"], rtol=1e-6)
    assert np.abs(grad - g["grad_mvp"]).max() <= 1e-5 * np.abs(g["grad_mvp"]).max()
    # BASELINE configs[0] on the GPU: zero-pose PLY as a single link
    z = np.load(os.path.join(GOLD, "xarm7_zeropos.npz"))
    c1 = np.load(os.path.join(GOLD, "config1_zeropos_320x240.npz"))
    sc1 = fused.LinkScene([z["vertices"]], [z["faces"]], dev)
    mask, loss, grad = run(fused, ctx, sc1, c1["mvp"], np.zeros((1, 240, 320), np.float32), dev)
    assert (mask == c1["mask"]).all() and np.allclose(loss, c1["loss"], rtol=1e-6)
    assert np.abs(grad - c1["grad_mvp"]).max() <= 1e-5 * np.abs(c1["grad_mvp"]).max()


def test_fused_is_bit_reproducible_and_forward_only_agrees(env, xarm7):
    fused, ctx, scene, dev = env
    H, W, B = 720, 1280, 8
    K, lp, Tc, mvp = workload(xarm7, H, W, 1.0, B, seed=0)
    ref = np.zeros((B, H, W), np.float32)
    a = run(fused, ctx, scene, mvp, ref, dev)
    b = run(fused, ctx, scene, mvp, ref, dev)
    assert all((x == y).all() for x, y in zip(a, b))   # no float atomics anywhere on the fused path
    with torch.no_grad():
        m2, l2 = fused.render_mask_loss(ctx, scene, torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev))
    assert (m2.cpu().numpy() == a[0]).all() and (l2.cpu().numpy() == a[1]).all()


def test_fused_equals_three_op_composition(env, xarm7):
    """RBSolver(use_fused=True) vs RBSolver(use_fused=False): the reference's own per-(frame, link) op sequence."""
    fused, ctx, scene, dev = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import perturb_pose
    H, W, B = 240, 320, 2
    K, lp, Tc, _ = workload(xarm7, H, W, 0.25, B, seed=5)
    rng = np.random.default_rng(1)
    ref = torch.tensor((rng.uniform(size=(B, H, W)) > 0.9).astype(np.float32), device=dev)
    batch = {"mask": ref, "link_poses": torch.tensor(lp, device=dev),
             "K": torch.tensor(K, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1),
             "Tc_c2b": torch.tensor(Tc, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    res = []
    for use_fused in (True, False):
        cfg = Cfg()
        cfg.model.rbsolver.H, cfg.model.rbsolver.W, cfg.model.rbsolver.use_fused = H, W, use_fused
        cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
        model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
        out, ld = model(batch)
        ld["mask_loss"].backward()
        res.append((out["rendered_masks"].detach().cpu().numpy(), float(ld["mask_loss"].detach()),
                    model.dof.grad.cpu().numpy(), out))
    (m0, l0, g0, o0), (m1, l1, g1, _) = res
    # the three-op path forms clip positions with torch.matmul (nvdiffrast_utils.py:18), the fused kernel with an fma
    # chain: positions differ by ~1 ulp, i.e. ~1e-5 pixel, which moves antialias blends by ~1e-5 (north_star bar: 1e-4)
    assert np.abs(m0 - m1).max() <= 1e-4
    assert abs(l0 - l1) <= 1e-4 * abs(l1)
    assert np.abs(g0 - g1).max() <= 2e-3 * np.abs(g1).max()
    assert set(o0) >= {"rendered_masks", "ref_masks", "error_maps", "metrics", "tsfm"}
    assert set(o0["metrics"]) == {"err_x", "err_y", "err_z", "err_trans", "err_rot"}


def test_full_size_properties(env, xarm7):
    """BASELINE configs[2] size (1280x720 x 8 views): properties that do not need the oracle."""
    fused, ctx, scene, dev = env
    H, W, B = 720, 1280, 8
    K, lp, Tc, mvp_gt = workload(xarm7, H, W, 1.0, B, seed=0, perturb=False)
    zeros = np.zeros((B, H, W), np.float32)
    mask, loss, _ = run(fused, ctx, scene, mvp_gt, zeros, dev)
    assert mask.min() >= 0 and mask.max() <= 1
    assert np.allclose(loss, (mask.astype(np.float64) ** 2).sum(axis=(1, 2)), rtol=1e-6)   # loss vs its own mask
    ref = (mask > 0.5).astype(np.float32)
    m2, l2, g2 = run(fused, ctx, scene, mvp_gt, ref, dev)
    assert (m2 == mask).all()                                # the reference mask does not influence the render
    frac = ((mask > 0) & (mask < 1)).sum()
    assert l2.sum() <= frac                                  # at the GT pose only antialiased pixels contribute
    # view permutation equivariance (independent shards: SURVEY 8e)
    perm = np.array([3, 0, 7, 1, 6, 2, 5, 4])
    m3, l3, g3 = run(fused, ctx, scene, mvp_gt[perm], ref[perm], dev)
    assert (m3 == m2[perm]).all() and (l3 == l2[perm]).all() and (g3 == g2[perm]).all()
    # a view is unchanged by what else is in the batch
    m4, l4, g4 = run(fused, ctx, scene, mvp_gt[:1], ref[:1], dev)
    assert (m4[0] == m2[0]).all() and l4[0] == l2[0] and (g4[0] == g2[0]).all()
    # link additivity below the clamp: rendering links {0..3} and {4..7} separately sums to the joint render wherever
    # the joint sum stays <= 1
    from easyhec_amd import fused as F
    sA = F.LinkScene([v for v, _ in xarm7.meshes[:4]], [f for _, f in xarm7.meshes[:4]], dev)
    sB = F.LinkScene([v for v, _ in xarm7.meshes[4:]], [f for _, f in xarm7.meshes[4:]], dev)
    mA, _, _ = run(fused, ctx, sA, mvp_gt[:2, :4], zeros[:2], dev)
    mB, _, _ = run(fused, ctx, sB, mvp_gt[:2, 4:], zeros[:2], dev)
    s = mA + mB
    ok = s <= 1.0
    assert np.abs(np.minimum(s, 1.0) - mask[:2])[ok].max() <= 2.4e-7


def test_overflow_is_reported_not_silent(env, oracle, xarm7):
    """A pathological checkerboard of pixel-sized quads in every one of 10 links (four blended pairs per covered
    pixel, 10 links deep in one tile).  Round 1's per-tile LDS list overflowed here (reported NaN); the per-job item
    slots + spill pool of the visibility-buffer chain hold it, so the result must now simply equal the oracle's.  The
    limits that remain (fixed-point accumulator range) still fail loudly: second half of the test."""
    fused, _, _, dev = env
    from easyhec_amd import dr
    H, W, L = 8, 32, 10
    vs, fs = [], []
    for l in range(L):
        v, f = [], []
        for y in range(H):
            for x in range(W):
                if (x + y) % 2 == 0:
                    cx, cy = (x + 0.5) / W * 2 - 1, (y + 0.5) / H * 2 - 1
                    hx, hy = 0.6 / W, 0.6 / H
                    n = len(v)
                    v += [[cx - hx, cy - hy, 0], [cx + hx, cy - hy, 0], [cx + hx, cy + hy, 0], [cx - hx, cy + hy, 0]]
                    f += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
        vs.append(np.array(v, np.float32))
        fs.append(np.array(f, np.int32))
    ctx2 = dr.RasterizeCudaContext()
    scene = fused.LinkScene(vs, fs, dev)
    mvp_np = np.tile(np.eye(4, dtype=np.float32)[None, None], (1, L, 1, 1))
    mvp_np[0, :, 3, 3] = 1.0 + 0.01 * np.arange(L)          # distinct w per link: distinct blend weights
    rng = np.random.default_rng(5)
    ref = (rng.uniform(size=(1, H, W)) > 0.5).astype(np.float32)
    verts = np.concatenate(vs)
    voff = np.cumsum([0] + [len(v) for v in vs]).astype(np.int32)
    toff = np.cumsum([0] + [len(f) for f in fs]).astype(np.int32)
    tris = np.concatenate([f + voff[i] for i, f in enumerate(fs)]).astype(np.int32)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp_np, ref)
    mask, loss, grad = run(fused, ctx2, scene, mvp_np, ref, dev)
    assert (mask == m_ref).all()
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max()
    assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    fused.check_status(ctx2)
    # the same scene with a spill pool of 100 items (EHR_VB_SPILL_ITEMS, read at plan time): the jobs that do not fit
    # report the overflow (NaN loss, raised status) and nothing is read or written outside the pool
    os.environ["EHR_VB_SPILL_ITEMS"] = "100"
    try:
        ctx3 = dr.RasterizeCudaContext()
        tm = torch.tensor(mvp_np, device=dev, requires_grad=True)
        _, loss_t = fused.render_mask_loss(ctx3, scene, tm, torch.tensor(ref, device=dev))
        loss_t.sum().backward()
        torch.cuda.synchronize()
    finally:
        del os.environ["EHR_VB_SPILL_ITEMS"]
    assert torch.isnan(loss_t).all() and torch.isnan(tm.grad).all()
    with pytest.raises(RuntimeError, match="overflow"):
        fused.check_status(ctx3)
    # the fixed-point accumulators saturate loudly too: the robot scaled by 1e9 (and the clip matrices' first three
    # columns by 1e-9) renders the same picture, but its gradients w.r.t. the matrix entries exceed the representable
    # +-2^31 -> NaN gradient + raised status, never a wrapped sum
    Hs, Ws = 120, 160
    K, lp, Tc, mvp_s = workload(xarm7, Hs, Ws, 0.125, 1, seed=2)
    normal = fused.LinkScene([v for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    big = fused.LinkScene([v * 1e9 for v, _ in xarm7.meshes], [f for _, f in xarm7.meshes], dev)
    scale = np.diag([1e-9, 1e-9, 1e-9, 1.0]).astype(np.float32)
    ref = torch.zeros((1, Hs, Ws), device=dev)
    ctx4, ctx5 = dr.RasterizeCudaContext(), dr.RasterizeCudaContext()
    t_n = torch.tensor(mvp_s, device=dev, requires_grad=True)
    t_b = torch.tensor(mvp_s @ scale, device=dev, requires_grad=True)
    m_n, l_n = fused.render_mask_loss(ctx4, normal, t_n, ref)
    m_b, l_b = fused.render_mask_loss(ctx5, big, t_b, ref)
    l_n.sum().backward()
    l_b.sum().backward()
    torch.cuda.synchronize()
    assert (m_n > 0).sum() > 100 and (m_b - m_n).abs().max() <= 1e-3   # same picture (up to the rescaling's rounding)
    assert torch.isfinite(t_n.grad).all() and float(t_n.grad.abs().max()) > 0
    assert torch.isnan(t_b.grad).all()
    fused.check_status(ctx4)
    with pytest.raises(RuntimeError, match="overflow"):
        fused.check_status(ctx5)


def test_franka_config4_full_size(oracle):
    """BASELINE configs[3]: Franka link0-7 + hand (133 676 triangles), 1920x1080, 16 views.  Bit-exact against the
    oracle on the first 3 views, oracle-free properties on all 16."""
    from easyhec_amd import dr, fused
    from easyhec_amd.robot import load_robot
    from easyhec_amd.synthetic import WORKLOADS, camera_Tc_c2b, make_views, perturb_pose
    dev = torch.device("cuda:0")
    fr = load_robot("franka")
    wl = WORKLOADS["franka_1920x1080_16view"]
    H, W, K, B = wl["H"], wl["W"], wl["K"], wl["views"]
    _, lp = make_views(fr, B, seed=0)
    Tc = camera_Tc_c2b(radius=wl["radius"], lift=wl["lift"])
    mvp = helpers.mvp_numpy(K, H, W, perturb_pose(Tc), lp)
    ctx = dr.RasterizeCudaContext()
    scene = fused.LinkScene([v for v, _ in fr.meshes], [f for _, f in fr.meshes], dev)
    rng = np.random.default_rng(4)
    ref = (rng.uniform(size=(B, H, W)) > 0.97).astype(np.float32)
    mask, loss, grad = run(fused, ctx, scene, mvp, ref, dev)
    verts, tris, toff, voff = helpers.scene_arrays(fr)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp[:3], ref[:3])
    assert (mask[:3] == m_ref).all()
    assert np.abs(loss[:3] - l_ref).max() <= 1e-6 * np.abs(l_ref).max()
    assert np.abs(grad[:3] - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
    assert mask.min() >= 0 and mask.max() <= 1 and np.isfinite(grad).all()
    for b in range(B):   # every view fully in frame, as the config asks
        ys, xs = np.nonzero(mask[b] > 0)
        assert 0 < xs.min() and xs.max() < W - 1 and 0 < ys.min() and ys.max() < H - 1
    assert np.allclose(loss, ((mask.astype(np.float64) - ref) ** 2).sum(axis=(1, 2)), rtol=1e-6)
    again = run(fused, ctx, scene, mvp, ref, dev)
    assert (again[0] == mask).all() and (again[1] == loss).all() and (again[2] == grad).all()


def test_franka_64_views_1080p_under_a_2gb_scratch_budget():
    """Franka at 1920x1080 with 64 views in ONE call -- 576 (view, link) units, ~11 GB of scratch if taken in one piece --
    with the per-chunk scratch bounded to 1.7 GB (EHR_VB_SCRATCH_MB; a process of its own: the budget is read once): the
    call splits into chunks of views, the context takes less than 2 GB of device memory all told (chunk scratch, static
    index, accumulators, spill pool), every view is finite and views 0-2 are bit-equal to a 3-view call."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env2 = dict(os.environ, EHR_VB_SCRATCH_MB="1700")
    out = subprocess.run([sys.executable, os.path.join(here, "chunk_worker.py")], env=env2, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["views"] == 64 and res["finite"] and res["loss_min"] > 0
    assert res["same_loss"] and res["same_grad"]
    # the context's scratch; the torch caching allocator's blocks for mvp.grad / loss (a few MB) are inside the figure
    assert res["scratch_bytes"] < 2.0e9, res["scratch_bytes"]


def test_fused_edge_cases(env, oracle, xarm7):
    """Empty and ragged inputs: nothing in view, a single link / single view, a lone huge triangle that is queued in
    every tile of the image, sizes that are not multiples of the 32x8 tile, and the largest supported square image."""
    fused, ctx, scene, dev = env
    # (1) robot behind the camera: every tile is empty -> loss = sum(ref^2), zero gradient, no NaN
    H, W, B = 96, 160, 2
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.125, B, seed=3, perturb=False)
    back = np.eye(4)
    back[2, 3] = -6.0                                                 # push the whole scene 6 m behind the camera
    mvp_behind = helpers.mvp_numpy(K, H, W, back @ Tc, lp)
    rng = np.random.default_rng(0)
    ref = (rng.uniform(size=(B, H, W)) > 0.7).astype(np.float32)
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp_behind, ref)
    mask, loss, grad = run(fused, ctx, scene, mvp_behind, ref, dev)
    assert (m_ref == 0).all() and (mask == 0).all() and (grad == 0).all() and np.isfinite(loss).all()
    assert np.allclose(loss, ref.reshape(B, -1).sum(1)) and np.allclose(loss, l_ref)
    # (2) one link, one view, ragged size
    v0, f0 = xarm7.meshes[2]
    sc1 = fused.LinkScene([v0], [f0], dev)
    H, W = 75, 101
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.08, 1, seed=5)
    mvp1 = mvp[:, 2:3].copy()
    ref = np.zeros((1, H, W), np.float32)
    toff1, voff1 = np.array([0, f0.shape[0]], np.int32), np.array([0, v0.shape[0]], np.int32)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(v0, f0, toff1, voff1, mvp1, ref)
    mask, loss, grad = run(fused, ctx, sc1, mvp1, ref, dev)
    assert (m_ref > 0).sum() > 20 and (mask == m_ref).all()
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max()
    assert np.abs(grad - g_ref).max() <= 1e-5 * max(np.abs(g_ref).max(), 1e-30)
    # (3) one triangle covering the whole image (queued in every tile; partly outside the frustum sideways)
    vt = np.array([[-30.0, -20.0, 0.0], [30.0, -20.0, 0.0], [0.0, 40.0, 0.0]], np.float32)
    ft = np.array([[0, 1, 2]], np.int32)
    sct = fused.LinkScene([vt], [ft], dev)
    H, W = 200, 328
    P = helpers.projection(np.array([[150.0, 0, W / 2], [0, 150.0, H / 2], [0, 0, 1]]), H, W)
    pose = np.eye(4)
    pose[2, 3] = 3.0
    mvpt = (P @ np.diag([1.0, -1.0, -1.0, 1.0]) @ pose).astype(np.float32)[None, None]
    ref = np.ones((1, H, W), np.float32)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(vt, ft, np.array([0, 1], np.int32), np.array([0, 3], np.int32), mvpt, ref)
    mask, loss, grad = run(fused, ctx, sct, mvpt, ref, dev)
    assert (m_ref == 1).all() and (mask == 1).all() and (loss == 0).all() and (l_ref == 0).all()
    # (4) the largest square image of the documented range (2048 x 2048), one view of the whole robot
    H = W = 2048
    K, lp, Tc, mvp = workload(xarm7, H, W, 1.6, 1, seed=9)
    ref = np.zeros((1, H, W), np.float32)
    mask, loss, grad = run(fused, ctx, scene, mvp, ref, dev)
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and 0.01 < (mask > 0.5).mean() < 0.6
    assert abs(float(loss[0]) - float((mask.astype(np.float64) ** 2).sum())) <= 1e-6 * float(loss[0])


def test_many_views_go_through_in_chunks(env, xarm7, oracle):
    """views x links above the 512 (view, link) units one pass of the chain handles (the reference batches a whole data
    set per step: batch_size 100 x 7-8 links), and a scratch budget that forces still smaller chunks: the call splits its
    views into chunks internally.  Every view's loss and gradient must equal, bit for bit, what the same view gives in a
    small single-chunk call; spot-checked against the oracle; the bound-reference path included."""
    fused, _, scene, dev = env
    from easyhec_amd import dr
    B, H, W, scale = 70, 96, 128, 0.1                   # 70 views x 8 links = 560 units -> 2 chunks (64 + 6)
    K, lp, Tc, mvp = workload(xarm7, H, W, scale, B, seed=11)
    rng = np.random.default_rng(11)
    ref = torch.tensor((rng.uniform(size=(B, H, W)) > 0.8).astype(np.float32), device=dev)
    tm = torch.tensor(mvp, device=dev)

    def call(ctx, sl, bound):
        n = sl.stop - sl.start
        r, m = ref[sl].contiguous(), tm[sl].contiguous()
        fused._ensure_plan(ctx, scene, n, H, W)
        fused.bind_ref(ctx, scene, r if bound else None)
        loss, grad = torch.empty((n,), device=dev), torch.empty((n, scene.num_links, 4, 4), device=dev)
        fused._launch(ctx, scene, m, r, None, loss, grad)
        torch.cuda.synchronize()
        fused.check_status(ctx)
        return loss, grad

    big = dr.RasterizeCudaContext()
    l_all, g_all = call(big, slice(0, B), False)
    l_bnd, g_bnd = call(big, slice(0, B), True)
    assert torch.equal(l_all, l_bnd) and torch.equal(g_all, g_bnd)
    small = dr.RasterizeCudaContext()
    for lo in (0, 30, 60):                               # 10-view single-chunk calls, one of them across the chunk border
        l_s, g_s = call(small, slice(lo, lo + 10), False)
        assert torch.equal(l_all[lo:lo + 10], l_s) and torch.equal(g_all[lo:lo + 10], g_s)
    os.environ["EHR_VB_SCRATCH_MB"] = "1"               # (read once per process by the library: only effective if first)
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    for b in (0, 65):
        m_ref, l_ref, g_ref = oracle.render_mask_loss(verts, tris, toff, voff, mvp[b:b + 1], ref[b:b + 1].cpu().numpy())
        assert abs(float(l_all[b]) - l_ref[0]) <= 1e-6 * abs(l_ref[0])
        assert np.abs(g_all[b].cpu().numpy() - g_ref[0]).max() <= 1e-5 * np.abs(g_ref).max()
    # the mask-output form in chunks: masks of the chunked call == masks of the small calls
    mask = torch.empty((B, H, W), device=dev)
    loss_m = torch.empty((B,), device=dev)
    fused._ensure_plan(big, scene, B, H, W)
    fused._launch(big, scene, tm, ref, mask, loss_m, None)
    torch.cuda.synchronize()
    assert torch.equal(loss_m, l_all)
    mref, _, _ = oracle.render_mask_loss(verts, tris, toff, voff, mvp[66:67], ref[66:67].cpu().numpy())
    assert (mask[66].cpu().numpy() == mref[0]).all()


def test_job_slots_limited_by_slack_report_overflow(env, xarm7):
    """ehr_fused_plan(slack > 0) provides only `slack` job slots per view tile; a close-up view in which the links' boxes
    overlap needs more than one: reported (NaN loss, raised status), never a silently incomplete image.  (The default
    plan has a slot for every (view, link, tile): the same call is fine there.)"""
    fused, _, scene, dev = env
    from easyhec_amd import _lib, dr
    import ctypes
    H, W, B = 64, 96, 2
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.075, B, seed=3)
    mvp[:, :, :2, :] *= 2.5                             # zoom: the robot fills the frame, the links' boxes overlap
    ctx = dr.RasterizeCudaContext()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ehr_fused_plan(ctx.handle, B, scene.num_links, scene.num_verts, scene.num_tris, H, W,
                                             ctypes.c_float(1.0), _lib.ptr(scene.verts), _lib.ptr(scene.tris),
                                             _lib.ptr(scene.tri_link), _lib.ptr(scene.opp)), "plan")
    ctx._plan = type("P", (), {"key": fused._plan_key(scene, B, H, W)})()
    loss = torch.empty((B,), device=dev)
    fused._launch(ctx, scene, torch.tensor(mvp, device=dev), torch.zeros((B, H, W), device=dev), None, loss, None)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all()
    with pytest.raises(RuntimeError, match="overflow"):
        fused.check_status(ctx)
    ctx2 = dr.RasterizeCudaContext()
    fused._ensure_plan(ctx2, scene, B, H, W)
    fused._launch(ctx2, scene, torch.tensor(mvp, device=dev), torch.zeros((B, H, W), device=dev), None, loss, None)
    torch.cuda.synchronize()
    fused.check_status(ctx2)
    assert torch.isfinite(loss).all() and float(loss.min()) > 100.0   # (SSE against an empty reference = covered area)


def test_default_launch_chain_recovers_from_a_slot_overflow(env, xarm7, monkeypatch):
    """the launch chain plans HALF a job slot per view tile by default (50 MB instead of 0.8 GB at
    8 views 720p x 8 links).  A close-up in which the links' boxes pile up needs more: the step reports it (NaN loss, dof and
    Adam untouched), RBSolverTrainer.fit plans again with a slot per (view, link, tile) and goes on -- and the solve ends
    exactly where a solve with every slot from the start ends."""
    fused, _, scene, dev = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.trainer import RBSolverTrainer
    H, W, B = 64, 96, 2
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5  # zoom: the robot fills the frame, the links' boxes overlap everywhere
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    cfg.solver.log_interval = 1
    ref = torch.zeros((B, H, W), device=dev)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(K, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    ends = []
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")   # (a 64 x 96 frame has 24 tiles: the default would give it every slot)
    for slack in (None, 0.0):
        model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
        tr = RBSolverTrainer(cfg, model, batch, fast=True)
        if slack is not None:  # every slot from the start
            tr.fast.slack = 0.0
            fused._ensure_plan(tr.fast.glctx, tr.fast.scene, B, H, W, slack=0.0)
            fused.bind_ref(tr.fast.glctx, tr.fast.scene, tr.fast.ref)
        else:
            assert tr.fast.slack == 1.0
        logs = []
        hist = tr.fit(num_steps=5, log=logs.append)   # five EFFECTIVE steps: the reported one is taken again
        if slack is None:
            assert any("job slots overflowed" in l for l in logs), logs  # the first step was the reported one
            assert tr.fast.slack == 0.0
        assert all(np.isfinite(l) for _, l in hist[-5:])
        ends.append((model.dof.detach().clone(), tr.fast.step_t.clone(), model.history_ops[:8].clone(), tr.global_steps))
    assert int(ends[0][1]) == int(ends[1][1]) == 5            # five real Adam steps either way
    assert ends[0][3] == ends[1][3] == 5
    assert torch.equal(ends[0][0], ends[1][0])                # ... to the same pose, bit for bit
    assert torch.equal(ends[0][2], ends[1][2])                # ... through the same history: one row per effective step
    assert float(ends[0][2][5:].abs().sum()) == 0.0


def test_an_unattended_stepping_loop_recovers_by_itself(env, xarm7, monkeypatch):
    """a caller that only ever calls trainer.step() -- never fit(), never looks at the loss --
    must not be left on the initial pose by a reported step.  step() polls the loss every ``check_every`` steps without
    waiting (pinned copy + event); a NaN there re-plans.  48 calls on the overflowing close-up: calls 1..32 are reported
    (the poll at call 16 starts the look, the one at call 32 sees it), calls 33..48 are real steps -- and they equal the
    first 16 steps of a solve that had every slot from the start, history rows included."""
    fused, _, scene, dev = env
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.trainer import RBSolverTrainer
    H, W, B = 64, 96, 2
    K, lp, Tc, mvp = workload(xarm7, H, W, 0.075, B, seed=3)
    K = np.array(K, dtype=np.float64)
    K[:2, :2] *= 2.5
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    ref = torch.zeros((B, H, W), device=dev)
    ref[:, 10:50, 20:70] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(K, dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    monkeypatch.setenv("EHR_VB_SLACK", "1.0")
    model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    tr = RBSolverTrainer(cfg, model, batch, fast=True)
    assert tr.fast.check_every == 16
    for i in range(48):
        tr.step()
        if i in (15, 31):
            torch.cuda.synchronize()   # (so that the look started at call 16 has certainly arrived by call 32)
    torch.cuda.synchronize()
    assert tr.fast.recoveries == ["job slots"] and tr.fast.slack == 0.0
    assert tr.fast.steps_done == 16
    monkeypatch.setenv("EHR_VB_SLACK", "0")
    model2 = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
    tr2 = RBSolverTrainer(cfg, model2, batch, fast=True)
    for _ in range(16):
        tr2.step()
    torch.cuda.synchronize()
    assert torch.equal(model.dof.detach(), model2.dof.detach())
    assert torch.equal(model.history_ops[:20], model2.history_ops[:20])
    assert float(model.history_ops[16:20].abs().sum()) == 0.0


def test_solver_step_switches_the_general_triangle_pass_on_when_a_step_needs_it(env, xarm7):
    """the solver step's chain does not launch the (normally empty) general-triangle pass.  A
    camera so close that triangles cross the near plane needs it: the first step reports that (NaN loss, dof and Adam
    untouched; ehr_fused_status -> EHR_ERR_RETRY), the pass joins the chain -- also the captured one -- and the solve ends
    exactly where a solve on a context that had the pass from the start ends."""
    fused, _, scene, dev = env
    from easyhec_amd import _lib
    from easyhec_amd.config import Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.trainer import RBSolverTrainer
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, scaled_K
    H, W, B = 240, 320, 2
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    K[:2, :2] *= 12.0                            # a 12x zoom from 45 cm: triangles of several hundred pixels, wider than the
    _, lp = make_views(xarm7, B, seed=4)         # 512 the 32-bit edge functions of the job kernel's rasterizer cover
    Tc = camera_Tc_c2b(radius=0.45, lift=0.2)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = np.asarray(Tc).tolist()
    cfg.solver.log_interval = 1
    ref = torch.zeros((B, H, W), device=dev)
    ref[:, 8:200, 10:300] = 1.0
    batch = {"mask": ref, "link_poses": torch.tensor(lp, dtype=torch.float32, device=dev),
             "K": torch.tensor(np.array(K), dtype=torch.float32, device=dev)[None].repeat(B, 1, 1)}
    ends = []
    for graph in (False, True, None):   # None: the pass switched on before the first step
        model = RBSolver(cfg, meshes=xarm7.meshes).to(dev)
        tr = RBSolverTrainer(cfg, model, batch, fast=True, graph=bool(graph))
        tr.fast.slack = 0.0             # (every job slot: this test is about the other report)
        fused._ensure_plan(tr.fast.glctx, tr.fast.scene, B, H, W, slack=0.0)
        fused.bind_ref(tr.fast.glctx, tr.fast.scene, tr.fast.ref)
        if graph:
            tr.fast.release_graph()
            tr.fast.capture()
        logs = []
        if graph is None:
            tr.step()                                                   # reported ...
            torch.cuda.synchronize()
            assert _lib.lib().ehr_fused_status(tr.fast.glctx.handle) == _lib.EHR_ERR_RETRY
            assert _lib.lib().ehr_fused_status(tr.fast.glctx.handle) == _lib.EHR_ERR_RETRY   # (until a step has run with it)
            assert int(tr.fast.step_t) == 0                            # ... and nothing moved
            hist = tr.fit(num_steps=5, log=logs.append)
            assert not any("general-triangle" in l for l in logs), logs
        else:
            hist = tr.fit(num_steps=5, log=logs.append)   # five EFFECTIVE steps: the reported first one is taken again
            assert any("general-triangle pass joins" in l for l in logs), logs
        assert all(np.isfinite(l) for _, l in hist[-5:]), hist
        ends.append((model.dof.detach().clone(), int(tr.fast.step_t)))
    assert [e[1] for e in ends] == [5, 5, 5]
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][0], ends[2][0])


@pytest.mark.parametrize("H,W,scale,B", [(720, 1280, 1.0, 8), (100, 150, 0.12, 3), (97, 131, 0.12, 2)])
def test_bound_reference_with_a_mask_output_fills_the_unowned_tiles(env, xarm7, H, W, scale, B):
    """Bound reference AND a mask output: the composite stage visits the job tiles only and stores zeros to every tile no
    job owns, without reading the reference there.  The mask, the loss and the gradient must equal the unbound full pass
    bit for bit -- into a buffer that held garbage, and again at another pose into the same buffer (tiles the robot left
    must be zero again).  (97 x 131: partial tiles on both edges, the scalar store form.)"""
    fused, _, scene, dev = env
    from easyhec_amd import dr
    ctx = dr.RasterizeCudaContext()
    rng = np.random.default_rng(H)
    ref = torch.tensor((rng.uniform(size=(B, H, W)) > 0.6).astype(np.float32), device=dev)
    mask_b = torch.full((B, H, W), float("nan"), device=dev)
    fused._ensure_plan(ctx, scene, B, H, W)
    for seed in (3, 4, 3):
        K, lp, Tc, mvp = workload(xarm7, H, W, scale, B, seed=seed)
        tm = torch.tensor(mvp, device=dev)
        res = []
        for bound in (False, True):
            fused.bind_ref(ctx, scene, ref if bound else None)
            mask = mask_b if bound else torch.full((B, H, W), float("nan"), device=dev)
            loss = torch.empty((B,), device=dev)
            grad = torch.empty((B, scene.num_links, 4, 4), device=dev)
            fused._launch(ctx, scene, tm, ref, mask, loss, grad)
            torch.cuda.synchronize()
            res.append((mask.clone(), loss.clone(), grad.clone()))
        for a, b in zip(res[0], res[1]):
            assert torch.equal(a, b)
        assert float(res[1][0].sum()) > 0 and float((res[1][0] == 0).float().mean()) > 0.5
    fused.check_status(ctx)


@pytest.mark.parametrize("H,W,scale,B", [(720, 1280, 1.0, 8), (100, 150, 0.12, 3)])
def test_bound_reference_is_bit_identical(env, xarm7, H, W, scale, B):
    """ehr_fused_bind_ref caches, per tile, the fixed-point sum(ref^2) the composite stage would add for a tile no link
    touches; with it the stage only visits tiles inside the link boxes.  Integer sums: loss and gradient must equal the
    unbound path BIT FOR BIT (random reference mask, so every tile has a non-trivial cached value), for several poses
    against the same binding, and re-binding after the contents changed must pick up the new contents."""
    fused, _, scene, dev = env
    from easyhec_amd import dr
    ctx = dr.RasterizeCudaContext()
    rng = np.random.default_rng(W)
    ref = torch.tensor(rng.uniform(size=(B, H, W)).astype(np.float32), device=dev)
    outs = []
    for seed in (1, 2):
        K, lp, Tc, mvp = workload(xarm7, H, W, scale, B, seed=seed)
        tm = torch.tensor(mvp, device=dev)
        res = []
        for bound in (False, True):
            fused.bind_ref(ctx, scene, ref if bound else None)
            loss = torch.empty((B,), device=dev)
            grad = torch.empty((B, scene.num_links, 4, 4), device=dev)
            fused._ensure_plan(ctx, scene, B, H, W)
            fused._launch(ctx, scene, tm, ref, None, loss, grad)
            torch.cuda.synchronize()
            res.append((loss.clone(), grad.clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        assert float(res[0][0].min()) > 0
        outs.append(res[1][0])
    assert not torch.equal(outs[0], outs[1])
    # new contents + re-bind; and the mask-output form agrees with both
    ref2 = torch.tensor((rng.uniform(size=(B, H, W)) > 0.7).astype(np.float32), device=dev)
    ref.copy_(ref2)
    fused.bind_ref(ctx, scene, ref)
    loss_b, loss_m = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
    mask = torch.empty((B, H, W), device=dev)
    fused._launch(ctx, scene, tm, ref, None, loss_b, None)
    fused._launch(ctx, scene, tm, ref, mask, loss_m, None)
    torch.cuda.synchronize()
    assert torch.equal(loss_b, loss_m)
    sse = ((mask.double() - ref.double()) ** 2).sum(dim=(1, 2))
    assert (loss_b.double() - sse).abs().max() <= 1e-6 * sse.max()
    fused.check_status(ctx)
