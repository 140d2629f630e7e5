"""The job kernel's box trim (the staging block of vb_raster_round and vb_trim_range in csrc/ehr_vbuf.hip): a staged triangle's box, clamped to the job's 34 x 10 region,
is cut down to the rows and columns on which all three edge functions can still be >= 0 before the walkers see it.  The
trim may never drop a covered pixel, so everything here is parity: identity-MVP scenes of triangles placed against the
32 x 8 tile grid (whose regions carry a 1-pixel halo) under the bars of tests/test_gpu_fused.py -- masks bit-equal to the
CPU oracle, loss 1e-6, gradient 1e-5, every (view, link) block to its own bar -- each under the eager and the lazy plan,
which must agree bit for bit; the coverage-only chains (scoring, overlap) against the oracle's integers; and a solve whose
launches and graph replay must end on the same bits, the jobs' cost hints being the only thing the trim changes between steps."""
import numpy as np
import pytest
import torch

import fused_loss_reference
from test_gpu_fused_loss import stateless
from test_gpu_pose_search import expected as overlap_expected

pytestmark = pytest.mark.gpu

TW, TH = 32, 8          # tile; a job's region is the tile plus one pixel all round
SHIFT = (0.37, -0.61)   # the second view: everything moved by a fraction of a pixel


class Tris:
    """Triangles in pixel coordinates (centre of pixel (ix, iy) = (ix + 0.5, iy + 0.5)) for an identity MVP."""

    def __init__(self, H, W):
        self.H, self.W, self.v, self.f = H, W, [], []

    def add(self, a, b, c, z=0.0, flip=False):
        z = np.broadcast_to(np.asarray(z, np.float64), (3,))
        pts = [[2.0 * p[0] / self.W - 1.0, 2.0 * p[1] / self.H - 1.0, zz] for p, zz in zip((a, b, c), z)]
        i = len(self.v)
        self.v.extend(pts[::-1] if flip else pts)
        self.f.append([i, i + 1, i + 2])

    def both(self, a, b, c, z=0.0):   # both windings
        self.add(a, b, c, z)
        self.add(a, b, c, z, flip=True)

    def arrays(self):
        return np.asarray(self.v, np.float32), np.asarray(self.f, np.int32)


def two_views(H, W):
    mvp = np.eye(4, dtype=np.float32)[None, None].repeat(2, axis=0)
    mvp[1, 0, 0, 3] = SHIFT[0] / W
    mvp[1, 0, 1, 3] = SHIFT[1] / H
    return mvp


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import fused
    return fused, torch.device("cuda:0")


def check_scene(env, oracle, monkeypatch, t, what, cover=(0.02, 0.9)):
    """Two views of the triangles `t` with a random binary reference: the eager and the lazy plan bit-equal, and the bars of
    tests/test_gpu_fused.py against the oracle.  -> the oracle's mask."""
    fused, dev = env
    from easyhec_amd import dr
    v, f = t.arrays()
    H, W = t.H, t.W
    mvp = two_views(H, W)
    ref = (np.random.default_rng(len(f)).uniform(size=(2, H, W)) > 0.5).astype(np.float32)
    toff, voff = np.array([0, f.shape[0]], np.int32), np.array([0, v.shape[0]], np.int32)
    m_ref, l_ref, g_ref = oracle.render_mask_loss(v, f, toff, voff, mvp, ref)
    assert cover[0] < (m_ref > 0).mean() < cover[1], (what, (m_ref > 0).mean())
    scene = fused.LinkScene([v], [f], dev)
    res = []
    for lazy in ("0", "1"):
        monkeypatch.setenv("EHR_VB_LAZY", lazy)   # (read by ehr_fused_plan: a fresh context plans afresh)
        res.append(stateless(fused, dr.RasterizeCudaContext(), scene, mvp, ref, dev))
    monkeypatch.delenv("EHR_VB_LAZY")
    for a, b in zip(*res):
        assert (a == b).all(), what + ": eager and lazy plans differ"
    mask, loss, grad = res[0]
    assert (mask == m_ref).all(), what
    assert np.abs(loss - l_ref).max() <= 1e-6 * np.abs(l_ref).max(), what
    assert np.abs(grad - g_ref).max() <= 1e-5 * np.abs(g_ref).max(), what
    fused_loss_reference.check_blocks(grad, fused_loss_reference.block_reference(oracle, [(v, f)], mvp, ref), what)
    return m_ref


def corner_slivers(H, W, n, seed, z=lambda rng: rng.uniform(-0.5, 0.5), thick=(0.2, 2.0), length=(24, 90)):
    """Slivers at random slopes that pass within a few pixels of a tile corner: the full box spans two to four tiles, of
    some of which the sliver only clips a corner, or nothing but its box."""
    rng = np.random.default_rng(seed)
    t = Tris(H, W)
    for _ in range(n):
        c = np.array([TW * rng.integers(1, W // TW + 1), TH * rng.integers(1, H // TH + 1)], np.float64)
        c = np.minimum(c, [W - 3, H - 3]) + rng.uniform(-3, 3, 2)
        ang = rng.uniform(0, 2 * np.pi)
        d = np.array([np.cos(ang), np.sin(ang)])
        ln = rng.uniform(*length)
        s = rng.uniform(0.2, 0.8)
        p = np.clip(c - s * ln * d, 1.5, [W - 1.5, H - 1.5])
        q = np.clip(c + (1 - s) * ln * d, 1.5, [W - 1.5, H - 1.5])
        m = 0.5 * (p + q) + rng.uniform(*thick) * np.array([-d[1], d[0]])
        t.add(p, q, m, z(rng), flip=rng.uniform() < 0.5)
    return t


def test_slivers_that_clip_tile_corners(env, oracle, monkeypatch):
    check_scene(env, oracle, monkeypatch, corner_slivers(96, 160, 220, 1), "corner slivers")


def test_ties_at_the_trimmed_bounds(env, oracle, monkeypatch):
    """Edges exactly through pixel centres on the rows and columns where a region begins and ends (the halo line, the
    tile's first and last line) and in mid tile: horizontal and vertical edges (a zero step along one axis, and an edge
    value of exactly 0 on the first or last line the trim keeps), 45-degree edges (quotients that are exact integers).  The
    triangle lies on either side of the edge and in either winding, so every tie rule decides some line."""
    H, W = 96, 160
    t = Tris(H, W)
    k = 0
    for ty in (1, 3, 5, 7, 9):
        for oy in (-1.5, -0.5, 0.5, 3.5, 6.5, 7.5):       # rows of centres around a tile border and inside the tile
            y = TH * ty + oy
            x0 = 6.5 + 11 * (k % 9)
            for up in (-1, 1):                              # the triangle above / below its horizontal edge
                t.both((x0, y), (x0 + 40.0, y), (x0 + 17.3, y + up * 2.6))
            k += 1
    for tx in (1, 2, 3, 4):
        for ox in (-1.5, -0.5, 0.5, 15.5, 30.5, 31.5):    # columns of centres around a tile border and inside the tile
            x = TW * tx + ox
            y0 = 3.5 + 9 * (k % 6)
            for side in (-1, 1):
                t.both((x, y0), (x, y0 + 37.0), (x + side * 2.6, y0 + 13.3))
            k += 1
    for tx in (1, 2, 3):
        for ty in (2, 5, 8):
            for o in (-0.5, 0.5, 1.5):                      # diagonals through centres, across a tile corner
                cx, cy = TW * tx + o, TH * ty + 0.5
                for sgn in (-1, 1):
                    a, b = (cx - 14.0, cy - sgn * 14.0), (cx + 14.0, cy + sgn * 14.0)
                    t.both(a, b, (cx + 3.0, cy - sgn * 1.0))
                    t.both(a, b, (cx - 3.0, cy + sgn * 1.0))
    check_scene(env, oracle, monkeypatch, t, "ties")


def test_triangles_that_reach_a_region_through_its_halo_or_not_at_all(env, oracle, monkeypatch):
    """Small triangles whose tip ends within a fraction of a pixel of the centres of a region's halo line -- the pixel just
    outside a tile -- so that the tip covers that one pixel, or stops short of it while the box still reaches it; from all
    four sides, both windings."""
    H, W = 96, 160
    rng = np.random.default_rng(7)
    t = Tris(H, W)
    for tx in range(1, W // TW):
        for ty in range(1, H // TH, 2):
            bx, by = TW * tx, TH * ty                       # a tile corner: the halo pixels are bx - 1 / by - 1 and bx / by
            for reach in (-0.45, -0.05, 0.05, 0.45, 1.05):  # how far the tip passes the halo pixel's centre
                yy = by + rng.uniform(1, 6)
                t.both((bx - 12.0, yy - 2.2), (bx - 12.0, yy + 2.4), (bx - 0.5 + reach, yy + 0.1))   # from the left into the tile right of bx
                t.both((bx + 12.0, yy - 2.2), (bx + 12.0, yy + 2.4), (bx + 0.5 - reach, yy + 0.1))
                xx = bx + rng.uniform(3, 28)
                t.both((xx - 2.2, by - 9.0), (xx + 2.4, by - 9.0), (xx + 0.1, by - 0.5 + reach))
                t.both((xx - 2.2, by + 9.0), (xx + 2.4, by + 9.0), (xx + 0.1, by + 0.5 - reach))
    check_scene(env, oracle, monkeypatch, t, "halo")


def test_boxes_of_span_width_that_trim_to_fewer_units(env, oracle, monkeypatch):
    """Steep slivers 13 to 16 pixels wide inside a tile and three to five tiles high: each region's clamped box is exactly
    VB_SPAN_GW (4) units wide, the sliver crosses it in a third of that -- the trimmed box goes to the unit walker; and
    16-pixel boxes that stay that wide (a flat triangle) beside them."""
    H, W = 96, 160
    rng = np.random.default_rng(3)
    t = Tris(H, W)
    for i in range(60):
        x0 = TW * rng.integers(0, W // TW) + rng.uniform(1, TW - 17)
        wd = rng.uniform(12.2, 15.8)
        y0 = rng.uniform(2, 40)
        ht = rng.uniform(24, 50)
        p, q = np.array([x0, y0]), np.array([x0 + wd, min(y0 + ht, H - 2)])
        if i % 2:
            p[0], q[0] = q[0], p[0]
        d = (q - p) / np.linalg.norm(q - p)
        t.add(p, q, 0.5 * (p + q) + rng.uniform(0.3, 2.5) * np.array([-d[1], d[0]]), rng.uniform(-0.5, 0.5), flip=i % 3 == 0)
    for i in range(12):
        x0, y0 = TW * (i % 5) + 8.3, 8 * i + 2.2
        t.add((x0, y0), (x0 + 15.6, y0 + 0.4), (x0 + 7.0, y0 + 5.1), 0.1, flip=i % 2 == 0)
    check_scene(env, oracle, monkeypatch, t, "span width")


def test_span_walker_boxes_with_empty_first_and_last_rows(env, oracle, monkeypatch):
    """Flat slivers a fraction of a pixel thick, 20 to 90 pixels long: their boxes stay wide enough for the span walker, and
    the rows at their two tips hold no pixel centre."""
    t = Tris(96, 160)
    rng = np.random.default_rng(5)
    for i in range(200):
        p = rng.uniform([3, 3], [70, 93])
        ln = rng.uniform(20, 88)
        q = np.array([p[0] + ln, np.clip(p[1] + rng.uniform(-0.12, 0.12) * ln, 2, 94)])
        d = (q - p) / np.linalg.norm(q - p)
        t.add(p, q, (0.3 + 0.4 * rng.uniform()) * (q - p) + p + rng.uniform(0.15, 0.7) * np.array([-d[1], d[0]]),
              rng.uniform(-0.5, 0.5), flip=i % 2 == 0)
    check_scene(env, oracle, monkeypatch, t, "empty rows", cover=(0.005, 0.9))


def test_regions_clamped_by_the_image_border(env, oracle, monkeypatch):
    """150 x 92: the last tile column is 22 pixels wide, the last tile row 4 high.  Slivers and small triangles across
    column 0, row 0, the last column and the last row, partly outside the image."""
    H, W = 92, 150
    rng = np.random.default_rng(9)
    t = Tris(H, W)
    for i in range(160):
        side = i % 4
        u = rng.uniform(0, 1)
        c = [(rng.uniform(-2, 3), u * H), (W - rng.uniform(-2, 3), u * H), (u * W, rng.uniform(-2, 3)), (u * W, H - rng.uniform(-2, 3))][side]
        ang = rng.uniform(0, 2 * np.pi)
        d = np.array([np.cos(ang), np.sin(ang)])
        ln = rng.uniform(6, 60)
        p, q = np.asarray(c) - 0.4 * ln * d, np.asarray(c) + 0.6 * ln * d
        p, q = np.clip(p, [-6, -6], [W + 6, H + 6]), np.clip(q, [-6, -6], [W + 6, H + 6])
        t.add(p, q, 0.5 * (p + q) + rng.uniform(0.2, 2.5) * np.array([-d[1], d[0]]), rng.uniform(-0.5, 0.5), flip=i % 3 == 0)
    for x, y in [(0.5, 0.5), (W - 0.5, 0.5), (0.5, H - 0.5), (W - 0.5, H - 0.5)]:   # edges through the corner pixels' centres
        t.both((x, y), (x + 9.0, y), (x, y + 9.0))
        t.both((x, y), (x - 9.0, y), (x, y - 9.0))
    check_scene(env, oracle, monkeypatch, t, "image border")


def test_depth_tested_triangles_among_ordinary_ones(env, oracle, monkeypatch):
    """Corner slivers of which every second one lies across the far plane (vertex depths 1 +- 0.02: drawn only where z / w
    <= 1, so its units are depth tested pixel by pixel and set their coverage themselves), the others well inside."""
    k = [0]

    def z(rng):
        k[0] += 1
        return rng.uniform(0.98, 1.02, 3) if k[0] % 2 else rng.uniform(-0.5, 0.9)

    t = corner_slivers(96, 160, 200, 11, z=z, thick=(0.5, 4.0))
    m_ref = check_scene(env, oracle, monkeypatch, t, "far plane")
    v, f = t.arrays()
    vi = v[f[1::2].reshape(-1)]                         # the ordinary ones alone
    fi = np.arange(vi.shape[0], dtype=np.int32).reshape(-1, 3)
    m_in, _, _ = oracle.render_mask_loss(vi, fi, np.array([0, len(fi)], np.int32), np.array([0, len(vi)], np.int32), two_views(96, 160),
                                         np.zeros((2, 96, 160), np.float32))
    assert ((m_ref > 0) & ~(m_in > 0)).sum() > 200, "the triangles at the far plane draw nothing of their own"


def test_coverage_only_chains_on_corner_slivers(env, oracle):
    """The scoring op and the overlap op (the job kernel's coverage-only instantiation) on the corner slivers at positive
    depth, Q = 3 candidates (the scene scaled a little about the image centre) x S = 2 views, against the oracle's integers."""
    fused, dev = env
    from easyhec_amd import dr, pose_search, space_explorer
    H, W, Q, S = 96, 160, 3, 2
    t = corner_slivers(H, W, 220, 2, z=lambda rng: rng.uniform(0.1, 0.6))
    v, f = t.arrays()
    mvp = np.empty((Q, S, 1, 4, 4), np.float32)
    for q in range(Q):
        mvp[q] = two_views(H, W)
        mvp[q, :, 0, 0, 0] = mvp[q, :, 0, 1, 1] = 1.0 - 0.07 * q
    link = np.zeros(v.shape[0], np.int32)
    s_ref, c_ref = oracle.mask_variance(v, f, link, mvp, H, W, return_counts=True)
    assert 0.02 < (c_ref > 0).mean() < 0.9 and s_ref.max() > 0
    scene = fused.LinkScene([v], [f], dev)
    ctx = dr.RasterizeCudaContext()
    _, score, counts = space_explorer.mask_variance(ctx, scene, torch.tensor(mvp, device=dev), H, W, return_counts=True)
    assert (counts.cpu().numpy() == c_ref).all()
    assert (score.cpu().numpy() == s_ref).all()
    _, c1 = oracle.mask_variance(v, f, link, np.ascontiguousarray(mvp.reshape(Q * S, 1, 1, 4, 4)), H, W, return_counts=True)
    masks = c1.reshape(Q, S, H, W) > 0
    ref = masks[1].astype(np.float32)
    i_ref, a_ref, r_ref = overlap_expected(masks, ref)
    inter, area, ref_area = pose_search.mask_overlap(ctx, scene, torch.tensor(mvp, device=dev), torch.tensor(ref, device=dev))
    assert (ref_area.cpu().numpy() == r_ref).all() and (area.cpu().numpy() == a_ref).all() and (inter.cpu().numpy() == i_ref).all()
    assert (i_ref < a_ref).any() and i_ref.min() > 0


def test_twenty_solver_steps_launched_and_replayed_end_on_the_same_bits(xarm7):
    """xArm7, 2 views of 160 x 120: the trim changes the cost a job reports, and with it which jobs the next step treats as
    long or heavy -- a schedule, not a result.  Twenty steps as launches and as replays of the captured graph: the same
    trajectory and end state, bit for bit, and the pose has moved."""
    from test_gpu_weighted_loss import assert_same_solve, solo_solve
    launched = solo_solve(xarm7, lambda b: b, steps=20, graph=False)
    replayed = solo_solve(xarm7, lambda b: b, steps=20, graph=True)
    assert_same_solve(launched, replayed)
    assert not torch.equal(launched[0][0], launched[0][-1])
