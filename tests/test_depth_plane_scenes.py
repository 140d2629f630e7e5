"""The scenes of tests/depth_plane_scenes.py on the CPU oracle alone: the conditions that keep the GPU cases of
tests/test_gpu_depth_planes.py from passing vacuously (the far plane really rejects pixels of some triangles and not of
others; the stack really holds several deferred lists' worth of unsafe units under drawn AND rejected pixels; the planes
really cut the robot; the extents really are 8191 / 8192 / 8193).  Measured counts are in the assertion messages."""
import numpy as np
import pytest

import depth_plane_scenes as D
import helpers


def alone(oracle, meshes, mvp, H, W):
    """Per view: (covered, drawn) pixel counts of every triangle rendered ALONE (range mode: one triangle per image) --
    covered: with z = 0 (coverage only), drawn: with its own depths (coverage and the depth planes)."""
    out = []
    for b in range(mvp.shape[0]):
        cov, drw = [], []
        for l, (v, f) in enumerate(meshes):
            pos = oracle.transform_pos(mvp[b, l], v)[0]
            flat = pos.copy()
            flat[:, 2] = 0.0
            rg = np.stack([np.arange(len(f)), np.ones(len(f))], axis=1).astype(np.int32)
            for lo in range(0, len(f), 200):
                r, _ = oracle.rasterize(pos, f, (H, W), ranges=rg[lo:lo + 200], grad_db=False)
                r0, _ = oracle.rasterize(flat, f, (H, W), ranges=rg[lo:lo + 200], grad_db=False)
                cov.append((r0[..., 3] != 0).sum(axis=(1, 2)))
                drw.append((r[..., 3] != 0).sum(axis=(1, 2)))
        out.append((np.concatenate(cov), np.concatenate(drw)))
    return out


# measured 2026-10-18 (partly, wholly, not rejected, no pixel centre) per view:
#   far_soup        (54, 60, 157, 209) (49, 61, 155, 215)
#   far_slivers     (38, 115, 226, 521) (38, 106, 225, 531)
#   far_perspective (36, 91, 172, 181) (38, 79, 190, 173)
@pytest.mark.parametrize("family", ["far_soup", "far_slivers", "far_perspective"])
def test_the_far_plane_rejects_some_pixels_of_some_triangles(oracle, family):
    meshes, mvp, H, W = getattr(D, family)()
    assert H <= 128 and W <= 160 and mvp.dtype == np.float32
    for b, (c, d) in enumerate(alone(oracle, meshes, mvp, H, W)):
        assert (d <= c).all()
        partly, wholly, none = int(((d > 0) & (d < c)).sum()), int(((c > 0) & (d == 0)).sum()), int(((c > 0) & (d == c)).sum())
        counts = (family, b, partly, wholly, none, int((c == 0).sum()))
        print("[far plane]", counts)
        assert partly >= 30 and wholly >= 30 and none >= 30, counts
    m2 = getattr(D, family)()
    assert all((a == b).all() for x, y in zip(meshes, m2[0]) for a, b in zip(x, y)) and (mvp == m2[1]).all()   # deterministic


def test_far_perspective_lands_on_both_sides_of_the_w_bar(oracle):
    meshes, mvp, H, W = D.far_perspective()
    r = []
    for l, (v, f) in enumerate(meshes):
        w = oracle.transform_pos(mvp[0, l], v)[0][:, 3][f]
        assert (w > 0).all()
        r.append(w.max(axis=1) / w.min(axis=1))
    r = np.concatenate(r)
    counts = (int(((r > 3.5) & (r <= 4)).sum()), int(((r > 4) & (r < 4.5)).sum()), int((r < 2).sum()))
    assert min(counts[:2]) >= 60 and counts[2] >= 200, counts        # measured: (120, 120, 240) +- the draw


def _masks(oracle, mesh, M, H, W):
    """coverage (z = 0) and drawn (own depths) masks of one mesh under one matrix, GL row order"""
    v, f = mesh
    pos = oracle.transform_pos(M, v)
    flat = pos.copy()
    flat[..., 2] = 0.0
    return (oracle.rasterize(flat, f, (H, W), grad_db=False)[0][0, :, :, 3] != 0,
            oracle.rasterize(pos, f, (H, W), grad_db=False)[0][0, :, :, 3] != 0)


# measured 2026-10-18, view 0 / view 1 of link 0 in the region of STACK_TILE: (unsafe units, rejected pixels, pixels only
# unsafe triangles draw, pixels under safe quads, job cost by the kernel's formula)
#   base  (5049, 57, 44, 155, 3177) (5051, 55, 46, 155, 3179)
#   wide  (4772, 86, 41, 129, 3007) (4783, 87, 38, 131, 3027)
#   heavy (7934, 48, 53, 155, 7086) (7940, 48, 53, 155, 7092)
@pytest.mark.parametrize("variant", D.STACK_VARIANTS)
def test_the_stack_holds_several_deferred_lists_under_drawn_and_rejected_pixels(oracle, variant):
    meshes, mvp, H, W = D.flagged_stack(variant)
    kinds = D.stack_kinds(variant)
    v, f = meshes[0]
    assert (kinds == 2).sum() >= 40 and (kinds == 0).sum() >= 8 and H <= 128 and W <= 160
    z = v[:, 2][f]
    assert ((z.max(axis=1) > 1) == (kinds > 0)).all() and (z[kinds > 0].min(axis=1) < 1).all()   # unsafe: straddles +1
    assert (z[kinds == 0].max(axis=1).astype(np.float64) < 1 - 1.1e-5).all() and (np.ptp(z[kinds == 0], axis=1) == 0).all()
    # index order interleaves safe and unsafe; so does depth: safe depths in front of, between and behind the unsafe ones
    first_safe, last_safe = np.nonzero(kinds == 0)[0][[0, -1]]
    assert (kinds[:first_safe] > 0).any() and (kinds[first_safe:last_safe] > 0).any()
    zs, zu = z[kinds == 0][:, 0], z[kinds > 0]
    assert (zs < zu.min()).any() and ((zs > zu.min()) & (zs < 1)).any()
    x0, y0, x1, y1 = D.stack_region()
    reg = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    for b in range(2):
        units = cost = 0
        cov_unsafe = np.zeros((H, W), bool)
        for i in np.nonzero(kinds > 0)[0]:
            c, _ = _masks(oracle, (v, f[i:i + 1]), mvp[b, 0], H, W)
            cov_unsafe |= c
            n = int(c[reg].sum())
            units += (n + 3) // 4           # a lower bound of its 4-pixel units in the region, whatever their alignment
            ys, xs = np.nonzero(c[reg])
            if n:
                bw, bh = np.ptp(xs) + 1, np.ptp(ys) + 1
                cost += 3 * bh if (bw + 3) // 4 >= D.VB_SPAN_GW else (n + 3) // 4
        cost += 256 * ((len(f) + 63) // 64)
        _, drawn = _masks(oracle, (v, f), mvp[b, 0], H, W)
        cov_safe, _ = _masks(oracle, (v, f[kinds == 0]), mvp[b, 0], H, W)
        tile = np.zeros((H, W), bool)
        tile[y0 + 1:y1, x0 + 1:x1] = True
        rejected = int((cov_unsafe & ~drawn & tile).sum())
        only_unsafe = int((drawn & ~cov_safe & tile).sum())
        safe_px = int((cov_safe & tile).sum())
        counts = (variant, b, units, rejected, only_unsafe, safe_px, cost)
        print("[stack]", counts)
        assert units >= 3 * D.VB_DL, counts
        assert rejected >= 8 and only_unsafe >= 8 and safe_px >= 8, counts      # two 4-pixel units' worth of each
        if variant == "heavy":
            assert cost >= 2 * D.VB_HEAVY_T, counts


def _robot_masks(oracle, robot, mvp, H, W):
    """per view: union over the links of (coverage, drawn, z/w > 0) -- GL row order"""
    out = []
    for b in range(mvp.shape[0]):
        acc = np.zeros((3, H, W), bool)
        for l, (v, f) in enumerate(robot.meshes):
            pos = oracle.transform_pos(mvp[b, l], v)
            flat = pos.copy()
            flat[..., 2] = 0.0
            r = oracle.rasterize(pos, f, (H, W), grad_db=False)[0][0]
            acc[0] |= oracle.rasterize(flat, f, (H, W), grad_db=False)[0][0, :, :, 3] != 0
            acc[1] |= r[..., 3] != 0
            acc[2] |= r[..., 2] > 0
        out.append(acc)
    return out


# measured 2026-10-18: far keeps 58 % / 49 % of the mask at 120 x 160 and 45 % / 67 % at 100 x 150; z/w > 0 differs from
# coverage on 468 / 619 / 129 / 164 pixels (120 x 160, near 0.6) and 145 / 362 / 179 / 472 (100 x 150, near 0.65), on none at near 0.3
@pytest.mark.parametrize("H,W,scale", D.ROBOT_SHAPES)
def test_the_planes_cut_the_robot(oracle, xarm7, H, W, scale):
    _, mvp_far, _, _ = D.robot_cut_by_far(xarm7, H, W, scale)
    _, mvp_std, _, _ = D.robot_cut_by_far(xarm7, H, W, scale, far=10.0)
    K, lp, _, Tc = D.robot_camera(xarm7, H, W, scale)
    assert (mvp_std == helpers.mvp_numpy(K, H, W, Tc, lp)).all()         # the defaults are today's planes
    verts, tris, toff, voff = helpers.scene_arrays(xarm7)
    zeros = np.zeros((2, H, W), np.float32)
    cut = oracle.render_mask_loss(verts, tris, toff, voff, mvp_far, zeros, want_grad=False)[0] > 0
    std = oracle.render_mask_loss(verts, tris, toff, voff, mvp_std, zeros, want_grad=False)[0] > 0
    for b in range(2):
        kept = cut[b].sum() / std[b].sum()
        print("[robot cut by far]", (H, W, b, int(cut[b].sum()), int(std[b].sum())))
        assert not (cut[b] & ~std[b]).any() and cut[b].sum() < std[b].sum(), (H, W, b)     # a strict subset
        assert 0.2 <= kept <= 0.8, (H, W, b, kept)
    # scoring: near = 0.6 (0.65 at 100 x 150) puts z/w = 0 inside the robot, nothing crosses the near plane; near = 0.3 puts it in front of it
    for near, cuts in ((D.SCORE_NEAR_CUT[H], True), (D.SCORE_NEAR_FRONT, False)):
        mvp = D.robot_scoring(xarm7, H, W, scale, near=near)
        for q in range(mvp.shape[0]):
            for s, (cov, drawn, pos) in enumerate(_robot_masks(oracle, xarm7, mvp[q], H, W)):
                assert (cov == drawn).all(), "a plane other than z/w = 0 rejects pixels"
                diff = int((cov != pos).sum())
                print("[robot scoring]", (H, W, near, q, s, int(cov.sum()), diff))
                assert (diff >= 100) if cuts else (diff == 0), (H, W, near, q, s, diff)
        for l, (v, _) in enumerate(xarm7.meshes):
            p = oracle.transform_pos(mvp[0, 0, l], v)[0]
            assert (p[:, 3] > 0).all() and (p[:, 2] + p[:, 3] > 0).all()   # nothing at or behind the near plane


@pytest.mark.parametrize("axis", ["x", "y"])
def test_the_extents_are_the_intended_integers(axis):
    meshes, mvp, H, W = D.extent_bar(axis)
    assert (H, W) == D.EXTENT_FRAMES[axis]
    ext = D.snapped_extents(meshes[0], mvp[0, 0], H, W, axis)
    want = D.extent_bar_intended(axis)
    assert (ext == want).all() and sorted(set(want.tolist())) == list(D.EXTENTS)
    other = D.snapped_extents(meshes[0], mvp[0, 0], H, W, "y" if axis == "x" else "x")
    assert other.max() < D.VB_FAST_EXTENT and (other <= 20 * 16).sum() >= len(want) // 2 - 1   # thin ones and fat ones
    S = D.snap(meshes[0], mvp[0, 0], H, W)[..., 0 if axis == "x" else 1]
    half = 8 * max(H, W)
    assert (S.min(axis=1) < -half).any() and (S.max(axis=1) > half).any()                       # some reach outside the frame
    e1, e2 = np.diff(D.snap(meshes[0], mvp[0, 0], H, W), axis=1).transpose(1, 0, 2)
    area2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert (area2 > 0).sum() == (area2 < 0).sum() == len(want) // 2                             # both windings
    for e in D.EXTENTS:                                                                         # one extent at a time
        m1, mv1, _, _ = D.extent_bar(axis, (e,))
        assert (D.snapped_extents(m1[0], mv1[0, 0], H, W, axis) == e).all() and len(m1[0][1]) == len(want) // 3
