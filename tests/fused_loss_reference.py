"""Float64 reference of the LAST stage of the fused mask-loss path (vb_composite_kernel in csrc/ehr_vbuf.hip, the same stage
inside ehr_solver_step) and the scenes its tests use.  CPU only, numpy, not collected by pytest.

The reference never decides coverage or a blend.  It takes the per-(view, link) antialiased images from the oracle's ops
(transform_pos -> rasterize -> antialias, colour 1.0 where a triangle was drawn) and only composes:

    sum32   float32 sum of the links' images IN LINK ORDER (the decision variable of the clamp and of the gate)
    mask    sum32 > 1 ? 1 : sum32
    loss    sum (mask - ref)^2 per view, float64
    gimg    2 (mask - ref) where sum32 <= 1, else 0          (torch.clamp's gradient)
    G       per (view, link): oracle.antialias_grad on gimg, contracted in float64 as  G[r][c] = sum_v gpos[v][r] * [x, y, z, 1][c]
    A       per (view, link): max_{r,c} sum_v |gpos[v][r]| * |h[v][c]|, the block's summation scale (reference alone)

Per-block gradient bar
----------------------
``block_bar = K_ROUNDINGS * 2^-24 * A[b, l]`` for all 16 entries of block (b, l); blocks with A == 0 must be exactly zero.
K_ROUNDINGS counts the float32 roundings one addend  g1[r] h1[c] + g2[r] h2[c]  of one blended pair can pass through between
the pair and the fixed-point accumulator in vb_composite_items, each of relative size <= 2^-24 of a partial sum that A bounds:

     3   the addend itself: two products and their sum (-ffp-contract=off: nothing is fused)
    11   serial adds in a lane's G[k]: vb_resolve_job keeps at most one item per entry (region pixel q, direction d) of its hit
         list, q < VB_RN = 340 pixels of the 34 x 10 region and d in {0, 1}, so a job's list (jn, slot + spill) has at most
         2 * VB_RN = 680 items; the 64 lanes of the composite wave take them in turn: ceil(680 / 64)
     6   the shuffle levels of wave_sum12 (offsets 32 .. 1)
     2   into fixed point and out: fix_of rounds each (tile, link) wave sum to 2^-32 ABSOLUTE, one rounding per tile the link
         has a job in; a block sums at most `tiles` of them, and tests/test_fused_loss_reference.py asserts
         A >= tiles * 2^-8 for every scene, which keeps all of them together below one unit of 2^-24 A; fix_get rounds the
         total once
    24   aa_pos_grad (csrc/ehr_device.h), longest chain, that of gp?w: w = 1/p.w (1); x1, y1, x2, y2 (3 each on top of w, the
         chain sees 2 of them: 6); dx, dy (1); db (3); iy (2); dby (1); iw (3); dby - x (1); gp?y (2); gp?w (4)
    --
    46

The oracle evaluates aa_pos_grad with the same float32 expressions, so the last item is slack unless the two compilers
round an expression differently; the oracle's own float32 sum of a vertex's pairs (gpos) is the reference's error and is
counted against the same budget.

Measured worst  |g - G| / (2^-24 A)  per case: MEASURED below, with the date and the command.
"""
import types

import numpy as np

import helpers

K_ROUNDINGS = 3 + 11 + 6 + 2 + 24
U = 2.0 ** -24

# Worst |g_gpu - G| / (2^-24 A) over the blocks of each case, MI355X, 2026-10-17, printed by the cases themselves under
#     pytest -m gpu tests/test_gpu_fused_loss.py tests/test_gpu_fused.py -s -k "soft or clamp or matches_oracle or span_walker"
# (the stateless and the bound form give the same figure: they are bit-equal).  The kernels stay within two units where the
# derivation allows K_ROUNDINGS = 46: the oracle and the kernels evaluate aa_pos_grad to the same bits, so what is left is the
# order of the float32 sums.  A figure above K_ROUNDINGS is a finding to explain by recomputing that block from the oracle's
# items (float order, or a wrong pair?), not a reason to widen the bar.
MEASURED = {
    "soft 120x160 uniform": 1.754, "soft 120x160 own_aa": 1.315, "soft 120x160 wide": 1.415,
    "soft 100x150 uniform": 1.740, "soft 100x150 own_aa": 1.310, "soft 100x150 wide": 0.895,
    "clamp ties binary": 1.820, "clamp ties uniform": 1.334, "solver step soft 120x160": 1.180,
    "test_fused_matches_oracle 120x160": 0.660, "test_fused_matches_oracle 480x640": 1.763,
    "test_fused_matches_oracle 100x150": 0.963, "span walker": 0.300,
}
# The scenes of tests/link_scenes.py (link counts 1 .. 32, ragged links, sub-tile images), MI355X, 2026-10-19, printed under
#     pytest -m gpu tests/test_gpu_link_scenes.py -s
# (uniform reference unless named; stateless and bound form bit-equal).  Larger than the robots' figures -- up to 5 units, and
# 11 on the 7 x 31 image, the largest of the suite -- and still a quarter of the derived bar.
MEASURED.update({
    "link scene full32": 2.635, "link scene full32 binary": 3.738, "link scene full32 wide": 1.775,
    "link scene full32_lazy": 1.777, "link scene units512": 4.044, "link scene units513": 3.581, "link scene prime7": 2.883,
    "link scene first_empty": 2.030, "link scene last_empty": 1.186, "link scene only_one_live": 1.813,
    "link scene L13x5": 3.368, "link scene L2": 0.550, "link scene L3": 0.548, "link scene L5": 1.324, "link scene L13": 2.740,
    "link scene L17": 4.928, "link scene L31": 1.791, "link scene sub_1x1": 0.000, "link scene sub_1x40": 0.659,
    "link scene sub_3x5": 0.403, "link scene sub_7x31": 11.066, "link scene sub_8x32": 4.011, "link scene sub_9x33": 1.147,
    "link scene sub_5x70": 3.739, "link scene sub_40x4": 1.003, "link scene full32 weights speckle": 1.998,
    "link scene full32 weights tiles": 2.405, "solver step link scene full32": 2.063, "solver step link scene L13": 2.971,
})


def block_bar(A):
    return K_ROUNDINGS * U * np.asarray(A, np.float64)


# ---- the oracle's per-(view, link) images ---------------------------------------------------------------------------------
def link_images(oracle, meshes, mvp, H, W):
    """-> si [B,L,H,W] float32 (GL row order: row 0 = bottom) and parts[b][l] = (pos, rast, colour, faces) for the backward."""
    B, L = mvp.shape[0], mvp.shape[1]
    si = np.zeros((B, L, H, W), np.float32)
    parts = []
    for b in range(B):
        row = []
        for l, (v, f) in enumerate(meshes):
            f = np.ascontiguousarray(f, np.int32)
            pos = oracle.transform_pos(mvp[b, l], v)
            rast, _ = oracle.rasterize(pos, f, [H, W], grad_db=False)
            col = (rast[..., 3:4] != 0).astype(np.float32)
            si[b, l] = oracle.antialias(col, rast, pos, f)[0, :, :, 0]
            row.append((pos, rast, col, f))
        parts.append(row)
    return si, parts


def composite_f64(si, ref):
    """si [B,L,H,W] in GL row order, ref [B,H,W] in image order (row 0 = top).  -> sum32 and gimg in GL row order, mask in image
    order, loss [B] float64."""
    si = np.asarray(si, np.float32)
    s = np.zeros(si.shape[:1] + si.shape[2:], np.float32)
    for l in range(si.shape[1]):                                   # np.float32 accumulation in link order
        s = (s + si[:, l]).astype(np.float32)
    m = np.where(s > np.float32(1), np.float32(1), s).astype(np.float32)
    e = m.astype(np.float64) - np.asarray(ref, np.float32)[:, ::-1].astype(np.float64)
    return types.SimpleNamespace(sum32=s, mask=np.ascontiguousarray(m[:, ::-1]), loss=(e * e).sum(axis=(1, 2)),
                                 gimg=np.where(s <= np.float32(1), 2.0 * e, 0.0))


def grad_mvp_f64(oracle, meshes, parts, gimg):
    """-> G [B,L,4,4] float64 and A [B,L] (see the module docstring)."""
    B, L = len(parts), len(meshes)
    G, A = np.zeros((B, L, 4, 4)), np.zeros((B, L))
    for b in range(B):
        dy = np.ascontiguousarray(gimg[b], np.float32)[None, :, :, None]
        for l, (v, _) in enumerate(meshes):
            pos, rast, col, f = parts[b][l]
            gpos = oracle.antialias_grad(col, rast, pos, f, dy)[1].reshape(-1, 4).astype(np.float64)
            h = np.concatenate([np.asarray(v, np.float64), np.ones((len(v), 1))], axis=1)
            G[b, l] = gpos.T @ h
            A[b, l] = (np.abs(gpos).T @ np.abs(h)).max()
    return G, A


def block_reference(oracle, meshes, mvp, ref):
    """Everything the reference says about one call: the composition and the per-block gradient with its scale."""
    H, W = ref.shape[1], ref.shape[2]
    si, parts = link_images(oracle, meshes, np.asarray(mvp, np.float32), H, W)
    c = composite_f64(si, ref)
    c.si = si
    c.G, c.A = grad_mvp_f64(oracle, meshes, parts, c.gimg)
    return c


def worst_block_ratio(grad, c):
    """max |grad - G| / (2^-24 A) over the blocks with A > 0; blocks with A == 0 must be exactly zero."""
    grad = np.asarray(grad, np.float64)
    dead = c.A == 0
    assert (grad[dead] == 0).all(), "a block the reference gives no gradient has one"
    if dead.all():
        return 0.0
    d = np.abs(grad - c.G).max(axis=(2, 3))
    return float((d[~dead] / (U * c.A[~dead])).max())


def check_blocks(grad, c, what):
    ratio = worst_block_ratio(grad, c)
    print(f"[block ratio] {what}: worst |g - G| / (2^-24 A) = {ratio:.3f} (bar {K_ROUNDINGS})")
    assert ratio <= K_ROUNDINGS, (what, ratio)
    return ratio


def check_against_oracle(mask, loss, grad, e, what):
    """The bars of every case that compares with the oracle (``e``: an ``expected()``)."""
    assert (mask == e.m_ref).all(), what                                          # masks bit-exact
    sse = ((mask.astype(np.float64) - e.ref.astype(np.float64)) ** 2).sum(axis=(1, 2))
    assert (np.abs(loss - sse) <= 1e-6 * np.abs(sse)).all(), what                 # per view, vs the float64 SSE of its own mask
    assert (np.abs(loss - e.l_ref) <= 1e-6 * np.abs(e.l_ref)).all(), what
    assert np.abs(grad - e.g_ref).max() <= 1e-5 * np.abs(e.g_ref).max(), what     # the suite's global bar
    assert (grad[:, :, 2, :] == 0).all(), what
    return check_blocks(grad, e.c, what)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def _scene(name, meshes, mvp, H, W, mvp_gt=None):
    meshes = [(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)) for v, f in meshes]
    return types.SimpleNamespace(name=name, meshes=meshes, mvp=np.ascontiguousarray(mvp, np.float32), H=H, W=W,
                                 B=mvp.shape[0], L=len(meshes), arrays=helpers.scene_arrays(types.SimpleNamespace(meshes=meshes)),
                                 mvp_gt=None if mvp_gt is None else np.ascontiguousarray(mvp_gt, np.float32))


# (H, W, scale of the 1280 x 720 intrinsics, views, zoom, seed of the joint angles): the vector path and the ragged path
# (W % 4 != 0, H % 8 != 0).  At these sizes most of the xArm7's triangles are smaller than a pixel and the antialiasing finds
# no silhouette pair on some links at all; zoom and seed are chosen so that at most a quarter of the (view, link) blocks
# are left without gradient (asserted in tests/test_fused_loss_reference.py).
SOFT_SHAPES = [(120, 160, 0.125, 2, 2.0, 2), (100, 150, 0.12, 3, 2.5, 6)]
SOFT_REFS = ("uniform", "own_aa", "wide")
TIE_REFS = ("binary", "uniform")


def scene_xarm7(robot, H, W, scale, B, zoom, seed):
    """xArm7 at a perturbed camera pose (what a solve starts from); mvp_gt: the unperturbed pose."""
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    K = np.array(scaled_K(XARM7_K_1280x720, scale, W, H, True), dtype=np.float64)
    K[:2, :2] *= zoom
    _, lp = make_views(robot, B, seed=seed)
    Tc = camera_Tc_c2b()
    return _scene(f"xarm7_{H}x{W}x{B}", robot.meshes, helpers.mvp_numpy(K, H, W, perturb_pose(Tc), lp), H, W,
                  mvp_gt=helpers.mvp_numpy(K, H, W, Tc, lp))


TIE_H, TIE_W = 64, 96


def scene_clamp_ties():
    """Four synthetic links under an identity MVP, pixel coordinates through px() (pixel (ix, iy)'s centre is (ix + 0.5, iy + 0.5)):

    (a) links 0 and 1 in alternating stripes that ABUT along slightly slanted shared lines (five near-vertical ones and two
        near-horizontal ones): on a pixel of a shared line link 0 contributes f and link 1 contributes 1 - f, f varying by row,
        and the float32 sum lands on 1.0f or an ulp or two either side;
    (b) link 2 covers a rectangle fully and link 3's silhouette runs inside it (1 + fraction: gate shut) and outside it (gate open);
    (c) a lattice of one-pixel holes, each surrounded by one small triangle of every link: three and four links contribute
        unequal fractions to one uncovered pixel, with the gate open.
    The second view is shifted by a fraction of a pixel."""
    H, W = TIE_H, TIE_W
    quads = [[] for _ in range(4)]

    def px(x, y):
        return [2.0 * x / W - 1.0, 2.0 * y / H - 1.0, 0.0]

    def quad(l, a, b, c, d):
        quads[l].append([px(*a), px(*b), px(*c), px(*d)])

    # (a) stripes between near-vertical lines x = x0 + s (y - 3), rows 3 .. 29; stripe k belongs to link k % 2
    lines = [(3.0, 0.0), (9.31, 0.043), (16.77, -0.061), (23.18, 0.087), (30.62, -0.029), (37.43, 0.071), (44.0, 0.0)]
    y0, y1 = 3.0, 29.0
    for k in range(len(lines) - 1):
        (xa, sa), (xb, sb) = lines[k], lines[k + 1]
        quad(k % 2, (xa, y0), (xb, y0), (xb + sb * (y1 - y0), y1), (xa + sa * (y1 - y0), y1))
    # ... and between near-horizontal lines y = y0 + s (x - 50), columns 50 .. 92
    hl = [(3.0, 0.0), (10.37, 0.052), (18.71, -0.037), (27.0, 0.0)]
    x0, x1 = 50.0, 92.0
    for k in range(len(hl) - 1):
        (ya, sa), (yb, sb) = hl[k], hl[k + 1]
        quad(k % 2, (x0, ya), (x1, ya + sa * (x1 - x0)), (x1, yb + sb * (x1 - x0)), (x0, yb))
    # (b) link 2: a rectangle; link 3: a slanted quad half inside it, half outside
    quad(2, (4.0, 34.0), (40.0, 34.0), (40.0, 60.0), (4.0, 60.0))
    quad(3, (22.3, 38.2), (58.7, 36.4), (60.1, 55.9), (24.9, 57.3))
    # (c) a lattice of 20 one-pixel holes.  Each hole is left uncovered by four small triangles, one per link, whose edges pass
    #     at chosen distances d < 0.5 from the hole's centre: left (link 0), right (1), above (2), below (3).  The hole gains
    #     0.5 - d from each, so three and four links contribute unequal fractions to one uncovered pixel; on most holes the four
    #     gains are drawn to add up to 1 (a thin quad would not do: the antialiasing looks for a pixel's edge in the pixel's
    #     own triangle only)
    rng = np.random.default_rng(1)
    fan = [[] for _ in range(4)]
    k, ext = 2.2, 2.6
    for j in range(4):
        for i in range(5):
            cx, cy = 65.5 + 6 * i, 37.5 + 6 * j
            if rng.uniform() < 0.6:
                while True:
                    g = rng.dirichlet([1.5] * 4)
                    if g.max() < 0.48 and g.min() > 0.01:
                        break
            else:
                g = rng.uniform(0.02, 0.3, 4)
            d = 0.5 - g[rng.permutation(4)]
            s = rng.uniform(-0.04, 0.04, 4) * k
            fan[0].append([px(cx - d[0] - s[0], cy - k), px(cx - d[0] + s[0], cy + k), px(cx - ext, cy)])
            fan[1].append([px(cx + d[1] - s[1], cy - k), px(cx + d[1] + s[1], cy + k), px(cx + ext, cy)])
            fan[2].append([px(cx - k, cy + d[2] - s[2]), px(cx + k, cy + d[2] + s[2]), px(cx, cy + ext)])
            fan[3].append([px(cx - k, cy - d[3] - s[3]), px(cx + k, cy - d[3] + s[3]), px(cx, cy - ext)])
    meshes = []
    for l in range(4):
        n = len(quads[l])
        v = np.asarray(quads[l], np.float32).reshape(-1, 3)
        f = [[4 * i, 4 * i + 1, 4 * i + 2] for i in range(n)] + [[4 * i, 4 * i + 2, 4 * i + 3] for i in range(n)]
        f += [[4 * n + 3 * i, 4 * n + 3 * i + 1, 4 * n + 3 * i + 2] for i in range(len(fan[l]))]
        meshes.append((np.concatenate([v, np.asarray(fan[l], np.float32).reshape(-1, 3)]), np.asarray(f, np.int32)))
    mvp = np.tile(np.eye(4, dtype=np.float32)[None, None], (2, 4, 1, 1))
    mvp[1, :, 0, 3] = 0.37 / W
    mvp[1, :, 1, 3] = -0.61 / H
    return _scene("clamp_ties_64x96", meshes, mvp, H, W)


def reference_mask(oracle, s, kind, seed=0):
    """The reference masks of the cases, [B,H,W] float32 in image order."""
    rng = np.random.default_rng(1000 * s.H + s.W + seed)
    shape = (s.B, s.H, s.W)
    if kind == "uniform":
        return rng.uniform(size=shape).astype(np.float32)
    if kind == "binary":
        return (rng.uniform(size=shape) > 0.5).astype(np.float32)
    if kind == "wide":
        return rng.uniform(-0.5, 2.0, size=shape).astype(np.float32)
    if kind == "own_aa":   # the oracle's antialiased mask at the unperturbed pose: e == 0 on many pixels, fractional on the silhouette
        verts, tris, toff, voff = s.arrays
        return oracle.render_mask_loss(verts, tris, toff, voff, s.mvp_gt, np.zeros(shape, np.float32), want_grad=False)[0]
    raise KeyError(kind)


def expected(oracle, s, ref):
    """The oracle's fused result on scene ``s`` and reference ``ref`` plus the float64 composition of the same call."""
    verts, tris, toff, voff = s.arrays
    e = types.SimpleNamespace(s=s, ref=np.ascontiguousarray(ref, np.float32))
    e.m_ref, e.l_ref, e.g_ref = oracle.render_mask_loss(verts, tris, toff, voff, s.mvp, e.ref)
    e.c = block_reference(oracle, s.meshes, s.mvp, e.ref)
    return e


_CACHE = {}


def scene_for(robot, key):
    """key: ("xarm7",) + an entry of SOFT_SHAPES, or ("ties",); built once per process."""
    if key not in _CACHE:
        _CACHE[key] = scene_clamp_ties() if key[0] == "ties" else scene_xarm7(robot, *key[1:])
    return _CACHE[key]


def expected_for(oracle, robot, key, kind):
    """``expected()`` of (scene key, reference kind), computed once per process and never written to."""
    k = (key, kind)
    if k not in _CACHE:
        s = scene_for(robot, key)
        _CACHE[k] = expected(oracle, s, reference_mask(oracle, s, kind))
    return _CACHE[k]


def tie_counts(c):
    """The clamp-tie conditions on a composition: pixels with two or more contributing links whose float32 sum is exactly 1, in
    (1, 1 + 4e-7], in [1 - 4e-7, 1); pixels with a sum of 1.5 or more; pixels with three or more contributing links."""
    n = (c.si != 0).sum(axis=1)
    s = c.sum32.astype(np.float64)
    two = n >= 2
    return {"one": int((two & (c.sum32 == np.float32(1))).sum()), "above": int((two & (s > 1) & (s <= 1 + 4e-7)).sum()),
            "below": int((two & (s < 1) & (s >= 1 - 4e-7)).sum()), "high": int((s >= 1.5).sum()), "three": int((n >= 3).sum())}
