"""numpy reference of the pose search's soft score: the capped squared Euclidean distance transform
in two forms (brute force over every foreground pixel; the separable exact form), the cost images, the cost sums under a
set of masks and the displacement ladder of the issue through the CPU oracle.  Integers throughout; the only float is
the final quotient."""
import numpy as np

import helpers

BRUTE_MAX = 40 * 70     # above this many pixels the separable form is the reference
LADDER_DX = (0.0, 0.05, 0.1, 0.2, 0.3, 0.45, 0.6, 0.8, 1.2, 3.0)    # metres along the camera's x axis


def foreground(ref):
    """ehr_mask_overlap's rule: foreground iff ref > 0.5f; NaN compares false and is background."""
    with np.errstate(invalid="ignore"):
        return np.asarray(ref, np.float32) > np.float32(0.5)


def edt_brute(fg, cap):
    """[H,W] bool -> int64 [H,W]: min(cap^2, min over the foreground of dx^2 + dy^2), every pair looked at."""
    H, W = fg.shape
    out = np.full((H, W), cap * cap, np.int64)
    ys, xs = np.nonzero(fg)
    if len(ys) == 0:
        return out
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2
    return np.minimum(out, d.min(axis=-1))


def edt_separable(fg, cap):
    """The same integers in the separable form: per column the distance g to the nearest foreground pixel of the column
    (a large number where it has none), then per row min over x' of (x - x')^2 + g[x']^2."""
    H, W = fg.shape
    far = 1 << 20
    g = np.full((H, W), far, np.int64)
    d = np.full(W, far, np.int64)
    for y in range(H):
        d = np.where(fg[y], 0, np.minimum(d + 1, far))
        g[y] = d
    d = np.full(W, far, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(fg[y], 0, np.minimum(d + 1, far))
        g[y] = np.minimum(g[y], d)
    x = np.arange(W)
    dx2 = (x[:, None] - x[None, :]) ** 2                       # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + (g[y] ** 2)[None, :]).min(axis=1)
    return np.minimum(out, cap * cap)


def edt(ref, cap):
    """ref [S,H,W] float -> int64 [S,H,W], by brute force where the image is small enough."""
    fg = foreground(ref)
    f = edt_brute if fg.shape[1] * fg.shape[2] <= BRUTE_MAX else edt_separable
    return np.stack([f(m, cap) for m in fg])


def isqrt(n):
    """floor(sqrt(n)) of non-negative int64, corrected in integers."""
    n = np.asarray(n, np.int64)
    r = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > n, r - 1, r)
    return np.where((r + 1) * (r + 1) <= n, r + 1, r)


def soft_costs(ref, cap, valid=None):
    """int64 [C,S,H,W]: [fg, k] with k = cap - floor(sqrt(d2)), or [fg & valid, k valid, valid]."""
    d2 = edt(ref, cap)
    fg = (d2 == 0).astype(np.int64)
    k = cap - isqrt(d2)
    if valid is None:
        return np.stack([fg, k])
    v = np.asarray(valid).astype(np.int64)
    return np.stack([fg * v, k * v, v])


def cost_sums(masks, cost):
    """masks [Q,S,H,W] bool, cost [C,S,H,W] integers -> (area [Q,S], sums [Q,S,C]) int64 (python-exact: int64 cannot
    overflow below 2^30 pixels of int32 values)."""
    cost = np.asarray(cost).astype(np.int64)
    area = masks.sum(axis=(2, 3)).astype(np.int64)
    sums = np.stack([(masks * cost[c][None]).sum(axis=(2, 3)) for c in range(cost.shape[0])], axis=-1).astype(np.int64)
    return area, sums


def soft_from_integers(area, inter, ksum, ref_area, cap):
    """float64 [Q]: mean over the views of ksum / (cap union), 1.0 where the union is empty."""
    union = area + ref_area[None] - inter
    per = np.where(union > 0, ksum.astype(np.float64) / (float(cap) * np.maximum(union, 1).astype(np.float64)), 1.0)
    return per.mean(axis=1)


def soft_scores(masks, ref, cap, valid=None):
    """dict(area, inter, ksum, ref_area, soft, xor) of bool masks [Q,S,H,W] against ref [S,H,W] (restricted to valid)."""
    cost = soft_costs(ref, cap, valid)
    area, sums = cost_sums(masks, cost)
    if valid is not None:
        area = sums[..., 2]
    inter, ksum = sums[..., 0], sums[..., 1]
    ref_area = cost[0].sum(axis=(1, 2))
    return dict(area=area, inter=inter, ksum=ksum, ref_area=ref_area, soft=soft_from_integers(area, inter, ksum, ref_area, cap),
                xor=(area + ref_area[None] - 2 * inter).sum(axis=1))


def oracle_masks(oracle, robot, mvp, H, W):
    """bool [Q,S,H,W] (row 0 = top): the oracle's non-antialiased masks of mvp [Q,S,L,4,4]."""
    Q, S, L = mvp.shape[:3]
    verts, tris, _, _ = helpers.scene_arrays(robot)
    vl = np.concatenate([np.full(v.shape[0], l, np.int32) for l, (v, _) in enumerate(robot.meshes)])
    _, c = oracle.mask_variance(verts, tris, vl, np.ascontiguousarray(mvp.reshape(Q * S, 1, L, 4, 4)), H, W, return_counts=True)
    assert c.max() <= 1
    return c.reshape(Q, S, H, W) > 0


def ladder_poses():
    """[10,4,4] float64: shift_x(dx) @ Tc_gt for the rungs of LADDER_DX; rung 0 is the ground truth."""
    from easyhec_amd.synthetic import camera_Tc_c2b
    Tc_gt = camera_Tc_c2b()
    out = []
    for dx in LADDER_DX:
        sh = np.eye(4)
        sh[0, 3] = dx
        out.append(sh @ Tc_gt)
    return np.stack(out)


_LADDER = {}


def ladder(oracle, robot):
    """The issue's setup, computed once: xArm7 at 120x160, three views, the ten rungs; the reference is rung 0's own
    masks.  -> dict(H, W, K, link_poses, poses, mvp [10,3,L,4,4], masks [10,3,H,W], ref [3,H,W] float32)."""
    if not _LADDER:
        from easyhec_amd.config import XARM7_K_1280x720
        from easyhec_amd.synthetic import make_views, scaled_K
        H, W = 120, 160
        K = scaled_K(XARM7_K_1280x720, 0.125, W, H, True)
        _, lp = make_views(robot, 3, seed=3)
        poses = ladder_poses()
        mvp = np.stack([helpers.mvp_numpy(K, H, W, Tc, lp) for Tc in poses])
        masks = oracle_masks(oracle, robot, mvp, H, W)
        _LADDER.update(H=H, W=W, K=K, link_poses=lp, poses=poses, mvp=mvp, masks=masks, ref=masks[0].astype(np.float32))
    return _LADDER
