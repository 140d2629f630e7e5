"""Float64 reference of the backward passes of dr.rasterize and dr.interpolate (csrc/ehr_raster.hip, csrc/ehr_interp_aa.hip)
and the scenes their tests sweep.  CPU only, numpy and torch-CPU, not collected by pytest.

The reference never decides coverage: it takes the triangle ids from ``rast[..., 3]`` and (u, v) from ``rast[..., :2]`` of the
oracle's image and evaluates the ops' formulas per covered pixel:

    interpolate              out = u a0 + v a1 + (1-u-v) a2;  grad_attr by np.add.at;  grad_rast = (sum dy (a0-a2), sum dy (a1-a2), 0, 0)
    pixel differentials      d attr/dX = du/dX (a0-a2) + dv/dX (a1-a2), gradients to attr and to rast_db
    d(u, v)/d pos            torch float64 autograd over  b0 = a0 / (at + copysign(1e-6, at))  (the guard is part of the op)
    d rast_db/d pos          torch float64 autograd over the four expressions of the shading (oracle/ehr_oracle.c, shade_pixel)

dr.antialias has no float64 twin: its pair analysis is a decision procedure, a second implementation would be a second oracle.
It stays on the oracle, which finite differences pin (tests/test_oracle_antialias.py, tests/test_ops_reference.py).

ORACLE_VS_F64 is the worst  max|oracle - f64| / max(1, max|f64|)  of the oracle's float32 backward passes over ``scenes()``
with the inputs of ``expected()``; the kernels are not involved.  tests/test_ops_reference.py holds the oracle within 2x of
it, tests/test_gpu_ops_grad.py holds the kernels within 4x of it (float32 atomics sum in arbitrary order where the oracle sums
serially; the number of addends per vertex differs by case).  Measured 2026-10-17 with

    pytest -m "not gpu" tests/test_ops_reference.py -s -k oracle_backward
"""
import types

import numpy as np
import torch

import helpers

ORACLE_VS_F64 = {
    "rasterize_grad": 5.63e-04,
    "rasterize_grad_db": 1.51e-05,
    "interpolate_grad_attr": 1.87e-06,
    "interpolate_grad_rast": 1.33e-07,
    "interpolate_da_grad_attr": 4.53e-07,
    "interpolate_da_grad_db": 8.96e-08,
}

# what the suite already asks of each quantity against the oracle (tests/test_gpu_ops.py), relative to max(1, max|ref|)
SUITE_TOL = {
    "rasterize_grad": 1e-5,
    "rasterize_grad_db": 1e-4,
    "interpolate_grad_attr": 1e-5,
    "interpolate_grad_rast": 1e-5,
    "interpolate_da_grad_attr": 1e-5,
    "interpolate_da_grad_db": 1e-6,
    "antialias_grad_pos": 1e-5,
    "antialias_grad_color": 1e-5,
}


def f64_bound(quantity):
    """The kernels' bound against the float64 reference, relative to max(1, max|ref|)."""
    e = ORACLE_VS_F64[quantity]
    return 4.0 * e if e > 0 else SUITE_TOL[quantity]


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


# ---- what a pixel refers to ---------------------------------------------------------------------------------------------
def triangle_ids(rast):
    """rast[..., 3] -> triangle id + 1 as int64 (ids above 2^24 are stored as bit patterns offset by 0x4a800000)."""
    f = np.ascontiguousarray(rast[..., 3], dtype=np.float32)
    big = f > 16777216.0
    return np.where(big, f.view(np.int32).astype(np.int64) - 0x4A800000, np.where(big, 0, f).astype(np.int64))


def _pixels(rast, tri, V):
    """Covered pixels: image, row, column and the three vertex indices of each.  A pixel whose id is 0, is > T or whose
    triangle refers to a vertex outside [0, V) is not covered."""
    tri = np.asarray(tri, np.int64)
    ids = triangle_ids(rast)
    ok = (ids >= 1) & (ids <= tri.shape[0])
    vi = tri[np.where(ok, ids - 1, 0)] if tri.shape[0] else np.zeros(ids.shape + (3,), np.int64)
    ok &= ((vi >= 0) & (vi < V)).all(-1)
    b, iy, ix = np.nonzero(ok)
    return b, iy, ix, vi[b, iy, ix]


def _attr3(attr):
    attr = np.asarray(attr, np.float64)
    return attr[None] if attr.ndim == 2 else attr


# ---- interpolate ------------------------------------------------------------------------------------------------------
def interpolate(attr, rast, tri):
    attr = _attr3(attr)
    Ba, V, A = attr.shape
    b, iy, ix, vi = _pixels(rast, tri, V)
    ab = b if Ba > 1 else np.zeros_like(b)
    u, v = rast[b, iy, ix, 0].astype(np.float64), rast[b, iy, ix, 1].astype(np.float64)
    out = np.zeros(rast.shape[:3] + (A,), np.float64)
    out[b, iy, ix] = (u[:, None] * attr[ab, vi[:, 0]] + v[:, None] * attr[ab, vi[:, 1]]
                      + (1.0 - u - v)[:, None] * attr[ab, vi[:, 2]])
    return out


def interpolate_grad(attr, rast, tri, dy):
    """-> (grad_attr [Ba,V,A], grad_rast [B,H,W,4])."""
    attr = _attr3(attr)
    Ba, V, A = attr.shape
    b, iy, ix, vi = _pixels(rast, tri, V)
    ab = b if Ba > 1 else np.zeros_like(b)
    u, v = rast[b, iy, ix, 0].astype(np.float64), rast[b, iy, ix, 1].astype(np.float64)
    d = np.asarray(dy, np.float64)[b, iy, ix]                                   # [N, A]
    ga = np.zeros_like(attr)
    for k, w in enumerate((u, v, 1.0 - u - v)):
        np.add.at(ga, (ab, vi[:, k]), w[:, None] * d)
    a0, a1, a2 = attr[ab, vi[:, 0]], attr[ab, vi[:, 1]], attr[ab, vi[:, 2]]
    gr = np.zeros(rast.shape, np.float64)
    gr[b, iy, ix, 0] = (d * (a0 - a2)).sum(-1)
    gr[b, iy, ix, 1] = (d * (a1 - a2)).sum(-1)
    return ga, gr


def _diff_index(diff_attrs, A):
    return np.arange(A) if isinstance(diff_attrs, str) else np.asarray(diff_attrs, np.int64)


def interpolate_da(attr, rast, rast_db, tri, diff_attrs="all"):
    """Attribute pixel differentials [B,H,W,2D]: (d/dX, d/dY) of attribute diff_attrs[i] at channels 2i, 2i+1."""
    attr = _attr3(attr)
    Ba, V, A = attr.shape
    idx = _diff_index(diff_attrs, A)
    b, iy, ix, vi = _pixels(rast, tri, V)
    ab = b if Ba > 1 else np.zeros_like(b)
    db = np.asarray(rast_db, np.float64)[b, iy, ix]                              # (du/dX, du/dY, dv/dX, dv/dY)
    a2 = attr[ab, vi[:, 2]][:, idx]
    d0, d1 = attr[ab, vi[:, 0]][:, idx] - a2, attr[ab, vi[:, 1]][:, idx] - a2     # [N, D]
    o = np.zeros((b.shape[0], 2 * idx.shape[0]), np.float64)
    o[:, 0::2] = db[:, 0:1] * d0 + db[:, 2:3] * d1
    o[:, 1::2] = db[:, 1:2] * d0 + db[:, 3:4] * d1
    out = np.zeros(rast.shape[:3] + (2 * idx.shape[0],), np.float64)
    out[b, iy, ix] = o
    return out


def interpolate_da_grad(attr, rast, rast_db, tri, dy_da, diff_attrs="all"):
    """-> (grad_attr [Ba,V,A], grad_rast_db [B,H,W,4]); the differentials do not depend on (u, v)."""
    attr = _attr3(attr)
    Ba, V, A = attr.shape
    idx = _diff_index(diff_attrs, A)
    b, iy, ix, vi = _pixels(rast, tri, V)
    ab = b if Ba > 1 else np.zeros_like(b)
    db = np.asarray(rast_db, np.float64)[b, iy, ix]
    g = np.asarray(dy_da, np.float64)[b, iy, ix]
    gx, gy = g[:, 0::2], g[:, 1::2]                                              # [N, D]
    a2 = attr[ab, vi[:, 2]][:, idx]
    d0, d1 = attr[ab, vi[:, 0]][:, idx] - a2, attr[ab, vi[:, 1]][:, idx] - a2
    gdb = np.zeros(rast.shape, np.float64)
    gdb[b, iy, ix] = np.stack([(gx * d0).sum(-1), (gy * d0).sum(-1), (gx * d1).sum(-1), (gy * d1).sum(-1)], axis=1)
    c0 = gx * db[:, 0:1] + gy * db[:, 1:2]                                       # d / d(a0 - a2)
    c1 = gx * db[:, 2:3] + gy * db[:, 3:4]                                       # d / d(a1 - a2)
    ga = np.zeros_like(attr)
    cols = np.broadcast_to(idx[None, :], c0.shape)
    for k, c in enumerate((c0, c1, -(c0 + c1))):
        np.add.at(ga, (ab[:, None], vi[:, k][:, None], cols), c)
    return ga, gdb


# ---- rasterize: (u, v) and rast_db as functions of pos ----------------------------------------------------------------
def _shade(pos, tri, rast, range_mode):
    """Per covered pixel, as torch float64 functions of ``pos``: uv [N,2] with the 1e-6 guard, db [N,4] without it (as the
    shading computes it); neither clamps the barycentrics.  Also the pixels' (image, row, column)."""
    V = pos.shape[-2]
    H, W = rast.shape[1], rast.shape[2]
    b, iy, ix, vi = _pixels(rast, tri, V)
    first = np.zeros_like(b) if range_mode else b * V                            # voff
    P = pos.reshape(-1, 4)[torch.as_tensor(first[:, None] + vi)]                 # [N, 3, 4]
    X, Y, Wc = P[..., 0], P[..., 1], P[..., 3]
    fx = torch.as_tensor((2.0 * ix + 1.0) / W - 1.0)[:, None]
    fy = torch.as_tensor((2.0 * iy + 1.0) / H - 1.0)[:, None]
    px, py = X - fx * Wc, Y - fy * Wc
    a0 = px[:, 1] * py[:, 2] - py[:, 1] * px[:, 2]
    a1 = px[:, 2] * py[:, 0] - py[:, 2] * px[:, 0]
    a2 = px[:, 0] * py[:, 1] - py[:, 0] * px[:, 1]
    at = (a0 + a1) + a2
    guarded = at + torch.copysign(torch.full_like(at, 1e-6), at.detach())
    uv = torch.stack([a0 / guarded, a1 / guarded], dim=1)
    iw = 1.0 / at
    b0, b1 = a0 * iw, a1 * iw
    dfx, dfy = (2.0 / W) * iw, (2.0 / H) * iw
    da0x, da0y = Y[:, 2] * Wc[:, 1] - Y[:, 1] * Wc[:, 2], X[:, 1] * Wc[:, 2] - X[:, 2] * Wc[:, 1]
    da1x, da1y = Y[:, 0] * Wc[:, 2] - Y[:, 2] * Wc[:, 0], X[:, 2] * Wc[:, 0] - X[:, 0] * Wc[:, 2]
    da2x, da2y = Y[:, 1] * Wc[:, 0] - Y[:, 0] * Wc[:, 1], X[:, 0] * Wc[:, 1] - X[:, 1] * Wc[:, 0]
    datx, daty = (da0x + da1x) + da2x, (da0y + da1y) + da2y
    db = torch.stack([dfx * (b0 * datx - da0x), dfy * (b0 * daty - da0y),
                      dfx * (b1 * datx - da1x), dfy * (b1 * daty - da1y)], dim=1)
    return uv, db, (b, iy, ix)


def _dense(vals, where, shape):
    out = np.zeros(shape, np.float64)
    out[where] = vals.detach().numpy()
    return out


def rasterize_uv(pos, tri, rast, range_mode=False):
    """(u, v) [B,H,W,2] of the triangles ``rast`` names, unclamped."""
    uv, _, where = _shade(torch.as_tensor(np.asarray(pos, np.float64)), tri, rast, range_mode)
    return _dense(uv, where, rast.shape[:3] + (2,))


def rasterize_db(pos, tri, rast, range_mode=False):
    """(du/dX, du/dY, dv/dX, dv/dY) [B,H,W,4] of the triangles ``rast`` names, from unclamped (u, v)."""
    _, db, where = _shade(torch.as_tensor(np.asarray(pos, np.float64)), tri, rast, range_mode)
    return _dense(db, where, rast.shape[:3] + (4,))


def _pos_grad(pos, tri, rast, g, range_mode, which):
    p = torch.as_tensor(np.asarray(pos, np.float64)).clone().requires_grad_(True)
    uv, db, where = _shade(p, tri, rast, range_mode)
    g = torch.as_tensor(np.asarray(g, np.float64)[where])
    loss = (uv * g[:, :2]).sum() if which == "uv" else (db * g).sum()
    (gp,) = torch.autograd.grad(loss, p)
    return gp.numpy()                                                            # (z is never read: its column is zero)


def rasterize_grad(pos, tri, rast, dy, range_mode=False):
    """d(u, v)/d pos contracted with dy [B,H,W,4] (only its first two channels count); pos's shape."""
    return _pos_grad(pos, tri, rast, dy, range_mode, "uv")


def rasterize_grad_db(pos, tri, rast, ddb, range_mode=False):
    """d rast_db/d pos contracted with ddb [B,H,W,4]; pos's shape."""
    return _pos_grad(pos, tri, rast, ddb, range_mode, "db")


# ---- the scenes the gradient tests sweep --------------------------------------------------------------------------------
def _scene(name, pos, tri, H, W, ranges=None, **kw):
    s = types.SimpleNamespace(name=name, pos=np.ascontiguousarray(pos, np.float32), tri=np.ascontiguousarray(tri, np.int32),
                              H=H, W=W, ranges=None if ranges is None else np.asarray(ranges, np.int32),
                              empty=(), min_covered=None, **kw)
    s.range_mode = ranges is not None
    s.B = s.pos.shape[0] if ranges is None else s.ranges.shape[0]
    s.V = s.pos.shape[-2]
    return s


def scene_instance(H, W):
    """a: instance mode, three different vertex sets of one random mesh."""
    rng = np.random.default_rng(H * 1000 + W)
    pos, tri = helpers.random_mesh(rng, 150 if H < 100 else 1500)
    posb = np.stack([pos, pos * np.array([1, -1, 1, 1], np.float32), pos[::-1].copy()])
    s = _scene(f"instance_{H}x{W}", posb, tri, H, W)
    s.min_covered = [H * W // 4] * 3
    return s


def scene_middle_empty(H, W):
    """b: a small object in images 0 and 2 (most 32 x 8 tiles stay empty), image 1 wholly behind the eye plane."""
    rng = np.random.default_rng(H * 1000 + W + 1)
    pos, tri = helpers.random_mesh(rng, 300, shared=True, size=0.12)
    imgs = []
    for centre in ((0.4, -0.3), None, (-0.35, 0.3)):
        p = pos.copy()
        if centre is None:
            p = -p                                                               # w < 0 at every vertex
        else:
            p[:, 0] = p[:, 0] * 0.35 + centre[0] * p[:, 3]
            p[:, 1] = p[:, 1] * 0.35 + centre[1] * p[:, 3]
        imgs.append(p)
    s = _scene(f"middle_empty_{H}x{W}", np.stack(imgs), tri, H, W)
    s.empty = (1,)
    s.min_covered = [200, 0, 200]
    return s


def scene_xarm7_links(oracle, robot):
    """c: the layout of rb_solver._batched_topology -- 2 frames x all links at 120 x 160, one image per (frame, link), one
    concatenated vertex array, triangles shifted per image, one (start, count) range per image."""
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, scaled_K
    H, W = 120, 160
    K = scaled_K(XARM7_K_1280x720, 0.125, W, H, True)
    _, lp = make_views(robot, 2, seed=1)
    mvp = helpers.mvp_numpy(K, H, W, camera_Tc_c2b(), lp)
    pos, tris, ranges, voff, toff = [], [], [], 0, 0
    for f in range(2):
        for l, (v, faces) in enumerate(robot.meshes):
            pos.append(oracle.transform_pos(mvp[f, l], v)[0])
            tris.append(np.asarray(faces, np.int32) + voff)
            ranges.append((toff, faces.shape[0]))
            voff += v.shape[0]
            toff += faces.shape[0]
    s = _scene("xarm7_links_120x160", np.concatenate(pos), np.concatenate(tris), H, W, ranges=ranges)
    s.min_covered = [30] * s.B
    return s


def scene_ragged_ranges():
    """d: range mode on one random mesh: the whole mesh, an interior slice, the last triangle alone, nothing."""
    rng = np.random.default_rng(11)
    pos, tri = helpers.random_mesh(rng, 120)
    T = tri.shape[0]
    s = _scene("ragged_ranges_50x83", pos, tri, 50, 83, ranges=[[0, T], [10, 50], [T - 1, 1], [0, 0]])
    s.empty = (3,)
    s.min_covered = [1000, 500, 10, 0]
    return s


def scene_db_range():
    """e (range mode): three images over shifted copies of one mesh, as many vertex slices in one array."""
    rng = np.random.default_rng(31)
    pos, tri = helpers.random_mesh(rng, 200)
    V, T = pos.shape[0], tri.shape[0]
    posb = np.concatenate([pos + np.float32(0.03 * i) * np.array([1, -1, 0, 0], np.float32) for i in range(3)])
    trib = np.concatenate([tri + i * V for i in range(3)])
    s = _scene("db_range_56x88", posb, trib, 56, 88, ranges=[[i * T, T] for i in range(3)])
    s.min_covered = [56 * 88 // 4] * 3
    return s


def scene_db_instance():
    """e (instance mode)."""
    s = scene_instance(56, 88)
    s.name = "db_instance_56x88"
    return s


def scenes(oracle, robot):
    """Every scene of tests/test_gpu_ops_grad.py (the case list ORACLE_VS_F64 is measured over)."""
    return [scene_instance(75, 101), scene_instance(200, 328), scene_middle_empty(75, 101), scene_middle_empty(200, 328),
            scene_xarm7_links(oracle, robot), scene_ragged_ranges(), scene_db_instance(), scene_db_range()]


def image_vertices(s, b):
    """Indices into the flat [*, 4] gradient of the vertices image ``b`` can touch."""
    if not s.range_mode:
        return np.arange(b * s.V, (b + 1) * s.V)
    t0, n = int(s.ranges[b, 0]), int(s.ranges[b, 1])
    return np.unique(s.tri[t0:t0 + n])


def half_zero_pairs(rng, shape):
    """A gradient for the pixel differentials in which about half of the (d/dX, d/dY) pairs are exactly zero."""
    g = rng.normal(size=shape).astype(np.float32)
    keep = rng.uniform(size=shape[:-1] + (shape[-1] // 2,)) < 0.5
    return g * np.repeat(keep, 2, axis=-1)


def expected(oracle, s, Ba, A, seed=0, diff_attrs=None):
    """The oracle's chain rasterize -> interpolate -> antialias and its backward on scene ``s`` with seeded attributes
    [Ba, V, A] and incoming gradients, and the float64 reference of every rasterize / interpolate gradient FOR THE SAME
    incoming gradient (the oracle's).  With ``diff_attrs`` also rast_db's and the pixel differentials' gradients."""
    rng = np.random.default_rng(seed)
    e = types.SimpleNamespace(s=s, Ba=Ba, A=A)
    rm = s.range_mode
    e.rast, e.db = oracle.rasterize(s.pos, s.tri, [s.H, s.W], ranges=s.ranges)
    e.attr = rng.uniform(0, 1, size=(Ba, s.V, A)).astype(np.float32)
    e.col = oracle.interpolate(e.attr, e.rast, s.tri)
    e.aa = oracle.antialias(e.col, e.rast, s.pos, s.tri)
    e.dy = rng.normal(size=e.aa.shape).astype(np.float32)
    e.g_col, e.gp_aa = oracle.antialias_grad(e.col, e.rast, s.pos, s.tri, e.dy)
    e.g_attr, e.g_rast = oracle.interpolate_grad(e.attr, e.rast, s.tri, e.g_col)
    e.gp_uv = oracle.rasterize_grad(s.pos, s.tri, e.rast, e.g_rast, rm)
    e.g_attr64, e.g_rast64 = interpolate_grad(e.attr, e.rast, s.tri, e.g_col)
    e.gp_uv64 = rasterize_grad(s.pos, s.tri, e.rast, e.g_rast, rm)
    if diff_attrs is not None:
        e.ddb = rng.normal(size=e.db.shape).astype(np.float32)
        e.gp_db = oracle.rasterize_grad_db(s.pos, s.tri, e.rast, e.ddb, rm)
        e.gp_db64 = rasterize_grad_db(s.pos, s.tri, e.rast, e.ddb, rm)
        e.da = oracle.interpolate_da(e.attr, e.rast, e.db, s.tri, diff_attrs)
        e.dy_da = half_zero_pairs(rng, e.da.shape)
        e.g_attr_da, e.g_db = oracle.interpolate_da_grad(e.attr, e.rast, e.db, s.tri, e.dy_da, diff_attrs)
        e.g_attr_da64, e.g_db64 = interpolate_da_grad(e.attr, e.rast, e.db, s.tri, e.dy_da, diff_attrs)
    return e


def oracle_errors(e):
    """{quantity: relative error of the oracle against the float64 reference} for one ``expected()``."""
    out = {"rasterize_grad": rel_err(e.gp_uv, e.gp_uv64), "interpolate_grad_attr": rel_err(e.g_attr, e.g_attr64),
           "interpolate_grad_rast": rel_err(e.g_rast, e.g_rast64)}
    if hasattr(e, "ddb"):
        out.update({"rasterize_grad_db": rel_err(e.gp_db, e.gp_db64), "interpolate_da_grad_attr": rel_err(e.g_attr_da, e.g_attr_da64),
                    "interpolate_da_grad_db": rel_err(e.g_db, e.g_db64)})
    return out


def check_preconditions(e):
    """A case must not pass vacuously: coverage per non-empty image, one blended pair per non-empty image, nothing in the
    images the scene calls empty."""
    s = e.s
    cov = (triangle_ids(e.rast) > 0).reshape(s.B, -1).sum(1)
    gflat = np.abs(e.gp_aa.reshape(-1, 4))
    for b in range(s.B):
        if b in s.empty:
            assert cov[b] == 0, (s.name, b, int(cov[b]))
        else:
            assert cov[b] > s.min_covered[b], (s.name, b, int(cov[b]), s.min_covered[b])
            assert gflat[image_vertices(s, b)].max() > 0, (s.name, b, "no blended pair")
    return cov


def empty_tiles(rast, b):
    """Number of 32 x 8 tiles of image ``b`` no triangle was drawn in (what the rasterizer's tile flags mark)."""
    ids = triangle_ids(rast)[b]
    H, W = ids.shape
    n = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 32):
            n += not (ids[ty:ty + 8, tx:tx + 32] > 0).any()
    return n


CASES_A = [(Ba, A) for Ba in (3, 1) for A in (1, 3, 7)]        # attribute layouts of cases a and b (Ba = 3 is Ba = B)
DIFF_SELECTIONS = ("all", (2, 0))


def case_list():
    """(scene name, Ba, A, diff_attrs) of every ``expected()`` tests/test_gpu_ops_grad.py compares the kernels with."""
    out = [(n, Ba, A, None) for n in ("instance_75x101", "instance_200x328", "middle_empty_75x101", "middle_empty_200x328")
           for Ba, A in CASES_A]
    out += [("xarm7_links_120x160", 1, 3, None), ("ragged_ranges_50x83", 1, 3, None)]
    out += [(n, Ba, 3, sel) for n in ("db_instance_56x88", "db_range_56x88") for Ba in (1, 3) for sel in DIFF_SELECTIONS]
    return out


_EXPECTED = {}


def expected_for(oracle, robot, name, Ba, A, diff_attrs=None):
    """``expected()`` of one entry of ``case_list()``, seeded by the entry, computed once per process."""
    key = (name, Ba, A, diff_attrs)
    if key not in _EXPECTED:
        if "scenes" not in _EXPECTED:
            _EXPECTED["scenes"] = {s.name: s for s in scenes(oracle, robot)}
        sel = list(diff_attrs) if isinstance(diff_attrs, tuple) else diff_attrs
        _EXPECTED[key] = expected(oracle, _EXPECTED["scenes"][name], Ba, A, seed=100 * Ba + A, diff_attrs=sel)
    return _EXPECTED[key]
