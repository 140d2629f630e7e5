"""Pins tests/ops_reference.py, the float64 reference of dr.rasterize's and dr.interpolate's backward passes, and measures the
oracle's float32 backward passes against it.  CPU only: no kernel is involved.

  * the reference's gradients equal central differences of its own forward functions, in instance mode (B = 2) and in
    range mode (two images over one vertex array);
  * the oracle stays within 2x of ORACLE_VS_F64 over the case list of tests/test_gpu_ops_grad.py;
  * oracle.antialias_grad in range mode equals finite differences of oracle.antialias where one vertex takes gradient from
    two images."""
import numpy as np
import pytest

import helpers
import ops_reference as R

# Central differences in float64 with step E: truncation E^2/6 |f'''|, rounding ~1e-16 |f| / E.  The forwards are rational in
# pos with the triangle's doubled area `at` as denominator (asserted >= 1e-2 below: |f'''| <= ~1e7 per unit of incoming
# gradient, a few hundred pixels each), bilinear in everything else: both terms stay under 1e-4 of the gradient's scale.
E = 1e-5
FD_TOL = 1e-4


def small_scene(oracle, range_mode):
    """12 large triangles over 8 shared vertices at 32 x 40; B = 2 images: two vertex sets (instance mode) or the whole
    mesh and its second half over one vertex array (range mode)."""
    rng = np.random.default_rng(4)
    pos, tri = helpers.random_mesh(rng, 12)
    if range_mode:
        ranges = np.array([[0, 12], [6, 6]], np.int32)
    else:
        pos, ranges = np.stack([pos, pos * np.array([1, -1, 1, 1], np.float32)]), None
    rast, db = oracle.rasterize(pos, tri, [32, 40], ranges=ranges)
    assert ((rast[..., 3] > 0).reshape(2, -1).sum(1) > 150).all()
    return rng, pos, tri, ranges, rast, db


def qualifying_vertices(oracle, pos, tri, ranges, rast):
    """Flat indices of the vertices of drawn triangles, and of those whose +-E moves (x, y or w) change no triangle id."""
    ids = R.triangle_ids(rast)
    V = pos.shape[-2]
    touched = set()
    for b in range(ids.shape[0]):
        for t in np.unique(ids[b][ids[b] > 0]) - 1:
            touched.update((0 if ranges is not None else b * V) + int(v) for v in tri[t])
    good = []
    for fv in sorted(touched):
        same = True
        for c in (0, 1, 3):
            for sgn in (1.0, -1.0):
                p = pos.astype(np.float64).reshape(-1, 4).copy()
                p[fv, c] += sgn * E
                r, _ = oracle.rasterize(p.reshape(pos.shape).astype(np.float32), tri, rast.shape[1:3], ranges=ranges)
                same = same and (r[..., 3] == rast[..., 3]).all()
        if same:
            good.append(fv)
    return sorted(touched), good


@pytest.mark.parametrize("range_mode", [False, True])
def test_rasterize_gradients_match_finite_differences_of_the_reference(oracle, range_mode):
    rng, pos, tri, ranges, rast, db = small_scene(oracle, range_mode)
    dy = rng.normal(size=rast.shape)
    ddb = rng.normal(size=db.shape)
    g_uv = R.rasterize_grad(pos, tri, rast, dy, range_mode)
    g_db = R.rasterize_grad_db(pos, tri, rast, ddb, range_mode)
    assert (g_uv[..., 2] == 0).all() and (g_db[..., 2] == 0).all()                # z is never read
    touched, good = qualifying_vertices(oracle, pos, tri, ranges, rast)
    assert len(touched) >= 6 and 2 * len(good) >= len(touched), (len(touched), len(good))
    # the forward the gradients belong to is the oracle's own image where nothing is clamped (u, v up to the 1e-6 guard)
    uv, dbf = R.rasterize_uv(pos, tri, rast, range_mode), R.rasterize_db(pos, tri, rast, range_mode)
    inner = (rast[..., 3] > 0) & (rast[..., 0] > 0) & (rast[..., 1] > 0) & (rast[..., 0] < 1) & (rast[..., 1] < 1)
    assert inner.sum() > 300
    assert np.abs(uv[inner] - rast[..., :2][inner]).max() < 1e-4 and R.rel_err(dbf[inner], db[inner]) < 1e-4
    p64 = pos.astype(np.float64)

    def loss_uv(p):
        return (R.rasterize_uv(p, tri, rast, range_mode) * dy[..., :2]).sum()

    def loss_db(p):
        return (R.rasterize_db(p, tri, rast, range_mode) * ddb).sum()

    for loss, g in ((loss_uv, g_uv), (loss_db, g_db)):
        scale = max(1.0, np.abs(g).max())
        worst = 0.0
        for fv in good:
            for c in (0, 1, 3):
                pp, pm = p64.reshape(-1, 4).copy(), p64.reshape(-1, 4).copy()
                pp[fv, c] += E
                pm[fv, c] -= E
                fd = (loss(pp.reshape(pos.shape)) - loss(pm.reshape(pos.shape))) / (2 * E)
                worst = max(worst, abs(fd - g.reshape(-1, 4)[fv, c]) / scale)
        print(f"{loss.__name__} range_mode={range_mode}: {len(good)}/{len(touched)} vertices, worst {worst:.2e} of the scale")
        assert worst <= FD_TOL


def _directional(loss, x, g, rng, n=4):
    """max over n random directions of |central difference - <g, direction>| relative to max(1, |<g, direction>|)."""
    worst = 0.0
    for _ in range(n):
        d = rng.normal(size=x.shape)
        fd = (loss(x + E * d) - loss(x - E * d)) / (2 * E)
        an = float((g * d).sum())
        worst = max(worst, abs(fd - an) / max(1.0, abs(an)))
    return worst


@pytest.mark.parametrize("range_mode", [False, True])
@pytest.mark.parametrize("Ba", [1, 2])
def test_interpolate_gradients_match_finite_differences_of_the_reference(oracle, range_mode, Ba):
    rng, pos, tri, ranges, rast, db = small_scene(oracle, range_mode)
    V, A = pos.shape[-2], 3
    attr = rng.normal(size=(Ba, V, A))
    r64, db64 = rast.astype(np.float64), db.astype(np.float64)
    dy = rng.normal(size=rast.shape[:3] + (A,))
    ga, gr = R.interpolate_grad(attr, rast, tri, dy)
    assert (gr[..., 2:] == 0).all() and (gr[rast[..., 3] == 0] == 0).all()

    def with_uv(uv):
        r = r64.copy()
        r[..., :2] = uv
        return r

    # per entry for the attributes (the image index of every atomic is what can go wrong), directions for the images
    for b in range(Ba):
        for v in range(V):
            for k in range(A):
                d = np.zeros_like(attr)
                d[b, v, k] = 1.0
                fd = ((R.interpolate(attr + E * d, r64, tri) - R.interpolate(attr - E * d, r64, tri)) * dy).sum() / (2 * E)
                assert abs(fd - ga[b, v, k]) <= FD_TOL * max(1.0, np.abs(ga).max()), (b, v, k)
    assert _directional(lambda uv: (R.interpolate(attr, with_uv(uv), tri) * dy).sum(), r64[..., :2], gr[..., :2], rng) <= FD_TOL
    for sel in ("all", [2, 0]):
        D = A if sel == "all" else len(sel)
        dy_da = R.half_zero_pairs(rng, rast.shape[:3] + (2 * D,)).astype(np.float64)
        ga2, gdb = R.interpolate_da_grad(attr, rast, db64, tri, dy_da, sel)
        assert (gdb[rast[..., 3] == 0] == 0).all()
        for b in range(Ba):
            for v in range(V):
                for k in range(A):
                    d = np.zeros_like(attr)
                    d[b, v, k] = 1.0
                    fd = ((R.interpolate_da(attr + E * d, rast, db64, tri, sel) - R.interpolate_da(attr - E * d, rast, db64, tri, sel))
                          * dy_da).sum() / (2 * E)
                    assert abs(fd - ga2[b, v, k]) <= FD_TOL * max(1.0, np.abs(ga2).max()), (sel, b, v, k)
        if sel != "all":
            assert (ga2[..., 1] == 0).all()                                        # the attribute that was not selected
        assert _directional(lambda x: (R.interpolate_da(attr, rast, x, tri, sel) * dy_da).sum(), db64, gdb, rng) <= FD_TOL


def test_reference_ignores_pixels_that_name_no_valid_triangle(oracle):
    """ids of 0, above T, or of a triangle with a vertex index outside [0, V): zero output, no gradient."""
    rng, pos, tri, ranges, rast, db = small_scene(oracle, False)
    tri = tri.copy()
    bad_t = int(R.triangle_ids(rast)[0].max()) - 1
    tri[bad_t, 1] = pos.shape[1] + 5
    rast = rast.copy()
    ys, xs = np.nonzero(rast[1, :, :, 3] > 0)
    rast[1, ys[0], xs[0], 3] = tri.shape[0] + 1
    attr = rng.normal(size=(1, pos.shape[1], 2))
    dead = (R.triangle_ids(rast) == bad_t + 1) | (R.triangle_ids(rast) > tri.shape[0]) | (rast[..., 3] == 0)
    assert (R.triangle_ids(rast) == bad_t + 1).any()
    ones = np.ones(rast.shape[:3] + (2,))
    assert (R.interpolate(attr, rast, tri)[dead] == 0).all()
    ga, gr = R.interpolate_grad(attr, rast, tri, ones)
    assert (gr[dead] == 0).all()
    ga_o, gr_o = oracle.interpolate_grad(attr, rast, tri, ones)
    assert R.rel_err(ga_o, ga) < 1e-5 and R.rel_err(gr_o, gr) < 1e-5
    assert R.rel_err(oracle.rasterize_grad(pos, tri, rast, np.ones_like(rast)), R.rasterize_grad(pos, tri, rast, np.ones_like(rast))) < 1e-3


def test_oracle_backward_passes_stay_within_twice_their_recorded_error(oracle, xarm7):
    """The measurement behind ORACLE_VS_F64: the oracle's float32 backward passes against the float64 reference over every
    case of tests/test_gpu_ops_grad.py, each case's preconditions included (they need the oracle alone)."""
    worst = {}
    for name, Ba, A, sel in R.case_list():
        e = R.expected_for(oracle, xarm7, name, Ba, A, sel)
        R.check_preconditions(e)
        if sel is not None:
            zero = ((e.dy_da[..., 0::2] == 0) & (e.dy_da[..., 1::2] == 0)).mean()
            assert 0.3 < zero < 0.7, (name, zero)
        for q, v in R.oracle_errors(e).items():
            worst[q] = max(worst.get(q, 0.0), v)
    print("ORACLE_VS_F64 = {")
    for q in R.ORACLE_VS_F64:
        print(f'    "{q}": {worst[q]:.2e},')
    print("}")
    assert set(worst) == set(R.ORACLE_VS_F64)
    for q, v in worst.items():
        assert v <= 2.0 * R.ORACLE_VS_F64[q], (q, v, R.ORACLE_VS_F64[q])


def test_scenes_meet_what_their_cases_assume(oracle, xarm7):
    """Checked here, where the oracle alone is enough, before a GPU is asked: image sizes, the empty image and the empty
    tiles of case b, shared vertices in case d."""
    sc = {s.name: s for s in R.scenes(oracle, xarm7)}
    for s in sc.values():   # partial 32 x 8 tiles at the image's edge, except at the solver's own 120 x 160
        assert s.H % 8 or s.W % 32 or s.name == "xarm7_links_120x160", s.name
    for name in ("middle_empty_75x101", "middle_empty_200x328"):
        e = R.expected_for(oracle, xarm7, name, 1, 1)
        cov = R.check_preconditions(e)
        assert cov[1] == 0 and cov[0] > 200 and cov[2] > 200
        assert R.empty_tiles(e.rast, 0) >= 1 and R.empty_tiles(e.rast, 2) >= 1
    d = sc["ragged_ranges_50x83"]
    shared = np.intersect1d(np.intersect1d(R.image_vertices(d, 0), R.image_vertices(d, 1)), R.image_vertices(d, 2))
    assert shared.size >= 1
    x = sc["xarm7_links_120x160"]
    assert x.B == 2 * len(xarm7.meshes) and x.V == 2 * sum(v.shape[0] for v, _ in xarm7.meshes)


def test_antialias_range_mode_gradient_matches_finite_differences(oracle):
    """oracle.antialias_grad in range mode: two images over ONE vertex array (the quad, and its first triangle alone), so every
    vertex of that triangle takes gradient from both images.  As test_antialias_gradients_match_finite_differences."""
    rng = np.random.default_rng(11)
    H, W = 40, 40
    pos = np.array([[-0.62, -0.55, 0.1, 1.0], [0.71, -0.38, 0.2, 1.2], [0.13, 0.66, -0.1, 0.9],
                    [-0.7, 0.5, 0.0, 1.1]], np.float32)
    tri = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    ranges = np.array([[0, 2], [0, 1]], np.int32)

    def render(p):
        rast, _ = oracle.rasterize(p, tri, [H, W], ranges=ranges)
        col = oracle.interpolate(np.ones((1, 4, 1), np.float32), rast, tri)
        return rast, col, oracle.antialias(col, rast, p, tri)

    rast, col, aa = render(pos)
    assert ((rast[..., 3] > 0).reshape(2, -1).sum(1) > 100).all()
    dy = rng.normal(size=aa.shape).astype(np.float32)
    _, gp = oracle.antialias_grad(col, rast, pos, tri, dy)
    assert gp.shape == pos.shape
    # each image alone gives its own share; the shared vertices' gradient is the sum of the two
    parts = []
    for b in range(2):
        one = np.zeros_like(dy)
        one[b] = dy[b]
        parts.append(oracle.antialias_grad(col, rast, pos, tri, one)[1])
        assert np.abs(parts[b][:3]).max() > 0
    assert np.abs(parts[0] + parts[1] - gp).max() <= 1e-5 * np.abs(gp).max() and (parts[1][3] == 0).all()
    checked = 0
    for vi in range(4):
        for c in (0, 1, 3):
            e = 1e-4
            pp, pm = pos.astype(np.float64).copy(), pos.astype(np.float64).copy()
            pp[vi, c] += e
            pm[vi, c] -= e
            (rp, _, ap), (rm, _, am) = render(pp.astype(np.float32)), render(pm.astype(np.float32))
            if not ((rp[..., 3] == rast[..., 3]).all() and (rm[..., 3] == rast[..., 3]).all()):
                continue  # a pixel changed owner: the forward is discontinuous there, skip this probe
            fd = float(((ap.astype(np.float64) - am) * dy).sum()) / (2 * e)
            assert abs(fd - gp[vi, c]) <= 3e-2 * max(1.0, abs(fd)), (vi, c, fd, gp[vi, c])
            checked += 1
    assert checked >= 8
