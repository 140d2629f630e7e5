"""Gradient parity of the three drop-in ops where the product runs them: batches, range mode, broadcast attributes, tile
flags -- every backward kernel of csrc/ehr_raster.hip and csrc/ehr_interp_aa.hip with B > 1.

Each backward kernel is handed the oracle's own incoming gradient (torch.autograd.grad with grad_outputs), so that its result
is compared for the same input: with the oracle at the suite's tolerances (1e-5 of max(1, max|ref|) for grad_attr, for grad_pos
through (u, v) and for antialias' grad_pos and colour gradient, 1e-4 for grad_pos through rast_db, 1e-6 for the gradient of
rast_db) and, for dr.rasterize and dr.interpolate, with the float64 reference of tests/ops_reference.py at 4 x ORACLE_VS_F64.
Forward outputs equal the oracle bit for bit.  The scenes, their seeded inputs and their preconditions live in
tests/ops_reference.py; tests/test_ops_reference.py checks them on the CPU.  Both forms of the rasterizer run every case."""
import os
import types

import numpy as np
import pytest
import torch

import ops_reference as R

pytestmark = pytest.mark.gpu
TOL = R.SUITE_TOL


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, dr
    assert os.path.exists(_lib.LIB_PATH)
    return dr, dr.RasterizeCudaContext(), torch.device("cuda:0")


@pytest.fixture(params=["direct", "queued"])
def raster_path(request):
    """Both forms of the drop-in rasterizer (ehr_raster.hip): the direct one (small launches: two kernels, a key image in
    global memory) and the queued one (count / allocate / fill / one workgroup per tile).  Same bits either way."""
    old = os.environ.get("EHR_RASTER_DIRECT_MAX")
    os.environ["EHR_RASTER_DIRECT_MAX"] = "0" if request.param == "queued" else "1000000000"
    yield request.param
    if old is None:
        del os.environ["EHR_RASTER_DIRECT_MAX"]
    else:
        os.environ["EHR_RASTER_DIRECT_MAX"] = old


def t(a, dev, grad=False):
    x = torch.tensor(np.ascontiguousarray(a), device=dev)
    if grad:
        x.requires_grad_(True)
    return x


def n(x):
    return x.detach().cpu().numpy()


def near(got, ref, tol, what):
    err = R.rel_err(n(got) if isinstance(got, torch.Tensor) else got, ref)
    print(f"{what}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, err, tol)


def same(got, ref, what):
    assert (n(got) == ref).all(), what


def rasterize(env, s, tp, tt, grad_db=True):
    dr, ctx, _ = env
    ranges = None if s.ranges is None else torch.tensor(s.ranges)
    return dr.rasterize(ctx, tp, tt, [s.H, s.W], ranges=ranges, grad_db=grad_db)


def chain(env, e, attr_grad=True, flags=True, boost=None):
    """rasterize -> interpolate -> antialias on the GPU with the inputs of ``e``, and every backward kernel run on the
    oracle's incoming gradient.  rasterize and antialias get a position leaf each, so each kernel's share of grad_pos is seen
    alone.  ``flags=False`` hands the later ops a copy of `rast` (still on the autograd graph) that carries no tile flags."""
    dr, _, dev = env
    s = e.s
    tp, tq, tt = t(s.pos, dev, True), t(s.pos, dev, True), t(s.tri, dev)
    ta = t(e.attr, dev, attr_grad)
    r, db = rasterize(env, s, tp, tt)
    assert dr._flags_of(r) is not None
    rr = r if flags else r.clone()
    assert (dr._flags_of(rr) is not None) == flags
    c, _ = dr.interpolate(ta, rr, tt)
    aa = dr.antialias(c, rr, tq, tt) if boost is None else dr.antialias(c, rr, tq, tt, pos_gradient_boost=boost)
    o = types.SimpleNamespace(r=r, db=db, c=c, aa=aa, tp=tp, tq=tq, ta=ta)
    o.g_col, o.gp_aa = torch.autograd.grad(aa, [c, tq], grad_outputs=t(e.dy, dev), retain_graph=True)
    if attr_grad:
        o.g_attr, o.g_rast = torch.autograd.grad(c, [ta, rr], grad_outputs=t(e.g_col, dev), retain_graph=True)
    else:
        (o.g_rast,), o.g_attr = torch.autograd.grad(c, [rr], grad_outputs=t(e.g_col, dev), retain_graph=True), None
    (o.gp_uv,) = torch.autograd.grad(r, [tp], grad_outputs=t(e.g_rast, dev), retain_graph=True)
    return o


def check_chain(o, e, boost=1.0):
    same(o.r, e.rast, "rast")
    same(o.db, e.db, "rast_db")
    same(o.c, e.col, "interpolate")
    same(o.aa, e.aa, "antialias")
    near(o.g_col, e.g_col, TOL["antialias_grad_color"], "antialias grad_color vs oracle")
    near(o.gp_aa, boost * e.gp_aa, TOL["antialias_grad_pos"], "antialias grad_pos vs oracle")
    if o.g_attr is not None:
        near(o.g_attr, e.g_attr, TOL["interpolate_grad_attr"], "interpolate grad_attr vs oracle")
        near(o.g_attr, e.g_attr64, R.f64_bound("interpolate_grad_attr"), "interpolate grad_attr vs f64")
    near(o.g_rast, e.g_rast, TOL["interpolate_grad_rast"], "interpolate grad_rast vs oracle")
    near(o.g_rast, e.g_rast64, R.f64_bound("interpolate_grad_rast"), "interpolate grad_rast vs f64")
    near(o.gp_uv, e.gp_uv, TOL["rasterize_grad"], "rasterize grad_pos (u, v) vs oracle")
    near(o.gp_uv, e.gp_uv64, R.f64_bound("rasterize_grad"), "rasterize grad_pos (u, v) vs f64")
    assert (n(o.gp_uv)[..., 2] == 0).all() and (n(o.gp_aa)[..., 2] == 0).all()


def end_to_end(o, e, dev):
    """One backward() through the whole chain, as a training step does it: the leaves' gradients are the sums."""
    (o.aa * t(e.dy, dev)).sum().backward()
    near(o.tq.grad, e.gp_aa, TOL["antialias_grad_pos"], "end to end: antialias' share of grad_pos")
    near(o.tp.grad, e.gp_uv, TOL["rasterize_grad"], "end to end: rasterize's share of grad_pos")
    if o.ta.requires_grad:
        near(o.ta.grad, e.g_attr, TOL["interpolate_grad_attr"], "end to end: grad_attr")


# ---- a: instance mode, B = 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ba,A", R.CASES_A)
@pytest.mark.parametrize("size", ["75x101", "200x328"])
def test_instance_mode_batch_of_three(env, oracle, xarm7, raster_path, size, Ba, A):
    """Three different vertex sets, attributes per image ([3, V, A]) and broadcast ([1, V, A]: grad_attr is the sum over the
    images, every image's atomics land in the one array)."""
    e = R.expected_for(oracle, xarm7, f"instance_{size}", Ba, A)
    R.check_preconditions(e)
    o = chain(env, e)
    assert tuple(o.g_attr.shape) == (Ba, e.s.V, A)
    check_chain(o, e)
    if Ba == 1:   # the sum over the images, each image's share from the float64 reference
        parts = []
        for b in range(3):
            only = np.zeros_like(e.g_col)
            only[b] = e.g_col[b]
            parts.append(R.interpolate_grad(e.attr, e.rast, e.s.tri, only)[0])
            assert np.abs(parts[b]).max() > 0
        near(o.g_attr, parts[0] + parts[1] + parts[2], R.f64_bound("interpolate_grad_attr"), "broadcast grad_attr vs sum of images")
    end_to_end(o, e, env[2])


# ---- b: the middle image empty, with the tile flags and without ---------------------------------------------------------
@pytest.mark.parametrize("Ba,A", R.CASES_A)
@pytest.mark.parametrize("size", ["75x101", "200x328"])
def test_empty_middle_image_with_and_without_tile_flags(env, oracle, xarm7, raster_path, size, Ba, A):
    e = R.expected_for(oracle, xarm7, f"middle_empty_{size}", Ba, A)
    cov = R.check_preconditions(e)
    assert cov[1] == 0 and cov[0] > 200 and cov[2] > 200
    assert R.empty_tiles(e.rast, 0) >= 1 and R.empty_tiles(e.rast, 2) >= 1
    runs = []
    for flags in (True, False):
        o = chain(env, e, flags=flags)
        check_chain(o, e)
        # the empty image: exactly nothing
        assert (o.gp_uv[1] == 0).all() and (o.gp_aa[1] == 0).all() and (o.g_rast[1] == 0).all()
        assert (o.c[1] == 0).all() and (o.aa[1] == 0).all()
        if Ba == 3:
            assert (o.g_attr[1] == 0).all()
        runs.append(o)
    w, wo = runs
    for k in ("r", "db", "c", "aa", "g_rast"):   # what the kernels gather: the same bits
        assert torch.equal(getattr(w, k), getattr(wo, k)), k
    for k, q in (("g_attr", "interpolate_grad_attr"), ("gp_uv", "rasterize_grad"), ("gp_aa", "antialias_grad_pos"),
                 ("g_col", "antialias_grad_color")):   # what they add up atomically
        near(getattr(w, k), n(getattr(wo, k)), TOL[q], f"{k} with flags vs without")
    end_to_end(wo, e, env[2])


# ---- c: range mode in the solver's batched layout -------------------------------------------------------------------------
def test_range_mode_in_the_solvers_batched_layout(env, oracle, xarm7, raster_path):
    """rb_solver._batched_topology's layout (2 frames x all links, one image each, one vertex array, shifted triangles, one
    range per image): first exactly as _forward_three_ops_batched calls the ops -- a [V, 1] colour of ones without gradient,
    flags carried onto the detached rast, grad_pos from antialias alone -- then with C = 3 colours that want a gradient."""
    dr, _, dev = env
    e = R.expected_for(oracle, xarm7, "xarm7_links_120x160", 1, 3)
    R.check_preconditions(e)
    s = e.s
    rng = np.random.default_rng(5)
    tp, tt = t(s.pos, dev, True), t(s.tri, dev)
    ones = torch.ones((s.V, 1), dtype=torch.float32, device=dev)
    rast, _ = rasterize(env, s, tp, tt, grad_db=False)
    det = dr.carry_tile_flags(rast, rast.detach())
    assert dr._flags_of(det) is not None
    color, _ = dr.interpolate(ones, det, tt)
    aa = dr.antialias(color, rast, tp, tt, topology_hash=dr.antialias_construct_topology_hash(tt))
    col_ref = oracle.interpolate(np.ones((1, s.V, 1), np.float32), e.rast, s.tri)
    same(rast, e.rast, "rast")
    same(color, col_ref, "interpolate")
    same(aa, oracle.antialias(col_ref, e.rast, s.pos, s.tri), "antialias")
    dy = rng.normal(size=tuple(aa.shape)).astype(np.float32)
    (aa * t(dy, dev)).sum().backward()
    _, gp_ref = oracle.antialias_grad(col_ref, e.rast, s.pos, s.tri, dy)
    for b in range(s.B):
        assert np.abs(gp_ref[R.image_vertices(s, b)]).max() > 0, b
    near(tp.grad, gp_ref, TOL["antialias_grad_pos"], "batched layout: grad_pos vs oracle")
    o = chain(env, e)
    check_chain(o, e)
    end_to_end(o, e, dev)


# ---- d: ragged ranges over shared vertices --------------------------------------------------------------------------------
def test_range_mode_with_ragged_ranges(env, oracle, xarm7, raster_path):
    """[0, T], an interior slice, the last triangle alone and [0, 0] over ONE vertex array: a vertex takes atomics from several
    images; the image with the empty range contributes exactly nothing."""
    dr, _, dev = env
    e = R.expected_for(oracle, xarm7, "ragged_ranges_50x83", 1, 3)
    R.check_preconditions(e)
    s = e.s
    shared = np.intersect1d(np.intersect1d(R.image_vertices(s, 0), R.image_vertices(s, 1)), R.image_vertices(s, 2))
    assert shared.size >= 1 and np.abs(e.gp_aa[shared]).max() > 0 and np.abs(e.gp_uv[shared]).max() > 0
    o = chain(env, e)
    check_chain(o, e)
    assert (o.r[3] == 0).all() and (o.c[3] == 0).all() and (o.aa[3] == 0).all() and (o.g_rast[3] == 0).all()
    # gradient arriving at the empty image ALONE moves nothing
    tp, tq, tt, ta = t(s.pos, dev, True), t(s.pos, dev, True), t(s.tri, dev), t(e.attr, dev, True)
    r, _ = rasterize(env, s, tp, tt)
    c, _ = dr.interpolate(ta, r, tt)
    aa = dr.antialias(c, r, tq, tt)
    only = np.zeros_like(e.dy)
    only[3] = e.dy[3]
    assert np.abs(only).max() > 0
    (aa * t(only, dev)).sum().backward()
    assert (tp.grad == 0).all() and (tq.grad == 0).all() and (ta.grad == 0).all()
    end_to_end(o, e, dev)


# ---- e: rast_db in batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", R.DIFF_SELECTIONS, ids=["all", "2-0"])
@pytest.mark.parametrize("Ba", [1, 3])
@pytest.mark.parametrize("mode", ["instance", "range"])
def test_rast_db_and_pixel_differentials_in_batches(env, oracle, xarm7, raster_path, mode, Ba, sel):
    dr, _, dev = env
    e = R.expected_for(oracle, xarm7, f"db_{mode}_56x88", Ba, 3, sel)
    R.check_preconditions(e)
    s = e.s
    zero = ((e.dy_da[..., 0::2] == 0) & (e.dy_da[..., 1::2] == 0)).mean()
    assert 0.3 < zero < 0.7
    tt = t(s.tri, dev)
    # rasterize's backward through rast_db alone, then through both outputs
    tp = t(s.pos, dev, True)
    r, db = rasterize(env, s, tp, tt)
    same(r, e.rast, "rast")
    same(db, e.db, "rast_db")
    assert db.requires_grad
    (g,) = torch.autograd.grad(db, [tp], grad_outputs=t(e.ddb, dev), retain_graph=True)
    near(g, e.gp_db, TOL["rasterize_grad_db"], "rasterize grad_pos (rast_db) vs oracle")
    near(g, e.gp_db64, R.f64_bound("rasterize_grad_db"), "rasterize grad_pos (rast_db) vs f64")
    assert (g[..., 2] == 0).all()
    (g2,) = torch.autograd.grad([r, db], [tp], grad_outputs=[t(e.g_rast, dev), t(e.ddb, dev)], retain_graph=True)
    both, both64 = e.gp_uv + e.gp_db, e.gp_uv64 + e.gp_db64
    near(g2, both, TOL["rasterize_grad_db"], "rasterize grad_pos (both outputs) vs oracle")
    f64_both = (R.f64_bound("rasterize_grad") * max(1.0, np.abs(e.gp_uv64).max())
                + R.f64_bound("rasterize_grad_db") * max(1.0, np.abs(e.gp_db64).max())) / max(1.0, np.abs(both64).max())
    near(g2, both64, f64_both, "rasterize grad_pos (both outputs) vs f64")   # (the two halves' bounds, added)
    # interpolate's pixel differentials: gradients to the attributes and to rast_db, and on through rast_db to pos
    ta = t(e.attr, dev, True)
    sel_arg = sel if isinstance(sel, str) else list(sel)
    out, da = dr.interpolate(ta, r, tt, rast_db=db, diff_attrs=sel_arg)
    same(out, e.col, "interpolate")
    same(da, e.da, "pixel differentials")
    g_attr, g_db = torch.autograd.grad(da, [ta, db], grad_outputs=t(e.dy_da, dev), retain_graph=True)
    assert tuple(g_attr.shape) == (Ba, s.V, 3)
    near(g_attr, e.g_attr_da, TOL["interpolate_da_grad_attr"], "differentials: grad_attr vs oracle")
    near(g_attr, e.g_attr_da64, R.f64_bound("interpolate_da_grad_attr"), "differentials: grad_attr vs f64")
    near(g_db, e.g_db, TOL["interpolate_da_grad_db"], "differentials: grad rast_db vs oracle")
    near(g_db, e.g_db64, R.f64_bound("interpolate_da_grad_db"), "differentials: grad rast_db vs f64")
    if not isinstance(sel, str):
        assert (g_attr[..., 1] == 0).all()   # attribute 1 was not selected
    # one backward() through both of interpolate's outputs down to the leaves
    ((out * t(e.g_col, dev)).sum() + (da * t(e.dy_da, dev)).sum()).backward()
    ga = e.g_attr + e.g_attr_da
    near(ta.grad, ga, TOL["interpolate_grad_attr"], "interpolate, both outputs: grad_attr vs oracle")
    gp = e.gp_uv + oracle.rasterize_grad_db(s.pos, s.tri, e.rast, e.g_db, s.range_mode)
    near(tp.grad, gp, TOL["rasterize_grad_db"], "interpolate, both outputs: grad_pos vs oracle")


# ---- f: pos_gradient_boost ------------------------------------------------------------------------------------------------
def test_pos_gradient_boost_scales_the_position_gradient_only(env, oracle, xarm7, raster_path):
    e = R.expected_for(oracle, xarm7, "instance_75x101", 3, 3)
    R.check_preconditions(e)
    plain, boosted = chain(env, e), chain(env, e, boost=2.5)
    check_chain(boosted, e, boost=2.5)
    assert torch.equal(plain.aa, boosted.aa) and torch.equal(plain.c, boosted.c)
    near(boosted.gp_aa, 2.5 * n(plain.gp_aa), TOL["antialias_grad_pos"], "boosted grad_pos vs 2.5 x unboosted")
    near(boosted.g_col, n(plain.g_col), TOL["antialias_grad_color"], "boosted colour gradient vs unboosted")
    assert float(plain.gp_aa.abs().max()) > 0


# ---- g: non-contiguous inputs and incoming gradients ------------------------------------------------------------------------
def test_non_contiguous_inputs_and_incoming_gradients(env, oracle, xarm7, raster_path):
    """pos as a slice of a wider tensor, attr as a strided slice, an incoming gradient made by expand() and one taken as a
    strided slice: the ops make them contiguous; the gradients are those of the contiguous call."""
    dr, _, dev = env
    e = R.expected_for(oracle, xarm7, "instance_75x101", 3, 3)
    s = e.s
    tt = t(s.tri, dev)
    wide = torch.zeros((3, s.V, 6), device=dev)
    wide[..., 1:5] = t(s.pos, dev)
    wide.requires_grad_(True)
    attr2 = torch.zeros((3, s.V, 6), device=dev)
    attr2[..., ::2] = t(e.attr, dev)
    attr2.requires_grad_(True)
    dy_px = np.random.default_rng(3).normal(size=(1, s.H, s.W, 1)).astype(np.float32)
    dy_full = np.ascontiguousarray(np.broadcast_to(dy_px, e.aa.shape))
    dy2 = torch.zeros(tuple(e.aa.shape[:3]) + (6,), device=dev)
    dy2[..., ::2] = t(e.dy, dev)
    grads = {}
    for kind in ("contiguous", "strided"):
        if kind == "contiguous":
            tp, ta = t(s.pos, dev, True), t(e.attr, dev, True)
            pos_in, attr_in, leaves = tp, ta, (tp, ta)
            gy_expand, gy_slice = t(dy_full, dev), t(e.dy, dev)
        else:
            pos_in, attr_in, leaves = wide[..., 1:5], attr2[..., ::2], (wide, attr2)
            gy_expand, gy_slice = t(dy_px, dev).expand(*e.aa.shape), dy2[..., ::2]
            assert not pos_in.is_contiguous() and not attr_in.is_contiguous()
            assert not gy_expand.is_contiguous() and not gy_slice.is_contiguous()
        r, _ = rasterize(env, s, pos_in, tt)
        c, _ = dr.interpolate(attr_in, r, tt)
        aa = dr.antialias(c, r, pos_in, tt)
        same(aa, e.aa, "antialias")
        out = []
        for gy in (gy_expand, gy_slice):
            gp, ga = torch.autograd.grad(aa, leaves, grad_outputs=gy, retain_graph=True)
            out.append((gp, ga) if kind == "contiguous" else (gp[..., 1:5], ga[..., ::2]))
            if kind == "strided":
                assert (gp[..., 0] == 0).all() and (gp[..., 5] == 0).all() and (ga[..., 1::2] == 0).all()
        grads[kind] = out
    # the strided incoming gradient is e.dy: the oracle's chain gives the sums
    near(grads["contiguous"][1][0], e.gp_aa + e.gp_uv, TOL["rasterize_grad"], "contiguous: grad_pos vs oracle")
    near(grads["contiguous"][1][1], e.g_attr, TOL["interpolate_grad_attr"], "contiguous: grad_attr vs oracle")
    for i, what in enumerate(("expanded dy", "sliced dy")):
        near(grads["strided"][i][0], n(grads["contiguous"][i][0]), TOL["rasterize_grad"], f"{what}: grad_pos vs contiguous")
        near(grads["strided"][i][1], n(grads["contiguous"][i][1]), TOL["interpolate_grad_attr"], f"{what}: grad_attr vs contiguous")
        assert float(grads["contiguous"][i][0].abs().max()) > 0 and float(grads["contiguous"][i][1].abs().max()) > 0


# ---- h: constant attributes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ba", [3, 1])
def test_constant_attributes_still_pass_the_gradient_to_rast(env, oracle, xarm7, raster_path, Ba):
    """attr without requires_grad: interp_grad_kernel runs with grad_attr = NULL; at B = 3 grad_rast is still the oracle's,
    and pos receives it through rasterize."""
    dr, _, dev = env
    e = R.expected_for(oracle, xarm7, "instance_75x101", Ba, 3)
    R.check_preconditions(e)
    o = chain(env, e, attr_grad=False)
    assert o.g_attr is None and float(o.g_rast.abs().max()) > 0
    for b in range(3):
        assert float(o.g_rast[b].abs().max()) > 0
    check_chain(o, e)
    end_to_end(o, e, dev)
    assert o.ta.grad is None
    # rast's only consumer is interpolate: pos gets everything through rasterize
    s = e.s
    tp, tt = t(s.pos, dev, True), t(s.tri, dev)
    r, _ = rasterize(env, s, tp, tt)
    c, _ = dr.interpolate(t(e.attr, dev), r, tt)
    (c * t(e.g_col, dev)).sum().backward()
    near(tp.grad, e.gp_uv, TOL["rasterize_grad"], "constant attributes: grad_pos through rasterize vs oracle")
    near(tp.grad, e.gp_uv64, R.f64_bound("rasterize_grad"), "constant attributes: grad_pos through rasterize vs f64")
