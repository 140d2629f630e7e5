"""The composite stage's item path after profiles/composite_requests.md: a tile's `jn`, reference, cached sum and the slot
values of its first VB_COMP_PRE = 2 in-range links are asked for in ONE round trip, before `jn` is known; a link's matrix is
a scalar load.  Links beyond VB_COMP_PRE go the old way, and so do the pairs (the first 64 of a slot were asked for in the
first round trip as well while this was measured: the cases cover that form too).  What is asked for a link that turns
out to hold nothing (jn = -1) must not be looked at, a link with a value and no pairs (jn = 0) must still count, and the sum
stays in link order.  The scenes are the smallest at which that request order can go wrong:

  stacked6_64x16   six links of four triangles stacked on 2 x 2 tiles: every tile has six links in range (more than
                   any VB_COMP_PRE in 1, 2, 4), the sum of three and more of them crosses 1 (the clamp) on a soft reference;
  sliver_128x64    a thin diagonal link first in link order, and a thin anti-diagonal one last, whose boxes hold every tile
                   while their triangles miss most (jn = -1), around a link that draws in tiles both miss;
  cover_128x64     one large link that covers whole tiles (jn = 0: a value, no pairs) under a small one;
  dots_96x24       24 one-pixel triangles inside one 32 x 8 tile: 96 blended pairs, 64 in the slot, 32 in the spill pool;
  ragged_98x42     W % 4 != 0 and H % 8 != 0: the scalar reference path and tile rows outside the image;
  overlap6_96x40   six overlapping links under a pose (link_scenes.scene) for the solver-step and multi-start forms.

Each case first checks on the CPU -- the oracle's per-link images and the links' pixel boxes -- that the situation it is
meant for occurs in its scene.  The bars are those of tests/test_gpu_atomic_spread.py: masks bit-exact, loss per view 1e-6,
grad_mvp 1e-5 globally and per block (fused_loss_reference.check_blocks), pose and moments at pose_reference's bar; forms
the project documents as bit-identical (bound against unbound reference, with against without a mask output, unit weights
against none, graph replay against eager steps) are compared byte for byte."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import link_scenes as S
import weighted_loss_reference as WR
from test_gpu_atomic_spread import check_step, problem, solo_after, solo_before, _np
from test_gpu_fused_loss import bound, link_scene, stateless
from test_gpu_weighted_loss import call as weighted_call, same

pytestmark = pytest.mark.gpu

TW, TH = 32, 8
PRE_MAX = 4   # the largest number of links the first round trip was measured with (1, 2, 4; 2 is built)


# ---- scenes in pixel coordinates under an identity matrix (fused_loss_reference.scene_clamp_ties' convention) -------------
def _px(x, y, W, H, z=0.0):
    return [2.0 * x / W - 1.0, 2.0 * y / H - 1.0, z]


def _mesh(tris_px, W, H):
    """tris_px: [n][3][2 or 3] pixel coordinates (GL rows: y up) and, optionally, a clip-space depth -> (verts, faces), three
    vertices of its own per triangle."""
    t = np.asarray(tris_px, np.float64)
    v = np.array([_px(*q, W=W, H=H) if len(q) == 2 else _px(q[0], q[1], W, H, q[2]) for q in t.reshape(-1, t.shape[-1])], np.float32)
    return v, np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


def _quad(a, b, c, d):
    return [[a, b, c], [a, c, d]]


def _pixel_scene(name, links, W, H, B=1):
    mvp = np.tile(np.eye(4, dtype=np.float32)[None, None], (B, len(links), 1, 1))
    for b in range(1, B):   # later views: shifted by a fraction of a pixel
        mvp[b, :, 0, 3] = 0.37 * b / W
        mvp[b, :, 1, 3] = -0.61 * b / H
    s = R._scene(name, [_mesh(t, W, H) for t in links], mvp, H, W)
    return s


def stacked6():
    W, H = 64, 16
    links = []
    for l in range(6):   # an X of two bands a pixel thick, flatter from link to link: in all four tiles, crossing near the centre
        y, t = 0.7 + 1.15 * l, 1.0
        # (the second band lies behind the first: where they cross, the nearer triangle is not a tie)
        links.append(_quad((3.2, y, 0.0), (60.7, 14.9 - y - t, 0.0), (60.7, 14.9 - y, 0.0), (3.2, y + t, 0.0)) +
                     _quad((3.4, 14.6 - y - t, 0.3), (60.5, y + 0.2, 0.3), (60.5, y + 0.2 + t, 0.3), (3.4, 14.6 - y, 0.3)))
    return _pixel_scene("stacked6_64x16", links, W, H)


def sliver():
    W, H = 128, 64
    diag = _quad((3.0, 2.2), (6.0, 2.0), (125.0, 60.5), (122.0, 61.2))
    block = _quad((5.3, 20.2), (30.7, 21.4), (29.2, 44.3), (6.9, 43.1)) + _quad((98.4, 21.3), (122.9, 20.1), (121.5, 43.6), (99.8, 44.2))
    anti = _quad((3.0, 61.0), (5.5, 61.5), (125.0, 3.5), (122.5, 2.5))
    return _pixel_scene("sliver_128x64", [diag, block, anti], W, H)


def cover():
    W, H = 128, 64
    big = _quad((3.4, 2.7), (124.2, 3.9), (123.1, 61.3), (4.8, 60.2))
    small = [[(50.2, 20.3), (77.9, 24.1), (61.4, 43.6)]]
    return _pixel_scene("cover_128x64", [big, small], W, H, B=2)


def dots():
    W, H = 96, 24
    rng = np.random.default_rng(7)
    tris = []
    for cy in (9, 11, 13):
        for cx in range(33, 64, 4):   # one triangle around the centre of pixel (cx, cy), inside tile (1, 1); it holds no other centre
            jx, jy = rng.uniform(-0.08, 0.08, 2)
            x, y = cx + 0.5 + jx, cy + 0.5 + jy
            tris.append([(x - 0.8, y - 0.55), (x + 0.8, y - 0.55), (x, y + 0.8)])
    far = _quad((4.2, 3.1), (20.7, 2.6), (21.9, 20.3), (5.1, 19.4))
    return _pixel_scene("dots_96x24", [far, tris], W, H)


PIXEL_SCENES = {"stacked6_64x16": stacked6, "sliver_128x64": sliver, "cover_128x64": cover, "dots_96x24": dots}
LINK_SCENES = {
    "ragged_98x42": dict(counts=[65, 3, 31], H=42, W=98, B=2, seed=51, cols=3, pitch=0.3, size=0.7, f=60.0),
    "overlap6_96x40": dict(counts=[5, 3, 7, 2, 9, 4], H=40, W=96, B=2, seed=52, cols=3, pitch=0.1, size=0.5, f=60.0),
}
_CACHE = {}


def scene_of(name):
    if name not in _CACHE:
        _CACHE[name] = PIXEL_SCENES[name]() if name in PIXEL_SCENES else S.scene(name=name, **LINK_SCENES[name])
    return _CACHE[name]


def expected_of(oracle, name):
    """The scene, its seeded soft reference and the oracle's result on it; made once, never written to."""
    k = (name, "expected")
    if k not in _CACHE:
        s = scene_of(name)
        _CACHE[k] = R.expected(oracle, s, R.reference_mask(oracle, s, "uniform"))
    return _CACHE[k]


# ---- what the CPU says about a scene --------------------------------------------------------------------------------------
def tiles_in_range(s, mvp, b):
    """[L, nty, ntx] bool: the tiles (GL rows) a link's pixel box, grown by the one-pixel halo, touches -- the tile range its
    jobs are made for.  The box is taken a pixel generous on every side, and the cases only count tiles well inside it."""
    ntx, nty = (s.W + TW - 1) // TW, (s.H + TH - 1) // TH
    out = np.zeros((s.L, nty, ntx), bool)
    for l, (v, f) in enumerate(s.meshes):
        if len(f) == 0:
            continue
        p = np.concatenate([v.astype(np.float64), np.ones((len(v), 1))], 1) @ np.asarray(mvp[b, l], np.float64).T
        x = (p[:, 0] / p[:, 3] + 1.0) * 0.5 * s.W
        y = (p[:, 1] / p[:, 3] + 1.0) * 0.5 * s.H
        x0, x1 = max(int(np.floor(x.min())) - 1, 0), min(int(np.ceil(x.max())) + 1, s.W - 1)
        y0, y1 = max(int(np.floor(y.min())) - 1, 0), min(int(np.ceil(y.max())) + 1, s.H - 1)
        out[l, y0 // TH:y1 // TH + 1, x0 // TW:x1 // TW + 1] = True
    return out


def tile_any(img, H, W):
    """[..., H, W] bool (GL rows) -> [..., nty, ntx]: does the tile hold a set pixel?"""
    nty, ntx = (H + TH - 1) // TH, (W + TW - 1) // TW
    pad = np.zeros(img.shape[:-2] + (nty * TH, ntx * TW), bool)
    pad[..., :H, :W] = img
    return pad.reshape(img.shape[:-2] + (nty, TH, ntx, TW)).any(axis=(-3, -1))


def region_any(img, H, W):
    """As tile_any for the tile grown by its one-pixel halo (what a job looks at)."""
    g = img.copy()
    g[..., 1:, :] |= img[..., :-1, :]
    g[..., :-1, :] |= img[..., 1:, :]
    h = g.copy()
    h[..., :, 1:] |= g[..., :, :-1]
    h[..., :, :-1] |= g[..., :, 1:]
    return tile_any(h, H, W)


def pair_count(cov, ty, tx):
    """Pairs of 4-neighbours, one covered and one not, with at least one pixel inside tile (tx, ty); cov [H, W] bool, GL rows."""
    H, W = cov.shape
    inside = np.zeros((H, W), bool)
    inside[ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW] = True
    n = ((cov[:, 1:] != cov[:, :-1]) & (inside[:, 1:] | inside[:, :-1])).sum()
    return int(n + ((cov[1:] != cov[:-1]) & (inside[1:] | inside[:-1])).sum())


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import dr, fused
    return fused, dr, torch.device("cuda:0")


def all_forms(fused, dr, dev, e, what):
    """Stateless call against the oracle; the bound form (sparse items) and the bound form with a mask output (FILL) give its
    bits; without a gradient the mask and the loss are still the call's."""
    s = e.s
    scene = link_scene(fused, s, dev)
    ctx = dr.RasterizeCudaContext()
    mask, loss, grad = stateless(fused, ctx, scene, s.mvp, e.ref, dev)
    R.check_against_oracle(mask, loss, grad, e, what + " stateless")
    ref = torch.tensor(e.ref, device=dev)
    _, loss_b, grad_b = bound(fused, ctx, scene, s.mvp, ref, dev)
    assert (loss_b == loss).all() and (grad_b == grad).all(), what + " bound"
    mask_f, loss_f, grad_f = bound(fused, ctx, scene, s.mvp, ref, dev, want_mask=True)
    assert (mask_f == mask).all() and (loss_f == loss).all() and (grad_f == grad).all(), what + " bound, mask output"
    # want_grad = 0, stateless and bound
    tm = torch.tensor(s.mvp, device=dev)
    for bind in (False, True):
        fused._ensure_plan(ctx, scene, s.B, s.H, s.W)
        fused.bind_ref(ctx, scene, ref if bind else None)
        m0, l0 = torch.full((s.B, s.H, s.W), float("nan"), device=dev), torch.empty((s.B,), device=dev)
        fused._launch(ctx, scene, tm, ref, m0, l0, None)
        torch.cuda.synchronize()
        fused.check_status(ctx)
        assert (m0.cpu().numpy() == mask).all() and (l0.cpu().numpy() == loss).all(), (what, "no gradient", bind)
    fused.bind_ref(ctx, scene, None)
    return scene, ctx, (mask, loss, grad)


# ---- the cases -------------------------------------------------------------------------------------------------------------
def test_more_links_in_range_than_the_first_round_trip_takes(env, oracle):
    fused, dr, dev = env
    e = expected_of(oracle, "stacked6_64x16")
    s = e.s
    assert S.n_tiles(s) == 4
    rng_ = tiles_in_range(s, s.mvp, 0)
    assert rng_.all() and s.L == 6 > PRE_MAX                     # six links in range of every tile
    drawn = region_any(e.c.si[0] > 0, s.H, s.W)                  # [L, nty, ntx]
    assert (drawn.sum(axis=0) >= PRE_MAX + 1).all()              # ... and at least five contribute a value to each
    # the clamp: sums above one, and pixels where a link beyond the first four changes the sum
    first4 = e.c.si[0, :PRE_MAX].sum(axis=0)
    assert (e.c.sum32[0] > 1).sum() >= 50 and ((e.c.si[0, PRE_MAX:].sum(axis=0) > 0) & (first4 < 1)).sum() >= 10
    all_forms(fused, dr, dev, e, "stacked6")


def test_links_in_range_that_hold_nothing(env, oracle):
    fused, dr, dev = env
    e = expected_of(oracle, "sliver_128x64")
    s = e.s
    inr = tiles_in_range(s, s.mvp, 0)
    drawn = region_any(e.c.si[0] > 0, s.H, s.W)
    assert inr[0].all() and inr[2].all()                          # the slivers' boxes hold every tile
    # tiles link 1 draws in while BOTH slivers, in range before and behind it in link order, hold nothing there
    only1 = drawn[1] & ~drawn[0] & ~drawn[2]
    assert only1.sum() >= 4, int(only1.sum())
    # tiles in range of the slivers alone where nobody draws (skipped), and tiles where a sliver draws beside link 1's range
    assert (~drawn.any(axis=0)).sum() >= 4 and (drawn[0] & ~drawn[1]).sum() >= 4
    all_forms(fused, dr, dev, e, "sliver")


def test_a_link_with_a_value_and_no_pairs(env, oracle):
    fused, dr, dev = env
    e = expected_of(oracle, "cover_128x64")
    s = e.s
    for b in range(s.B):
        full = ~region_any(e.c.si[b, 0] < 1, s.H, s.W)            # tiles whose whole region link 0 covers: a value, no pair
        assert full.sum() >= 6
        assert (full & region_any((e.c.si[b, 1] > 0) & (e.c.si[b, 1] < 1), s.H, s.W)).sum() >= 1   # ... some under link 1's silhouette
        assert (full & ~region_any(e.c.si[b, 1] > 0, s.H, s.W)).sum() >= 3                         # ... some alone
    all_forms(fused, dr, dev, e, "cover")


def test_more_pairs_than_a_slot_holds(env, oracle):
    fused, dr, dev = env
    e = expected_of(oracle, "dots_96x24")
    s = e.s
    cov = e.c.si[0, 1] >= 0.5                                     # link 1's covered pixels: the centres the dots surround
    assert cov.sum() == 24 and tile_any(cov, s.H, s.W).sum() == 1 and tile_any(cov, s.H, s.W)[1, 1]
    assert pair_count(cov, 1, 1) == 96 > 64                       # four pairs a dot, all of one slot
    assert (e.c.A[0] > 0).all()
    all_forms(fused, dr, dev, e, "dots")


def test_an_image_that_is_no_multiple_of_the_tile(env, oracle):
    fused, dr, dev = env
    e = expected_of(oracle, "ragged_98x42")
    s = e.s
    assert s.W % 4 != 0 and s.H % TH != 0
    top = tile_any(e.c.si.sum(axis=1) > 0, s.H, s.W)[:, -1]       # the tile row that hangs over the image's edge is drawn in
    assert top.any(), "no link reaches the last tile row"
    all_forms(fused, dr, dev, e, "ragged")


@pytest.mark.parametrize("name", ["stacked6_64x16", "ragged_98x42"])
def test_weighted_forms(env, oracle, name):
    """Unit weights change no bit (stateless, bound, bound with a mask output); binary weights against the oracle on the
    hidden reference (weighted_loss_reference), bound form bit-equal."""
    fused, dr, dev = env
    e = expected_of(oracle, name)
    s = e.s
    scene, ctx = link_scene(fused, s, dev), dr.RasterizeCudaContext()
    ref = torch.tensor(e.ref, device=dev)
    base = weighted_call(fused, ctx, scene, s.mvp, ref, None, dev)
    R.check_against_oracle(*base, e, name + " no weights")
    ones = torch.ones_like(ref)
    assert same(base, weighted_call(fused, ctx, scene, s.mvp, ref, ones, dev))
    for want_mask in (False, True):
        assert same(base, weighted_call(fused, ctx, scene, s.mvp, ref, ones, dev, bind=True, want_mask=want_mask))
    w = WR.binary_weight("speckle", e.m_ref, seed=5)
    eh = R.expected(oracle, s, WR.hidden_reference(e.ref, w, e.m_ref))
    wt = torch.tensor(w, device=dev)
    got = weighted_call(fused, ctx, scene, s.mvp, ref, wt, dev)
    R.check_against_oracle(*got, eh, name + " speckle weights")
    sse = WR.weighted_sse(got[0], e.ref, w)
    assert (np.abs(got[1] - sse) <= 1e-6 * np.abs(sse)).all()
    for want_mask in (False, True):
        assert same(got, weighted_call(fused, ctx, scene, s.mvp, ref, wt, dev, bind=True, want_mask=want_mask))
    fused.check_status(ctx)


def overlap_problem(oracle, dev):
    s = scene_of("overlap6_96x40")
    k = ("overlap6_96x40", "ref")
    if k not in _CACHE:
        _CACHE[k] = R.reference_mask(oracle, s, "uniform")
    return s, _CACHE[k]


def many_in_range(s, mvp):
    """Tiles of view 0 with three or more links in range (more than the first round trip takes) at the step's own mvp."""
    return int((tiles_in_range(s, mvp, 0).sum(axis=0) >= 3).sum())


def test_two_solver_steps_eager_and_replayed(env, oracle):
    from easyhec_amd.fast import FusedPoseStep
    fused, _, dev = env
    s, ref = overlap_problem(oracle, dev)
    _, make, batch = problem(s, ref, dev)
    ma, mb = make(), make()
    fa, fb = FusedPoseStep(ma, batch, slack=0.0), FusedPoseStep(mb, batch, slack=0.0)
    fb.capture()
    for it in range(2):
        before = solo_before(fa, ma)
        fa.step()
        fb.step()
        after = solo_after(fa, ma)
        assert many_in_range(s, after["mvp"]) >= 4
        check_step(oracle, s, ref, fa, before, after, f"overlap6 step {it}")
        for name in ("mvp", "tc_jac", "loss_b", "grad_mvp", "red", "loss", "grad", "exp_avg", "exp_avg_sq", "step_t"):
            assert torch.equal(getattr(fa, name), getattr(fb, name)), (it, name)
        assert torch.equal(ma.dof.data, mb.dof.data), it
    fused.check_status(fa.glctx)
    fused.check_status(fb.glctx)
    fb.release_graph()


def test_multi_start_step(env, oracle):
    """P = 2 hypotheses x 2 views share the two reference images (the SHARED instantiation)."""
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts
    fused, _, dev = env
    s, ref = overlap_problem(oracle, dev)
    cfg, make, batch = problem(s, ref, dev)
    starts = sample_starts(np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64), 2, 0.01, 1.5, seed=3)
    ms = MultiStartPoseStep(make(), batch, starts, slack=0.0)
    assert ms.P == 2 and ms.Bv == 2 and ms.L == 6
    dof0 = _np(ms.dof)
    ms.step()
    torch.cuda.synchronize()
    for p in range(2):
        v = slice(p * ms.Bv, (p + 1) * ms.Bv)
        after = dict(mvp=_np(ms.mvp[v]), loss_b=_np(ms.loss_b[v]), grad_mvp=_np(ms.grad_mvp[v]), red=_np(ms.red[p]),
                     tc_jac=_np(ms.tc_jac[p]), dof=_np(ms.dof[p]), m=_np(ms.exp_avg[p]), v=_np(ms.exp_avg_sq[p]))
        assert many_in_range(s, after["mvp"]) >= 4
        check_step(oracle, s, ref, ms, (dof0[p], np.zeros(6, np.float32), np.zeros(6, np.float32), 0), after, f"overlap6 multi p{p}")
    fused.check_status(ms.glctx)
