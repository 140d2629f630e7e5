"""Float64 reference of the WEIGHTED mask loss (ehr_fused_bind_weight) on top of
tests/fused_loss_reference.py, and the weight patterns its tests use.  CPU only, numpy, not collected by pytest.

Composition, per pixel, as the contract states it:

    e    = m - r            float32 (the kernel's subtraction: the exact difference, rounded once)
    we   = w * e            float32
    loss = sum  we * e      summed in float64 (the products are exact in float64)
    gimg = 2 we  where sum32 <= 1, else 0          (2 we is exact)

so the reference's gimg carries the kernel's own roundings of e and we, and the per-block bar of fused_loss_reference stays
K_ROUNDINGS * 2^-24 * A: the weight adds no rounding to the budget.  With w == 1, we == e: the composition is
composite_f64's with e rounded to float32 -- identical wherever m - r is a float32 (r == 0, r == m, and most binary r).
"""
import types

import numpy as np

import fused_loss_reference as R


def composite_weighted(si, ref, w):
    """si [B,L,H,W] in GL row order; ref, w [B,H,W] in image order (row 0 = top; w may hold fewer images: view b reads image
    b % len(w)).  -> sum32, gimg, we in GL row order, mask in image order, loss [B] float64."""
    c = R.composite_f64(si, ref)
    B = c.sum32.shape[0]
    w = np.asarray(w, np.float32)
    w = w[np.arange(B) % w.shape[0]]
    m = np.ascontiguousarray(c.mask[:, ::-1])                                   # GL order, float32
    r = np.asarray(ref, np.float32)[:, ::-1]
    e = (m - r).astype(np.float32)
    we = (w[:, ::-1] * e).astype(np.float32)
    loss = (we.astype(np.float64) * e.astype(np.float64)).sum(axis=(1, 2))
    gimg = np.where(c.sum32 <= np.float32(1), 2.0 * we.astype(np.float64), 0.0)
    return types.SimpleNamespace(sum32=c.sum32, mask=c.mask, loss=loss, gimg=gimg, we=we, e=e)


def block_reference_weighted(oracle, meshes, mvp, ref, w):
    """fused_loss_reference.block_reference with weights: the composition above, G and A through grad_mvp_f64."""
    H, W = ref.shape[1], ref.shape[2]
    si, parts = R.link_images(oracle, meshes, np.asarray(mvp, np.float32), H, W)
    c = composite_weighted(si, ref, w)
    c.si = si
    c.G, c.A = R.grad_mvp_f64(oracle, meshes, parts, c.gimg)
    return c


def weighted_sse(mask, ref, w):
    """float64 sum w (mask - ref)^2 per view of a given mask (the loss bar's reference: the GPU's own mask goes in)."""
    B = mask.shape[0]
    w = np.asarray(w, np.float64)
    w = w[np.arange(B) % w.shape[0]]
    return (w * (mask.astype(np.float64) - np.asarray(ref, np.float64)) ** 2).sum(axis=(1, 2))


# ---- weight patterns ---------------------------------------------------------------------------------------------------
BINARY_PATTERNS = ("rectangle", "speckle", "tiles", "view0")
TILE_W, TILE_H = 32, 8      # the composite stage's tile, in GL rows (row 0 = bottom)


def _tile_rows(H, ty):
    """image rows (row 0 = top) of tile row ty"""
    lo, hi = TILE_H * ty, min(TILE_H * ty + TILE_H, H)
    return slice(H - hi, H - lo)


def binary_weight(kind, m_ref, seed=0):
    """[B,H,W] float32 of zeros and ones for a scene whose oracle mask is m_ref (image order).
    rectangle: per view the middle third (in y) of the foreground's bounding box, grown to whole 32x8 tiles, is zero: it cuts the arm;
    speckle:   half of the pixels, at random;
    tiles:     a checkerboard of whole tiles is zero, tiles under the robot included;
    view0:     view 0 is zero everywhere."""
    B, H, W = m_ref.shape
    w = np.ones((B, H, W), np.float32)
    if kind == "speckle":
        return (np.random.default_rng(77 + seed).uniform(size=(B, H, W)) > 0.5).astype(np.float32)
    if kind == "view0":
        w[0] = 0
        return w
    ntx, nty = (W + TILE_W - 1) // TILE_W, (H + TILE_H - 1) // TILE_H
    if kind == "tiles":
        for ty in range(nty):
            for tx in range(ntx):
                if (tx + ty) % 2 == 0:
                    w[:, _tile_rows(H, ty), TILE_W * tx:TILE_W * tx + TILE_W] = 0
        return w
    if kind == "rectangle":
        for b in range(B):
            ys, xs = np.nonzero(m_ref[b] > 0)
            a, z = (xs.min() // TILE_W) * TILE_W, -(-(xs.max() + 1) // TILE_W) * TILE_W   # the box's columns, whole tiles
            gl0, gl1 = H - 1 - ys.max(), H - ys.min()                            # GL rows of the box
            m0, m1 = gl0 + (gl1 - gl0) // 3, gl0 + 2 * (gl1 - gl0) // 3          # ... their middle third, whole tile rows
            for ty in range(m0 // TILE_H, -(-m1 // TILE_H)):
                w[b, _tile_rows(H, ty), a:z] = 0
        return w
    raise KeyError(kind)


def real_weight(shape, seed=0):
    """uniform in [0, 2], float32"""
    return np.random.default_rng(4242 + seed).uniform(0.0, 2.0, size=shape).astype(np.float32)


def zeroed_tiles_with_a_job(w, si):
    """How many (view, tile)s have all their weights zero AND hold a job: a pixel some link's antialiased image touches
    (si [B,L,H,W] in GL row order).  A lower bound of the kernel's notion (its jobs also cover a link box's empty tiles)."""
    B, H, W = w.shape
    touched = (np.asarray(si) != 0).any(axis=1)[:, ::-1]                         # image order
    n = 0
    for b in range(B):
        for ty in range((H + TILE_H - 1) // TILE_H):
            rows = _tile_rows(H, ty)
            for tx in range((W + TILE_W - 1) // TILE_W):
                cols = slice(TILE_W * tx, TILE_W * tx + TILE_W)
                if touched[b, rows, cols].any() and not w[b, rows, cols].any():
                    n += 1
    return n


def hidden_reference(ref, w, m_ref):
    """ref' = where(w, ref, mask): a pixel with e == 0 contributes exactly what a pixel with w == 0 does."""
    return np.where(np.asarray(w) != 0, ref, m_ref).astype(np.float32)


_CACHE = {}


def expected_binary(oracle, robot, key, kind, pattern):
    """(w, fused_loss_reference.expected on ref' = where(w, ref, oracle mask)) of (scene key, reference kind, pattern); once per process."""
    k = (key, kind, pattern)
    if k not in _CACHE:
        e = R.expected_for(oracle, robot, key, kind)
        w = binary_weight(pattern, e.m_ref)
        _CACHE[k] = (w, R.expected(oracle, e.s, hidden_reference(e.ref, w, e.m_ref)))
    return _CACHE[k]


def expected_real(oracle, robot, key, kind):
    """(w, e, c): uniform [0, 2] weights, the unweighted expected() of the case and the weighted block reference."""
    k = (key, kind, "real")
    if k not in _CACHE:
        e = R.expected_for(oracle, robot, key, kind)
        w = real_weight(e.ref.shape)
        _CACHE[k] = (w, e, block_reference_weighted(oracle, e.s.meshes, e.s.mvp, e.ref, w))
    return _CACHE[k]
