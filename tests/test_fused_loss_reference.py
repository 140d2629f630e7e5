"""CPU side of tests/test_gpu_fused_loss.py: the oracle's fused restatement is pinned against the float64 composition of the
oracle's own ops on soft and out-of-range reference masks (before any kernel is compared with it), and every scene meets
what its GPU case assumes, so that a later change of seed or geometry cannot silently empty a case."""
import numpy as np
import pytest

import fused_loss_reference as R

XARM7_KEYS = [("xarm7",) + shape for shape in R.SOFT_SHAPES]
CASES = [(key, kind) for key in XARM7_KEYS for kind in R.SOFT_REFS] + [(("ties",), kind) for kind in R.TIE_REFS]
IDS = [f"{k[0]}{'' if len(k) == 1 else '_%dx%d' % (k[1], k[2])}-{kind}" for k, kind in CASES]


@pytest.mark.parametrize("key,kind", CASES, ids=IDS)
def test_oracle_equals_the_composition_on_soft_references(oracle, xarm7, key, kind):
    """oracle.render_mask_loss == transform_pos -> rasterize -> antialias per (view, link), summed in float32 in link order,
    clamped, compared with a real-valued reference in float64, and back through antialias_grad with a float64 contraction."""
    e = R.expected_for(oracle, xarm7, key, kind)
    c = e.c
    assert (e.m_ref == c.mask).all()
    assert np.abs(e.l_ref - c.loss).max() <= 1e-6 * np.abs(c.loss).max()
    # the oracle contracts its float32 gpos in float64 as well: what is left is the rounding of the float64 sum to float32,
    # and the order of the float64 adds (1e-12 of the block's scale is generous for a few thousand of them)
    assert (np.abs(e.g_ref - c.G) <= 2.0 ** -24 * np.abs(c.G) + 1e-12 * c.A[:, :, None, None] + 1e-37).all()
    assert (e.g_ref[:, :, 2, :] == 0).all() and (c.G[:, :, 2, :] == 0).all()
    assert np.abs(c.G).max() > 0


@pytest.mark.parametrize("key,kind", CASES, ids=IDS)
def test_scenes_meet_what_their_gpu_cases_assume(oracle, xarm7, key, kind):
    e = R.expected_for(oracle, xarm7, key, kind)
    s, c = e.s, e.c
    # the per-block bar: few dead blocks, and every live block's scale far above the fixed-point grid (module docstring)
    dead = c.A == 0
    assert dead.mean() <= 0.25, (s.name, dead)
    tiles = ((s.W + 31) // 32) * ((s.H + 7) // 8)
    assert (c.A[~dead] >= tiles * 2.0 ** -8).all(), (s.name, c.A)
    # the per-view SSE stays inside the accumulators' contract (< 2^31), by orders of magnitude
    assert c.loss.max() < 2.0 ** 31 * 1e-3
    covered = (c.sum32 > 0)
    assert 0.02 < covered.mean() < 0.9
    frac = covered & (c.sum32 < 1)
    assert frac.sum() >= 50                                        # antialiased pixels: where blended pairs end
    assert (c.gimg[frac] != 0).mean() > 0.5                        # ... and most of them carry gradient
    if kind in ("uniform", "wide"):                                # the reference is real-valued where it matters
        ref_gl = e.ref[:, ::-1]
        assert ((ref_gl[frac] != 0) & (ref_gl[frac] != 1)).mean() > 0.5
    if kind == "own_aa":                                           # e == 0 exactly on many covered pixels, fractional on others
        err = c.mask - e.ref
        assert ((err == 0) & (c.mask > 0)).sum() >= 100 and ((err != 0) & (np.abs(err) < 1)).sum() >= 100
    if kind == "wide":
        assert e.ref.min() < -0.4 and e.ref.max() > 1.9
    if key[0] == "ties":
        n = R.tie_counts(c)
        assert n["one"] >= 10 and n["above"] >= 10 and n["below"] >= 10 and n["high"] >= 50, n
        assert n["three"] >= 100, n                                # the holes: three and four links on one pixel ...
        many = (c.si != 0).sum(axis=1) >= 3
        assert (many & (c.sum32 <= 1) & (c.gimg != 0)).sum() >= 10  # ... with the gate open
        # (the ORDER of the link sum is not observable here or in any scene of this size: the fractions lie on a grid of
        #  2^-21 or coarser, sums up to 1 are exact in any order, and the order-dependent sums are all above 1)
        # shut and open gates both occur next to fractional values, and the tie pixels' gate is open: they carry gradient
        tie = ((c.si != 0).sum(axis=1) >= 2) & (c.sum32 == np.float32(1))
        assert (c.gimg[tie] != 0).sum() >= 10 or kind == "binary"
        assert ((c.sum32 > 1) & (c.sum32 < 2)).sum() >= 50
