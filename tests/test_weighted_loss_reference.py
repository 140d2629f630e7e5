"""tests/weighted_loss_reference.py on the CPU: the weighted composition against fused_loss_reference.composite_f64 where the
two must agree, and the conditions the GPU cases (tests/test_gpu_weighted_loss.py) rely on their weight patterns to meet."""
import numpy as np
import pytest

import fused_loss_reference as R
import weighted_loss_reference as WR

XARM7_KEYS = [("xarm7",) + shape for shape in R.SOFT_SHAPES]
CASES = [(k, "uniform") for k in XARM7_KEYS] + [(XARM7_KEYS[0], "own_aa"), (("ties",), "uniform"), (("ties",), "binary")]
IDS = ["%s-%s" % ("x".join(str(v) for v in k[1:3]) or "ties", kind) for k, kind in CASES]


def test_the_library_exports_the_binding_call():
    from easyhec_amd import _lib
    assert _lib.has_weighted_loss()
    assert len(_lib.SIGNATURES["ehr_fused_bind_weight"][1]) == 4
    assert _lib.lib().ehr_version() == 8  # the symbol, not the version, is the capability check


@pytest.mark.parametrize("key,kind", CASES, ids=IDS)
def test_unit_weights_reproduce_the_unweighted_composition(oracle, xarm7, key, kind):
    """w == 1.  On a reference where m - r is a float32 (r == 0: e == m) the weighted composition IS composite_f64, exactly.
    On the case's own reference it is composite_f64 with e rounded to float32 once (the kernel's e, which composite_f64
    keeps in float64): gimg equal after that rounding, loss within 2^-23."""
    e = R.expected_for(oracle, xarm7, key, kind)
    ones = np.ones_like(e.ref)
    zero = np.zeros_like(e.ref)
    c0, cw = R.composite_f64(e.c.si, zero), WR.composite_weighted(e.c.si, zero, ones)
    assert (cw.sum32 == c0.sum32).all() and (cw.mask == c0.mask).all()
    assert (cw.gimg == c0.gimg).all() and (cw.loss == c0.loss).all()
    cw = WR.composite_weighted(e.c.si, e.ref, ones)
    assert (cw.we == cw.e).all() and (cw.mask == e.c.mask).all()
    assert (cw.gimg == e.c.gimg.astype(np.float32).astype(np.float64)).all()
    exact = cw.gimg == e.c.gimg
    assert exact.mean() > 0.5
    assert (np.abs(cw.loss - e.c.loss) <= 2.0 ** -23 * e.c.loss).all()
    one_image = WR.composite_weighted(e.c.si, e.ref, ones[:1])                   # shared weights: view b reads image b % 1
    assert (one_image.gimg == cw.gimg).all() and (one_image.loss == cw.loss).all()


@pytest.mark.parametrize("pattern", WR.BINARY_PATTERNS)
@pytest.mark.parametrize("key,kind", CASES[:3], ids=IDS[:3])
def test_binary_weights_equal_the_hidden_reference(oracle, xarm7, key, kind, pattern):
    """Binary w on ref equals the unweighted composition on ref' = where(w, ref, mask): a pixel with e == 0 contributes what
    a pixel with w == 0 does (gimg after the float32 rounding of e, loss within 2^-23; zero exactly where w == 0)."""
    e = R.expected_for(oracle, xarm7, key, kind)
    w = WR.binary_weight(pattern, e.m_ref)
    assert set(np.unique(w)) <= {0.0, 1.0}
    cw = WR.composite_weighted(e.c.si, e.ref, w)
    ch = R.composite_f64(e.c.si, WR.hidden_reference(e.ref, w, e.m_ref))
    assert (cw.gimg == ch.gimg.astype(np.float32).astype(np.float64)).all()
    assert (cw.gimg[w[:, ::-1] == 0] == 0).all() and (ch.gimg[w[:, ::-1] == 0] == 0).all()
    assert (np.abs(cw.loss - ch.loss) <= 2.0 ** -23 * ch.loss).all()
    assert (np.abs(cw.loss - WR.weighted_sse(cw.mask, e.ref, w)) <= 2.0 ** -23 * ch.loss).all()


@pytest.mark.parametrize("pattern", WR.BINARY_PATTERNS)
@pytest.mark.parametrize("key", XARM7_KEYS, ids=lambda k: "%dx%d" % (k[1], k[2]))
def test_binary_patterns_meet_their_conditions(oracle, xarm7, key, pattern):
    """Every pattern leaves at least a quarter of the (view, link) blocks with a gradient (A > 0) and takes some away; the
    rectangle, the tile checkerboard and the zero view blank at least one whole 32x8 tile that holds a job.  (The speckle
    cannot blank a tile: its own condition is that it removes 40-60 % of the pixels that carry a gradient.)"""
    e = R.expected_for(oracle, xarm7, key, "uniform")
    w, eh = WR.expected_binary(oracle, xarm7, key, "uniform", pattern)
    assert (eh.c.A > 0).mean() >= 0.25, (eh.c.A > 0).mean()
    live = e.c.gimg != 0
    hidden = live & (w[:, ::-1] == 0)
    assert hidden.any() and (eh.c.gimg[hidden] == 0).all()
    if pattern == "speckle":
        assert 0.4 <= hidden.sum() / live.sum() <= 0.6
        assert WR.zeroed_tiles_with_a_job(w, e.c.si) == 0
    else:
        assert WR.zeroed_tiles_with_a_job(w, e.c.si) >= 1
    if pattern == "view0":
        assert (eh.c.A[0] == 0).all() and (eh.c.A[1:] > 0).any()


@pytest.mark.parametrize("key,kind", CASES[:4], ids=IDS[:4])
def test_real_weights_meet_their_conditions(oracle, xarm7, key, kind):
    """Uniform [0, 2]: both ends are drawn, no block loses its gradient to the weights, and the weighted loss is the float64
    sum of w (m - r)^2 to within the float32 roundings of e and we."""
    w, e, c = WR.expected_real(oracle, xarm7, key, kind)
    assert w.min() >= 0 and w.min() < 0.01 and w.max() > 1.99 and w.max() <= 2
    assert ((c.A > 0) == (e.c.A > 0)).all()
    sse = WR.weighted_sse(c.mask, e.ref, w)
    assert (np.abs(c.loss - sse) <= 3 * 2.0 ** -24 * sse).all()
    assert not (c.gimg == e.c.gimg).all()
