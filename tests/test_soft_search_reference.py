"""The pose search's soft score without a GPU: the two forms of the reference distance transform agree, the score
arithmetic on hand-made integers, and the displacement ladder through the CPU oracle -- the soft IoU falls strictly with
the displacement while ``xor`` ranks a pose that left the image ahead of a 10 cm miss."""
import numpy as np
import pytest
import torch

import soft_search_reference as ssr


def six_valued(rng, shape):
    return np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], np.float32)[rng.integers(0, 6, shape)]


@pytest.mark.parametrize("H,W,cap", [(1, 1, 1), (5, 7, 1), (5, 7, 3), (9, 33, 5), (40, 70, 16), (40, 70, 300)])
def test_brute_force_and_separable_distance_transforms_agree(H, W, cap):
    rng = np.random.default_rng(H * W + cap)
    sparse = np.zeros((H, W), np.float32)
    sparse[rng.integers(0, H, 3), rng.integers(0, W, 3)] = 1.0
    corner = np.zeros((H, W), np.float32)
    corner[H - 1, 0] = 1.0
    for ref in (six_valued(rng, (H, W)), sparse, corner, np.zeros((H, W), np.float32), np.ones((H, W), np.float32)):
        fg = ssr.foreground(ref)
        a, b = ssr.edt_brute(fg, cap), ssr.edt_separable(fg, cap)
        assert a.dtype == b.dtype == np.int64 and (a == b).all()
        assert ((a == 0) == fg).all() and a.max() <= cap * cap
        if not fg.any():
            assert (a == cap * cap).all()
    # the corner pixel's distances are plain to write down
    yy, xx = np.mgrid[0:H, 0:W]
    assert (ssr.edt_brute(ssr.foreground(corner), cap) == np.minimum(cap * cap, (yy - (H - 1)) ** 2 + xx ** 2)).all()


def test_reference_uses_the_separable_form_above_the_brute_force_size():
    assert 40 * 70 <= ssr.BRUTE_MAX < 120 * 160
    rng = np.random.default_rng(0)
    ref = (rng.random((1, 41, 70)) > 0.97).astype(np.float32)
    assert (ssr.edt(ref, 9)[0] == ssr.edt_brute(ssr.foreground(ref[0]), 9)).all()     # (41x70 goes the separable way)


def test_isqrt_is_exact_around_every_square_up_to_the_largest_cap():
    r = np.arange(1, 4097, dtype=np.int64)
    for off in (-1, 0, 1):
        assert (ssr.isqrt(r * r + off) == (r - 1 if off < 0 else r)).all()
    assert ssr.isqrt(np.array([0]))[0] == 0


def disc(H, W, cy, cx, rad):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad


def test_soft_iou_scores_on_hand_made_integers():
    from easyhec_amd.pose_search import soft_iou_scores
    H, W, cap = 24, 32, 4
    ref = np.zeros((2, H, W), np.float32)
    ref[0] = disc(H, W, 12, 14, 5)                      # view 1's reference stays empty
    fg = ref > 0.5
    dil = np.zeros_like(fg)                              # the reference dilated by one pixel (4-neighbourhood)
    dil[0] = fg[0] | np.roll(fg[0], 1, 0) | np.roll(fg[0], -1, 0) | np.roll(fg[0], 1, 1) | np.roll(fg[0], -1, 1)
    far = np.zeros_like(fg)
    far[0, :3, -3:] = True                               # further than cap from the disc
    masks = np.stack([fg, np.zeros_like(fg), dil, far])
    want = ssr.soft_scores(masks, ref, cap)
    soft = soft_iou_scores(torch.tensor(want["area"]), torch.tensor(want["inter"]), torch.tensor(want["ksum"]),
                           torch.tensor(want["ref_area"]), cap)
    assert soft.dtype == torch.float64 and soft.shape == (4,)
    assert np.array_equal(soft.numpy(), want["soft"])
    # render == ref: 1.0 in view 0; view 1 has an empty union: 1.0 as well
    assert soft[0].item() == 1.0
    # an empty render: 0 in view 0, the empty union of view 1 counts 1.0
    assert soft[1].item() == 0.5 and want["ksum"][1, 0] == 0
    # one pixel of dilation: below 1, and worth what the ring's k = cap - 1 says
    n, ring = int(fg[0].sum()), int(dil[0].sum() - fg[0].sum())
    assert ring > 0 and soft[2].item() < 1.0
    assert soft[2].item() == 0.5 * ((cap * n + (cap - 1) * ring) / (cap * (n + ring)) + 1.0)
    # no rendered pixel within cap of the reference: 0
    assert want["ksum"][3, 0] == 0 and soft[3].item() == 0.5
    # a single view with a non-empty reference shows the plain 0 and 1
    one = soft_iou_scores(want["area"][:, :1], want["inter"][:, :1], want["ksum"][:, :1], want["ref_area"][:1], cap)   # anything as_tensor takes
    assert one.tolist()[0] == 1.0 and one.tolist()[1] == 0.0 and one.tolist()[3] == 0.0 and 0.0 < one.tolist()[2] < 1.0


def test_soft_costs_match_the_reference_on_the_cpu():
    """The torch expression that builds the cost images (k in float64) against the integer reference."""
    from easyhec_amd.pose_search import soft_costs
    rng = np.random.default_rng(3)
    ref = six_valued(rng, (2, 9, 33))
    ref[1] = 0.0
    ref[1, 8, 32] = 1.0
    valid = rng.random((2, 9, 33)) > 0.3
    for cap in (1, 5, 300):
        d2 = torch.tensor(ssr.edt(ref, cap).astype(np.int32))
        assert np.array_equal(soft_costs(d2, cap).numpy(), ssr.soft_costs(ref, cap))
        assert np.array_equal(soft_costs(d2, cap, torch.tensor(valid)).numpy(), ssr.soft_costs(ref, cap, valid))
        assert soft_costs(d2, cap).dtype == torch.int32


def test_cpu_tensors_raise():
    from easyhec_amd.pose_search import mask_cost, mask_distance
    with pytest.raises(RuntimeError):
        mask_distance(None, torch.zeros(1, 8, 8), 3)
    with pytest.raises(RuntimeError):
        mask_cost(None, None, torch.zeros(2, 1, 2, 4, 4), torch.zeros(1, 8, 8, dtype=torch.int32))
    with pytest.raises(ValueError):
        mask_distance(None, torch.zeros(8, 8), 3)


def test_header_declares_and_library_exports_the_soft_search():
    import os
    import re
    from easyhec_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ehr.h")).read(), flags=re.S)
    for name, nargs, needs in (("ehr_mask_distance", 8, ("const float* ref", "int cap_px", "int32_t* d2")),
                               ("ehr_mask_cost", 17, ("const int32_t* cost", "int C", "int64_t* sums", "int chunk_views"))):
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"include/ehr.h does not declare {name}"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]) and all(n in args for n in needs), name
    assert _lib.has_soft_search() and _lib.lib().ehr_version() == 8   # the symbols, not the version, are the capability check


def test_displacement_ladder_soft_is_monotone_where_xor_is_not(oracle, xarm7):
    lad = ssr.ladder(oracle, xarm7)
    masks, ref = lad["masks"], lad["ref"]
    assert masks[0].all(axis=(1, 2)).sum() == 0 and masks[0].any(axis=(1, 2)).all()
    assert not masks[8].any() and not masks[9].any()            # 1.2 m and 3 m: out of the frame
    xor = None
    for cap in (16, 64):
        got = ssr.soft_scores(masks, ref, cap)
        soft, xor = got["soft"], got["xor"]
        assert soft[0] == 1.0 and xor[0] == 0
        assert (np.diff(soft[:9]) < 0).all(), soft              # strictly down the first nine rungs
        assert soft[8] == 0.0 and soft[9] == 0.0
        assert list(np.argsort(-soft[:8], kind="stable")) == list(range(8))
    # ... while xor ranks a pose that renders nothing ahead of the 10 cm miss, and is not monotone in between
    ref_area = int(ssr.foreground(ref).sum())
    assert xor[8] == ref_area and xor[9] == ref_area
    assert xor[8] < xor[2] and xor[9] < xor[2]
    assert (np.diff(xor[3:8]) < 0).any() and (np.diff(xor[3:8]) > 0).any()
