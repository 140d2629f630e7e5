"""Pins tests/info_scene_cases.py on the CPU, with the oracle alone: the conditions under which the GPU cases of
tests/test_gpu_information_scenes.py can see a wrong index in vb_info_kernel -- counted pixels in every view, an exact count,
probed pixels on almost every (view, link) unit, entries with scale, and empty links that contribute nothing."""
import numpy as np
import pytest

import info_scene_cases as C
import link_scenes as S


@pytest.mark.parametrize("case", C.CASES)
def test_cases_have_something_to_compare(oracle, case):
    s = C.scene_of(case)
    D, _, e = C.expected(oracle, case, 6)
    rd = C.rendered(oracle, case)
    dead = C.empty_links(s)
    missing, live = C.unprobed_units(s, rd)
    share = float((e.S > 0).mean())
    print(f"[info scenes] {case}: L {s.L} B {s.B} {s.H}x{s.W}, count {e.count.tolist()}, probes {int(rd.nprobe.sum())}, "
          f"{missing} of {live} units with a triangle unprobed, entries with scale {share:.4f}")
    # no cancelling pixel: the kernel's count must be the reference's
    assert (e.count == e.count_max).all()
    assert (rd.nprobe[:, dead] == 0).all()
    if case in C.ALL_ZERO:
        assert (e.count == 0).all() and (e.S == 0).all() and (e.Sg == 0).all() and (e.info == 0).all() and (e.grad == 0).all()
        return
    assert (e.count > 0).all()
    # (an image smaller than a tile leaves the outer links of the lattice outside the frame: half of the units there)
    assert (2 if case in S.SUBTILE else 4) * missing <= live
    if case in C.COUNTS:
        assert e.count.tolist() == C.COUNTS[case]
    if case in C.COUNT_RANGES:
        assert (e.count.min(), e.count.max()) == C.COUNT_RANGES[case]
    if case in C.UNPROBED:
        assert (missing, live) == C.UNPROBED[case]
    # the z translation has no scale, every other pair of the six has one in every view
    z = np.zeros(6, bool)
    z[2] = True
    assert (e.S[:, z] == 0).all() and (e.S[:, :, z] == 0).all() and (e.Sg[:, z] == 0).all()
    assert (e.S[:, ~z][:, :, ~z] > 0).all() and (e.Sg[:, ~z] > 0).all() and share == 25.0 / 36.0
    assert (np.abs(e.info) <= e.S * (1 + 1e-12)).all() and (np.abs(e.grad) <= e.Sg * (1 + 1e-12)).all()


@pytest.mark.parametrize("case", C.MANY_N)
def test_scale_share_rises_with_N_and_N_1_has_scale(oracle, case):
    shares = []
    for N in (1, 6, 32):
        _, _, e = C.expected(oracle, case, N)
        # (the x translation alone leaves the J of a few vertical pairs within rounding of zero: at N = 1 such a pixel may or
        # may not count, at most 3 in a view of these scenes; information_reference.check holds the kernel between the two)
        print(f"[info scenes] {case} N={N}: pixels that may or may not count {(e.count_max - e.count).tolist()}")
        assert ((e.count == e.count_max) if N > 1 else (e.count_max - e.count <= 3)).all() and (e.count > 50).all()
        shares.append(float((e.S > 0).mean()))
    print(f"[info scenes] {case}: entries with scale at N = 1, 6, 32: {shares}")
    assert shares[0] == 1.0 and shares[1] == 25.0 / 36.0 and shares[2] == (31.0 / 32.0) ** 2


def test_a_block_of_an_empty_link_contributes_nothing(oracle):
    """Tangents that live on the empty links alone give a reference that is zero everywhere; garbage in the empty links'
    blocks changes no bit of it."""
    for case in ("full32", "first_empty", "last_empty", "only_one_live"):
        s = C.scene_of(case)
        dead = C.empty_links(s)
        assert dead.any() and not dead.all()
        D, _, e = C.expected(oracle, case, 6)
        only = D.copy()
        only[:, :, ~dead] = 0
        eo = C.reference(oracle, case, only)
        assert (np.abs(only) > 0).any() and (eo.S == 0).all() and (eo.info == 0).all() and (eo.count == 0).all()
        junk = D.copy()
        junk[:, :, dead] = 1e30
        ej = C.reference(oracle, case, junk)
        assert (ej.info == e.info).all() and (ej.grad == e.grad).all() and (ej.count == e.count).all()


def test_wave_count_thresholds():
    """The N of THRESHOLDS lie on both sides of every drop of vb_info_launch's waves per workgroup, at U = 64 and U = 512."""
    for case, want in (("full32", {12: 4, 13: 2, 28: 2, 29: 1}), ("units512", {11: 4, 12: 2, 26: 2, 27: 1, 28: 1})):
        s = C.scene_of(case)
        U = s.B * s.L
        assert U == (64 if case == "full32" else 512)
        assert {N: C.waves_per_workgroup(N, U) for N in C.THRESHOLDS[case]} == want


def test_lm_poses_lie_where_they_should_and_the_reference_is_finite():
    """The poses of tests/test_gpu_lm_tangent_shapes.py: under the clamp of the exponential map, one float32 step either side
    of it, and far from it; lm_reference.tangents is finite at each, and its rotation tangents differ across the clamp (the
    gradient of the clamped angle is cut below it)."""
    import lm_reference as LR
    d = C.lm_dofs()
    assert C.squared_angle(d["identity"]) == 0 and C.squared_angle(d["w1e-3"]) < 1.1e-6
    assert C.squared_angle(d["below_clamp"]) < 1e-4 <= C.squared_angle(d["above_clamp"])
    assert (d["below_clamp"] != d["above_clamp"]).sum() == 1
    assert abs(np.sqrt(C.squared_angle(d["w0.3"])) - 0.3) < 1e-6
    s = C.scene_of("full32")
    K32, lp32 = s.K.astype(np.float32), s.link_poses.astype(np.float32)
    refs = {}
    for name in C.LM_DOFS:
        _, ref, Sabs = LR.tangents(d[name], K32, s.H, s.W, 0.001, 10.0, lp32)
        assert ref.shape == (6, s.B, s.L, 4, 4) and np.isfinite(ref).all() and np.isfinite(Sabs).all() and (np.abs(ref) <= Sabs * (1 + 1e-12)).all()
        refs[name] = ref
    jump = np.abs(refs["above_clamp"][3:] - refs["below_clamp"][3:]).max() / np.abs(refs["below_clamp"][3:]).max()
    same = np.abs(refs["above_clamp"][:3] - refs["below_clamp"][:3]).max() / np.abs(refs["below_clamp"][:3]).max()
    print(f"[info scenes] tangents across the clamp: rotations move by {jump:.2e} of their size, translations by {same:.2e}")
    assert jump > 1e-6 > same


def test_nested_references_agree_on_their_common_block(oracle):
    """The reference of the first n tangents is the n x n block of the reference of more: what the bit comparison of the
    wave-count cases rests on.  count is the same for every n >= 6: the six generators leave no pixel with a pair at zero."""
    Ns = C.THRESHOLDS["full32"]
    D, refs = C.nested(oracle, "full32", Ns)
    big = refs[max(Ns)]
    for n in Ns:
        e = refs[n]
        assert np.allclose(e.info, big.info[:, :n, :n], rtol=1e-12, atol=0) and np.allclose(e.grad, big.grad[:, :n], rtol=1e-12, atol=0)
        assert (e.count == big.count).all() and (e.count == e.count_max).all()
        assert (e.count == C.expected(oracle, "full32", 6)[2].count).all()
