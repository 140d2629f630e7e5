"""Pins tests/information_reference.py, the float64 reference of ehr_mask_information, the tangent builders and the report of
easyhec_amd/information.py, and the scenes of tests/test_gpu_information.py -- on the CPU, with the oracle alone."""
import numpy as np
import pytest
import torch

import fused_loss_reference as R
import information_reference as IR

KEYS = [("xarm7",) + shape for shape in R.SOFT_SHAPES] + [("ties",)]


@pytest.mark.parametrize("key", KEYS, ids=["120x160", "100x150", "ties"])
def test_gradient_agrees_with_the_block_reference(oracle, xarm7, key):
    """grad_ref[b,k] = sum_l <G[b,l], dmvp[k,b,l]> of fused_loss_reference.block_reference: the same oracle pairs, summed per
    probed pixel here and per image there, so within that module's float32 scale A contracted with |dmvp|."""
    e0 = R.expected_for(oracle, xarm7, key, "uniform")
    D, _, e = IR.expected_for(oracle, xarm7, key, "uniform", 17)
    D64 = D.astype(np.float64)
    g2 = np.einsum("blrc,kblrc->bk", e0.c.G, D64)
    bar = np.einsum("bl,kbl->bk", R.block_bar(e0.c.A), np.abs(D64).sum(axis=(3, 4)))
    d = np.abs(g2 - e.grad)
    print(f"[info reference] {e0.s.name}: worst |grad_ref - <G, dmvp>| / bar = {(d / bar).max():.4f}")
    assert (d <= bar).all() and np.abs(e.grad).max() > 0
    assert (e.info == e.info.transpose(0, 2, 1)).all() and (np.diagonal(e.info, axis1=1, axis2=2) >= 0).all()
    assert (np.abs(e.info) <= e.S * (1 + 1e-12)).all() and (np.abs(e.grad) <= e.Sg * (1 + 1e-12)).all()
    if key[0] != "ties":          # no pixel of the robot scenes has a J within rounding of zero: their count is exact
        assert (e.count == e.count_max).all() and (e.count > 0).all()


def test_probing_every_pixel_finds_nothing_outside_the_probe_set(oracle, xarm7):
    s = R.scene_for(xarm7, ("ties",))
    D = IR.tangents_for(xarm7, ("ties",), 17)
    soft = IR.rendered(oracle, s.meshes, s.mvp, s.H, s.W)
    every = IR.rendered(oracle, s.meshes, s.mvp, s.H, s.W, probe="all")
    assert every.nprobe.sum() == s.B * s.L * s.H * s.W and soft.nprobe.sum() < every.nprobe.sum() / 4
    Js, As = IR.pixel_jacobians(s.meshes, soft.probes, (s.B, s.H, s.W), D)
    Je, Ae = IR.pixel_jacobians(s.meshes, every.probes, (s.B, s.H, s.W), D)
    assert (Js == Je).all() and (As == Ae).all() and (As > 0).any()


# ---- tangent builders against finite differences ----------------------------------------------------------------------------
def _close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() <= rel * np.abs(b).max()


def test_tangent_builders_match_finite_differences(oracle, xarm7):
    from easyhec_amd import information as I
    p = IR.gauge_problem(oracle, xarm7)
    K, lp, dof = torch.from_numpy(p.K), torch.from_numpy(p.lp), I._f64(p.dof)
    f = lambda K_, d_, lp_: I._mvp64(K_, p.H, p.W, d_, lp_, 0.001, 10.0)
    T = I.pose_tangents(K, p.H, p.W, dof, lp)
    assert T.shape == (6,) + tuple(lp.shape) and T.dtype == torch.float64
    h = 1e-6
    for i in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[i] = h
        assert _close(T[i], (f(K, dof + e, lp) - f(K, dof - e, lp)) / (2 * h), 1e-7), i
    # the float64 product is fused.mvp_matrices' (float32 there)
    from easyhec_amd import fused
    from easyhec_amd.se3 import se3_exp_map
    Tc32 = se3_exp_map(p.dof[None]).permute(0, 2, 1)[0]
    m32 = fused.mvp_matrices(K.float(), p.H, p.W, Tc32, lp.float())
    assert _close(m32.double(), f(K, dof, lp), 1e-5)
    # intrinsics: every name, and the tied focal length
    th = torch.tensor([0.01, -0.02, 0.003, -0.004], dtype=torch.float64)
    Ti, names = I.intrinsics_tangents(K, th, ("f", "cx", "cy"), p.H, p.W, dof, lp)
    assert names == ["theta[f]", "theta[cx]", "theta[cy]"]
    from easyhec_amd.intrinsics_calib import intrinsics_from_theta
    for col, de in zip(Ti, ([1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1])):
        de = torch.tensor(de, dtype=torch.float64) * h
        fd = (f(I._K_of_theta(K, th + de, p.H, p.W), dof, lp) - f(I._K_of_theta(K, th - de, p.H, p.W), dof, lp)) / (2 * h)
        assert _close(col, fd, 1e-7)
    K32 = intrinsics_from_theta(p.K.astype(np.float32), th.numpy(), p.H, p.W)
    assert _close(I._K_of_theta(torch.from_numpy(p.K.astype(np.float32).astype(np.float64)), th, p.H, p.W), K32, 2e-7)
    # joints: the central difference against a step ten times smaller and against the analytic twist of a revolute joint
    off = np.zeros(p.rb.chain.dof)
    Tj = I.joint_tangents(p.rb, p.q, off, [0, 3], K, p.H, p.W, dof)
    Tj2 = I.joint_tangents(p.rb, p.q, off, [0, 3], K, p.H, p.W, dof, h=1e-5)
    assert Tj.shape == (2,) + tuple(lp.shape) and _close(Tj, Tj2, 1e-7)
    # joint 0 of the arm without its base link: the offset's tangent is a rotation of everything rendered about the base
    # axis, i.e. a combination of the six pose tangents -- the gauge, exactly
    A = T.reshape(6, -1).T.numpy()
    coef, res, _, _ = np.linalg.lstsq(A, Tj[0].reshape(-1).numpy(), rcond=None)
    assert np.abs(A @ coef - Tj[0].reshape(-1).numpy()).max() <= 1e-6 * np.abs(Tj[0].numpy()).max()
    coef3 = np.linalg.lstsq(A, Tj[1].reshape(-1).numpy(), rcond=None)[0]
    assert np.abs(A @ coef3 - Tj[1].reshape(-1).numpy()).max() >= 1e-2 * np.abs(Tj[1].numpy()).max()


# ---- the report ---------------------------------------------------------------------------------------------------------------
def test_report_algebra():
    from easyhec_amd.information import InformationReport
    rng = np.random.default_rng(0)
    Jm = rng.normal(size=(40, 5)) * np.array([1.0, 1e3, 1e-2, 5.0, 0.0])          # mixed units; parameter 4 is never seen
    Jm[:, 3] = 2.0 * Jm[:, 0] + 1e-3 * rng.normal(size=40)                          # parameter 3 nearly repeats parameter 0
    Hv = np.stack([Jm[:20].T @ Jm[:20], Jm[20:].T @ Jm[20:]])
    names = ["a", "b", "c", "d", "dead"]
    r = InformationReport(Hv, names, count=[20, 20], loss=[3.0, 4.0])
    assert r.no_information == ["dead"] and np.allclose(r.H, Jm.T @ Jm) and len(r.eigenvalues) == 4
    assert np.allclose(np.diag(r.scaled), 1.0) and abs(r.eigenvalues.sum() - 4.0) < 1e-12
    weak = r.weak_directions(1e-3)
    assert len(weak) == 1 and {nm for nm, _ in weak[0][1][:2]} == {"a", "d"} and r.eigenvectors[4].tolist() == [0.0] * 4
    assert r.condition > 1e6
    # the Schur complement is the inverse of the covariance block (on the seen parameters)
    live = [0, 1, 2, 3]
    cov = np.linalg.inv(r.H[np.ix_(live, live)])
    m = r.marginal_information(["a", "b"])
    assert np.allclose(np.linalg.inv(m), cov[:2, :2], rtol=1e-5)
    assert abs(r.sigma2() - 7.0 / 35.0) < 1e-15 and np.allclose(r.covariance()[:4, :4], r.sigma2() * cov, rtol=1e-5)
    assert (r.covariance()[4] == 0).all()


# ---- the gauge scenes (tests/test_gpu_information.py::test_reports_*) --------------------------------------------------------
def test_gauge_scenes_show_their_gauges(oracle, xarm7):
    """The conditions the GPU report tests rely on, for the reference alone.  Figures (profiles/information.md):
    joint 0 freed, no base link: scaled eigenvalues 4e-16 | 1.3e-2 ...; frozen: 7e-3 ... 3.0, condition 416;
    rig: marginal information of offset[0] 9e-10 for the camera that does not see the base, 29.07 with the second camera."""
    from easyhec_amd.information import InformationReport
    p = IR.gauge_problem(oracle, xarm7)
    _, _, names, e = IR.gauge_reference(oracle, p, [0])
    r = InformationReport(e.info, names, e.grad, e.count, e.loss)
    tol = IR.scaled_tolerance(r.H, e.S.sum(axis=0), e.L)
    print(f"[gauge] free joint 0: eigenvalues {r.eigenvalues}, direction {r.direction(0)[:4]}, kernel tolerance {tol:.2e}")
    assert abs(r.eigenvalues[0]) * 1e3 <= r.eigenvalues[1] and tol * 10 <= r.eigenvalues[1]   # the gap, and the bar resolves it
    top = [nm for nm, _ in r.direction(0)[:3]]
    assert "offset[0]" in top and any(nm in top for nm in ("dof[3]", "dof[4]", "dof[5]"))
    weak = r.weak_directions(1e-3)
    assert len(weak) == 1 and abs(r.marginal_information("offset[0]")[0, 0]) <= 1e-9 * r.H[6, 6]
    _, _, names0, e0 = IR.gauge_reference(oracle, p, [])
    r0 = InformationReport(e0.info, names0)
    print(f"[gauge] control: eigenvalues {r0.eigenvalues}, condition {r0.condition:.0f}")
    assert r0.weak_directions(1e-3) == [] and (r0.eigenvalues[:-1] / r0.eigenvalues[1:]).min() >= 0.1 and r0.condition < 1e3
    # the rig: camera A frames the base link out (its own marginal information of offset[0] is zero: the gauge), camera B
    # from another azimuth sees the base
    pa = IR.gauge_problem(oracle, xarm7, IR.GAUGE_AZIMUTHS[0], base=True, frame_base_out=True)
    pb = IR.gauge_problem(oracle, xarm7, IR.GAUGE_AZIMUTHS[1], base=True)
    ea, eb = IR.gauge_reference(oracle, pa, [0])[3], IR.gauge_reference(oracle, pb, [0])[3]
    assert ea.nprobe[:, 0].sum() == 0 and eb.nprobe[:, 0].sum() > 0                 # who sees the base link
    ra = InformationReport(ea.info, names)
    Hc, _ = IR.embed_rig([ea, eb], 1)
    rig = InformationReport(Hc, [f"cam{c}.dof[{i}]" for c in range(2) for i in range(6)] + ["offset[0]"])
    ma, mr = ra.marginal_information("offset[0]")[0, 0], rig.marginal_information("offset[0]")[0, 0]
    print(f"[gauge] rig: marginal information of offset[0]: camera A alone {ma:.3e}, rig {mr:.3e}")
    assert mr >= 1e3 * max(abs(ma), 1e-9 * ra.H[6, 6]) and mr > 1.0
