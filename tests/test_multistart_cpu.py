"""Multi-start solve, the parts that need no GPU: the C ABI declares and exports the batched step, the start sampler is
deterministic and has the requested spread, the ranking rule, and the loud failure on CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_multi_start_step():
    from easyhec_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "ehr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+ehr_solver_step_multi\s*\(([^;]*)\)\s*;", text)
    assert m, "include/ehr.h does not declare ehr_solver_step_multi"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 39 and "int P" in args and "int Bv" in args and not any("defer_adam" in a for a in args)
    assert re.search(r"int\s+ehr_fused_bind_ref_shared\s*\(", text)
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(so, "ehr_solver_step_multi") and hasattr(so, "ehr_fused_bind_ref_shared")
    assert _lib.has_multistart()
    assert len(_lib.SIGNATURES["ehr_solver_step_multi"][1]) == len(args)
    assert _lib.lib().ehr_version() == 8  # the symbol, not the version, is the capability check


def test_sample_starts_is_deterministic_and_start_zero_is_the_init():
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.synthetic import camera_Tc_c2b
    Tc = camera_Tc_c2b()
    a, b = sample_starts(Tc, 16, 0.03, 4.0, seed=5), sample_starts(Tc, 16, 0.03, 4.0, seed=5)
    assert a.shape == (16, 4, 4) and a.dtype == np.float64 and np.array_equal(a, b)
    assert np.array_equal(a[0], Tc)
    assert not np.array_equal(a, sample_starts(Tc, 16, 0.03, 4.0, seed=6))
    assert np.array_equal(sample_starts(Tc, 4, 0.03, 4.0, seed=5), a[:4])  # a prefix of the larger draw
    for T in a:  # rigid poses
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and np.allclose(T[3], [0, 0, 0, 1])


@pytest.mark.parametrize("ts,rs", [(0.03, 4.0), (0.06, 8.0)])
def test_sample_starts_has_the_requested_spread(ts, rs):
    """start = init @ exp([dt, drot]) with dt ~ N(0, ts) m, drot ~ N(0, rs) deg per axis: over 4000 draws the sample standard
    deviation of every component is within 5 % of the request (its own standard error is 1.1 %)."""
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.synthetic import camera_Tc_c2b
    Tc = camera_Tc_c2b()
    D = np.linalg.inv(Tc)[None] @ sample_starts(Tc, 4001, ts, rs, seed=0)[1:]
    dt = D[:, :3, 3]
    ang = np.degrees(np.arccos(np.clip((np.trace(D[:, :3, :3], axis1=1, axis2=2) - 1) / 2, -1, 1)))
    axis = np.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], axis=1)
    rot = axis / np.linalg.norm(axis, axis=1, keepdims=True) * ang[:, None]  # rotation vectors, degrees
    assert np.all(np.abs(dt.std(axis=0) / ts - 1) < 0.05), dt.std(axis=0)
    assert np.all(np.abs(rot.std(axis=0) / rs - 1) < 0.05), rot.std(axis=0)
    assert np.all(np.abs(dt.mean(axis=0)) < 0.1 * ts) and np.all(np.abs(rot.mean(axis=0)) < 0.1 * rs)


def test_ranking_puts_nan_last_and_breaks_ties_by_index():
    from easyhec_amd.multistart import rank_losses
    nan = float("nan")
    assert rank_losses([3.0, nan, 1.0, 1.0, nan, 0.5]) == [5, 2, 3, 0, 1, 4]
    assert rank_losses([nan, nan]) == [0, 1]
    assert rank_losses(torch.tensor([2.0, 2.0, 2.0]).numpy()) == [0, 1, 2]
    assert rank_losses([float("inf"), nan, 7.0]) == [2, 0, 1]


def test_cpu_tensors_raise(xarm7):
    from easyhec_amd.config import Cfg
    from easyhec_amd.multistart import MultiStartPoseStep, sample_starts, solve_multistart
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = 48, 64
    cfg.model.rbsolver.init_Tc_c2b = camera_Tc_c2b().tolist()
    model = RBSolver(cfg, meshes=xarm7.meshes[:2])  # on the CPU
    batch = {"mask": torch.zeros(1, 48, 64), "link_poses": torch.eye(4)[None, None].repeat(1, 2, 1, 1),
             "K": torch.eye(3)[None]}
    starts = sample_starts(camera_Tc_c2b(), 3)
    with pytest.raises(RuntimeError):
        MultiStartPoseStep(model, batch, starts)
    with pytest.raises(RuntimeError):
        solve_multistart(cfg, model, batch, starts, 2)
    with pytest.raises(ValueError):
        sample_starts(np.eye(3), 2)
    if torch.cuda.is_available():  # a model on the device with a batch left on the CPU
        with pytest.raises(RuntimeError):
            MultiStartPoseStep(model.cuda(), batch, starts)
