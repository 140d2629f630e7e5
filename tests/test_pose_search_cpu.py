"""Pose search, the parts that need no GPU: the C ABI declares and exports the overlap op, the score arithmetic on
hand-written integers, the batched candidate matrices against the per-pose expression, and the loud failure on CPU
tensors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_overlap_op():
    from easyhec_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "ehr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+ehr_mask_overlap\s*\(([^;]*)\)\s*;", text)
    assert m, "include/ehr.h does not declare ehr_mask_overlap"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 17 and "const float* ref" in args and "int64_t* overlap" in args and "int64_t* ref_area" in args
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ehr_mask_overlap")
    assert _lib.has_pose_search()
    assert len(_lib.SIGNATURES["ehr_mask_overlap"][1]) == len(args)
    assert _lib.lib().ehr_version() == 8  # the symbol, not the version, is the capability check


def test_overlap_scores_on_hand_written_integers():
    from easyhec_amd.pose_search import overlap_scores
    #                 view 0            view 1 (reference empty)
    inter = torch.tensor([[6, 0], [0, 0], [10, 0]])
    area = torch.tensor([[8, 3], [0, 0], [10, 0]])
    ref_area = torch.tensor([10, 0])
    xor, iou = overlap_scores(inter, area, ref_area)
    assert xor.dtype == torch.int64 and iou.dtype == torch.float64
    # candidate 0: |xor| = (8 + 10 - 12) + 3 = 9; IoU = mean(6 / 12, 0 / 3)
    # candidate 1: renders nothing: |xor| = 10; IoU = mean(0 / 10, empty union -> 1)
    # candidate 2: the reference itself: |xor| = 0; IoU = mean(1, empty union -> 1)
    assert xor.tolist() == [9, 10, 0]
    assert iou.tolist() == [0.25, 0.5, 1.0]
    xor_np, _ = overlap_scores(inter.numpy(), area.numpy(), ref_area.numpy())   # anything as_tensor takes
    assert xor_np.tolist() == [9, 10, 0]


def test_candidate_mvps_is_the_per_pose_expression_batched():
    from easyhec_amd.fused import mvp_matrices
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.pose_search import candidate_mvps
    from easyhec_amd.synthetic import camera_Tc_c2b
    g = torch.Generator().manual_seed(0)
    K = torch.tensor([[300.0, 0, 80], [0, 300.0, 60], [0, 0, 1]])
    lp = torch.eye(4).repeat(3, 2, 1, 1)
    lp[..., :3, 3] = torch.randn((3, 2, 3), generator=g) * 0.1
    Tc = torch.tensor(sample_starts(camera_Tc_c2b(), 5, seed=1), dtype=torch.float32)
    got = candidate_mvps(K, 120, 160, Tc, lp)
    assert got.shape == (5, 3, 2, 4, 4)
    for q in range(5):
        assert torch.allclose(got[q], mvp_matrices(K, 120, 160, Tc[q], lp), rtol=1e-6, atol=1e-7)


def test_cpu_tensors_raise(xarm7):
    from easyhec_amd.config import Cfg
    from easyhec_amd.pose_search import mask_overlap, search_starts, solve_global
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = 48, 64
    cfg.model.rbsolver.init_Tc_c2b = camera_Tc_c2b().tolist()
    model = RBSolver(cfg, meshes=xarm7.meshes[:2])  # on the CPU
    batch = {"mask": torch.zeros(1, 48, 64), "link_poses": torch.eye(4)[None, None].repeat(1, 2, 1, 1),
             "K": torch.eye(3)[None]}
    with pytest.raises(RuntimeError):
        search_starts(model, batch, camera_Tc_c2b(), 8, 2)
    with pytest.raises(RuntimeError):
        solve_global(cfg, model, batch, camera_Tc_c2b(), 8, 2, 3)
    with pytest.raises(RuntimeError):
        mask_overlap(None, None, torch.zeros(2, 1, 2, 4, 4), torch.zeros(1, 48, 64))
    with pytest.raises(ValueError):
        mask_overlap(None, None, torch.zeros(2, 1, 2, 4), torch.zeros(1, 48, 64))
