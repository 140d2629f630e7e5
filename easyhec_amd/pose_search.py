"""Pose search: score candidate camera poses by mask overlap, hand the best to the multi-start solve.

The solve of :class:`easyhec_amd.fast.FusedPoseStep` is local, and :func:`easyhec_amd.multistart.sample_starts` draws its
starts blind.  Here a few thousand candidate poses are scored against the observed masks in ONE ``ehr_mask_overlap`` call
(include/ehr.h): per (candidate, view) the exact integers |render|, |render & ref| and |ref|, from
which the non-antialiased SSE of the solver (``xor``) and the silhouette IoU follow.  The best candidates become the starts
of :func:`easyhec_amd.multistart.solve_multistart`; start 0 is always the pose the caller already has, and every
hypothesis equals its solo solve bit for bit, so searching is never worse than not searching.  HIP only: CPU tensors
raise, there is no fallback."""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .multistart import rank_losses, sample_starts, solve_multistart

__all__ = ["mask_overlap", "mask_overlap_valid", "overlap_scores", "candidate_mvps", "search_starts", "solve_global", "PoseSearchResult"]


def mask_overlap(glctx, scene, mvp, ref, chunk_views=0):
    """mvp [Q,S,L,4,4] float32 (candidate pose q seen in real view s), ref [S,H,W] float masks (row 0 = top, foreground iff
    > 0.5), both on the HIP device -> ``(inter [Q,S], area [Q,S], ref_area [S])``, int64 on the device:
    ``area`` = |render|, ``inter`` = |render & ref_s|, ``ref_area`` = |ref_s|; exact and order independent."""
    if mvp.dim() != 5 or mvp.shape[-2:] != (4, 4):
        raise ValueError("mvp must be [Q,S,L,4,4]")
    if ref.dim() != 3:
        raise ValueError("ref must be [S,H,W]")
    if not mvp.is_cuda or not ref.is_cuda:
        raise RuntimeError("mask_overlap: tensors must live on the HIP device (there is no CPU path)")
    if not _lib.has_pose_search():
        raise RuntimeError("libehr_hip.so has no ehr_mask_overlap: rebuild it (python -m easyhec_amd.build)")
    Q, S, L = mvp.shape[:3]
    if L != scene.num_links:
        raise ValueError(f"mvp has {L} links, the scene {scene.num_links}")
    if ref.shape[0] != S:
        raise ValueError(f"mvp has {S} views, ref {ref.shape[0]}")
    if ref.device != mvp.device:
        raise ValueError("mvp and ref must be on the same device")
    H, W = int(ref.shape[1]), int(ref.shape[2])
    mvp = mvp.contiguous().float()
    ref = ref.contiguous().float()
    overlap = torch.empty((Q, S, 2), dtype=torch.int64, device=mvp.device)
    ref_area = torch.empty((S,), dtype=torch.int64, device=mvp.device)
    with torch.cuda.device(mvp.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().ehr_mask_overlap(glctx.handle, _lib.ptr(scene.verts), _lib.ptr(scene.tris),
                                               _lib.ptr(scene.vert_link), _lib.ptr(mvp), _lib.ptr(ref), Q, S, L,
                                               scene.num_verts, scene.num_tris, H, W, _lib.ptr(overlap), _lib.ptr(ref_area),
                                               int(chunk_views), stream), "ehr_mask_overlap")
    return overlap[..., 0], overlap[..., 1], ref_area


def mask_overlap_valid(glctx, scene, mvp, ref, weight, chunk_views=0):
    """:func:`mask_overlap` restricted to the pixels a per-pixel loss weight trusts, ``valid = weight > 0`` ([S,H,W], the
    ``batch['weight']`` of a weighted solve): ``inter`` = |render & ref & valid|, ``area`` = |render & valid|, ``ref_area`` =
    |ref & valid|, so that :func:`overlap_scores` gives ``xor_valid = |render & valid| + |ref & valid| - 2 |render & ref &
    valid|`` and the IoU on the valid pixels.  Two ``ehr_mask_overlap`` calls, exact integers: one against ``valid`` as the
    reference, one against ``ref & valid``."""
    if weight.shape != ref.shape or weight.device != ref.device:
        raise ValueError("weight must have ref's shape and device")
    valid = (weight > 0).float()
    area_v, _, _ = mask_overlap(glctx, scene, mvp, valid, chunk_views=chunk_views)
    inter_v, _, ref_area_v = mask_overlap(glctx, scene, mvp, (ref > 0.5).float() * valid, chunk_views=chunk_views)
    return inter_v, area_v, ref_area_v


def overlap_scores(inter, area, ref_area):
    """``(xor [Q] int64, iou [Q] float64)`` from the integers of :func:`mask_overlap` (any device).
    ``xor[q] = sum_s (area + ref_area - 2 inter)`` = sum_s |render xor ref_s|: for binary masks the solver's SSE without
    antialiasing, summed over the views.  ``iou[q]`` = mean over the views of inter / (area + ref_area - inter), 1.0 where
    the union is empty."""
    inter, area = torch.as_tensor(inter).long(), torch.as_tensor(area).long()
    ra = torch.as_tensor(ref_area).long().to(inter.device)[None, :]
    xor = (area + ra - 2 * inter).sum(dim=1)
    union = area + ra - inter
    iou = torch.where(union > 0, inter.double() / union.clamp(min=1).double(), torch.ones_like(union, dtype=torch.float64))
    return xor, iou.mean(dim=1)


def candidate_mvps(K, H, W, Tc_c2b, link_poses, n=0.001, f=10.0):
    """[Q,Bv,L,4,4] = proj(K) @ (opencv2blender @ (Tc_c2b[q] @ link_poses[v,l])): the projection, flip and association of
    :func:`easyhec_amd.fused.mvp_matrices`, for Q candidate poses in one batched expression on Tc_c2b's device."""
    from .nvdiffrast_utils import K_to_projection, opencv2blender
    proj = K_to_projection(K, H, W, n=n, f=f).to(Tc_c2b.device)
    o2b = opencv2blender(device=Tc_c2b.device)
    Tc_c2l = Tc_c2b[:, None, None] @ link_poses[None]
    return proj @ (o2b @ Tc_c2l)


@dataclass
class PoseSearchResult:
    starts: np.ndarray          # [P,4,4] float64: Tc_init, then the best P - 1 other candidates in rank order
    candidates: np.ndarray      # [Q(+extra),4,4] float64 every scored pose; candidate 0 is Tc_init
    xor: torch.Tensor           # [Q] int64 (CPU): sum over the views of |render xor ref|
    iou: torch.Tensor           # [Q] float64 (CPU): mean silhouette IoU over the views
    ranking: list               # candidate indices, best (smallest xor) first, ties by index
    inter: torch.Tensor         # [Q,Bv] int64 (CPU)
    area: torch.Tensor          # [Q,Bv] int64 (CPU)
    ref_area: torch.Tensor      # [Bv] int64 (CPU)


def search_starts(model, batch, Tc_init, Q, P, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0, extra=None, chunk_views=0):
    """Scores Q candidate poses around ``Tc_init`` (:func:`easyhec_amd.multistart.sample_starts`: candidate 0 is ``Tc_init``
    itself; ``extra`` [E,4,4]: further poses of the caller's, scored after them) against ``batch['mask']`` in one
    :func:`mask_overlap` call and returns the P starts for :func:`easyhec_amd.multistart.solve_multistart`: start 0 is
    ALWAYS ``Tc_init``, then the best P - 1 other candidates by ``xor`` (ascending, ties by index).  With per-pixel weights
    (``batch['weight']``) the candidates are ranked on the valid pixels only (:func:`mask_overlap_valid`); the integers
    returned are then the restricted ones."""
    for k in ("mask", "link_poses", "K"):
        if not torch.is_tensor(batch[k]) or batch[k].device.type != "cuda":
            raise RuntimeError(f"search_starts: batch['{k}'] must be a tensor on the HIP device (there is no CPU path)")
    dev = batch["mask"].device
    if P < 1 or Q < P:
        raise ValueError("search_starts: need 1 <= P <= Q")
    Tc_init = np.asarray(Tc_init, dtype=np.float64)
    cands = sample_starts(Tc_init, Q, trans_sigma_m, rot_sigma_deg, seed=seed)
    if extra is not None:
        cands = np.concatenate([cands, np.asarray(extra, dtype=np.float64).reshape(-1, 4, 4)])
    H, W = model.H, model.W
    ref = batch["mask"].to(dev, torch.float32)
    lp = batch["link_poses"].to(dev, torch.float32)
    mvp = candidate_mvps(batch["K"][0].to(dev, torch.float32), H, W, torch.tensor(cands, dtype=torch.float32, device=dev), lp)
    if batch.get("weight") is not None:
        inter, area, ref_area = mask_overlap_valid(model._ensure_renderer().glctx, model._ensure_scene(), mvp, ref,
                                                   batch["weight"].to(dev, torch.float32), chunk_views=chunk_views)
    else:
        inter, area, ref_area = mask_overlap(model._ensure_renderer().glctx, model._ensure_scene(), mvp, ref,
                                             chunk_views=chunk_views)
    xor, iou = overlap_scores(inter, area, ref_area)
    xor, iou = xor.cpu(), iou.cpu()
    ranking = rank_losses(xor.numpy())
    picked = [0] + [i for i in ranking if i != 0][:P - 1]
    return PoseSearchResult(starts=cands[picked].copy(), candidates=cands, xor=xor, iou=iou, ranking=ranking,
                            inter=inter.cpu(), area=area.cpu(), ref_area=ref_area.cpu())


def solve_global(cfg, model, batch, Tc_init, Q, P, num_steps, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0, tail=20,
                 slack=None, extra=None):
    """:func:`search_starts`, then :func:`easyhec_amd.multistart.solve_multistart` from its starts ->
    ``(PoseSearchResult, MultiStartResult)``; ``model.dof`` holds the winner.  Hypothesis 0 is the plain solve from
    ``Tc_init``, bit for bit, so the winner's tail loss never exceeds it."""
    search = search_starts(model, batch, Tc_init, Q, P, trans_sigma_m, rot_sigma_deg, seed, extra=extra)
    return search, solve_multistart(cfg, model, batch, search.starts, num_steps, tail=tail, slack=slack)
