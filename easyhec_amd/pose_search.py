"""Pose search: score candidate camera poses by mask overlap, hand the best to the multi-start solve.

The solve of :class:`easyhec_amd.fast.FusedPoseStep` is local, and :func:`easyhec_amd.multistart.sample_starts` draws its
starts blind.  Here a few thousand candidate poses are scored against the observed masks in ONE ``ehr_mask_overlap`` call
(include/ehr.h): per (candidate, view) the exact integers |render|, |render & ref| and |ref|, from
which the non-antialiased SSE of the solver (``xor``) and the silhouette IoU follow.  The best candidates become the starts
of :func:`easyhec_amd.multistart.solve_multistart`; start 0 is always the pose the caller already has, and every
hypothesis equals its solo solve bit for bit, so searching is never worse than not searching.

``xor`` only means something while a candidate still overlaps the observed mask: without overlap it is area + ref_area,
which ranks a candidate by how small it renders.  ``score="soft"`` ranks by a soft IoU built on the
exact distance transform of the observed masks (``ehr_mask_distance``) and the cost sums of ``ehr_mask_cost``: it falls
with the distance to the observed mask for as long as the render is within ``cap_px`` pixels of it, so the candidates may
be drawn tens of centimetres and degrees wide.  HIP only: CPU tensors raise, there is no fallback."""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .fast import _hip_device
from .multistart import rank_losses, sample_starts, solve_multistart

__all__ = ["mask_overlap", "mask_overlap_valid", "overlap_scores", "mask_distance", "mask_cost", "soft_costs", "soft_iou_scores", "candidate_mvps",
           "search_starts", "solve_global", "PoseSearchResult"]


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


def mask_distance(glctx, ref, cap_px):
    """ref [S,H,W] float masks on the HIP device (row 0 = top, foreground iff > 0.5, NaN is background) -> ``d2 [S,H,W]``
    int32 on the device: the exact squared Euclidean distance to the nearest foreground pixel of the same view, capped at
    ``cap_px ** 2`` (0 on the foreground; ``cap_px ** 2`` everywhere in a view without foreground).  ``cap_px`` in
    [1, 4096].  Launches only: no synchronisation."""
    if ref.dim() != 3:
        raise ValueError("ref must be [S,H,W]")
    if not ref.is_cuda:
        raise RuntimeError("mask_distance: ref must live on the HIP device (there is no CPU path)")
    if not _lib.has_soft_search():
        raise RuntimeError("libehr_hip.so has no ehr_mask_distance: rebuild it (python -m easyhec_amd.build)")
    S, H, W = (int(n) for n in ref.shape)
    ref = ref.contiguous().float()
    d2 = torch.empty((S, H, W), dtype=torch.int32, device=ref.device)
    with torch.cuda.device(ref.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().ehr_mask_distance(glctx.handle, _lib.ptr(ref), S, H, W, int(cap_px), _lib.ptr(d2), stream),
                   "ehr_mask_distance")
    return d2


def mask_cost(glctx, scene, mvp, cost, chunk_views=0):
    """mvp [Q,S,L,4,4] float32 as for :func:`mask_overlap`, cost [S,H,W] or [C,S,H,W] integer images (row 0 = top, any
    int32 values, C <= 4), both on the HIP device -> ``(area [Q,S], sums [Q,S,C])``, int64 on the device: ``area`` =
    |render|, ``sums[q,s,c]`` = the sum of ``cost[c,s]`` over the pixels of the render; exact and order independent.  The
    op reads int32: a wider integer tensor is converted, so its values must fit."""
    if mvp.dim() != 5 or mvp.shape[-2:] != (4, 4):
        raise ValueError("mvp must be [Q,S,L,4,4]")
    if cost.dim() == 3:
        cost = cost[None]
    if cost.dim() != 4:
        raise ValueError("cost must be [S,H,W] or [C,S,H,W]")
    if not mvp.is_cuda or not cost.is_cuda:
        raise RuntimeError("mask_cost: tensors must live on the HIP device (there is no CPU path)")
    if not _lib.has_soft_search():
        raise RuntimeError("libehr_hip.so has no ehr_mask_cost: rebuild it (python -m easyhec_amd.build)")
    if cost.dtype.is_floating_point or cost.dtype == torch.bool:
        raise ValueError("cost must be an integer tensor (its values are summed exactly)")
    Q, S, L = mvp.shape[:3]
    C = int(cost.shape[0])
    if L != scene.num_links:
        raise ValueError(f"mvp has {L} links, the scene {scene.num_links}")
    if not 1 <= C <= 4:
        raise ValueError(f"cost has {C} channels, 1 to 4 are supported")
    if cost.shape[1] != S:
        raise ValueError(f"mvp has {S} views, cost {cost.shape[1]}")
    if cost.device != mvp.device:
        raise ValueError("mvp and cost must be on the same device")
    H, W = int(cost.shape[2]), int(cost.shape[3])
    mvp = mvp.contiguous().float()
    cost = cost.contiguous().to(torch.int32)
    sums = torch.empty((Q, S, C + 1), dtype=torch.int64, device=mvp.device)
    with torch.cuda.device(mvp.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().ehr_mask_cost(glctx.handle, _lib.ptr(scene.verts), _lib.ptr(scene.tris), _lib.ptr(scene.vert_link),
                                            _lib.ptr(mvp), _lib.ptr(cost), C, Q, S, L, scene.num_verts, scene.num_tris, H, W,
                                            _lib.ptr(sums), int(chunk_views), stream), "ehr_mask_cost")
    return sums[..., 0], sums[..., 1:]


def soft_iou_scores(area, inter, ksum, ref_area, cap_px):
    """``soft [Q]`` float64 from the integers of :func:`mask_cost` (any device): per (candidate, view)
    ``ksum / (cap_px * union)`` with ``union = area + ref_area - inter`` (1.0 where the union is empty), then the mean over
    the views.  ``ksum`` is the sum over the render of ``k = cap_px - floor(sqrt(d2))``: ``cap_px`` on the reference,
    falling to 0 at ``cap_px`` pixels from it, so ``ksum <= cap_px * area <= cap_px * union`` and

    * ``0 <= soft <= 1``;
    * ``soft == 1`` iff every view renders exactly its reference (every rendered pixel on the reference and none of the
      reference left over);
    * ``soft == 0`` iff no render comes within ``cap_px`` pixels of its reference (a render that left the image
      included)."""
    area, inter, ksum = torch.as_tensor(area).long(), torch.as_tensor(inter).long(), torch.as_tensor(ksum).long()
    ra = torch.as_tensor(ref_area).long().to(area.device)[None, :]
    union = area + ra - inter
    soft = torch.where(union > 0, ksum.double() / (float(cap_px) * union.clamp(min=1).double()),
                       torch.ones_like(union, dtype=torch.float64))
    return soft.mean(dim=1)


def soft_costs(d2, cap_px, valid=None):
    """The cost images of the soft score from ``d2 [S,H,W]`` (:func:`mask_distance`), int32 on its device:
    ``[fg, k]`` with ``fg = d2 == 0`` and ``k = cap_px - floor(sqrt(d2))`` (in float64: exact for every d2 <= 4096 ** 2), or
    ``[fg & valid, k * valid, valid]`` under a bool ``valid [S,H,W]``."""
    fg = (d2 == 0).to(torch.int32)
    k = int(cap_px) - torch.floor(torch.sqrt(d2.double())).to(torch.int32)
    if valid is None:
        return torch.stack([fg, k])
    v = valid.to(torch.int32)
    return torch.stack([fg * v, k * v, v])


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
    ranking: list               # candidate indices, best first (smallest xor, or largest soft), ties by index
    inter: torch.Tensor         # [Q,Bv] int64 (CPU)
    area: torch.Tensor          # [Q,Bv] int64 (CPU)
    ref_area: torch.Tensor      # [Bv] int64 (CPU)
    soft: torch.Tensor = None   # [Q] float64 (CPU): the soft IoU (soft_iou_scores); None under score="xor"
    score: str = "xor"          # what `ranking` was made by


def search_starts(model, batch, Tc_init, Q, P, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0, extra=None, chunk_views=0,
                  score="xor", cap_px=None):
    """Scores Q candidate poses around ``Tc_init`` (:func:`easyhec_amd.multistart.sample_starts`: candidate 0 is ``Tc_init``
    itself; ``extra`` [E,4,4]: further poses of the caller's, scored after them) against ``batch['mask']`` in one
    :func:`mask_overlap` call and returns the P starts for :func:`easyhec_amd.multistart.solve_multistart`: start 0 is
    ALWAYS ``Tc_init``, then the best P - 1 other candidates by ``xor`` (ascending, ties by index).  With per-pixel weights
    (``batch['weight']``) the candidates are ranked on the valid pixels only (:func:`mask_overlap_valid`); the integers
    returned are then the restricted ones.

    ``score="soft"``: one :func:`mask_distance` of the masks (``cap_px``, default ``max(H, W) // 4``) and one
    :func:`mask_cost` call instead; the candidates are ranked by :func:`soft_iou_scores`, descending, ties by index.
    ``xor`` and ``iou`` are still filled in, from the same call's integers.  Under weights every cost image is multiplied
    by ``valid = weight > 0`` and a third channel gives the restricted area."""
    if score not in ("xor", "soft"):
        raise ValueError(f"search_starts: score must be 'xor' or 'soft', got {score!r}")
    dev = _hip_device("search_starts", model, batch)
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
    glctx, scene, soft = model._ensure_renderer().glctx, model._ensure_scene(), None
    if score == "soft":
        cap = max(H, W) // 4 if cap_px is None else int(cap_px)
        d2 = mask_distance(glctx, ref, cap)
        valid = None
        if batch.get("weight") is not None:
            if batch["weight"].shape != ref.shape:
                raise ValueError("weight must have the masks' shape")
            valid = batch["weight"].to(dev) > 0
        cost = soft_costs(d2, cap, valid)
        area, sums = mask_cost(glctx, scene, mvp, cost, chunk_views=chunk_views)
        inter, ksum = sums[..., 0], sums[..., 1]
        if valid is not None:
            area = sums[..., 2]
        ref_area = cost[0].sum(dim=(1, 2), dtype=torch.int64)
        soft = soft_iou_scores(area, inter, ksum, ref_area, cap).cpu()
    elif batch.get("weight") is not None:
        inter, area, ref_area = mask_overlap_valid(glctx, scene, mvp, ref, batch["weight"].to(dev, torch.float32),
                                                   chunk_views=chunk_views)
    else:
        inter, area, ref_area = mask_overlap(glctx, scene, mvp, ref, chunk_views=chunk_views)
    xor, iou = overlap_scores(inter, area, ref_area)
    xor, iou = xor.cpu(), iou.cpu()
    ranking = rank_losses(xor.numpy() if soft is None else -soft.numpy())
    picked = [0] + [i for i in ranking if i != 0][:P - 1]
    return PoseSearchResult(starts=cands[picked].copy(), candidates=cands, xor=xor, iou=iou, ranking=ranking,
                            inter=inter.cpu(), area=area.cpu(), ref_area=ref_area.cpu(), soft=soft, score=score)


def solve_global(cfg, model, batch, Tc_init, Q, P, num_steps, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0, tail=20,
                 slack=None, extra=None, score="xor", cap_px=None):
    """:func:`search_starts`, then :func:`easyhec_amd.multistart.solve_multistart` from its starts ->
    ``(PoseSearchResult, MultiStartResult)``; ``model.dof`` holds the winner.  Hypothesis 0 is the plain solve from
    ``Tc_init``, bit for bit, so the winner's tail loss never exceeds it.  ``score`` and ``cap_px`` go to
    :func:`search_starts`."""
    search = search_starts(model, batch, Tc_init, Q, P, trans_sigma_m, rot_sigma_deg, seed, extra=extra, score=score, cap_px=cap_px)
    return search, solve_multistart(cfg, model, batch, search.starts, num_steps, tail=tail, slack=slack)
