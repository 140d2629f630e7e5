"""Multi-start Levenberg-Marquardt: P start poses of ONE calibration problem refined together, one launch chain per iteration
whatever P is (``ehr_lm_linearize_multi`` / ``ehr_lm_update_multi`` in include/ehr.h, csrc/ehr_lm.hip; DESIGN.md section 6m,
INTEGRATION.md 4a-8).

:func:`easyhec_amd.multistart.solve_multistart` advances P hypotheses in one chain, but by Adam: a learning rate, a fixed number
of steps, a ranking by the mean of a noisy tail.  :func:`easyhec_amd.lm.solve_lm` has none of those -- it is monotone, stops
by itself and ends on an exact loss -- but takes one hypothesis.  Here hypothesis p on real view j is virtual view
``p * Bv + j`` of ONE ``ehr_mask_information`` call (a view's result depends on nothing but the view), the linearisation is one
thread per matrix over all of them, and the update is one workgroup per hypothesis on its own state block:

    ehr_lm_linearize_multi  ->  ehr_mask_information (P * Bv views)  ->  ehr_lm_update_multi

Every hypothesis is, bit for bit, its solo ``solve_lm`` on a ``FusedPoseStep`` built on that start
(tests/test_gpu_lm_multi.py).  Pose only: no joint offsets, no intrinsics.  HIP only; no fallback.

This module holds what is particular to P starts: the context of its own, the tiled reference, the two ``_multi`` C calls
and the ranked result.  The iteration and the solve loop are :mod:`easyhec_amd.lm`'s, the slot policy and the recovery
:class:`easyhec_amd.chain_step._PlannedContext`'s."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, dr, fused
from .chain_step import _PlannedContext
from .fast import _hip_device, _private_weight
from .lm import WHY, _LmDriver, _no_prior_arguments, _run_to_convergence
from .multistart import _starts_to_dof, rank_losses
from .se3 import se3_exp_map

__all__ = ["MultiStartLM", "MultiLmResult", "solve_lm_multi", "solve_global_lm", "group_basins"]

NAMES = [f"dof[{i}]" for i in range(6)]


def group_basins(poses, ranking, trans_tol_m=1e-3, rot_tol_deg=0.1):
    """Which hypotheses ended on the same optimum.  ``poses`` [P,4,4] (``Tc_c2b``), ``ranking``: the hypotheses best first.
    Walks them in rank order: a hypothesis joins the FIRST basin whose representative -- its best-ranked member -- lies
    within both tolerances of it (``|t_a - t_b|`` in metres, the angle of ``R_a^T R_b`` in degrees), otherwise it opens a
    basin.  A pose that is not finite forms a basin of its own, behind the others.  Returns the basins as lists of hypothesis
    indices, each in rank order, the basin of the best hypothesis first.  The defaults are the 1 mm / 0.1 degrees this
    package's tests call "the same pose".  Pure numpy."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    basins, lost = [], []
    for p in ranking:
        T = poses[p]
        if not np.isfinite(T).all():
            lost.append([p])
            continue
        for basin in basins:
            R = poses[basin[0]]
            cos = np.clip((np.trace(R[:3, :3].T @ T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
            if np.linalg.norm(R[:3, 3] - T[:3, 3]) <= trans_tol_m and np.degrees(np.arccos(cos)) <= rot_tol_deg:
                basin.append(p)
                break
        else:
            basins.append([p])
    return basins + lost


class MultiStartLM(_PlannedContext, _LmDriver):
    """:class:`easyhec_amd.lm.LevenbergMarquardt` for P hypotheses of one problem (``starts``: [P,4,4] poses or [P,6] dofs, as
    for :class:`easyhec_amd.multistart.MultiStartPoseStep`).  ``lambda0``, ``ftol``, ``lambda_max``, ``log_rows``: as there,
    per hypothesis; ``slack``: job slots per tile of a VIRTUAL view, as for the launch-chain steps.

    It works on a rasterizer context of its OWN and the model's scene: the model is read (meshes, image size), never written,
    and its context keeps its plan.  State lives in this object: ``dof`` [P,6] (a trial is in it between iterations),
    ``state_block`` [P,EHR_LM_STATE_DOUBLES] float64, ``log`` [P,log_rows,4].  ``K`` and ``link_poses`` are shared by the
    hypotheses, and so are the weights ([Bv,H,W], view b reads image b % Bv).  The reference masks are NOT: the information op
    has no shared-reference form, so a private copy is tiled P times -- ``P * Bv * H * W * 4`` bytes, 236 MB for 8 hypotheses
    x 8 views at 1280x720 -- beside the context's scratch for ``P * Bv`` views.

    ``iterate(n)`` enqueues n iterations of every hypothesis and never synchronises (a hypothesis that is done only has its
    accepted pose restored; its views are still rendered); ``state()`` makes one copy; ``finalize()`` leaves the accepted
    poses in ``dof``.  The buffers, the guard and the iteration are :class:`easyhec_amd.lm._LmDriver`'s; the slot policy, the
    plan with its bindings and ``recover_from_overflow()`` -- call it when iterations were reported -- are
    :class:`easyhec_amd.chain_step._PlannedContext`'s, as for the launch-chain steps."""
    who = "MultiStartLM"

    def __init__(self, model, batch, starts, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, near=0.001, far=10.0,
                 slack=None):
        self.dev = dev = _hip_device("MultiStartLM", model, batch)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("MultiStartLM: not available while a graph is being captured: ehr_mask_information sizes its "
                               "scratch on the first call")
        if not _lib.has_lm_multi():
            raise RuntimeError("this libehr_hip.so has no multi-start Levenberg-Marquardt kernels (ehr_lm_linearize_multi): "
                               "rebuild it")
        if not _lib.has_information():
            raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")
        self.model = model
        self.scene = model._ensure_scene()
        self.glctx = dr.RasterizeCudaContext(device=dev)
        self.H, self.W = model.H, model.W
        self.weight = _private_weight(batch, dev)
        self.link_poses = batch["link_poses"].to(dev, torch.float32).contiguous()
        self.K = batch["K"][0].to(dev, torch.float32).contiguous()
        self.Bv, self.L = self.link_poses.shape[0], self.link_poses.shape[1]
        self.dof = _starts_to_dof(starts).to(dev)
        P = self.dof.shape[0]
        self.B = P * self.Bv  # virtual views
        self.N, self.names = 6, list(NAMES)
        ref = batch["mask"].to(dev, torch.float32)
        assert self.L == self.scene.num_links and ref.shape == (self.Bv, self.H, self.W)
        assert self.weight is None or self.weight.shape == ref.shape
        self.ref = ref.repeat(P, 1, 1).contiguous()  # private and tiled: [P*Bv,H,W]
        self.near, self.far = near, far
        self._init_driver(P, lambda0, ftol, lambda_max, log_rows)
        self._init_plan(slack)  # (job slots per VIRTUAL view)

    def _linearize(self, stream):
        _lib.check(_lib.lib().ehr_lm_linearize_multi(
            _lib.ptr(self.dof), _lib.ptr(self.K), _lib.ptr(self.link_poses), self.P, self.Bv, self.L, self.H, self.W,
            ctypes.c_float(self.near), ctypes.c_float(self.far), _lib.ptr(self.mvp), _lib.ptr(self.dmvp), stream),
            "ehr_lm_linearize_multi")

    def _update(self, stream, finalize=0):
        o = self.out
        _lib.check(_lib.lib().ehr_lm_update_multi(
            _lib.ptr(o.info), _lib.ptr(o.grad), _lib.ptr(o.count), _lib.ptr(o.loss), self.P, self.Bv, self.N,
            _lib.ptr(self.dof), ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max), int(finalize),
            _lib.ptr(self.state_block), _lib.ptr(self.log), self.log_rows, stream), "ehr_lm_update_multi")

    def state(self):
        """:meth:`easyhec_amd.lm._LmDriver.states`: the P state blocks as a list of namespaces (one copy; synchronises)."""
        return self.states()

    def memory_bytes(self):
        """Device memory of this solve's context (``ehr_ctx_scratch_bytes``) plus the tiled reference."""
        return self.glctx.scratch_bytes() + self.ref.numel() * 4


@dataclass
class MultiLmResult:
    dofs: torch.Tensor          # [P,6] accepted dof of every hypothesis (CPU)
    losses: np.ndarray          # [P] float64 F_acc: the exact summed loss at the accepted pose (NaN: nothing accepted)
    ranking: list               # hypothesis indices, best first (NaN last, ties by index)
    winner: int
    iterations: list            # per hypothesis, like LmResult's
    accepted: list
    rejected: list
    reported: list
    done: list
    why: list                   # the reason each stopped ("max_iters" where it did not stop by itself)
    trajectories: list          # per hypothesis [iterations,4]
    report: object              # the winner's InformationReport
    basins: list                # group_basins of the accepted poses: do the starts agree on one optimum?
    recoveries: list = field(default_factory=list)
    states: list = None         # the final state namespaces
    lm: object = None           # the MultiStartLM object (lm.calls - iterations[p]: iterations p sat through when done)


def _result(ms, recoveries):
    S = ms.state()
    dofs = ms.dof.cpu().clone()
    losses = np.array([s.F_acc if s.accepted else float("nan") for s in S], dtype=np.float64)
    ranking = rank_losses(losses)
    w = ranking[0]
    poses = se3_exp_map(dofs.double()).permute(0, 2, 1).numpy()
    return MultiLmResult(
        dofs=dofs, losses=losses, ranking=ranking, winner=w, iterations=[s.iterations for s in S],
        accepted=[s.accepted for s in S], rejected=[s.rejected for s in S], reported=[s.reported for s in S],
        done=[bool(s.done) for s in S], why=[WHY[s.why].split(":")[0] if s.done else "max_iters" for s in S],
        trajectories=[ms.trajectory(p) for p in range(ms.P)], report=ms.report(w, S[w]),
        basins=group_basins(poses, ranking), recoveries=recoveries, states=S, lm=ms)


def solve_lm_multi(model, batch, starts, max_iters=50, check_every=5, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, near=0.001,
                   far=10.0, slack=None, prior_sigma=None, sigma2=None, prior_mean=None):
    """:func:`easyhec_amd.lm.solve_lm` for P starts at once, with its loop: the hypotheses are polled every ``check_every``
    iterations; reported iterations are recovered from the way ``_ChainStep`` recovers a step (at most 4 rounds, then it
    raises) and taken again; it stops when every hypothesis is done, or when the hypotheses still running have taken
    ``max_iters`` EFFECTIVE iterations (the one that has taken fewest counts), and ends with the accepted poses in the
    object's ``dof``.  The hypotheses are ranked by ``F_acc``, an exact loss (float64 sum of the views' losses at the
    accepted pose) -- no tail mean.  The model is NOT written.  Returns a :class:`MultiLmResult`.  A prior argument
    (``prior_sigma``, ``sigma2``, ``prior_mean``) is refused: the multi-start solve is pose-only."""
    _no_prior_arguments("solve_lm_multi", prior_sigma, sigma2, prior_mean)
    ms = MultiStartLM(model, batch, starts, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max,
                      log_rows=max_iters + 4 * check_every + 8, near=near, far=far, slack=slack)
    recoveries = _run_to_convergence(ms, max_iters, check_every, ms.recover_from_overflow,
                                     lambda: fused.check_status(ms.glctx), "solve_lm_multi")
    return _result(ms, recoveries)


def solve_global_lm(model, batch, Tc_init, Q, P, max_iters=50, check_every=5, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0,
                    extra=None, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, slack=None, score="xor", cap_px=None, prior_sigma=None,
                    sigma2=None, prior_mean=None):
    """A global solve that needs no tuning: :func:`easyhec_amd.pose_search.search_starts` (Q candidates scored by mask
    overlap, the best P kept), then :func:`solve_lm_multi` from its starts -> ``(PoseSearchResult, MultiLmResult)``.  The
    winner's accepted dof is written into ``model.dof``; ``history_ops`` and any Adam state stay untouched, as for
    ``solve_lm``.  Hypothesis 0 is ``Tc_init``: it is the plain ``solve_lm`` from there bit for bit, so the winner's loss
    never exceeds it.  ``score`` and ``cap_px`` go to ``search_starts`` (``score="soft"``: the soft IoU, which still ranks
    candidates that no longer overlap the observed masks, so the draw may be wide).  A prior argument is refused, as by
    ``solve_lm_multi``."""
    _no_prior_arguments("solve_global_lm", prior_sigma, sigma2, prior_mean)
    from .pose_search import search_starts
    search = search_starts(model, batch, Tc_init, Q, P, trans_sigma_m, rot_sigma_deg, seed, extra=extra, score=score, cap_px=cap_px)
    res = solve_lm_multi(model, batch, search.starts, max_iters=max_iters, check_every=check_every, lambda0=lambda0, ftol=ftol,
                         lambda_max=lambda_max, slack=slack)
    with torch.no_grad():
        model.dof.data.copy_(res.dofs[res.winner])
    return search, res
