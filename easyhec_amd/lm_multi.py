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
(tests/test_gpu_lm_multi.py).  Pose only: no joint offsets, no intrinsics.  HIP only; no fallback."""
import ctypes
import os
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, dr, fused, information
from .fast import _private_weight
from .lm import WHY, state_namespace
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


def _check_batch(who, model, batch):
    dev = model.dof.device
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs on a HIP device only: move the model with .cuda() first (there is no CPU path)")
    for k in ("mask", "link_poses", "K"):
        if not torch.is_tensor(batch[k]) or batch[k].device.type != "cuda":
            raise RuntimeError(f"{who}: batch['{k}'] must be a tensor on the HIP device")
    return dev


class MultiStartLM:
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
    poses in ``dof``."""

    def __init__(self, model, batch, starts, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, near=0.001, far=10.0,
                 slack=None):
        self.dev = dev = _check_batch("MultiStartLM", model, batch)
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
        self.P = P = self.dof.shape[0]
        self.B = B = P * self.Bv  # virtual views
        self.N, self.names = 6, list(NAMES)
        ref = batch["mask"].to(dev, torch.float32)
        assert self.L == self.scene.num_links and ref.shape == (self.Bv, self.H, self.W)
        assert self.weight is None or self.weight.shape == ref.shape
        self.ref = ref.repeat(P, 1, 1).contiguous()  # private and tiled: [P*Bv,H,W]
        self.near, self.far = near, far
        self.ftol, self.lambda_max, self.lambda0 = float(ftol), float(lambda_max), float(lambda0)
        self.mvp = torch.empty((B, self.L, 4, 4), device=dev)
        self.dmvp = torch.empty((6, B, self.L, 4, 4), device=dev)
        self.out = information._outputs(6, B, self.L, dev, True, False)
        st = np.zeros((P, _lib.LM_STATE_DOUBLES))
        st[:, _lib.LM_STATE["lambda"]], st[:, _lib.LM_STATE["nu"]] = self.lambda0, 2.0
        self.state_block = torch.from_numpy(st).to(dev)
        self.log_rows = int(log_rows)
        self.log = torch.full((P, self.log_rows, 4), float("nan"), dtype=torch.float64, device=dev)
        self.calls = 0  # iterations enqueued so far: a hypothesis's `iterations` falls behind it once it is done
        # job slots per virtual view: _ChainStep's rule
        if slack is None and "EHR_VB_SLACK" not in os.environ:
            ntiles = ((self.W + 31) // 32) * ((self.H + 7) // 8)
            self.slack = max(0.5, 256.0 / ntiles)
        else:
            self.slack = float(os.environ["EHR_VB_SLACK"]) if slack is None else float(slack)
        self._plan_and_bind()

    def _plan_and_bind(self):
        fused._ensure_plan(self.glctx, self.scene, self.B, self.H, self.W, slack=self.slack)
        if self.weight is not None:  # (the weights first: binding them unbinds the reference)
            fused.bind_weight(self.glctx, self.scene, self.weight, views=self.B)
        fused.bind_ref(self.glctx, self.scene, self.ref, views=self.B)

    def recover_from_overflow(self):
        """Call when iterations were reported.  Synchronises.  What :meth:`easyhec_amd.chain_step._ChainStep.recover_from_overflow`
        does, on this object's context: "general-triangle pass" (the context launches it from now on), "job slots" (planned
        again with a slot for every (view, link, tile), weights and reference bound again), or False where the context reports
        nothing.  Raises on any other overflow."""
        with torch.cuda.device(self.dev):
            rc = _lib.lib().ehr_fused_status(self.glctx.handle)
        if rc == 0:
            return False
        if rc == _lib.EHR_ERR_RETRY:
            return "general-triangle pass"
        if self.slack == 0.0:
            _lib.check(rc, "fused render")
        self.slack = 0.0
        self._plan_and_bind()
        return "job slots"

    # -- guards: the context is this object's own, but nothing keeps a caller from rendering with it ---------------------------
    def _guard(self):
        plan = getattr(self.glctx, "_plan", None)
        if plan is None or plan.key != fused._plan_key(self.scene, self.B, self.H, self.W):
            raise RuntimeError("MultiStartLM: its context holds another plan (somebody else rendered with it)")
        if getattr(self.glctx, "_bound_weight", None) is not self.weight:
            raise RuntimeError("MultiStartLM: the weights bound to its context are not its own (somebody else used the "
                               "context)")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("MultiStartLM: not available while a graph is being captured")

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

    def iterate(self, n=1):
        """Enqueue ``n`` iterations of every hypothesis on the current stream; never synchronises."""
        self._guard()
        o = self.out
        with torch.cuda.device(self.dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(int(n)):
                self._linearize(stream)
                information._launch(self.glctx, self.scene, self.mvp, self.dmvp, self.ref, o.info, o.grad, o.count, o.loss,
                                    None)
                self._update(stream)
                self.calls += 1
        return self

    def finalize(self):
        """Leave the ACCEPTED pose of every hypothesis in ``dof``.  Enqueued; never synchronises."""
        with torch.cuda.device(self.dev):
            self._update(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), finalize=1)
        return self

    def state(self):
        """The P state blocks as a list of namespaces with the fields of :meth:`easyhec_amd.lm.LevenbergMarquardt.state` (one
        copy of [P,EHR_LM_STATE_DOUBLES]; synchronises)."""
        s = self.state_block.cpu().numpy()
        return [state_namespace(s[p], self.N) for p in range(self.P)]

    def trajectory(self, p):
        """Hypothesis p's [iterations,4] float64 (CPU), as :meth:`easyhec_amd.lm.LevenbergMarquardt.trajectory`."""
        n = min(int(self.state_block[p, _lib.LM_STATE["iterations"]].item()), self.log_rows)
        return self.log[p, :n].cpu().numpy()

    def report(self, p, state=None):
        """The :class:`easyhec_amd.information.InformationReport` of hypothesis p's accepted point, from its state block."""
        s = self.state()[p] if state is None else state
        return information.InformationReport(s.H[None], self.names, s.g[None], [s.count], [s.F_acc])

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
                   far=10.0, slack=None):
    """:func:`easyhec_amd.lm.solve_lm` for P starts at once, with its loop: the hypotheses are polled every ``check_every``
    iterations; reported iterations are recovered from the way ``_ChainStep`` recovers a step (at most 4 rounds, then it
    raises) and taken again; it stops when every hypothesis is done, or when the hypotheses still running have taken
    ``max_iters`` EFFECTIVE iterations (the one that has taken fewest counts), and ends with the accepted poses in the
    object's ``dof``.  The hypotheses are ranked by ``F_acc``, an exact loss (float64 sum of the views' losses at the
    accepted pose) -- no tail mean.  The model is NOT written.  Returns a :class:`MultiLmResult`."""
    ms = MultiStartLM(model, batch, starts, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max,
                      log_rows=max_iters + 4 * check_every + 8, near=near, far=far, slack=slack)
    recoveries, rounds, seen = [], 0, 0
    while True:
        S = ms.state()
        reported = sum(s.reported for s in S)
        if reported > seen:
            seen = reported
            what = ms.recover_from_overflow()
            if what:
                recoveries.append(what)
            rounds += 1
            if rounds > 4:
                fused.check_status(ms.glctx)
                raise RuntimeError("solve_lm_multi: iterations keep being reported as not taken (NaN loss)")
        running = [s.iterations - s.reported for s in S if not s.done]
        if not running or min(running) >= max_iters:
            break
        ms.iterate(min(check_every, max_iters - min(running)))
    ms.finalize()
    return _result(ms, recoveries)


def solve_global_lm(model, batch, Tc_init, Q, P, max_iters=50, check_every=5, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0,
                    extra=None, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, slack=None, score="xor", cap_px=None):
    """A global solve that needs no tuning: :func:`easyhec_amd.pose_search.search_starts` (Q candidates scored by mask
    overlap, the best P kept), then :func:`solve_lm_multi` from its starts -> ``(PoseSearchResult, MultiLmResult)``.  The
    winner's accepted dof is written into ``model.dof``; ``history_ops`` and any Adam state stay untouched, as for
    ``solve_lm``.  Hypothesis 0 is ``Tc_init``: it is the plain ``solve_lm`` from there bit for bit, so the winner's loss
    never exceeds it.  ``score`` and ``cap_px`` go to ``search_starts`` (``score="soft"``: the soft IoU, which still ranks
    candidates that no longer overlap the observed masks, so the draw may be wide)."""
    from .pose_search import search_starts
    search = search_starts(model, batch, Tc_init, Q, P, trans_sigma_m, rot_sigma_deg, seed, extra=extra, score=score, cap_px=cap_px)
    res = solve_lm_multi(model, batch, search.starts, max_iters=max_iters, check_every=check_every, lambda0=lambda0, ftol=ftol,
                         lambda_max=lambda_max, slack=slack)
    with torch.no_grad():
        model.dof.data.copy_(res.dofs[res.winner])
    return search, res
