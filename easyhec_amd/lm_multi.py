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
(tests/test_gpu_lm_multi.py).  HIP only; no fallback.

With ``robot=`` or ``free_intrinsics=`` every hypothesis also owns joint offsets, intrinsics and, if asked for, a Gaussian prior
(INTEGRATION.md 4a-11): everything that can differ between hypotheses is a per-hypothesis array --
``offsets`` [P,J], ``theta`` [P,4], ``K`` [P,3,3], ``link_poses`` [P*Bv,L,4,4], ``joint_frames`` [P*Bv,J,6] -- and the chain is

    [ehr_joint_forward_multi]  ->  ehr_lm_linearize_multi_calib  ->  ehr_mask_information  ->  ehr_lm_update_multi_calib

Hypothesis p is then, bit for bit, its solo ``solve_lm`` on a ``JointPoseStep``, ``IntrinsicsPoseStep`` or
``JointIntrinsicsPoseStep`` built on start p (tests/test_gpu_lm_multi_calib.py).  (The ADAM multi-start step,
:class:`easyhec_amd.multistart.MultiStartPoseStep`, stays pose-only: its hypotheses share one ``link_poses`` and one ``K``.)

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
from .joint_calib import _JointForward, arm_table, free_joint_list, with_recorded_link_poses
from .lm import WHY, _LmDriver, _no_prior_arguments, _run_to_convergence, make_prior
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
    package's tests call "the same pose".  Pose-based also where offsets or intrinsics are free: two hypotheses in one basin
    agree on ``Tc_c2b``, whatever their offsets and ``K`` are.  Pure numpy."""
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
    ``state_block`` [P,EHR_LM_STATE_DOUBLES] float64, ``log`` [P,log_rows,4].  In the pose-only form ``K`` and ``link_poses`` are
    shared by the hypotheses (with ``robot=`` / ``free_intrinsics=`` each has its own: the constructor's docstring), and so are
    the weights ([Bv,H,W], view b reads image b % Bv).  The reference masks are NOT: the information op
    has no shared-reference form, so a private copy is tiled P times -- ``P * Bv * H * W * 4`` bytes, 236 MB for 8 hypotheses
    x 8 views at 1280x720 -- beside the context's scratch for ``P * Bv`` views.

    ``iterate(n)`` enqueues n iterations of every hypothesis and never synchronises (a hypothesis that is done only has its
    accepted pose restored; its views are still rendered); ``state()`` makes one copy; ``finalize()`` leaves the accepted
    poses in ``dof``.  The buffers, the guard and the iteration are :class:`easyhec_amd.lm._LmDriver`'s; the slot policy, the
    plan with its bindings and ``recover_from_overflow()`` -- call it when iterations were reported -- are
    :class:`easyhec_amd.chain_step._PlannedContext`'s, as for the launch-chain steps."""
    who = "MultiStartLM"
    hypothesis_priors = False  # (True with free offsets or intrinsics: the update then takes [P,N] prior rows)

    def __init__(self, model, batch, starts, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, near=0.001, far=10.0,
                 slack=None, *, robot=None, qpos=None, free=None, free_intrinsics=None, init_offset=None, prior=None):
        """robot, qpos, free, init_offset: :class:`easyhec_amd.joint_calib.JointPoseStep`'s -- every hypothesis fits the free
        joints' offsets, from ``init_offset`` ([J], or [P,J] for a row each; default 0); a ``robot.mounted(link)`` view makes
        it the eye-in-hand solve (``ehr_joint_forward_multi_mounted``; the starts are then poses camera<-mount); free_intrinsics:
        :class:`easyhec_amd.intrinsics_calib.IntrinsicsPoseStep`'s ``free`` -- every hypothesis fits its own ``theta`` / ``K``
        from ``batch["K"][0]``.  Without both, the object is the pose-only one (N = 6, the ``_multi`` C calls).  With either,
        ``names`` / ``N`` follow :func:`easyhec_amd.lm.parameter_layout`'s order -- dof, free offsets, free intrinsics --
        and the state also holds ``offsets`` [P,J], ``theta`` [P,4], ``K0``, ``K`` [P,3,3], ``link_poses`` [P*Bv,L,4,4] (the
        kinematics kernel's where a robot is given, never ``batch["link_poses"]``; the batch's repeated P times otherwise)
        and ``joint_frames`` [P*Bv,J,6].  prior: an :class:`easyhec_amd.lm.LmPrior` with [P,N] rows (``make_prior(this)``)."""
        calib = robot is not None or free_intrinsics is not None
        seen = dict(batch, link_poses=batch["mask"]) if robot is not None and "link_poses" not in batch else batch
        self.dev = dev = _hip_device("MultiStartLM", model, seen)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("MultiStartLM: not available while a graph is being captured: ehr_mask_information sizes its "
                               "scratch on the first call")
        if not _lib.has_lm_multi():
            raise RuntimeError("this libehr_hip.so has no multi-start Levenberg-Marquardt kernels (ehr_lm_linearize_multi): "
                               "rebuild it")
        if not _lib.has_information():
            raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")
        if robot is None and (free is not None or qpos is not None or init_offset is not None):
            raise ValueError("MultiStartLM: free, qpos and init_offset describe free JOINTS and need robot= (the arm's joint "
                             "table); the free intrinsics are free_intrinsics=")
        if calib and not _lib.has_lm_multi_calib():
            raise RuntimeError("this libehr_hip.so has no multi-start kernels for joint offsets and intrinsics "
                               "(ehr_lm_update_multi_calib): rebuild it")
        self.model = model
        self.scene = model._ensure_scene()
        self.H, self.W = model.H, model.W
        self.weight = _private_weight(batch, dev)
        self.dof = _starts_to_dof(starts).to(dev)
        P = self.dof.shape[0]
        self.kin, self.free_joints, self.free_intrinsics, self.F, self.J = None, [], None, 0, 0
        self.free4_mask, self.tie_focal, self.free_list = 0, 0, None
        names = list(NAMES)
        if robot is not None:
            table, J, qp = arm_table(robot, qpos, batch, "MultiStartLM")
            batch = with_recorded_link_poses(robot, qp, batch, "MultiStartLM")
        recorded = batch["link_poses"].to(dev, torch.float32).contiguous()
        self.Bv, self.L = recorded.shape[0], recorded.shape[1]
        self.B = P * self.Bv  # virtual views
        if robot is not None:
            if qp.shape[0] != self.Bv or len(table["use"]) != self.L:
                raise ValueError(f"MultiStartLM: qpos {qp.shape} / {len(table['use'])} rendered links do not match the batch's "
                                 f"{self.Bv} views of {self.L} links")
            self.robot, self.table, self.J = robot, table, J
            self.free_joints = free_joint_list(table, J, free)
            self.F = len(self.free_joints)
            self.kin = _JointForward(table, J, qp, self.free_joints, None, dev)
            self.free_list = torch.tensor(self.free_joints, dtype=torch.int32, device=dev) if self.F else None
            off = np.zeros((P, J), dtype=np.float32)
            if init_offset is not None:
                off[:] = np.asarray(init_offset, dtype=np.float32).reshape(-1, J)  # ([J] for all, or a row each)
            self.offsets = torch.from_numpy(off).to(dev)
            self.link_poses = torch.empty((self.B, self.L, 4, 4), device=dev)
            self.joint_frames = torch.empty((self.B, J, 6), device=dev)
            self._forward_kinematics = self._launch_kinematics  # (_LmDriver: ahead of every linearisation)
            names += [f"offset[{j}]" for j in self.free_joints]
        elif calib:
            self.link_poses = recorded.repeat(P, 1, 1, 1).contiguous()
        else:
            self.link_poses = recorded
        self.K = batch["K"][0].to(dev, torch.float32).contiguous()
        if free_intrinsics is not None:
            from .intrinsics_calib import _parse_free, _refuse
            _refuse(batch, {})
            mask, self.tie_focal, self.free_intrinsics = _parse_free(free_intrinsics)
            self.free4_mask = sum(1 << i for i in range(4) if mask[i])
            names += [f"theta[{n}]" for n in self.free_intrinsics]
        if calib:  # every hypothesis its own K (theta == 0: K0's bits, as intrinsics_from_theta gives them)
            self.K0 = self.K
            self.K = self.K0.repeat(P, 1, 1).contiguous()
            self.theta = torch.zeros((P, 4), device=dev)
        self.calib, self.hypothesis_priors = calib, bool(self.F or self.free4_mask)
        self.N, self.names = len(names), names
        self.glctx = dr.RasterizeCudaContext(device=dev)
        ref = batch["mask"].to(dev, torch.float32)
        assert self.L == self.scene.num_links and ref.shape == (self.Bv, self.H, self.W)
        assert self.weight is None or self.weight.shape == ref.shape
        self.ref = ref.repeat(P, 1, 1).contiguous()  # private and tiled: [P*Bv,H,W]
        self.near, self.far = near, far
        self._init_driver(P, lambda0, ftol, lambda_max, log_rows)
        self._init_plan(slack)  # (job slots per VIRTUAL view)
        if self.kin is not None:
            with torch.cuda.device(dev):
                self._launch_kinematics(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        if prior is not None:
            self.set_prior(prior)

    def set_prior(self, prior):
        if prior is not None:
            if not (self.F or self.free4_mask):
                raise ValueError("MultiStartLM: no prior is available for the multi-start solve: it is pose-only, and the prior "
                                 "is for offsets and intrinsics (pass robot= or free_intrinsics=)")
            if tuple(prior.weight.shape) != (self.P, self.N) or tuple(prior.mean.shape) != (self.P, self.N):
                raise ValueError(f"MultiStartLM: the prior holds a row per hypothesis, [{self.P},{self.N}] (make_prior on this "
                                 f"object), not {tuple(prior.weight.shape)}")
        return super().set_prior(prior)

    def _launch_kinematics(self, stream):
        k = self.kin
        tab = [_lib.ptr(t) for t in k.t]
        out = (_lib.ptr(k.qpos), _lib.ptr(self.offsets), self.P, self.Bv, _lib.ptr(self.link_poses), _lib.ptr(self.joint_frames),
               stream)
        if k.mount is None:
            _lib.check(_lib.lib().ehr_joint_forward_multi(*tab, k.N, k.J, self.L, *out), "ehr_joint_forward_multi")
        else:  # a camera on a link of the arm (robot.mounted(...)): the poses and joint frames in the mount's frame
            _lib.check(_lib.lib().ehr_joint_forward_multi_mounted(*tab, k.N, k.J, self.L, k.mount[0], k.mount[1], *out),
                       "ehr_joint_forward_multi_mounted")

    def _linearize(self, stream):
        near, far = ctypes.c_float(self.near), ctypes.c_float(self.far)
        if not self.calib:
            _lib.check(_lib.lib().ehr_lm_linearize_multi(
                _lib.ptr(self.dof), _lib.ptr(self.K), _lib.ptr(self.link_poses), self.P, self.Bv, self.L, self.H, self.W,
                near, far, _lib.ptr(self.mvp), _lib.ptr(self.dmvp), stream), "ehr_lm_linearize_multi")
            return
        k, F = self.kin, self.F
        _lib.check(_lib.lib().ehr_lm_linearize_multi_calib(
            _lib.ptr(self.dof), _lib.ptr(self.K), _lib.ptr(self.link_poses), self.P, self.Bv, self.L, self.H, self.W, near, far,
            _lib.ptr(self.joint_frames if F else None), _lib.ptr(k.upstream if F else None), _lib.ptr(k.jkind if F else None),
            _lib.ptr(self.free_list), F, self.J, self.free4_mask, self.tie_focal, self.N, _lib.ptr(self.mvp),
            _lib.ptr(self.dmvp), stream), "ehr_lm_linearize_multi_calib")

    def _update(self, stream, finalize=0):
        o = self.out
        if not self.calib:
            _lib.check(_lib.lib().ehr_lm_update_multi(
                _lib.ptr(o.info), _lib.ptr(o.grad), _lib.ptr(o.count), _lib.ptr(o.loss), self.P, self.Bv, self.N,
                _lib.ptr(self.dof), ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max), int(finalize),
                _lib.ptr(self.state_block), _lib.ptr(self.log), self.log_rows, stream), "ehr_lm_update_multi")
            return
        intr = self.free4_mask != 0
        pw, pm = self._prior_ptrs() if self.prior is not None else (None, None)
        _lib.check(_lib.lib().ehr_lm_update_multi_calib(
            _lib.ptr(o.info), _lib.ptr(o.grad), _lib.ptr(o.count), _lib.ptr(o.loss), self.P, self.Bv, self.N,
            _lib.ptr(self.dof), _lib.ptr(self.offsets if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
            _lib.ptr(self.theta if intr else None), self.free4_mask, self.tie_focal, _lib.ptr(self.K0 if intr else None),
            _lib.ptr(self.K if intr else None), self.H, self.W, ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max),
            int(finalize), _lib.ptr(self.state_block), _lib.ptr(self.log), self.log_rows, pw, pm, stream),
            "ehr_lm_update_multi_calib")

    def parameters(self):
        """[P,N] float32 (host): every hypothesis's parameters as the tensors hold them, in ``names``' order.  Synchronises."""
        out = [self.dof.cpu().numpy()]
        if self.F:
            out.append(self.offsets.cpu().numpy()[:, self.free_joints])
        if self.free4_mask:
            first = {"f": 0, "fx": 0, "fy": 1, "cx": 2, "cy": 3}
            out.append(self.theta.cpu().numpy()[:, [first[n] for n in self.free_intrinsics]])
        return np.concatenate(out, axis=1).astype(np.float32)

    def joint_kinds(self):
        return self.kin.jkind.cpu().numpy() if self.kin is not None else None

    def evaluate_each(self):
        """``[(loss_p, count_p)]`` of ONE :meth:`easyhec_amd.lm._LmDriver.evaluate` of all hypotheses at their current
        parameters -- each the sums a solo ``evaluate()`` of hypothesis p forms.  Synchronises."""
        self.evaluate()
        Bv = self.Bv
        return [(float(self.out.loss[p * Bv:(p + 1) * Bv].double().sum().item()),
                 int(self.out.count[p * Bv:(p + 1) * Bv].sum().item())) for p in range(self.P)]

    def data_losses(self):
        """[P] float64: the summed per-view loss of every hypothesis at its CURRENT parameters, from one evaluation of all of
        them, added as the update kernel adds it (from 0.0 in view order) -- after ``finalize()`` the data's part of
        ``F_acc``, exactly: ``F_acc`` is this plus ``F_prior`` in one addition.  Synchronises."""
        self.evaluate()
        loss = self.out.loss.cpu().numpy().reshape(self.P, self.Bv)
        out = np.zeros(self.P, dtype=np.float64)
        for b in range(self.Bv):
            out = out + loss[:, b].astype(np.float64)
        return out

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
    names: list = None          # the N parameters of a hypothesis, in the solve's order
    offsets: torch.Tensor = None    # [P,J] accepted joint offsets (CPU); None without a robot
    thetas: torch.Tensor = None     # [P,4] accepted intrinsics parameters (CPU); None in the pose-only form
    Ks: torch.Tensor = None         # [P,3,3] the K of every hypothesis (CPU); None in the pose-only form
    data_losses: np.ndarray = None  # [P] the summed per-view loss at the accepted point (== losses without a prior); under a
    #                                 prior evaluated once more there, so that data_losses + prior_losses == losses exactly
    prior_losses: np.ndarray = None  # [P] F_prior: the prior's term at the accepted point
    prior: object = None        # the LmPrior the solve ran under ([P,N] rows, ONE sigma2 for all hypotheses), or None
    posterior: object = None    # under a prior: the winner's posterior report, as LmResult's

    def write_into(self, step):
        """Copy hypothesis ``winner``'s ``dof``, offsets, ``theta`` and ``K`` into ``step`` -- a ``JointPoseStep``,
        ``IntrinsicsPoseStep`` or ``JointIntrinsicsPoseStep`` (``FusedPoseStep`` for a pose-only result) with the SAME free
        joints and the same free intrinsics, else ValueError naming the difference -- and rerun its forward kinematics, so that
        Adam, ``information_of`` or the explorer go on from the winner.  Returns ``step``."""
        ms, w = self.lm, self.winner
        mine = (list(ms.free_joints) if ms.kin is not None else None, ms.free_intrinsics)
        theirs = (list(step.free_joints) if getattr(step, "kinematics", None) is not None else None,
                  getattr(step, "free_intrinsics", None))
        if mine[0] != theirs[0]:
            raise ValueError(f"write_into: the solve had free joints {mine[0]}, the step has {theirs[0]} (None: no joint table)")
        if mine[1] != theirs[1]:
            raise ValueError(f"write_into: the solve had free intrinsics {mine[1]}, the step has {theirs[1]} (None: K is fixed)")
        with torch.no_grad():
            step.model.dof.data.copy_(self.dofs[w])
            if mine[0] is not None:
                step.offsets.copy_(self.offsets[w])
            if mine[1] is not None:
                step.theta.copy_(self.thetas[w])
                step.K.copy_(self.Ks[w])
        if mine[0] is not None:
            step.corrected_link_poses()
        return step


def _result(ms, recoveries):
    S = ms.state()
    dofs = ms.dof.cpu().clone()
    losses = np.array([s.F_acc if s.accepted else float("nan") for s in S], dtype=np.float64)
    prior_losses = np.array([getattr(s, "F_prior", 0.0) for s in S], dtype=np.float64)
    calib, prior = getattr(ms, "calib", False), getattr(ms, "prior", None)  # (the pose-only form: no more than it ever held)
    ranking = rank_losses(losses)
    w = ranking[0]
    poses = se3_exp_map(dofs.double()).permute(0, 2, 1).numpy()
    return MultiLmResult(
        dofs=dofs, losses=losses, ranking=ranking, winner=w, iterations=[s.iterations for s in S],
        accepted=[s.accepted for s in S], rejected=[s.rejected for s in S], reported=[s.reported for s in S],
        done=[bool(s.done) for s in S], why=[WHY[s.why].split(":")[0] if s.done else "max_iters" for s in S],
        trajectories=[ms.trajectory(p) for p in range(ms.P)], report=ms.report(w, S[w]),
        basins=group_basins(poses, ranking), recoveries=recoveries, states=S, lm=ms, names=list(ms.names),
        offsets=ms.offsets.cpu().clone() if calib and ms.kin is not None else None,
        thetas=ms.theta.cpu().clone() if calib else None, Ks=ms.K.cpu().clone() if calib else None,
        data_losses=np.where(np.isnan(losses), losses, ms.data_losses()) if prior is not None else losses.copy(),
        prior_losses=prior_losses, prior=prior,
        posterior=ms.posterior(w, S[w]) if prior is not None else None)


def solve_lm_multi(model, batch, starts, max_iters=50, check_every=5, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, near=0.001,
                   far=10.0, slack=None, prior_sigma=None, sigma2=None, prior_mean=None, *, robot=None, qpos=None, free=None,
                   free_intrinsics=None, init_offset=None):
    """:func:`easyhec_amd.lm.solve_lm` for P starts at once, with its loop: the hypotheses are polled every ``check_every``
    iterations; reported iterations are recovered from the way ``_ChainStep`` recovers a step (at most 4 rounds, then it
    raises) and taken again; it stops when every hypothesis is done, or when the hypotheses still running have taken
    ``max_iters`` EFFECTIVE iterations (the one that has taken fewest counts), and ends with the accepted parameters in the
    object's tensors.  The hypotheses are ranked by ``F_acc``, an exact loss (float64 sum of the views' losses at the
    accepted point; under a prior the total objective) -- no tail mean.  The model is NOT written.  Returns a
    :class:`MultiLmResult`.

    ``robot``, ``qpos``, ``free``, ``free_intrinsics``, ``init_offset``: :class:`MultiStartLM`'s -- every hypothesis then fits
    its own joint offsets and / or intrinsics.  ``prior_sigma``, ``sigma2``, ``prior_mean``: :func:`easyhec_amd.lm.make_prior`'s,
    accepted ONLY when offsets or intrinsics are free (``sigma2=None``: the minimum over the hypotheses; the value used is
    ``result.prior.sigma2``, which a solo ``solve_lm`` can be given).  In the pose-only form a prior argument is refused."""
    pose_only = robot is None and free_intrinsics is None
    _no_prior_arguments("solve_lm_multi", prior_sigma, sigma2, prior_mean, allowed=not pose_only)
    ms = MultiStartLM(model, batch, starts, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max,
                      log_rows=max_iters + 4 * check_every + 8, near=near, far=far, slack=slack, robot=robot, qpos=qpos,
                      free=free, free_intrinsics=free_intrinsics, init_offset=init_offset)
    if prior_sigma is not None:
        if not (ms.F or ms.free4_mask):  # (a robot with no free joint: still the pose alone)
            _no_prior_arguments("solve_lm_multi", prior_sigma, sigma2, prior_mean)
        ms.set_prior(make_prior(ms, prior_sigma, sigma2, prior_mean))
    recoveries = _run_to_convergence(ms, max_iters, check_every, ms.recover_from_overflow,
                                     lambda: fused.check_status(ms.glctx), "solve_lm_multi")
    return _result(ms, recoveries)


def solve_global_lm(model, batch, Tc_init, Q, P, max_iters=50, check_every=5, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0,
                    extra=None, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, slack=None, score="xor", cap_px=None, prior_sigma=None,
                    sigma2=None, prior_mean=None, *, robot=None, qpos=None, free=None, free_intrinsics=None, init_offset=None):
    """A global solve that needs no tuning: :func:`easyhec_amd.pose_search.search_starts` (Q candidates scored by mask
    overlap, the best P kept), then :func:`solve_lm_multi` from its starts -> ``(PoseSearchResult, MultiLmResult)``.  The
    winner's accepted dof is written into ``model.dof``; ``history_ops`` and any Adam state stay untouched, as for
    ``solve_lm``.  Hypothesis 0 is ``Tc_init``: it is the plain ``solve_lm`` from there bit for bit, so the winner's loss
    never exceeds it.  ``score`` and ``cap_px`` go to ``search_starts`` (``score="soft"``: the soft IoU, which still ranks
    candidates that no longer overlap the observed masks, so the draw may be wide).  ``robot`` ... ``init_offset`` and the
    prior arguments go to ``solve_lm_multi`` (the search itself scores poses with the recorded link poses and the given
    ``K``); in the pose-only form a prior argument is refused, as there.  Only the winner's ``dof`` is written into the
    model: its offsets, ``theta`` and ``K`` go into a step object with ``result.write_into(step)``."""
    _no_prior_arguments("solve_global_lm", prior_sigma, sigma2, prior_mean,
                        allowed=robot is not None or free_intrinsics is not None)
    from .pose_search import search_starts
    search = search_starts(model, batch, Tc_init, Q, P, trans_sigma_m, rot_sigma_deg, seed, extra=extra, score=score, cap_px=cap_px)
    res = solve_lm_multi(model, batch, search.starts, max_iters=max_iters, check_every=check_every, lambda0=lambda0, ftol=ftol,
                         lambda_max=lambda_max, slack=slack, prior_sigma=prior_sigma, sigma2=sigma2, prior_mean=prior_mean,
                         robot=robot, qpos=qpos, free=free, free_intrinsics=free_intrinsics, init_offset=init_offset)
    with torch.no_grad():
        model.dof.data.copy_(res.dofs[res.winner])
    return search, res
