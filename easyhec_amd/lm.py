"""Levenberg-Marquardt on the information matrix of the mask loss (``ehr_lm_linearize`` / ``ehr_lm_update`` in
include/ehr.h, csrc/ehr_lm.hip).

Every solve of this package is first-order Adam with a learning rate per parameter group.  ``ehr_mask_information`` gives,
for any parameters, the Gauss-Newton matrix, the gradient and the loss of the fused mask loss in one stream-ordered call;
:class:`LevenbergMarquardt` turns that into a damped Gauss-Newton iteration that runs on the device without a host round trip

    [ehr_joint_forward, if joints are free]  ->  ehr_lm_linearize  ->  ehr_mask_information  ->  ehr_lm_update

on an existing step object's own context, plan, bound reference, weights and parameter tensors: scale-free (no learning rate
per group), monotone (a trial is kept only if its loss is strictly lower) and self-stopping.  The matrix it ends on is the
information matrix at the solution, so :func:`solve_lm` returns the :class:`easyhec_amd.information.InformationReport` of the
accepted point without another call.

It is a refinement BESIDE Adam, not a new default: it does not touch Adam's moments, step counters or ``history_ops``, has no
weight decay unless asked for one -- a Gaussian prior towards the given intrinsics, zero offsets or any other mean
(:func:`make_prior`, ``solve_lm(..., prior_sigma=...)``) -- and far from the optimum its quadratic model
is poor
(the squared error of binary silhouettes is linear in the displacement): the accept / reject rule, not the model, makes it
safe.  It renders the float32 matrix ``ehr_pose_forward`` builds -- the loss it minimises is the loss the Adam solve reports,
bit for bit -- where :func:`easyhec_amd.information.information_of` renders a float64-built one.  HIP only; no fallback.

The iteration and the solve loop are written once, for P state blocks: ``_LmDriver`` owns the
buffers, the guard, ``iterate`` / ``finalize`` and the reading of the state, ``_run_to_convergence`` the polling loop.
:class:`LevenbergMarquardt` is the driver with one block on a step object's context;
:class:`easyhec_amd.lm_multi.MultiStartLM` is the driver with P blocks on a context of its own;
:class:`easyhec_amd.lm_rig.RigLM` is the driver with one block over the C contexts of a camera rig (section 6o)."""
import ctypes
import types
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib, fused, information

__all__ = ["LevenbergMarquardt", "LmResult", "LmPrior", "make_prior", "solve_lm", "WHY"]

WHY = {0: "running", 1: "ftol: the predicted reduction is below ftol * loss", 2: "lambda_max: the damping reached its limit",
       3: "step: every parameter's step is below float32's spacing", 4: "factorisation: the damped matrix kept failing to factor"}


def _refuse(step):
    """The steps the iteration cannot drive, each with its reason (worded like ``information._refuse``)."""
    from .multistart import MultiStartPoseStep
    from .rig_calib import RigJointStep
    if isinstance(step, MultiStartPoseStep):
        raise ValueError("solve_lm: not available for the multi-start step: its hypotheses are separate solves; ask for the "
                         "winner's FusedPoseStep")
    if isinstance(step, RigJointStep):
        raise ValueError("solve_lm: not available for a rig: it is one system over several contexts; that solve is "
                         "solve_lm_rig(rig_step) (easyhec_amd.lm_rig)")
    if getattr(step, "distributed", False) or getattr(step, "rccl", False) or getattr(step, "p2p", False):
        raise ValueError("solve_lm: not available for a data-parallel job: each rank holds its own views, and the matrices "
                         "are not exchanged")
    for attr in ("glctx", "scene", "ref", "link_poses", "K", "model"):
        if not hasattr(step, attr):
            raise TypeError(f"solve_lm: {type(step).__name__} is not a launch-chain step (FusedPoseStep, JointPoseStep, "
                            "IntrinsicsPoseStep, JointIntrinsicsPoseStep)")
    if step.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("solve_lm: not available while a graph is being captured: ehr_mask_information sizes its scratch "
                           "on the first call")
    if not _lib.has_lm():
        raise RuntimeError("this libehr_hip.so has no Levenberg-Marquardt kernels (ehr_lm_linearize): rebuild it")
    if not _lib.has_information():
        raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")


def parameter_layout(step):
    """The parameters ``step`` optimises, in the order of :func:`easyhec_amd.information.information_of`, and what
    ``ehr_lm_linearize`` needs to know of them: a namespace of ``names``, ``N``, ``kin`` (the step's joint table on the device, or
    None), ``free`` (the free joints), ``F``, ``J``, ``free4_mask`` and ``tie_focal``."""
    kin = getattr(step, "kinematics", None)
    free = list(step.free_joints) if kin is not None else []
    names = [f"dof[{i}]" for i in range(6)] + [f"offset[{j}]" for j in free]
    free4_mask, tie_focal = 0, 0
    if hasattr(step, "free_intrinsics"):
        from .intrinsics_calib import _parse_free
        mask, tie_focal, nm = _parse_free(step.free_intrinsics)
        free4_mask = sum(1 << i for i in range(4) if mask[i])
        names += [f"theta[{n}]" for n in nm]
    return types.SimpleNamespace(names=names, N=len(names), kin=kin, free=free, F=len(free), J=kin.J if kin is not None else 0,
                                 free4_mask=free4_mask, tie_focal=tie_focal)


def launch_linearize(step, lay, free_list, link_poses, joint_frames, B, mvp, dmvp, stream):
    """``ehr_lm_linearize`` at the step's current parameters (``model.dof``, ``K``) for B views given by ``link_poses`` [B,L,4,4]
    (and ``joint_frames`` [B,J,6] where joints are free; ``free_list``: ``lay.free`` as an int32 device tensor) -> ``mvp``
    [B,L,4,4], ``dmvp`` [N,B,L,4,4]."""
    kin, F = lay.kin, lay.F
    _lib.check(_lib.lib().ehr_lm_linearize(
        _lib.ptr(step.model.dof.data), _lib.ptr(step.K), _lib.ptr(link_poses), B, step.L, step.H, step.W,
        ctypes.c_float(step.near), ctypes.c_float(step.far), _lib.ptr(joint_frames if F else None),
        _lib.ptr(kin.upstream if F else None), _lib.ptr(kin.jkind if F else None), _lib.ptr(free_list),
        F, lay.J, lay.free4_mask, lay.tie_focal, lay.N, _lib.ptr(mvp), _lib.ptr(dmvp), stream), "ehr_lm_linearize")


def state_namespace(s, N):
    """One state block of ``ehr_lm_update`` (``s``: its EHR_LM_STATE_DOUBLES float64 on the host) as the namespace
    :meth:`LevenbergMarquardt.state` documents."""
    ns = types.SimpleNamespace(**{k: float(s[i]) for k, i in _lib.LM_STATE.items()})
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        setattr(ns, k, int(getattr(ns, k)))
    ns.theta = s[_lib.LM_THETA:_lib.LM_THETA + N].copy()
    ns.delta = s[_lib.LM_DELTA:_lib.LM_DELTA + N].copy()
    ns.g = s[_lib.LM_G:_lib.LM_G + N].copy()
    ns.H = s[_lib.LM_H:_lib.LM_H + 32 * 32].reshape(32, 32)[:N, :N].copy()
    ns.raw = s
    return ns


class _LmDriver:
    """The Levenberg-Marquardt iteration for P state blocks, whatever it drives: the buffers, the guard, the launch chain
    of an iteration and the reading of the state.  It renders through a list of UNITS, ``units``: a unit carries what one
    ``ehr_mask_information`` call works on -- ``glctx``, ``scene``, ``ref``, ``weight``, ``B`` (the views of the plan), ``H``,
    ``W``, ``L``, ``N`` (its tangents) -- gets ``mvp``, ``dmvp`` and the information outputs ``out`` from
    :meth:`_init_driver`, and provides ``_linearize(stream)`` and, where it has one, ``_forward_kinematics(stream)``, which
    is launched ahead of every linearisation and behind the finalising update.  ``label`` names it in the guard's messages.
    A driver with one context is its own one unit (:class:`LevenbergMarquardt`, :class:`easyhec_amd.lm_multi.MultiStartLM`);
    the rig has one per camera (:class:`easyhec_amd.lm_rig.RigLM`).  A subclass sets ``dev``, ``N`` (the parameters of a
    state block) and ``names``, calls :meth:`_init_driver`, and provides the ONE C call ``_update(stream, finalize=0)``.
    ``who`` names the owner in the guard's messages."""
    who, label, _forward_kinematics, prior = "solve_lm", "", None, None
    # the state block's size, the parameters it has room for and its reading are the driver's: None is ehr_lm_update's
    # (_lib.LM_STATE_DOUBLES, _lib.LM_MAX_PARAMS, read when the buffers are made); the rig's block-arrow update has a larger
    # block of its own (easyhec_amd.lm_rig)
    state_doubles = max_params = None

    def _namespace(self, s):
        """One state block (``s``: its float64 words on the host) as the namespace :meth:`states` documents."""
        return state_namespace(s, self.N)

    def set_prior(self, prior):
        """Take an :class:`LmPrior` made for this driver's parameters (None: no prior, today's update).  Set before the first
        iteration: ``F_acc`` of an accepted point carries the prior's term."""
        if prior is not None:
            if not isinstance(prior, LmPrior):
                raise TypeError(f"{self.who}: prior is an LmPrior (make_prior), not {type(prior).__name__}")
            if list(prior.names) != list(self.names):
                raise ValueError(f"{self.who}: the prior was made for {list(prior.names)}, the solve optimises "
                                 f"{list(self.names)}")
            if not _lib.has_lm_prior():
                raise RuntimeError("this libehr_hip.so has no prior form of the update (ehr_lm_update_prior): rebuild it")
            if getattr(self, "calls", 0):
                raise RuntimeError(f"{self.who}: the prior is set before the first iteration")
        self.prior = prior
        return self

    def _prior_ptrs(self):
        return _lib.ptr(self.prior.weight), _lib.ptr(self.prior.mean)

    def evaluate(self):
        """(summed loss, summed count) of ONE ``ehr_mask_information`` evaluation of every unit at the current parameters; the
        state block is not touched.  Synchronises."""
        self._guard()
        with torch.cuda.device(self.dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for u in self.units:
                if u._forward_kinematics is not None:
                    u._forward_kinematics(stream)
                u._linearize(stream)
                o = u.out
                information._launch(u.glctx, u.scene, u.mvp, u.dmvp, u.ref, o.info, o.grad, o.count, o.loss, None)
        loss, count = 0.0, 0
        for u in self.units:
            loss += float(u.out.loss.double().sum().item())
            count += int(u.out.count.sum().item())
        return loss, count

    def _init_driver(self, P, lambda0, ftol, lambda_max, log_rows, units=None):
        N, dev = self.N, self.dev
        max_params = _lib.LM_MAX_PARAMS if self.max_params is None else self.max_params
        if N > max_params:
            raise ValueError(f"{self.who}: the step optimises {N} parameters; the kernels take {max_params}")
        self.P = P
        self.ftol, self.lambda_max, self.lambda0 = float(ftol), float(lambda_max), float(lambda0)
        self.units = [self] if units is None else list(units)
        for u in self.units:
            u.mvp = torch.empty((u.B, u.L, 4, 4), device=dev)
            u.dmvp = torch.empty((u.N, u.B, u.L, 4, 4), device=dev)
            u.out = information._outputs(u.N, u.B, u.L, dev, True, False)
        st = np.zeros((P, _lib.LM_STATE_DOUBLES if self.state_doubles is None else self.state_doubles))
        st[:, _lib.LM_STATE["lambda"]], st[:, _lib.LM_STATE["nu"]] = self.lambda0, 2.0
        self.state_block = self._state = torch.from_numpy(st).to(dev)  # (a subclass may publish views of the two)
        self.log_rows = int(log_rows)
        self.log = self._log = torch.full((P, self.log_rows, 4), float("nan"), dtype=torch.float64, device=dev)
        self.calls = 0  # iterations enqueued so far: a hypothesis's `iterations` falls behind it once it is done

    # -- guards: a context is shared state; never iterate on a plan or on weights that are not the owner's -------------------
    def _guard(self):
        for u in self.units:
            plan = getattr(u.glctx, "_plan", None)
            if plan is None or plan.key != fused._plan_key(u.scene, u.B, u.H, u.W):
                raise RuntimeError(f"{self.who}: {u.label}its context holds another plan (somebody else rendered with it): "
                                   "plan and bind again first (a step object does when it takes a step)")
            if getattr(u.glctx, "_bound_weight", None) is not u.weight:
                raise RuntimeError(f"{self.who}: {u.label}the weights bound to its context are not its own (somebody else "
                                   "used the context): bind them again first (a step object does when it takes a step)")
        if self.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self.who}: not available while a graph is being captured")

    def iterate(self, n=1):
        """Enqueue ``n`` iterations (of every hypothesis) on the current stream; never synchronises.  After ``done`` an
        iteration only restores the accepted parameters."""
        self._guard()
        with torch.cuda.device(self.dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for _ in range(int(n)):
                for u in self.units:
                    if u._forward_kinematics is not None:
                        u._forward_kinematics(stream)
                    u._linearize(stream)
                    o = u.out
                    information._launch(u.glctx, u.scene, u.mvp, u.dmvp, u.ref, o.info, o.grad, o.count, o.loss, None)
                self._update(stream)
                self.calls += 1
        return self

    def finalize(self):
        """Leave the ACCEPTED parameters in the owner's tensors.  Enqueued; never synchronises."""
        with torch.cuda.device(self.dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._update(stream, finalize=1)
            for u in self.units:
                if u._forward_kinematics is not None:
                    u._forward_kinematics(stream)
        return self

    def states(self):
        """The P state blocks as a list of namespaces (one copy of [P,EHR_LM_STATE_DOUBLES]; synchronises): lambda, nu,
        F_acc, pred, rho, F_trial, the counters iterations / accepted / rejected / reported / retries, done, why, last,
        count, F_prior (the prior's term of F_acc; 0 without a prior) and theta [N], delta [N], g [N], H [N,N] of the accepted
        point (H and g: the data's own, under a prior too)."""
        s = self._state.cpu().numpy()
        return [self._namespace(s[p]) for p in range(self.P)]

    def trajectory(self, p):
        """Hypothesis p's [iterations, 4] float64 (CPU): per iteration the trial's loss (NaN: reported), 1 accepted / 0
        rejected / -1 reported, lambda after the iteration, and the gain ratio rho (NaN unless accepted).  Synchronises."""
        n = min(int(self._state[p, _lib.LM_STATE["iterations"]].item()), self.log_rows)
        return self._log[p, :n].cpu().numpy()

    def report(self, p, state=None):
        """The :class:`easyhec_amd.information.InformationReport` of hypothesis p's accepted point, from its state block."""
        s = self.states()[p] if state is None else state
        data_loss = s.F_acc - getattr(s, "F_prior", 0.0)
        return information.InformationReport(s.H[None], self.names, s.g[None], [s.count], [data_loss])

    def posterior(self, p=0, state=None):
        """Under a prior: the :class:`easyhec_amd.information.InformationReport` over ``H_views = [H_data, diag(weight)]`` and
        the matching gradients at the accepted point; its ``sigma2()`` is the prior's (the variance the weights were formed
        with), so ``covariance()`` is the posterior's.  None without a prior."""
        if self.prior is None:
            return None
        s = self.states()[p] if state is None else state
        w, mu = self.prior.weight.cpu().numpy(), self.prior.mean.cpu().numpy()
        if w.ndim == 2:  # (a P-block driver's prior: one row per hypothesis)
            w, mu = w[p], mu[p]
        gp = np.where(w != 0, 2.0 * w * (s.theta - np.where(w != 0, mu, 0.0)), 0.0)
        rep = information.InformationReport(np.stack([s.H, np.diag(w)]), self.names, np.stack([s.g, gp]), [s.count], [s.F_acc])
        sigma2 = self.prior.sigma2
        rep.sigma2 = lambda: sigma2
        return rep


class LevenbergMarquardt(_LmDriver):
    """Drives ``step`` (``FusedPoseStep``, ``JointPoseStep``, ``IntrinsicsPoseStep`` or ``JointIntrinsicsPoseStep``) by
    Levenberg-Marquardt iterations on the parameters it optimises, in the order of
    :func:`easyhec_amd.information.information_of` (``names``).  ``lambda0``, ``ftol``, ``lambda_max``: the damping's start,
    and the stopping rule's two thresholds (include/ehr.h, ``ehr_lm_update``); ``log_rows``: iterations the device log holds.

    ``iterate(n)`` enqueues n iterations and never synchronises; ``state()`` makes one small copy; ``finalize()`` leaves the
    accepted parameters in the step's tensors (``model.dof``, the offsets, ``theta`` and ``K``; the link poses follow the
    offsets; a trial is in them between iterations).  ``state_block`` [EHR_LM_STATE_DOUBLES] and ``log`` [log_rows,4] are the
    one hypothesis's."""

    def __init__(self, step, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, prior=None):
        _refuse(step)
        self.step, self.dev = step, step.dev
        self.glctx, self.scene, self.ref, self.weight = step.glctx, step.scene, step.ref, getattr(step, "weight", None)
        self.B, self.L, self.H, self.W = step.B, step.L, step.H, step.W
        self.layout = lay = parameter_layout(step)
        self.names, self.N, self.kin, self.F, self.J = lay.names, lay.N, lay.kin, lay.F, lay.J
        self.free4_mask, self.tie_focal = lay.free4_mask, lay.tie_focal
        self.free_list = torch.tensor(lay.free, dtype=torch.int32, device=self.dev) if lay.free else None
        self._init_driver(1, lambda0, ftol, lambda_max, log_rows)
        self.state_block, self.log = self._state[0], self._log[0]  # (views: the same memory)
        self.set_prior(prior)

    def _linearize(self, stream):
        st = self.step
        launch_linearize(st, self.layout, self.free_list, st.link_poses, st.joint_frames if self.F else None, st.B, self.mvp,
                         self.dmvp, stream)

    def _update(self, stream, finalize=0):
        st, o = self.step, self.out
        intr = self.free4_mask != 0
        args = (_lib.ptr(o.info), _lib.ptr(o.grad), _lib.ptr(o.count), _lib.ptr(o.loss), st.B, self.N,
                _lib.ptr(st.model.dof.data), _lib.ptr(st.offsets if self.F else None), _lib.ptr(self.free_list), self.F, self.J,
                _lib.ptr(st.theta if intr else None), self.free4_mask, self.tie_focal, _lib.ptr(st.K0 if intr else None),
                _lib.ptr(st.K if intr else None), st.H, st.W, ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max),
                int(finalize), _lib.ptr(self.state_block), _lib.ptr(self.log), self.log_rows)
        if self.prior is None:
            _lib.check(_lib.lib().ehr_lm_update(*args, stream), "ehr_lm_update")
        else:
            _lib.check(_lib.lib().ehr_lm_update_prior(*args, *self._prior_ptrs(), stream), "ehr_lm_update_prior")

    def parameters(self):
        """The N parameters as the step's tensors hold them, in ``names``' order (float32, host).  Synchronises."""
        st = self.step
        out = [st.model.dof.detach().cpu().numpy().reshape(-1)[:6]]
        if self.F:
            out.append(st.offsets.detach().cpu().numpy()[list(self.layout.free)])
        if self.free4_mask:
            th = st.theta.detach().cpu().numpy()
            first = {"f": 0, "fx": 0, "fy": 1, "cx": 2, "cy": 3}
            out.append(np.array([th[first[nm[6:-1]]] for nm in self.names[6 + self.F:]], dtype=np.float32))
        return np.concatenate(out).astype(np.float32)

    def joint_kinds(self):
        return self.kin.jkind.cpu().numpy() if self.kin is not None else None

    def _forward_kinematics(self, stream):
        if self.kin is not None:
            self.kin.launch(self.step, stream)

    def state(self):
        """The state block as one namespace: :meth:`_LmDriver.states` of the one hypothesis."""
        return self.states()[0]

    def trajectory(self):
        """[iterations, 4] float64 (CPU): :meth:`_LmDriver.trajectory` of the one hypothesis.  Synchronises."""
        return super().trajectory(0)

    def report(self, state=None):
        """The :class:`easyhec_amd.information.InformationReport` of the accepted point, from the state block alone (the
        data's report, under a prior too)."""
        return super().report(0, state)

    def posterior(self, state=None):
        """:meth:`_LmDriver.posterior` of the one hypothesis."""
        return super().posterior(0, state)


# ---- the prior ------------------------------------------------------------------------------------------------------------
@dataclass
class LmPrior:
    """A diagonal Gaussian prior for a Levenberg-Marquardt solve: ``F = sum_views w (mask - ref)^2 + sum_k weight_k (theta_k -
    mean_k)^2`` with ``weight_k = sigma2 / sigma_k^2`` (0 where there is no prior on parameter k)."""
    weight: torch.Tensor        # [N] float64, device: p_k, in loss units per squared parameter unit
    mean: torch.Tensor          # [N] float64, device: mu_k
    # (for the P hypotheses of a MultiStartLM both are [P,N]: every row of ``weight`` the same, ``mean`` a row per hypothesis)
    sigma: np.ndarray           # [N] float64: one standard deviation per parameter, inf where there is none
    sigma2: float               # the residual variance that puts prior and data in the same units; fixed for the solve
    names: list


def _prior_kinds(names, joint_kind):
    """``info_explorer.parameter_kinds`` extended to the rig's ``camK.dof[i]`` names."""
    from .info_explorer import parameter_kinds
    return parameter_kinds([nm.split(".", 1)[1] if nm.startswith("cam") and "." in nm else nm for nm in names], joint_kind)


def _no_prior_arguments(who, prior_sigma, sigma2, prior_mean, allowed=False):
    """``allowed``: the solve takes a prior (then ``sigma2`` / ``prior_mean`` need ``prior_sigma``); otherwise it is the multi-start
    solve in its pose-only form, which refuses all three."""
    if allowed:
        if prior_sigma is None and (sigma2 is not None or prior_mean is not None):
            raise ValueError(f"{who}: sigma2 and prior_mean belong to a prior: pass prior_sigma as well")
        return
    if prior_sigma is not None or sigma2 is not None or prior_mean is not None:
        raise ValueError(f"{who}: no prior is available for the multi-start solve: it is pose-only, and the prior is for "
                         "offsets and intrinsics (solve_lm and solve_lm_rig take one)")


def make_prior(driver_or_step, prior_sigma, sigma2=None, prior_mean=None):
    """The :class:`LmPrior` of a solve.  ``driver_or_step``: a :class:`LevenbergMarquardt` or
    :class:`easyhec_amd.lm_rig.RigLM`, or the step object one would drive (a driver is then made for the call), or a
    :class:`easyhec_amd.lm_multi.MultiStartLM` with free offsets or intrinsics (below).

    ``prior_sigma``: ``"default"`` -- ``info_explorer.PRIOR_SIGMA`` by kind for the offsets and the intrinsics, NO prior on a
    pose coordinate; a dict by parameter name or by kind (what it does not mention gets none); a number (every parameter); or
    a sequence of N (``inf`` or None: none).  ``prior_mean``: None, a dict by name, or a sequence of N; where it says nothing
    an offset's mean is 0, an intrinsics parameter's 0 (the given K) and a pose coordinate's its value NOW.  ``sigma2``: a
    positive number, or None for ``loss / max(count - N, 1)`` of ONE ``ehr_mask_information`` evaluation at the current
    parameters (the explorer's formula, ``InformationReport.sigma2``'s): one synchronising read; it then stays fixed for the
    solve and is recorded in the result.  That default is meant for a polish from near the optimum: far from it the loss is
    large, so it OVERWEIGHTS the prior -- pass a value there.

    For the P hypotheses of a ``MultiStartLM``: ``mean`` is [P,N] -- a pose coordinate's default is ITS hypothesis's value now,
    what ``prior_mean`` names holds for every hypothesis -- and ``weight`` [P,N] has every row equal:
    ONE ``sigma2`` for all hypotheses, or their objectives could not be ranked against each other.  With ``sigma2=None`` it is
    the MINIMUM over the hypotheses of ``loss_p / max(count_p - N, 1)`` from one evaluation of all of them: a far start's loss
    overweights the prior (above), and the best start's residual variance is the least overweighting one available.

    ValueError, with the reason: a sigma <= 0 or NaN, a mean that is not finite under a finite sigma, a wrong length, unknown
    names, ``sigma2 <= 0``."""
    from .info_explorer import PRIOR_SIGMA
    drv = driver_or_step
    if not isinstance(drv, _LmDriver):
        from .rig_calib import RigJointStep
        if isinstance(drv, RigJointStep):
            from .lm_rig import RigLM
            drv = RigLM(drv)
        else:
            drv = LevenbergMarquardt(drv)
    # hypothesis_priors: True for a P-block driver whose update takes [P,N] prior rows, False for one in its pose-only form
    blocks = getattr(drv, "hypothesis_priors", None)
    if blocks is False or (drv.P != 1 and not blocks) or not hasattr(drv, "parameters"):
        raise ValueError("make_prior: no prior is available for the multi-start solve (pose-only)")
    names, N = list(drv.names), drv.N
    kinds = _prior_kinds(names, drv.joint_kinds())
    # sigma
    if isinstance(prior_sigma, str):
        if prior_sigma != "default":
            raise ValueError(f"make_prior: prior_sigma {prior_sigma!r}: the one word is 'default'")
        sig = [PRIOR_SIGMA[kd] if kd in ("revolute", "prismatic", "focal", "principal") else np.inf for kd in kinds]
    elif isinstance(prior_sigma, dict):
        unknown = [k for k in prior_sigma if k not in names and k not in PRIOR_SIGMA]
        if unknown:
            raise ValueError(f"make_prior: prior_sigma {unknown}: keys are parameter names {names} or kinds {list(PRIOR_SIGMA)}")
        sig = [prior_sigma.get(nm, prior_sigma.get(kd, np.inf)) for nm, kd in zip(names, kinds)]
    elif np.ndim(prior_sigma) == 0 and prior_sigma is not None:
        sig = [prior_sigma] * N
    else:
        if prior_sigma is None or len(prior_sigma) != N:
            raise ValueError(f"make_prior: prior_sigma is 'default', a dict, a number or a sequence of N = {N} ({names})")
        sig = list(prior_sigma)
    sig = np.array([np.inf if x is None else float(x) for x in sig], dtype=np.float64)
    if np.isnan(sig).any() or (sig <= 0).any():
        raise ValueError(f"make_prior: every sigma is > 0 (inf or None: no prior), got {dict(zip(names, sig.tolist()))}")
    has = np.isfinite(sig)
    # mean
    now = drv.parameters().astype(np.float64)  # [N], or [P,N] for the blocks: everything below works on the last axis
    mean = np.where([kd in ("translation", "rotation") for kd in kinds], now, 0.0)
    if isinstance(prior_mean, dict):
        unknown = [k for k in prior_mean if k not in names]
        if unknown:
            raise ValueError(f"make_prior: prior_mean {unknown}: keys are parameter names {names}")
        for k, v in prior_mean.items():
            mean[..., names.index(k)] = float(v)
    elif prior_mean is not None:
        if np.ndim(prior_mean) != 1 or len(prior_mean) != N:
            raise ValueError(f"make_prior: prior_mean is None, a dict by name or a sequence of N = {N} ({names})")
        mean = np.broadcast_to(np.array([float(x) for x in prior_mean], dtype=np.float64), now.shape).copy()
    if not np.isfinite(mean[..., has]).all():
        raise ValueError(f"make_prior: the mean under a finite sigma is finite, got {dict(zip(names, mean.T.tolist()))}")
    mean = np.where(has, mean, 0.0)
    # sigma2
    if sigma2 is None:
        if blocks:
            pairs = drv.evaluate_each()
            loss, count = [ls for ls, _ in pairs], [ct for _, ct in pairs]
            each = [ls / max(ct - N, 1) for ls, ct in pairs]
            sigma2 = min(each) if np.isfinite(each).all() else float("nan")
        else:
            loss, count = drv.evaluate()
            sigma2 = loss / max(count - N, 1)
        if not (np.isfinite(sigma2) and sigma2 > 0):
            raise ValueError(f"make_prior: the evaluation at the current parameters gives sigma2 = {sigma2} (loss {loss}, count "
                             f"{count}): pass sigma2")
    elif not (np.isfinite(sigma2) and sigma2 > 0):
        raise ValueError(f"make_prior: sigma2 must be finite and > 0, got {sigma2}")
    weight = np.where(has, float(sigma2) / np.where(has, sig, 1.0) ** 2, 0.0)
    if not np.isfinite(weight).all():
        raise ValueError(f"make_prior: sigma2 / sigma^2 overflows: {dict(zip(names, weight.tolist()))}")
    weight = np.broadcast_to(weight, now.shape).copy()  # (the blocks: every row the same)
    return LmPrior(torch.from_numpy(weight).to(drv.dev), torch.from_numpy(mean).to(drv.dev), sig, float(sigma2), names)


@dataclass
class LmResult:
    loss: float                 # F_acc: the summed per-view loss at the accepted point
    iterations: int
    accepted: int
    rejected: int
    reported: int
    done: bool
    why: str                    # the reason it stopped ("max_iters" where it did not stop by itself)
    trajectory: np.ndarray      # [iterations,4]: loss, accepted flag, lambda, rho per iteration
    report: object              # InformationReport at the accepted point
    recoveries: list = field(default_factory=list)
    state: object = None        # the final state namespace
    lm: object = None           # the LevenbergMarquardt object
    data_loss: float = None     # F_acc - F_prior: the summed per-view loss at the accepted point (== loss without a prior)
    prior_loss: float = 0.0     # F_prior: sum_k p_k (theta_k - mu_k)^2 at the accepted point
    prior: object = None        # the LmPrior the solve ran under (sigma2 included), or None
    posterior: object = None    # under a prior: InformationReport over [H_data, diag(weight)]; covariance() is the posterior's


def _run_to_convergence(driver, max_iters, check_every, recover, check_status, who):
    """The polling loop of :func:`solve_lm` and :func:`easyhec_amd.lm_multi.solve_lm_multi`.  Every round reads the
    driver's states once.  If more iterations were reported than before (NaN loss: not taken), ``recover()`` is called and
    what it did (if anything) is noted -- at most 4 such rounds, the fifth calls ``check_status()`` and raises in ``who``'s
    name.  The hypotheses that are not done have each taken ``iterations - reported`` EFFECTIVE iterations: the loop ends
    when none is left or the one that has taken fewest has taken ``max_iters``, otherwise ``check_every`` more (at most the
    rest) are enqueued.  Ends with ``finalize()``; returns what the recoveries did, in order."""
    recoveries, rounds, seen = [], 0, 0
    while True:
        S = driver.states()
        reported = sum(s.reported for s in S)
        if reported > seen:
            seen = reported
            what = recover()
            if what:
                recoveries.append(what)
            rounds += 1
            if rounds > 4:
                check_status()
                raise RuntimeError(f"{who}: iterations keep being reported as not taken (NaN loss)")
        running = [s.iterations - s.reported for s in S if not s.done]
        if not running or min(running) >= max_iters:
            break
        driver.iterate(min(check_every, max_iters - min(running)))
    driver.finalize()
    return recoveries


def result_of(lm, recoveries):
    """The :class:`LmResult` of a finished one-block solve (``solve_lm``, ``solve_lm_rig``)."""
    s = lm.state()
    why = WHY[s.why].split(":")[0] if s.done else "max_iters"
    return LmResult(s.F_acc, s.iterations, s.accepted, s.rejected, s.reported, bool(s.done), why, lm.trajectory(),
                    lm.report(s), recoveries, s, lm, s.F_acc - s.F_prior, s.F_prior, lm.prior, lm.posterior(s))


def solve_lm(step, max_iters=50, check_every=5, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, prior_sigma=None, sigma2=None,
             prior_mean=None):
    """Levenberg-Marquardt on ``step``'s parameters from where they are: at most ``max_iters`` EFFECTIVE iterations (a
    reported one -- the plan's job slots overflowed, the view needs the general-triangle pass -- is recovered from the way
    ``_ChainStep`` recovers a step, and taken again), ``done`` polled every ``check_every`` iterations.  Ends with the accepted
    parameters in the step's tensors; a captured chain stays valid.  Returns an :class:`LmResult`.

    ``prior_sigma`` (None: no prior, today's solve bit for bit), ``sigma2``, ``prior_mean``: :func:`make_prior`'s -- the solve
    is then the MAP estimate: ``loss`` is the total objective, ``data_loss`` and ``prior_loss`` its two parts, ``report`` the
    data's report and ``posterior`` the posterior's."""
    lm = LevenbergMarquardt(step, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max, log_rows=max_iters + 4 * check_every + 8)
    _no_prior_arguments("solve_lm", prior_sigma, sigma2, prior_mean, allowed=True)
    if prior_sigma is not None:
        lm.set_prior(make_prior(lm, prior_sigma, sigma2, prior_mean))

    def recover():
        what = step.recover_from_overflow() if hasattr(step, "recover_from_overflow") else False
        if what and hasattr(step, "recoveries"):
            step.recoveries.append(what)
        return what

    recoveries = _run_to_convergence(lm, max_iters, check_every, recover, lambda: fused.check_status(step.glctx), "solve_lm")
    return result_of(lm, recoveries)
