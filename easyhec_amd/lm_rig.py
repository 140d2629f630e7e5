"""Levenberg-Marquardt over a camera rig: every camera's pose and the SHARED joint offsets as ONE damped Gauss-Newton system
(``ehr_lm_update_rig`` in include/ehr.h, csrc/ehr_lm.hip).

:class:`easyhec_amd.rig_calib.RigJointStep` fits C fixed cameras that watch one arm by first-order Adam with two hand-set
learning rates and no stopping rule.  A rig mixes metres, radians and joint angles over C + 1 parameter groups, and the
offsets couple the cameras: exactly where a scale-free, monotone, self-stopping iteration pays.  The system is
:func:`easyhec_amd.information.rig_information`'s -- ``cam0.dof[0..5]``, ``cam1.dof[0..5]``, ..., ``offset[j]`` for the free
joints, ``N = 6 C + F <= 32`` -- and one iteration is, on one stream and eagerly,

    per camera   ehr_joint_forward (the shared offsets) -> ehr_lm_linearize -> ehr_mask_information     on that camera's context
    once         ehr_lm_update_rig        the cameras' sums embedded and added in camera order, then ehr_lm_update's steps

With one camera it is :func:`easyhec_amd.lm.solve_lm` on a ``JointPoseStep`` bit for bit (tests/test_gpu_lm_rig.py).  A
reported call is rig-wide, as a reported Adam step of the rig is: no pose and no offset moves.  Like ``solve_lm`` it is a
refinement BESIDE Adam: the moments, every group's step counter, ``history_ops`` and the history cursors stay untouched, and
``rig_step.step()`` works afterwards.  HIP only; no fallback.

This module holds what is particular to a rig: the unit per camera, the host array of ``ehr_lm_rig_camera`` and the one C
call.  The iteration and the solve loop are :mod:`easyhec_amd.lm`'s (``_LmDriver``, ``_run_to_convergence``), the recovery
``RigJointStep``'s own.  Out of scope: intrinsics in a rig, multi-start or a global search over a rig, data-parallel rigs,
graph capture, more than 32 parameters, information-gain exploration for a rig."""
import ctypes

import numpy as np
import torch

from . import _lib
from .lm import _LmDriver, _run_to_convergence, launch_linearize, make_prior, parameter_layout, result_of

__all__ = ["RigLM", "solve_lm_rig"]


class _CameraUnit:
    """One camera of the rig as a render unit of ``_LmDriver``: its context, plan, bound reference and weights, and the two
    launches ahead of its ``ehr_mask_information``.  ``N`` = 6 + F: its pose and the shared offsets."""

    def __init__(self, c, cam):
        self.cam, self.label = cam, f"camera {c}: "
        self.glctx, self.scene, self.ref, self.weight = cam.glctx, cam.scene, cam.ref, getattr(cam, "weight", None)
        self.B, self.L, self.H, self.W = cam.B, cam.L, cam.H, cam.W
        self.layout = lay = parameter_layout(cam)
        self.N, self.F = lay.N, lay.F
        self.free_list = torch.tensor(lay.free, dtype=torch.int32, device=cam.dev) if lay.free else None

    def _forward_kinematics(self, stream):
        self.cam.kinematics.launch(self.cam, stream)

    def _linearize(self, stream):
        cam = self.cam
        launch_linearize(cam, self.layout, self.free_list, cam.link_poses, cam.joint_frames if self.F else None, cam.B, self.mvp,
                         self.dmvp, stream)


def _refuse(rig):
    from .rig_calib import RigJointStep
    if not isinstance(rig, RigJointStep):
        raise TypeError(f"solve_lm_rig: {type(rig).__name__} is not a RigJointStep (the other step objects: solve_lm)")
    if rig.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("solve_lm_rig: not available while a graph is being captured: ehr_mask_information sizes its scratch "
                           "on the first call")
    if not _lib.has_lm_rig():
        raise RuntimeError("this libehr_hip.so has no rig Levenberg-Marquardt kernel (ehr_lm_update_rig): rebuild it")
    if not _lib.has_lm() or not _lib.has_information():
        raise RuntimeError("this libehr_hip.so has no Levenberg-Marquardt / information kernels (ehr_lm_linearize, "
                           "ehr_mask_information): rebuild it")
    C, F = rig.C, len(rig.free_joints)
    if 6 * C + F > _lib.LM_MAX_PARAMS:
        raise ValueError(f"solve_lm_rig: {C} cameras and {F} free joints are {6 * C + F} parameters; the kernels take "
                         f"{_lib.LM_MAX_PARAMS}: this free set leaves room for {(_lib.LM_MAX_PARAMS - F) // 6} cameras")


class RigLM(_LmDriver):
    """Drives a :class:`easyhec_amd.rig_calib.RigJointStep` by Levenberg-Marquardt iterations on its ``6 C + F`` parameters, in
    the order of :func:`easyhec_amd.information.rig_information` (``names``): ONE state block over C contexts.  ``lambda0``,
    ``ftol``, ``lambda_max``, ``log_rows``: :class:`easyhec_amd.lm.LevenbergMarquardt`'s.

    ``iterate(n)`` enqueues n iterations and never synchronises; ``state()`` makes one small copy; ``finalize()`` leaves the
    accepted poses in every ``model.dof`` and the accepted offsets in ``rig.offsets``, and every camera's link poses follow (a
    trial is in them between iterations).  ``units[c]`` holds camera c's ``mvp``, ``dmvp`` and information outputs ``out``;
    ``mvp``, ``dmvp`` and ``out`` are the lists of them.  ``state_block`` [EHR_LM_STATE_DOUBLES] and ``log`` [log_rows,4] are
    the one system's."""
    who = "solve_lm_rig"

    def __init__(self, rig_step, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, prior=None):
        _refuse(rig_step)
        self.rig, self.dev = rig_step, rig_step.dev
        self.C, self.J = rig_step.C, rig_step.J
        free = list(rig_step.free_joints)
        self.F, self.N = len(free), 6 * self.C + len(free)
        self.names = [f"cam{c}.dof[{i}]" for c in range(self.C) for i in range(6)] + [f"offset[{j}]" for j in free]
        self.free_list = torch.tensor(free, dtype=torch.int32, device=self.dev) if free else None
        self._init_driver(1, lambda0, ftol, lambda_max, log_rows, units=[_CameraUnit(c, cam) for c, cam in enumerate(rig_step.cameras)])
        self.mvp, self.dmvp, self.out = [u.mvp for u in self.units], [u.dmvp for u in self.units], [u.out for u in self.units]
        self.state_block, self.log = self._state[0], self._log[0]  # (views: the same memory)
        self._cams, self._cams_key = None, None
        self.set_prior(prior)

    def _camera_array(self):
        """The HOST array of ``ehr_lm_rig_camera``; built once, and again whenever a pointer in it has changed (a model's
        ``dof`` storage replaced, a unit's buffers swapped)."""
        p = lambda t: t.data_ptr()
        rows = [(p(u.out.info), p(u.out.grad), p(u.out.count), p(u.out.loss), p(u.cam.model.dof.data), u.B) for u in self.units]
        if rows != self._cams_key:
            self._cams, self._cams_key = (_lib.LmRigCamera * self.C)(*[_lib.LmRigCamera(*r) for r in rows]), rows
        return self._cams

    def _update(self, stream, finalize=0):
        args = (self._camera_array(), self.C, _lib.ptr(self.rig.offsets if self.F else None), _lib.ptr(self.free_list), self.F,
                self.J, ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max), int(finalize), _lib.ptr(self.state_block),
                _lib.ptr(self.log), self.log_rows)
        if self.prior is None:
            _lib.check(_lib.lib().ehr_lm_update_rig(*args, stream), "ehr_lm_update_rig")
        else:
            _lib.check(_lib.lib().ehr_lm_update_rig_prior(*args, *self._prior_ptrs(), stream), "ehr_lm_update_rig_prior")

    def parameters(self):
        """The ``6 C + F`` parameters as the rig's tensors hold them, in ``names``' order (float32, host).  Synchronises."""
        out = [cam.model.dof.detach().cpu().numpy().reshape(-1)[:6] for cam in self.rig.cameras]
        if self.F:
            out.append(self.rig.offsets.detach().cpu().numpy()[[int(j) for j in self.free_list.cpu().numpy()]])
        return np.concatenate(out).astype(np.float32)

    def joint_kinds(self):
        kin = self.units[0].layout.kin
        return kin.jkind.cpu().numpy() if kin is not None else None

    def state(self):
        """The state block as one namespace: :meth:`easyhec_amd.lm._LmDriver.states` of the one system."""
        return self.states()[0]

    def trajectory(self):
        """[iterations, 4] float64 (CPU): :meth:`easyhec_amd.lm._LmDriver.trajectory` of the one system.  Synchronises."""
        return super().trajectory(0)

    def report(self, state=None):
        """The :class:`easyhec_amd.information.InformationReport` of the ``6 C + F`` system at the accepted point (the data's,
        under a prior too)."""
        return super().report(0, state)

    def posterior(self, state=None):
        """:meth:`easyhec_amd.lm._LmDriver.posterior` of the one system."""
        return super().posterior(0, state)


def solve_lm_rig(rig_step, max_iters=50, check_every=5, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, prior_sigma=None, sigma2=None,
                 prior_mean=None):
    """:func:`easyhec_amd.lm.solve_lm` for a rig, with its loop: Levenberg-Marquardt on every camera's pose and the shared
    offsets from where they are, at most ``max_iters`` EFFECTIVE iterations (a reported one is rig-wide; every camera's
    context is recovered the way the rig's Adam solve recovers them -- ``recoveries`` reads "camera c: job slots" -- and the
    iteration is taken again), ``done`` polled every ``check_every`` iterations.  Ends with the accepted poses in every
    ``model.dof``, the accepted offsets in ``rig_step.offsets`` and the link poses at them.  Returns an
    :class:`easyhec_amd.lm.LmResult`: ``loss`` is the summed loss over all views of all cameras, ``report`` the
    ``InformationReport`` of the ``6 C + F`` system with ``rig_information``'s names.  ``prior_sigma`` (None: no prior),
    ``sigma2``, ``prior_mean``: :func:`easyhec_amd.lm.make_prior`'s over the rig's names -- with ``"default"`` the shared offsets
    are held near zero and no camera's pose is; the result's ``data_loss``, ``prior_loss``, ``prior`` and ``posterior`` as for
    ``solve_lm``."""
    lm = RigLM(rig_step, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max, log_rows=max_iters + 4 * check_every + 8)
    if prior_sigma is None and (sigma2 is not None or prior_mean is not None):
        raise ValueError("solve_lm_rig: sigma2 and prior_mean belong to a prior: pass prior_sigma as well")
    if prior_sigma is not None:
        lm.set_prior(make_prior(lm, prior_sigma, sigma2, prior_mean))
    notes = _run_to_convergence(lm, max_iters, check_every, rig_step._recover_and_note, rig_step._check_status, "solve_lm_rig")
    return result_of(lm, [what for did in notes for what in did])
