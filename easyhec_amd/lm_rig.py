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

``solver="arrow"`` (``ehr_lm_update_rig_arrow``) solves the same system by block
elimination on its block-arrow form: every camera may free its own intrinsics (``free_intrinsics``), which ride in that
camera's block -- ``cam0.dof[0..5]``, ``cam0.theta[...]``, ``cam1.dof[0..5]``, ..., ``offset[j]`` -- and the limit of 32
parameters is gone (16 cameras, ``F + I_c <= 26`` per camera, ``N <= 182``).  A wrong focal length of one camera is then fitted
where it belongs instead of being absorbed into the shared offsets.  The default solve stays ``ehr_lm_update_rig``, bit for bit.

This module holds what is particular to a rig: the unit per camera, the host arrays of ``ehr_lm_rig_camera`` /
``ehr_lm_rig_arrow_camera`` and the one C call.  The iteration and the solve loop are :mod:`easyhec_amd.lm`'s (``_LmDriver``,
``_run_to_convergence``), the recovery ``RigJointStep``'s own.  Out of scope: intrinsics in the rig's ADAM step, multi-start or
a global search over a rig, data-parallel rigs, graph capture, information-gain exploration for a rig."""
import ctypes
import types

import numpy as np
import torch

from . import _lib
from .lm import _LmDriver, _run_to_convergence, launch_linearize, make_prior, parameter_layout, result_of

__all__ = ["RigLM", "solve_lm_rig"]


class _CameraUnit:
    """One camera of the rig as a render unit of ``_LmDriver``: its context, plan, bound reference and weights, and the two
    launches ahead of its ``ehr_mask_information``.  ``N`` = 6 + F: its pose and the shared offsets -- plus, for the arrow
    solve, the intrinsics ``free`` names (``theta`` [4], ``K0`` and the camera's own ``K`` buffer are then the unit's)."""

    def __init__(self, c, cam, free=None):
        self.cam, self.label = cam, f"camera {c}: "
        self.glctx, self.scene, self.ref, self.weight = cam.glctx, cam.scene, cam.ref, getattr(cam, "weight", None)
        self.B, self.L, self.H, self.W = cam.B, cam.L, cam.H, cam.W
        self.layout = lay = parameter_layout(cam)
        self.theta = self.K0 = None
        self.theta_names, self.elements = [], []
        if free:
            from .intrinsics_calib import _NAMES, _parse_free
            mask, tie, self.theta_names = _parse_free(free)
            self.elements = [0 if n == "f" else _NAMES[n] for n in self.theta_names]   # the theta element each parameter reads
            self.layout = lay = types.SimpleNamespace(**dict(
                vars(lay), names=lay.names + [f"theta[{n}]" for n in self.theta_names], N=lay.N + len(self.theta_names),
                free4_mask=sum(1 << i for i in range(4) if mask[i]), tie_focal=tie))
            # the intrinsics as given, and the buffer the update writes and the camera's chain and linearisation read: the
            # solve's own, never the caller's tensor
            self.theta = torch.zeros(4, device=cam.dev)
            self.K0 = cam.K.detach().clone().contiguous()
            cam.K = self.K0.clone()
        self.N, self.F = lay.N, lay.F
        self.free_list = torch.tensor(lay.free, dtype=torch.int32, device=cam.dev) if lay.free else None

    def _forward_kinematics(self, stream):
        self.cam.kinematics.launch(self.cam, stream)

    def _linearize(self, stream):
        cam = self.cam
        launch_linearize(cam, self.layout, self.free_list, cam.link_poses, cam.joint_frames if self.F else None, cam.B, self.mvp,
                         self.dmvp, stream)


def _refuse(rig, arrow=False):
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
    if arrow:
        if not _lib.has_lm_rig_arrow():
            raise RuntimeError("this libehr_hip.so has no block-arrow rig update (ehr_lm_update_rig_arrow): rebuild it")
    elif 6 * C + F > _lib.LM_MAX_PARAMS:
        raise ValueError(f"solve_lm_rig: {C} cameras and {F} free joints are {6 * C + F} parameters; the kernels take "
                         f"{_lib.LM_MAX_PARAMS}: this free set leaves room for {(_lib.LM_MAX_PARAMS - F) // 6} cameras "
                         '(solver="arrow" has no such limit)')


def _per_camera_free(rig, free_intrinsics):
    """``free_intrinsics`` as one canonical tuple of names per camera (``()``: that camera's ``K`` is fixed).  One free set --
    a name, or a sequence of names -- holds for every camera; a sequence with an entry that is not a name (None, a tuple, a
    list) has one entry per camera."""
    from .intrinsics_calib import _parse_free, _refuse as refuse_intrinsics
    fi, C = free_intrinsics, rig.C
    if fi is None or isinstance(fi, str) or all(isinstance(x, str) for x in fi):
        per = [fi] * C
    else:
        per = list(fi)
        if len(per) != C:
            raise ValueError(f"solve_lm_rig: free_intrinsics= has {len(per)} entries for {C} cameras")
    out = []
    for c, (cam, free) in enumerate(zip(rig.cameras, per)):
        names = tuple(_parse_free(free)[2]) if free else ()
        if names:
            if not _lib.has_intrinsics():
                raise RuntimeError("this libehr_hip.so has no intrinsics kernel (ehr_intrinsics_backward_adam): rebuild it")
            try:
                refuse_intrinsics({"K": cam.batch_K}, {})
            except ValueError as e:
                raise ValueError(f"solve_lm_rig: camera {c}: {e}") from None
        if len(rig.free_joints) + len(names) > _lib.LM_ARROW_MAX_SHARED:
            raise ValueError(f"solve_lm_rig: camera {c}: {len(rig.free_joints)} free joints and {len(names)} free intrinsics; "
                             f"a camera's own system takes 6 + {_lib.LM_ARROW_MAX_SHARED} parameters")
        out.append(names)
    return out


def arrow_state_namespace(s, P, F):
    """One state block of ``ehr_lm_update_rig_arrow`` (``s``: its EHR_LM_ARROW_STATE_DOUBLES float64 on the host; ``P``: the
    cameras' block sizes) as :func:`easyhec_amd.lm.state_namespace`'s namespace, the packed ``H_acc`` expanded to the dense
    [N,N] matrix in the system's order."""
    L = _lib
    S0 = int(sum(P))
    N = S0 + F
    ns = types.SimpleNamespace(**{k: float(s[i]) for k, i in L.LM_STATE.items()})
    for k in ("iterations", "accepted", "rejected", "reported", "done", "why", "last", "count", "retries"):
        setattr(ns, k, int(getattr(ns, k)))
    ns.theta = s[L.LM_ARROW_THETA:L.LM_ARROW_THETA + N].copy()
    ns.delta = s[L.LM_ARROW_DELTA:L.LM_ARROW_DELTA + N].copy()
    ns.g = s[L.LM_ARROW_G:L.LM_ARROW_G + N].copy()
    H, b = np.zeros((N, N)), 0
    PB, FS = L.LM_ARROW_MAX_BLOCK, L.LM_ARROW_MAX_SHARED
    for c, Pc in enumerate(P):
        at = L.LM_ARROW_H + c * L.LM_ARROW_CAMERA_STRIDE
        panel = s[at:at + L.LM_ARROW_BORDER_T].reshape(PB, L.LM_ARROW_PANEL_STRIDE)
        other = s[at + L.LM_ARROW_BORDER_T:at + L.LM_ARROW_CAMERA_STRIDE].reshape(FS, PB)
        H[b:b + Pc, b:b + Pc] = panel[:Pc, :Pc]
        H[b:b + Pc, S0:] = panel[:Pc, PB:PB + F]
        H[S0:, b:b + Pc] = other[:F, :Pc]
        b += Pc
    H[S0:, S0:] = s[L.LM_ARROW_CORNER:L.LM_ARROW_CORNER + FS * FS].reshape(FS, FS)[:F, :F]
    ns.H = H
    ns.raw = s
    return ns


class RigLM(_LmDriver):
    """Drives a :class:`easyhec_amd.rig_calib.RigJointStep` by Levenberg-Marquardt iterations on its ``6 C + F`` parameters, in
    the order of :func:`easyhec_amd.information.rig_information` (``names``): ONE state block over C contexts.  ``lambda0``,
    ``ftol``, ``lambda_max``, ``log_rows``: :class:`easyhec_amd.lm.LevenbergMarquardt`'s.

    ``iterate(n)`` enqueues n iterations and never synchronises; ``state()`` makes one small copy; ``finalize()`` leaves the
    accepted poses in every ``model.dof`` and the accepted offsets in ``rig.offsets``, and every camera's link poses follow (a
    trial is in them between iterations).  ``units[c]`` holds camera c's ``mvp``, ``dmvp`` and information outputs ``out``;
    ``mvp``, ``dmvp`` and ``out`` are the lists of them.  ``state_block`` [EHR_LM_STATE_DOUBLES] and ``log`` [log_rows,4] are
    the one system's.

    ``solver``: ``"dense"`` is ``ehr_lm_update_rig`` on a dense [32][32] system (``6 C + F <= 32``, no intrinsics);
    ``"arrow"`` is ``ehr_lm_update_rig_arrow``, block elimination on the block-arrow system: any rig of up to 16 cameras with
    ``F + I_c <= 26`` per camera, ``state_block`` [EHR_LM_ARROW_STATE_DOUBLES].  None: ``"arrow"`` if ``free_intrinsics`` is
    given, else ``"dense"``.  ``free_intrinsics``: one free set for every camera (a name or a sequence of names out of "f",
    "fx", "fy", "cx", "cy"), or a sequence with one entry per camera, each a tuple of names, None or () (that camera's ``K``
    is fixed).  A camera with free intrinsics gets its own ``theta`` [4] (zeros), ``K0`` (a clone of its ``K``) and its own
    ``K`` buffer in ``rig_step.cameras[c].K``, which its chain, the linearisation and the rig's Adam step read from then on;
    the caller's tensor is never written (``K0`` is the camera's ``K`` when THIS driver is made: a second solve starts its
    ``theta`` at zero around the first one's result).  ``names`` are then ``cam0.dof[0..5]``, ``cam0.theta[...]``, ``cam1.dof[0..5]``, ...,
    ``offset[j]``; ``state()`` expands the packed ``H_acc`` to the dense [N,N] matrix, so ``report()``, ``posterior()`` and
    :func:`easyhec_amd.lm.make_prior` work through ``names`` unchanged; ``intrinsics()`` returns every camera's ``K``."""
    who = "solve_lm_rig"

    def __init__(self, rig_step, lambda0=1e-3, ftol=1e-6, lambda_max=1e6, log_rows=256, prior=None, free_intrinsics=None,
                 solver=None):
        if solver is None:
            solver = "dense" if free_intrinsics is None else "arrow"
        if solver not in ("dense", "arrow"):
            raise ValueError(f"solve_lm_rig: solver {solver!r}: 'dense' (ehr_lm_update_rig, at most 32 parameters) or 'arrow' "
                             "(ehr_lm_update_rig_arrow: block elimination, per-camera intrinsics)")
        if solver == "dense" and free_intrinsics is not None:
            raise ValueError("solve_lm_rig: free_intrinsics needs solver='arrow': the dense rig update has no intrinsics")
        self.solver = solver
        _refuse(rig_step, arrow=solver == "arrow")
        self.rig, self.dev = rig_step, rig_step.dev
        self.C, self.J = rig_step.C, rig_step.J
        free = list(rig_step.free_joints)
        self.F = len(free)
        per = _per_camera_free(rig_step, free_intrinsics) if solver == "arrow" else [()] * self.C
        units = [_CameraUnit(c, cam, per[c]) for c, cam in enumerate(rig_step.cameras)]
        self.block_sizes = [6 + len(u.theta_names) for u in units]
        self.N = sum(self.block_sizes) + self.F
        self.names = [nm for c, u in enumerate(units) for nm in
                      [f"cam{c}.dof[{i}]" for i in range(6)] + [f"cam{c}.theta[{n}]" for n in u.theta_names]] + \
                     [f"offset[{j}]" for j in free]
        self.free_list = torch.tensor(free, dtype=torch.int32, device=self.dev) if free else None
        if solver == "arrow":
            self.state_doubles, self.max_params = _lib.LM_ARROW_STATE_DOUBLES, _lib.LM_ARROW_MAX_PARAMS
        self._init_driver(1, lambda0, ftol, lambda_max, log_rows, units=units)
        self.mvp, self.dmvp, self.out = [u.mvp for u in self.units], [u.dmvp for u in self.units], [u.out for u in self.units]
        self.state_block, self.log = self._state[0], self._log[0]  # (views: the same memory)
        self._cams, self._cams_key = None, None
        self.set_prior(prior)

    def _namespace(self, s):
        if self.solver == "arrow":
            return arrow_state_namespace(s, self.block_sizes, self.F)
        return super()._namespace(s)

    def _camera_array(self):
        """The HOST array of ``ehr_lm_rig_camera`` (``ehr_lm_rig_arrow_camera`` for the arrow solve); built once, and again
        whenever a pointer in it has changed (a model's ``dof`` storage replaced, a unit's buffers swapped)."""
        p = lambda t: None if t is None else t.data_ptr()
        rows = [(p(u.out.info), p(u.out.grad), p(u.out.count), p(u.out.loss), p(u.cam.model.dof.data), u.B) for u in self.units]
        kind = _lib.LmRigCamera
        if self.solver == "arrow":
            kind = _lib.LmRigArrowCamera
            rows = [r[:5] + (p(u.theta), p(u.K0), p(u.cam.K if u.theta is not None else None), u.B, u.H, u.W,
                             u.layout.free4_mask, u.layout.tie_focal) for r, u in zip(rows, self.units)]
        if rows != self._cams_key:
            self._cams, self._cams_key = (kind * self.C)(*[kind(*r) for r in rows]), rows
        return self._cams

    def _update(self, stream, finalize=0):
        if self.solver == "arrow":
            pw, pm = self._prior_ptrs() if self.prior is not None else (None, None)
            _lib.check(_lib.lib().ehr_lm_update_rig_arrow(
                self._camera_array(), self.C, _lib.ptr(self.rig.offsets if self.F else None), _lib.ptr(self.free_list), self.F,
                self.J, ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max), int(finalize), _lib.ptr(self.state_block),
                _lib.ptr(self.log), self.log_rows, pw, pm, stream), "ehr_lm_update_rig_arrow")
            return
        args = (self._camera_array(), self.C, _lib.ptr(self.rig.offsets if self.F else None), _lib.ptr(self.free_list), self.F,
                self.J, ctypes.c_double(self.ftol), ctypes.c_double(self.lambda_max), int(finalize), _lib.ptr(self.state_block),
                _lib.ptr(self.log), self.log_rows)
        if self.prior is None:
            _lib.check(_lib.lib().ehr_lm_update_rig(*args, stream), "ehr_lm_update_rig")
        else:
            _lib.check(_lib.lib().ehr_lm_update_rig_prior(*args, *self._prior_ptrs(), stream), "ehr_lm_update_rig_prior")

    def parameters(self):
        """The N parameters as the rig's tensors hold them, in ``names``' order (float32, host).  Synchronises."""
        out = []
        for u in self.units:
            out.append(u.cam.model.dof.detach().cpu().numpy().reshape(-1)[:6])
            if u.theta is not None:
                out.append(u.theta.cpu().numpy()[u.elements])
        if self.F:
            out.append(self.rig.offsets.detach().cpu().numpy()[[int(j) for j in self.free_list.cpu().numpy()]])
        return np.concatenate(out).astype(np.float32)

    def intrinsics(self):
        """A list with one [3,3] float32 ``K`` per camera (CPU, copies) at the current parameters: the one that camera renders
        with (a trial's between iterations, the accepted one after ``finalize()``).  Synchronises."""
        return [cam.K.detach().cpu().clone() for cam in self.rig.cameras]

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
                 prior_mean=None, free_intrinsics=None, solver=None):
    """:func:`easyhec_amd.lm.solve_lm` for a rig, with its loop: Levenberg-Marquardt on every camera's pose and the shared
    offsets from where they are, at most ``max_iters`` EFFECTIVE iterations (a reported one is rig-wide; every camera's
    context is recovered the way the rig's Adam solve recovers them -- ``recoveries`` reads "camera c: job slots" -- and the
    iteration is taken again), ``done`` polled every ``check_every`` iterations.  Ends with the accepted poses in every
    ``model.dof``, the accepted offsets in ``rig_step.offsets`` and the link poses at them.  Returns an
    :class:`easyhec_amd.lm.LmResult`: ``loss`` is the summed loss over all views of all cameras, ``report`` the
    ``InformationReport`` of the ``6 C + F`` system with ``rig_information``'s names.  ``prior_sigma`` (None: no prior),
    ``sigma2``, ``prior_mean``: :func:`easyhec_amd.lm.make_prior`'s over the rig's names -- with ``"default"`` the shared offsets
    are held near zero and no camera's pose is; the result's ``data_loss``, ``prior_loss``, ``prior`` and ``posterior`` as for
    ``solve_lm``.

    ``free_intrinsics`` (one free set for every camera, or a list with one entry per camera; None or () there: that camera's
    ``K`` is fixed) and ``solver`` are :class:`RigLM`'s: with intrinsics free the solve ends with every camera's accepted ``K``
    in ``rig_step.cameras[c].K`` (``result.lm.intrinsics()``), the prior's ``"default"`` also holds them near the given ``K``,
    and ``rig_step.step()`` renders with the refined ``K`` afterwards."""
    lm = RigLM(rig_step, lambda0=lambda0, ftol=ftol, lambda_max=lambda_max, log_rows=max_iters + 4 * check_every + 8,
               free_intrinsics=free_intrinsics, solver=solver)
    if prior_sigma is None and (sigma2 is not None or prior_mean is not None):
        raise ValueError("solve_lm_rig: sigma2 and prior_mean belong to a prior: pass prior_sigma as well")
    if prior_sigma is not None:
        lm.set_prior(make_prior(lm, prior_sigma, sigma2, prior_mean))
    notes = _run_to_convergence(lm, max_iters, check_every, rig_step._recover_and_note, rig_step._check_status, "solve_lm_rig")
    return result_of(lm, [what for did in notes for what in did])
