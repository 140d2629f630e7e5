"""Camera-rig calibration: several fixed cameras watch one arm and share one set of joint offsets.

From one viewpoint some joint zero errors are gauges -- joint 0's is absorbed by a camera rotation, and four views of one camera
do not pin six offsets (:mod:`easyhec_amd.joint_calib`).  The offsets are a property of the arm: every camera
that watches it constrains the same numbers, and a second viewpoint is what breaks those gauges.

:class:`RigJointStep` drives C launch chains, one per camera, each on its own ``RBSolver`` (own ``dof``, ``history_ops`` and
rasterizer context) and its own batch (own ``K``, image size, views, masks, optional ``weight``, ``qpos``), and ONE finish launch
(csrc/ehr_joint.hip, include/ehr.h):

    per camera   ehr_joint_forward             qpos_c + the SHARED offsets -> that camera's link_poses and joint axes
                 ehr_solver_step(defer_adam)   the three-launch chain, which stops after ``red``
    once         ehr_rig_backward_adam         sum of the offset gradients over the cameras / all views; every camera's pose
                                               Adam and the offsets' Adam -- or, if ANY camera reports its step, nothing at all

The objective is the mean per-view loss over all views of all cameras.  A reported step (NaN loss) is rig-wide: no pose and no
offset moves, every chain re-uses its history row, and the protocol around it -- the non-blocking look at the loss, the
recovery of every camera's context, the loop that takes an exact number of effective steps -- lives here, once.  Out of scope:
graph capture (a context owns one graph, the rig has C contexts; eager launches are this package's default), a data-parallel
job and the multi-start step."""
import ctypes
from dataclasses import dataclass, field

import torch

from . import _lib, fused
from .chain_step import _ReportedStepProtocol, check_solver_settings
from .fast import _f, refuse_unsupported
from .joint_calib import JointPoseStep, check_free_joints, offsets_group

__all__ = ["RigJointStep", "RigResult", "solve_rig"]

MAX_CAMERAS = 16  # EHR_RIG_MAX_CAMERAS


class _RigCameraStep(JointPoseStep):
    """One camera of the rig: ``JointPoseStep``'s construction (the table and the qpos / link_poses checks, the forward
    launch) around the rig's ONE offsets' group, with the camera's element of the rig's ``loss``, a chain that stops after
    ``red`` and no finish launch of its own."""

    def __init__(self, model, batch, robot, qpos, free, offsets, loss, **kw):
        self._init_joint(model, batch, robot, qpos, free, offsets, False, dict(kw, loss=loss, defer_adam=True))


def _per_camera(v, C, name):
    if isinstance(v, (list, tuple)):
        if len(v) != C:
            raise ValueError(f"RigJointStep: {name}= has {len(v)} entries for {C} cameras")
        return list(v)
    return [v] * C


class RigJointStep(_ReportedStepProtocol):
    def __init__(self, models, batches, robot, qpos=None, *, free=None, offset_lr=None, offset_weight_decay=None,
                 init_offset=None, **kw):
        """models / batches: one :class:`easyhec_amd.rb_solver.RBSolver` and one batch per camera; robot: the one arm they
        watch.  qpos: a list with one [B_c, <= J] array per camera (default: every ``batch["qpos"]``).  free, offset_lr,
        offset_weight_decay, init_offset: :class:`JointPoseStep`'s, for the ONE offsets' group (``free`` may include joint 0:
        a second viewpoint tells its zero error from a camera rotation).  ``kw``: ``FusedPoseStep``'s keywords, shared by the
        cameras; ``slack``, ``near`` and ``far`` may be a list with one entry per camera."""
        models, batches = list(models), list(batches)
        C = len(models)
        refuse_unsupported(
            kw, _lib.has_rig,
            "a camera rig is not available for the multi-start step: its hypotheses share one link_poses, and the search "
            "over a rig is out of scope",
            "a camera rig is not available for a data-parallel job: the cameras' sums are joined on one device, and the "
            "offset gradient is not exchanged",
            "this libehr_hip.so has no rig kernel (ehr_rig_backward_adam): rebuild it")
        if getattr(robot, "mount_link", None) is not None:
            raise ValueError(f"RigJointStep: a camera rig with a camera mounted on the arm (link {robot.mount_link!r}) is not "
                             "available: the rig's finish launch takes one upstream mask for all cameras, and a mounted camera "
                             "needs its own.  Calibrate the mounted camera on its own (JointPoseStep, solve_lm), or pass the "
                             "robot's .base for a rig of fixed cameras")
        if not 1 <= C <= MAX_CAMERAS or len(batches) != C:
            raise ValueError(f"RigJointStep: {C} models / {len(batches)} batches; a rig has 1..{MAX_CAMERAS} cameras and one "
                             "batch per camera")
        if len({id(m) for m in models}) != C:
            raise ValueError("RigJointStep: the same model object was passed twice: every camera needs its own RBSolver (its "
                             "pose, history and rasterizer context)")
        if len({m.dof.device for m in models}) != 1:
            raise ValueError("RigJointStep: the cameras' models must live on one device")
        qpos = _per_camera(None, C, "qpos") if qpos is None else list(qpos)
        if len(qpos) != C:
            raise ValueError(f"RigJointStep: qpos= has {len(qpos)} entries for {C} cameras")
        per = {k: _per_camera(kw.pop(k), C, k) for k in ("slack", "near", "far") if k in kw}
        self.C, self.dev, self.robot = C, models[0].dof.device, robot
        # the ONE offsets' group, which every camera's forward launch reads and the rig's finish launch updates, and the
        # ``loss [C]`` the finish launch writes camera by camera: both handed to the cameras' constructors
        self.offsets_group = g = offsets_group(robot, self.dev, init_offset, offset_lr, offset_weight_decay, kw)
        self.offsets, self.offset_grad, self.offset_lr, self.offset_wd = g.param, g.grad, g.lr, g.wd
        self.offset_exp_avg, self.offset_exp_avg_sq, self.offset_step_t = g.exp_avg, g.exp_avg_sq, g.step_t
        self.loss = torch.zeros((C,), device=self.dev)
        self.cameras = [_RigCameraStep(models[c], batches[c], robot, qpos[c], free, g, self.loss[c:c + 1],
                                       **dict(kw, **{k: v[c] for k, v in per.items()})) for c in range(C)]
        for cam, batch in zip(self.cameras, batches):
            cam.batch_K = batch["K"]  # as given, every view's: read only (solve_lm_rig judges it where intrinsics are freed)
        first = self.cameras[0]
        if any(cam.L != first.L for cam in self.cameras):
            raise ValueError(f"RigJointStep: the cameras render {[cam.L for cam in self.cameras]} links: one robot, one link count")
        self.L, self.J, self.free_joints, self.kinematics = first.L, first.J, list(first.free_joints), first.kinematics
        self.lr, self.wd, self.betas, self.eps = first.lr, first.wd, first.betas, first.eps
        self._cams_dev, self._cams_key = None, None
        # the protocol around a reported step is _ChainStep's own (chain_step._ReportedStepProtocol): a non-blocking look at
        # ``loss [C]`` every `check_every` steps; ``recoveries`` holds "camera c: what its context recovered from", in order
        self._init_protocol()

    # -- launches ---------------------------------------------------------------------------------------------------
    def _camera_array(self):
        """The device array of ``ehr_rig_camera``; built once, and again whenever any pointer in it has changed (a model's
        ``dof`` storage replaced, a buffer reallocated)."""
        p = lambda t: t.data_ptr()
        rows = [(p(cam.grad_mvp), p(cam.tc_jac), p(cam.K), p(cam.link_poses), p(cam.joint_frames), p(cam.red),
                 p(cam.model.dof.data), p(cam.exp_avg), p(cam.exp_avg_sq), p(cam.step_t), p(cam.loss), p(cam.grad), cam.B, cam.H,
                 cam.W, float(cam.near), float(cam.far)) for cam in self.cameras]
        if rows != self._cams_key:
            arr = (_lib.RigCamera * self.C)(*[_lib.RigCamera(*r) for r in rows])
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self._cams_dev, self._cams_key = host.to(self.dev), rows
        return self._cams_dev

    def step(self):
        """Enqueue one optimisation step of the whole rig on the current stream.  Returns the (device) tensor ``loss [C]``:
        every camera's mean mask loss BEFORE the update; all NaN for a reported step.  Never synchronises."""
        with torch.cuda.device(self.dev):
            cams = self._camera_array()
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            for cam in self.cameras:
                cam._host_copies_stale()
                if getattr(cam.glctx, "_bound_weight", None) is not cam.weight:
                    cam._plan_and_bind()  # somebody else used the context with other weights since: bind this camera's again
                cam._enqueue(False, stream=stream)
            (b1, b2), fw, g = self.betas, self.kinematics, self.offsets_group
            _lib.check(_lib.lib().ehr_rig_backward_adam(
                _lib.ptr(cams), self.C, self.L, self.J, _lib.ptr(fw.upstream), _lib.ptr(fw.jkind), _lib.ptr(fw.free),
                _lib.ptr(g.param), _lib.ptr(g.exp_avg), _lib.ptr(g.exp_avg_sq), _lib.ptr(g.step_t), _f(self.lr), _f(g.lr),
                _f(b1), _f(b2), _f(self.eps), _f(self.wd), _f(g.wd), _lib.ptr(g.grad), stream), "ehr_rig_backward_adam")
            self._calls += 1
            if self._calls % self.check_every == 0:
                self._poll()
        return self.loss

    def capture(self):
        raise RuntimeError("capture(): graph capture of the rig step is out of scope -- a rasterizer context owns one graph and "
                           f"the rig has {self.C} contexts; step() enqueues the launches eagerly")

    # -- reported steps ---------------------------------------------------------------------------------------------
    def _recover_and_note(self):
        """Ask every camera's context what its last steps met (``recover_from_overflow``: synchronises) and note it."""
        did = []
        for c, cam in enumerate(self.cameras):
            what = cam.recover_from_overflow()
            if what:
                did.append(f"camera {c}: {what}")
        self.recoveries.extend(did)
        return did

    @property
    def steps_done(self):
        """The offsets' counter: it advances on real steps of the rig only.  Reading it synchronises."""
        return int(self.offset_step_t.item())

    def _check_status(self):
        for cam in self.cameras:
            fused.check_status(cam.glctx)

    # -- results ----------------------------------------------------------------------------------------------------
    def corrected_link_poses(self):
        """A list with one [B_c,L,4,4] float32 tensor per camera (device, copies): the link poses at the CURRENT offsets."""
        return [cam.corrected_link_poses() for cam in self.cameras]

    def state_dict(self):
        """torch.optim.Adam-shaped: parameter groups 0..C-1 are the cameras' poses, group C the offsets; plus the offsets
        themselves, which no model holds."""
        every = [cam.pose_group for cam in self.cameras] + [self.offsets_group]
        group0 = self.cameras[0]._group0()
        return {"state": {i: g.state_entry() for i, g in enumerate(every)},
                "param_groups": [g.param_group(group0, i) for i, g in enumerate(every)],
                "joint_offsets": {"offsets": self.offsets.cpu().clone(), "free": list(self.free_joints), "cameras": self.C}}

    def load_state_dict(self, sd):
        """Inverse of :meth:`state_dict`.  Refuses a state saved with another camera count, another free set or other group
        settings: the moments of one problem mean nothing in another."""
        jo, groups = sd.get("joint_offsets"), sd.get("param_groups", [])
        if jo is None or int(jo.get("cameras", -1)) != self.C or len(groups) != self.C + 1:
            raise ValueError(f"load_state_dict: the state is not a rig's of {self.C} cameras (it has {len(groups)} parameter groups)")
        check_free_joints(jo, self.free_joints, "rig")
        every = [cam.pose_group for cam in self.cameras] + [self.offsets_group]
        for i, g in enumerate(every):
            g.check_saved(groups[i], f"group {i}", "rig")
        for i, g in enumerate(every):
            g.load_state(sd["state"][i], jo["offsets"] if g is self.offsets_group else None)


@dataclass
class RigResult:
    offsets: torch.Tensor       # [J] fitted joint zero offsets (rad / m, CPU); 0 where the joint was not free
    losses: torch.Tensor        # [num_steps, C] every camera's loss of every effective step, before its update (CPU)
    dofs: torch.Tensor          # [C, 6] final camera pose coordinates (CPU); also left in every ``model.dof``
    recoveries: list = field(default_factory=list)  # what the cameras' chains recovered from, in order
    step: object = None         # the RigJointStep (corrected_link_poses(), state_dict())


def solve_rig(cfg, models, batches, robot, num_steps, qpos=None, **kw):
    """``num_steps`` EFFECTIVE steps of the rig solve with the optimiser settings of ``cfg.solver`` (Adam: lr, weight
    decay): a reported step is recovered from and taken again.  ``kw``: :class:`RigJointStep`'s keywords."""
    rig = RigJointStep(models, batches, robot, qpos, **{**check_solver_settings(cfg), **kw})
    losses = rig.take_effective_steps(num_steps, "solve_rig")[:num_steps]
    dofs = torch.stack([cam.model.dof.detach().cpu().clone() for cam in rig.cameras])
    return RigResult(rig.offsets.cpu().clone(), losses, dofs, list(rig.recoveries), rig)
