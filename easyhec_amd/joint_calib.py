"""Joint-offset calibration: fit the arm's joint zero errors together with the camera pose.

``link_poses`` is a constant of every other solve in this package: forward kinematics of the recorded ``qpos``, computed once.
That trusts the joint encoders completely; an arm that was re-homed or has been in a collision carries zero errors of a degree
or two, which no camera pose explains, and which the pose-only solve quietly absorbs into ``Tc_c2b``.

:class:`JointPoseStep` is :class:`easyhec_amd.fast.FusedPoseStep` with two more launches around the chain, which itself does
not change (csrc/ehr_joint.hip, include/ehr.h):

    ehr_joint_forward        qpos + offsets -> link_poses (float64 kinematics, rounded once), joint axes
    ehr_solver_step          the three-launch chain: reads link_poses, leaves grad_mvp and the pose it rendered
    ehr_joint_backward_adam  grad_mvp -> d loss / d offsets -> Adam on the free joints (a parameter group of its own)

Stepping, graph capture, the look at the loss every 16 steps and the recovery from a reported step are ``_ChainStep``'s: on a
reported step (NaN loss) the offsets and their Adam state stay untouched like the pose's, the next forward launch writes the
same ``link_poses`` again, and the chain recovers as it always does.  Not available for a data-parallel job (the offset
gradient would need an exchange of its own) nor for the Adam multi-start step (``MultiStartPoseStep``: its hypotheses share
one ``link_poses``; the multi-start Levenberg-Marquardt solve, :mod:`easyhec_amd.lm_multi`, gives every hypothesis its own).

Eye-in-hand: with ``robot.mounted(link)`` (:class:`easyhec_amd.robot.MountedRobot`) the camera rides on that link, the pose the
step fits is ``X = T_cam<-mount``, and the forward launch is ``ehr_joint_forward_mounted``: link poses and joint frames in the
mount's frame, the sign of the joints that move the mount folded into their axes, so that the chain and the finish launch
above run unchanged on the table's relative ``upstream`` mask.  :func:`default_free_joints` then leaves
out the joint that moves the mount link itself, a gauge with X."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .chain_step import check_solver_settings
from .fast import POSE_LR, POSE_WEIGHT_DECAY, FusedPoseStep, _f, refuse_unsupported
from .param_group import AdamGroup

__all__ = ["JointPoseStep", "JointOffsetResult", "solve_joint_offsets", "joint_kinds", "default_free_joints"]


def joint_kinds(table):
    """[J] int32: the kind (1 revolute, 2 prismatic) of every active joint of a ``joint_table``."""
    qidx = np.asarray(table["qidx"])
    out = np.zeros(int(qidx.max()) + 1 if qidx.size else 0, dtype=np.int32)
    out[qidx[qidx >= 0]] = np.asarray(table["kind"])[qidx >= 0]
    return out


def default_free_joints(table):
    """Arm joints 1..6: every revolute joint but the first, and no gripper joint.  A zero error of joint 0 turns everything
    downstream about the base axis; only the base link's own silhouette tells that apart from a camera rotation.

    For a mounted table (a camera on a link of the arm, ``UrdfChain.joint_table(mount=...)``): the revolute arm joints between
    the root and the mount, joint 0 included (the base moves in the camera's frame), but NOT the joint that moves the mount
    link itself (:func:`mount_gauge_joint`), and no joint below the mount.  A zero error of the mount's own joint only turns
    the camera against everything that does not ride with the mount, which ``X = T_cam<-mount`` already does: over those links
    it is an exact gauge with X.  Freeing it explicitly stays possible.  With a prior on it (``solve_lm``'s
    prior_sigma) the prior decides the split.  Without one, that joint and X share a direction the views pin weakly or not at
    all: Levenberg-Marquardt's damping keeps the step finite and leaves the split where the start put it, Adam divides it by
    the two learning rates, the loss is unaffected, and ``information_of`` names the joint and X's rotation in its weakest
    direction.  Joint 0 is in the list, and is the weak one of it: in the mount's frame its zero error moves the base link
    alone, about its own axis, so only the base's asymmetries pin it, and only in the views that show the base: where few
    do, hold it with a prior, or pass ``free=`` without it."""
    arm = np.flatnonzero(joint_kinds(table) == 1).tolist()[:7]
    if "mount" not in table:
        return arm[1:]
    gauge = mount_gauge_joint(table)
    return [j for j in arm if (int(table["mount_upstream"]) >> j) & 1 and j != gauge]


def mount_gauge_joint(table):
    """The active joint nearest the mount on its way to the root: the one that moves the mount link itself.  None for a mount
    that no active joint moves."""
    i = int(table["mount"])
    while i >= 0:
        if table["qidx"][i] >= 0:
            return int(table["qidx"][i])
        i = int(table["parent"][i])
    return None


def _check_table(t, J):
    """The kernels trust the table (it is device memory to them): refuse a malformed one here."""
    N = int(t["parent"].shape[0])
    if not 1 <= N <= 64 or not 1 <= J <= 32:
        raise ValueError(f"joint offsets: {N} links / {J} active joints; the kernels take up to 64 links and 32 joints")
    par, qidx, use = np.asarray(t["parent"]), np.asarray(t["qidx"]), np.asarray(t["use"])
    if par[0] != -1 or (par[1:] < 0).any() or (par[1:] >= np.arange(1, N)).any():
        raise ValueError("joint offsets: a parent must precede its child, and link 0 is the root")
    if (qidx >= J).any() or (use < 0).any() or (use >= N).any():
        raise ValueError("joint offsets: table index out of range")
    moved = qidx[qidx >= 0]
    if np.unique(moved).size != moved.size:  # (mimic joints: the forward kernel keeps ONE link per active joint)
        raise ValueError("joint offsets: an active joint moves more than one link (mimic joints are not supported)")
    for k in ("origin", "kind", "axis", "qidx"):
        if np.asarray(t[k]).shape[0] != N:
            raise ValueError(f"joint offsets: table entry {k!r} has the wrong length")


def arm_table(robot, qpos, batch, who):
    """What every solve with free joints reads of the arm (``who``: its name in the messages): ``robot.joint_table()`` checked,
    the articulation's dof J, and the recorded joint vectors (``qpos``, default ``batch["qpos"]``) as [B,J] float64,
    zero-padded to J like the dataset does -> ``(table, J, qp)``."""
    if qpos is None:
        if "qpos" not in batch:
            raise ValueError(f"{who} needs the recorded joint vectors: pass qpos= or batch['qpos']")
        qpos = batch["qpos"]
    table = robot.joint_table()
    J = int(robot.chain.dof)
    _check_table(table, J)
    q = np.asarray(qpos.detach().cpu() if torch.is_tensor(qpos) else qpos, dtype=np.float64)
    q = np.atleast_2d(q)
    qp = np.zeros((q.shape[0], J))
    qp[:, :min(J, q.shape[1])] = q[:, :J]
    return table, J, qp


def with_recorded_link_poses(robot, qp, batch, who):
    """A copy of ``batch`` whose ``link_poses`` are the forward kinematics of the recorded ``qp``.  batch["link_poses"] is
    optional for a solve with free joints and never rendered from: the forward kernel writes the solve's own buffer from qpos +
    offsets.  One that is given must be the kinematics of the recorded qpos (what the dataset computes) -- a batch whose link
    poses and joint vectors belong to different frames is refused, not silently overruled."""
    batch = dict(batch)
    fk0 = robot.link_poses_batch(qp)
    if "link_poses" in batch:
        given = batch["link_poses"].detach().cpu().double().numpy()
        if given.shape != fk0.shape or np.abs(given - fk0).max() > 1e-5:
            raise ValueError(f"{who}: batch['link_poses'] is not the forward kinematics of qpos (to 1e-5): the "
                             "joint vectors and the link poses must describe the same views")
    else:
        batch["link_poses"] = torch.from_numpy(fk0).float()
    return batch


def free_joint_list(table, J, free):
    """The free joints of a solve, sorted: ``free`` (default :func:`default_free_joints`), every one an active joint."""
    free = default_free_joints(table) if free is None else [int(j) for j in free]
    if any(j < 0 or j >= J for j in free):
        raise ValueError(f"free joints {free}: active joints are 0..{J - 1}")
    return sorted(set(free))


def mount_args(table):
    """``(mount, mount_upstream)`` of a mounted table (``UrdfChain.joint_table(mount=...)``), or None for a camera in the base
    frame.  A mounted table needs the mounted entry points: a library without them is refused here, not worked around."""
    if "mount" not in table:
        return None
    if not _lib.has_mounted():
        raise RuntimeError("this libehr_hip.so has no mounted forward kernels (ehr_joint_forward_mounted): rebuild it")
    m = int(table["mount"])
    if not 0 <= m < int(table["parent"].shape[0]):
        raise ValueError(f"joint offsets: mount {m} is not a node of the table")
    return m, int(table["mount_upstream"])


def joint_forward(t, N, J, L, mount, qpos, offset, B, link_poses, joint_frames, stream):
    """One forward launch: ``ehr_joint_forward``, or ``ehr_joint_forward_mounted`` where ``mount`` (:func:`mount_args`) is
    given.  t: the six device arrays of the table."""
    tab = [_lib.ptr(x) for x in t]
    out = (_lib.ptr(qpos), _lib.ptr(offset), B, _lib.ptr(link_poses), _lib.ptr(joint_frames), stream)
    if mount is None:
        _lib.check(_lib.lib().ehr_joint_forward(*tab, N, J, L, *out), "ehr_joint_forward")
    else:
        _lib.check(_lib.lib().ehr_joint_forward_mounted(*tab, N, J, L, mount[0], mount[1], *out), "ehr_joint_forward_mounted")


class _JointForward:
    """The launch before the chain: qpos + offsets -> the step's ``link_poses`` and ``joint_frames``.  Holds what describes
    the arm on the device (the joint table, the recorded joint vectors, the free mask) and the offsets' group, which a rig's
    cameras share."""

    def __init__(self, table, J, qp, free_joints, offsets, dev):
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)
        self.N, self.J, self.offsets, self.free_joints = int(table["parent"].shape[0]), J, offsets, free_joints
        self.t = [up(table[k], dt) for k, dt in (("parent", np.int32), ("origin", np.float64), ("kind", np.int32),
                                                 ("axis", np.float64), ("qidx", np.int32), ("use", np.int32))]
        self.upstream = up(np.asarray(table["upstream"]).astype(np.uint32).view(np.int32), np.int32)
        self.jkind = up(joint_kinds(table), np.int32)
        mask = np.zeros(J, dtype=np.int32)
        mask[free_joints] = 1
        self.free = up(mask, np.int32)
        self.qpos = up(qp, np.float64)
        self.mount = mount_args(table)

    def launch(self, step, stream):
        joint_forward(self.t, self.N, self.J, step.L, self.mount, self.qpos, self.offsets.param, step.B, step.link_poses,
                      step.joint_frames, stream)


class _JointFinish:
    """The launch after the chain: grad_mvp -> d loss / d offsets -> Adam on the free joints; and the offsets' part of the
    state dict: parameter group 1 and the offsets themselves, which no model holds."""
    rewrites_K = False

    def __init__(self, forward):
        self.fw = forward

    def launch(self, step, stream):
        fw, g, (b1, b2) = self.fw, self.fw.offsets, step.betas
        _lib.check(_lib.lib().ehr_joint_backward_adam(
            _lib.ptr(step.grad_mvp), _lib.ptr(step.tc_jac), _lib.ptr(step.K), step.B, step.L, fw.J, step.H, step.W,
            _f(step.near), _f(step.far), _lib.ptr(step.link_poses), _lib.ptr(step.joint_frames), _lib.ptr(fw.upstream),
            _lib.ptr(fw.jkind), _lib.ptr(step.red), _lib.ptr(fw.free), _lib.ptr(g.param), _lib.ptr(g.exp_avg),
            _lib.ptr(g.exp_avg_sq), _lib.ptr(g.step_t), _f(g.lr), _f(b1), _f(b2), _f(step.eps), _f(g.wd), _lib.ptr(g.grad),
            stream), "ehr_joint_backward_adam")

    def add_state(self, step, sd):
        g = self.fw.offsets
        sd["state"][1] = g.state_entry()
        sd["param_groups"].append(g.param_group(sd["param_groups"][0], 1))
        sd["joint_offsets"] = {"offsets": g.param.cpu().clone(), "free": list(self.fw.free_joints)}

    def check_state(self, step, sd):
        check_free_joints(sd.get("joint_offsets"), self.fw.free_joints, "step")
        if len(sd.get("param_groups", [])) > 1:
            self.fw.offsets.check_saved(sd["param_groups"][1], "the offsets' group", "step")

    def load_state(self, step, sd):
        """A pose-only state dict (``FusedPoseStep``'s) leaves the offsets' group as it is."""
        self.fw.offsets.load_state(sd.get("state", {}).get(1), (sd.get("joint_offsets") or {}).get("offsets"))


def check_free_joints(jo, free_joints, owner):
    # the moments of a joint that was not free are zero and its offset was never fitted: a different mask would mix them
    if jo is not None and sorted(int(j) for j in jo["free"]) != free_joints:
        raise ValueError(f"load_state_dict: the state was saved with free joints {sorted(jo['free'])}, this {owner} has "
                         f"{free_joints}")


def offsets_group(robot, dev, init_offset, offset_lr, offset_weight_decay, kw):
    """The offsets' Adam group, a fresh one: ``offset_lr`` / ``offset_weight_decay`` default to the pose's, which are among
    ``FusedPoseStep``'s keywords ``kw`` or its defaults."""
    J = int(robot.chain.dof)
    return AdamGroup(J, dev, kw.get("lr", POSE_LR) if offset_lr is None else float(offset_lr),
                     kw.get("weight_decay", POSE_WEIGHT_DECAY) if offset_weight_decay is None else float(offset_weight_decay),
                     np.zeros(J, dtype=np.float32) if init_offset is None else np.asarray(init_offset, dtype=np.float32).reshape(J))


class JointPoseStep(FusedPoseStep):
    def __init__(self, model, batch, robot, qpos=None, *, free=None, offset_lr=None, offset_weight_decay=None,
                 init_offset=None, **kw):
        """robot: :class:`easyhec_amd.robot.Robot` (its ``joint_table()`` describes the chain); qpos [B, <= J]: the recorded
        joint vectors (default ``batch["qpos"]``; zero-padded to the articulation's dof like the dataset does).
        free: active-joint indices whose offsets are fitted (default :func:`default_free_joints`); offset_lr /
        offset_weight_decay: the offsets' Adam group (defaults: the pose's; the weight decay is the prior towards zero
        offsets); init_offset [J]: where the offsets start (default 0).  Everything else is ``FusedPoseStep``'s."""
        refuse_unsupported(
            kw, _lib.has_joint_offsets,
            "joint offsets are not available for the multi-start step: its hypotheses share one link_poses",
            "joint offsets are not available for a data-parallel job: the offset gradient is not exchanged",
            "this libehr_hip.so has no joint-offset kernels (ehr_joint_forward): rebuild it")
        g = offsets_group(robot, model.dof.device, init_offset, offset_lr, offset_weight_decay, kw)
        self._init_joint(model, batch, robot, qpos, free, g, True, kw)

    def _init_joint(self, model, batch, robot, qpos, free, offsets, finish, kw):
        """offsets: the offsets' group -- this step's own, or the one a rig's cameras share; finish: whether the
        step finishes with ``ehr_joint_backward_adam`` (a rig's camera does not: the rig's one finish launch follows)."""
        table, J, qp = arm_table(robot, qpos, batch, "JointPoseStep")
        batch = with_recorded_link_poses(robot, qp, batch, "JointPoseStep")
        FusedPoseStep.__init__(self, model, batch, **kw)
        dev = self.dev
        if qp.shape[0] != self.B or len(table["use"]) != self.L:
            raise ValueError(f"JointPoseStep: qpos {qp.shape} / {len(table['use'])} rendered links do not match the batch's "
                             f"{self.B} views of {self.L} links")
        self.robot, self.table, self.J = robot, table, J
        self.free_joints = free_joint_list(table, J, free)
        self.offsets_group = g = offsets
        self.offset_lr, self.offset_wd = g.lr, g.wd
        self.offsets, self.offset_grad = g.param, g.grad
        self.offset_exp_avg, self.offset_exp_avg_sq, self.offset_step_t = g.exp_avg, g.exp_avg_sq, g.step_t
        self.kinematics = fw = _JointForward(table, J, qp, self.free_joints, g, dev)
        self._before, self._after = (fw,), ((_JointFinish(fw),) if finish else ())
        # the buffer the forward kernel writes and the chain reads: this object's own, never the caller's tensor
        self.link_poses = torch.empty((self.B, self.L, 4, 4), device=dev)
        self.joint_frames = torch.empty((self.B, J, 6), device=dev)
        self.corrected_link_poses()  # (the first forward launch: ``link_poses`` hold the kinematics before any step)

    def corrected_link_poses(self):
        """[B,L,4,4] float32 (device, a copy): the link poses at the CURRENT offsets, for what comes after the solve (the
        space explorer, tools/validate.py)."""
        with torch.cuda.device(self.dev):
            self.kinematics.launch(self, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return self.link_poses.clone()


@dataclass
class JointOffsetResult:
    offsets: torch.Tensor       # [J] fitted joint zero offsets (rad / m, CPU); 0 where the joint was not free
    losses: torch.Tensor        # [num_steps] loss of every effective step, before its update (CPU)
    dof: torch.Tensor           # [6] final camera pose coordinates (CPU); also left in ``model.dof``
    recoveries: list = field(default_factory=list)  # what the chain recovered from, in order
    step: object = None         # the JointPoseStep (corrected_link_poses(), state_dict())


def solve_joint_offsets(cfg, model, batch, robot, num_steps, qpos=None, capture=True, **kw):
    """``num_steps`` EFFECTIVE steps of the joint solve with the optimiser settings of ``cfg.solver`` (Adam: lr, weight
    decay), from a captured graph, with the loop ``RBSolverTrainer.fit`` uses: a reported step is recovered from and taken
    again.  ``kw``: :class:`JointPoseStep`'s keywords."""
    js = JointPoseStep(model, batch, robot, qpos, **{**check_solver_settings(cfg), **kw})
    if capture:
        js.capture()
    losses = js.take_effective_steps(num_steps, "solve_joint_offsets")[:num_steps, 0]
    js.release_graph()
    return JointOffsetResult(js.offsets.cpu().clone(), losses, model.dof.detach().cpu().clone(), list(js.recoveries), js)
