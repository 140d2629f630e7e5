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
gradient would need an exchange of its own) nor for the multi-start step (its hypotheses share one ``link_poses``)."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .fast import FusedPoseStep, _f

__all__ = ["JointPoseStep", "JointOffsetResult", "solve_joint_offsets", "joint_kinds", "default_free_joints"]


def joint_kinds(table):
    """[J] int32: the kind (1 revolute, 2 prismatic) of every active joint of a ``joint_table``."""
    qidx = np.asarray(table["qidx"])
    out = np.zeros(int(qidx.max()) + 1 if qidx.size else 0, dtype=np.int32)
    out[qidx[qidx >= 0]] = np.asarray(table["kind"])[qidx >= 0]
    return out


def default_free_joints(table):
    """Arm joints 1..6: every revolute joint but the first, and no gripper joint.  A zero error of joint 0 turns everything
    downstream about the base axis; only the base link's own silhouette tells that apart from a camera rotation."""
    return [j for j in np.flatnonzero(joint_kinds(table) == 1).tolist()[1:7]]


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


class JointPoseStep(FusedPoseStep):
    def __init__(self, model, batch, robot, qpos=None, *, free=None, offset_lr=None, offset_weight_decay=None,
                 init_offset=None, **kw):
        """robot: :class:`easyhec_amd.robot.Robot` (its ``joint_table()`` describes the chain); qpos [B, <= J]: the recorded
        joint vectors (default ``batch["qpos"]``; zero-padded to the articulation's dof like the dataset does).
        free: active-joint indices whose offsets are fitted (default :func:`default_free_joints`); offset_lr /
        offset_weight_decay: the offsets' Adam group (defaults: the pose's; the weight decay is the prior towards zero
        offsets); init_offset [J]: where the offsets start (default 0).  Everything else is ``FusedPoseStep``'s."""
        if "starts" in kw:
            # (nothing combines the two: MultiStartPoseStep has no hook for these kernels.  A call ported from
            #  MultiStartPoseStep(model, batch, starts) gets the reason instead of a TypeError about a keyword.)
            raise ValueError("joint offsets are not available for the multi-start step: its hypotheses share one link_poses")
        pg = kw.get("process_group")
        if kw.get("rccl") or kw.get("p2p") or (dist.is_available() and dist.is_initialized() and dist.get_world_size(pg) > 1):
            raise ValueError("joint offsets are not available for a data-parallel job: the offset gradient is not exchanged")
        if not _lib.has_joint_offsets():
            raise RuntimeError("this libehr_hip.so has no joint-offset kernels (ehr_joint_forward): rebuild it")
        if qpos is None:
            if "qpos" not in batch:
                raise ValueError("JointPoseStep needs the recorded joint vectors: pass qpos= or batch['qpos']")
            qpos = batch["qpos"]
        table = robot.joint_table()
        J = int(robot.chain.dof)
        _check_table(table, J)
        q = np.asarray(qpos.detach().cpu() if torch.is_tensor(qpos) else qpos, dtype=np.float64)
        q = np.atleast_2d(q)
        qp = np.zeros((q.shape[0], J))
        qp[:, :min(J, q.shape[1])] = q[:, :J]
        off0 = np.zeros(J, dtype=np.float32) if init_offset is None else np.asarray(init_offset, dtype=np.float32).reshape(J)
        batch = dict(batch)
        # batch["link_poses"] is optional here and never rendered from: the forward kernel writes this object's own buffer
        # from qpos + offsets.  One that is given must be the kinematics of the recorded qpos (what the dataset computes) --
        # a batch whose link poses and joint vectors belong to different frames is refused, not silently overruled.
        fk0 = robot.link_poses_batch(qp)
        if "link_poses" in batch:
            given = batch["link_poses"].detach().cpu().double().numpy()
            if given.shape != fk0.shape or np.abs(given - fk0).max() > 1e-5:
                raise ValueError("JointPoseStep: batch['link_poses'] is not the forward kinematics of qpos (to 1e-5): the "
                                 "joint vectors and the link poses must describe the same views")
        else:
            batch["link_poses"] = torch.from_numpy(fk0).float()
        super().__init__(model, batch, **kw)
        dev = self.dev
        if qp.shape[0] != self.B or len(table["use"]) != self.L:
            raise ValueError(f"JointPoseStep: qpos {qp.shape} / {len(table['use'])} rendered links do not match the batch's "
                             f"{self.B} views of {self.L} links")
        self.robot, self.table, self.J, self.N = robot, table, J, int(table["parent"].shape[0])
        free = default_free_joints(table) if free is None else [int(j) for j in free]
        if any(j < 0 or j >= J for j in free):
            raise ValueError(f"free joints {free}: active joints are 0..{J - 1}")
        self.free_joints = sorted(set(free))
        mask = np.zeros(J, dtype=np.int32)
        mask[self.free_joints] = 1
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=dt)).to(dev)
        self._t = {k: up(table[k], dt) for k, dt in (("parent", np.int32), ("origin", np.float64), ("kind", np.int32),
                                                    ("axis", np.float64), ("qidx", np.int32), ("use", np.int32))}
        self._upstream = up(np.asarray(table["upstream"]).astype(np.uint32).view(np.int32), np.int32)
        self._jkind = up(joint_kinds(table), np.int32)
        self._free = up(mask, np.int32)
        self.qpos = up(qp, np.float64)
        self.offset_lr = self.lr if offset_lr is None else float(offset_lr)
        self.offset_wd = self.wd if offset_weight_decay is None else float(offset_weight_decay)
        # the second Adam parameter group: a fresh one unless load_state_dict restores it
        self.offsets = up(off0, np.float32)
        self.offset_exp_avg = torch.zeros(J, device=dev)
        self.offset_exp_avg_sq = torch.zeros(J, device=dev)
        self.offset_step_t = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.offset_grad = torch.zeros(J, device=dev)
        # the buffer the forward kernel writes and the chain reads: this object's own, never the caller's tensor
        self.link_poses = torch.empty((self.B, self.L, 4, 4), device=dev)
        self.joint_frames = torch.empty((self.B, J, 6), device=dev)
        with torch.cuda.device(dev):
            self._launch_forward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    # -- launches ---------------------------------------------------------------------------------------------------
    def _launch_forward(self, stream):
        t = self._t
        _lib.check(_lib.lib().ehr_joint_forward(
            _lib.ptr(t["parent"]), _lib.ptr(t["origin"]), _lib.ptr(t["kind"]), _lib.ptr(t["axis"]), _lib.ptr(t["qidx"]),
            _lib.ptr(t["use"]), self.N, self.J, self.L, _lib.ptr(self.qpos), _lib.ptr(self.offsets), self.B,
            _lib.ptr(self.link_poses), _lib.ptr(self.joint_frames), stream), "ehr_joint_forward")

    def _enqueue(self, want_mask, stream=None):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._launch_forward(stream)
        super()._enqueue(want_mask, stream=stream)
        b1, b2 = self.betas
        _lib.check(_lib.lib().ehr_joint_backward_adam(
            _lib.ptr(self.grad_mvp), _lib.ptr(self.tc_jac), _lib.ptr(self.K), self.B, self.L, self.J, self.H, self.W,
            _f(self.near), _f(self.far), _lib.ptr(self.link_poses), _lib.ptr(self.joint_frames), _lib.ptr(self._upstream),
            _lib.ptr(self._jkind), _lib.ptr(self.red), _lib.ptr(self._free), _lib.ptr(self.offsets),
            _lib.ptr(self.offset_exp_avg), _lib.ptr(self.offset_exp_avg_sq), _lib.ptr(self.offset_step_t),
            _f(self.offset_lr), _f(b1), _f(b2), _f(self.eps), _f(self.offset_wd), _lib.ptr(self.offset_grad), stream),
            "ehr_joint_backward_adam")

    # -- results ----------------------------------------------------------------------------------------------------
    def corrected_link_poses(self):
        """[B,L,4,4] float32 (device, a copy): the link poses at the CURRENT offsets, for what comes after the solve (the
        space explorer, tools/validate.py)."""
        with torch.cuda.device(self.dev):
            self._launch_forward(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return self.link_poses.clone()

    def state_dict(self):
        """``FusedPoseStep.state_dict`` with a second parameter group (index 1: the offsets' Adam state) and the offsets
        themselves, which no model holds."""
        sd = super().state_dict()
        sd["state"][1] = {"step": self.offset_step_t.float().cpu().reshape(()), "exp_avg": self.offset_exp_avg.cpu().clone(),
                          "exp_avg_sq": self.offset_exp_avg_sq.cpu().clone()}
        g = dict(sd["param_groups"][0])
        g.update(lr=self.offset_lr, weight_decay=self.offset_wd, params=[1])
        sd["param_groups"].append(g)
        sd["joint_offsets"] = {"offsets": self.offsets.cpu().clone(), "free": list(self.free_joints)}
        return sd

    def load_state_dict(self, sd):
        """Inverse of :meth:`state_dict`; a pose-only state dict (``FusedPoseStep``'s) restores the pose's group and leaves
        the offsets' as it is."""
        jo = sd.get("joint_offsets")
        if jo is not None and sorted(int(j) for j in jo["free"]) != self.free_joints:
            # the moments of a joint that was not free are zero and its offset was never fitted: a different mask would mix them
            raise ValueError(f"load_state_dict: the state was saved with free joints {sorted(jo['free'])}, this step has "
                             f"{self.free_joints}")
        groups = sd.get("param_groups", [])
        if len(groups) > 1:
            g = groups[1]
            if float(g.get("lr", self.offset_lr)) != self.offset_lr or float(g.get("weight_decay", self.offset_wd)) != self.offset_wd:
                raise ValueError(f"load_state_dict: the offsets' group was saved with lr {g.get('lr')} / weight decay "
                                 f"{g.get('weight_decay')}, this step has {self.offset_lr} / {self.offset_wd}")
        super().load_state_dict(sd)
        st = sd.get("state", {}).get(1)
        if st is not None:
            self.offset_exp_avg.copy_(torch.as_tensor(st["exp_avg"], dtype=torch.float32).reshape(self.J))
            self.offset_exp_avg_sq.copy_(torch.as_tensor(st["exp_avg_sq"], dtype=torch.float32).reshape(self.J))
            self.offset_step_t.fill_(int(round(float(torch.as_tensor(st["step"]).reshape(-1)[0]))))
        if jo is not None:
            self.offsets.copy_(torch.as_tensor(jo["offsets"], dtype=torch.float32).reshape(self.J))


@dataclass
class JointOffsetResult:
    offsets: torch.Tensor       # [J] fitted joint zero offsets (rad / m, CPU); 0 where the joint was not free
    losses: torch.Tensor        # [num_steps] loss of every effective step, before its update (CPU)
    dof: torch.Tensor           # [6] final camera pose coordinates (CPU); also left in ``model.dof``
    recoveries: list = field(default_factory=list)  # what the chain recovered from, in order
    step: object = None         # the JointPoseStep (corrected_link_poses(), state_dict())


def _check_solver_settings(cfg, kw):
    """The solver-settings check of the one-call solves (this one and ``rig_calib.solve_rig``); fills in ``cfg.solver``'s lr
    and weight decay where ``kw`` has none."""
    if cfg.solver.do_grad_clip or cfg.solver.optimizer != "Adam":
        raise ValueError("the launch chain implements the reference's default solver only (Adam, no gradient clipping)")
    kw.setdefault("lr", cfg.solver.max_lr)
    kw.setdefault("weight_decay", cfg.solver.weight_decay)


def solve_joint_offsets(cfg, model, batch, robot, num_steps, qpos=None, capture=True, **kw):
    """``num_steps`` EFFECTIVE steps of the joint solve with the optimiser settings of ``cfg.solver`` (Adam: lr, weight
    decay), from a captured graph, with the loop ``RBSolverTrainer.fit`` uses: a reported step is recovered from and taken
    again.  ``kw``: :class:`JointPoseStep`'s keywords."""
    _check_solver_settings(cfg, kw)
    js = JointPoseStep(model, batch, robot, qpos, **kw)
    if capture:
        js.capture()
    kept = []
    for remaining, _ in js.effective_rounds(num_steps, "solve_joint_offsets"):
        for _ in range(remaining):  # (a reported step's loss is NaN and is dropped below: num_steps finite ones remain)
            kept.append(js.step().clone())
    torch.cuda.synchronize(js.dev)
    losses = torch.cat(kept).cpu() if kept else torch.zeros(0)
    losses = losses[~torch.isnan(losses)][:num_steps]
    js.release_graph()
    return JointOffsetResult(js.offsets.cpu().clone(), losses, model.dof.detach().cpu().clone(), list(js.recoveries), js)
