"""Intrinsics refinement: fit the focal lengths and the principal point together with the camera pose.

``K`` is a constant of every other solve in this package: a factory or checkerboard value, typically off by a per cent or so
in focal length and a few pixels in principal point.  At 1 m a 1 % focal error is a 1 cm depth error, which the pose-only
solve quietly absorbs into ``Tc_c2b``.

:class:`IntrinsicsPoseStep` is :class:`easyhec_amd.fast.FusedPoseStep` with one more launch after the chain, which itself does
not change (csrc/ehr_intrinsics.hip, include/ehr.h):

    ehr_solver_step               the three-launch chain: reads K from device memory, leaves grad_mvp and the pose it rendered
    ehr_intrinsics_backward_adam  grad_mvp -> d loss / d theta -> Adam on the free elements (a parameter group of its own)
                                  -> the K the next step's chain reads

The parameters are four dimensionless numbers ``theta``:

    fu = K0[0,0] exp(theta0)    fv = K0[1,1] exp(theta1)    cu = K0[0,2] + W theta2    cv = K0[1,2] + H theta3

of the order of 1e-2, which is why the pose's learning rate is a sane default for them; the weight decay on ``theta`` is the
prior towards the intrinsics as given.  The default free set is the TIED focal length only (``free=("f",)``): a
principal-point shift is nearly a small camera rotation at these fields of view -- a gauge the masks barely fix, like joint
0's zero error in the joint-offset solve -- so ``"cx"`` / ``"cy"`` are for the caller who knows the views pin it.

Stepping, graph capture, the look at the loss every 16 steps and the recovery from a reported step are ``_ChainStep``'s: on a
reported step (NaN loss) ``theta``, its Adam state and ``K`` stay untouched like the pose's, the chain renders the same ``K``
again and recovers as it always does.  :class:`JointIntrinsicsPoseStep` composes this with the joint-offset solve.

Out of scope: the camera rig (per-camera intrinsics inside ``ehr_rig_backward_adam``'s all-or-nothing step), data-parallel
and multi-start solves, lens distortion, skew, per-view intrinsics, and the autograd (``use_fused=True``) path."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, joint_calib
from .fast import FusedPoseStep, _f
from .joint_calib import JointPoseStep

__all__ = ["IntrinsicsPoseStep", "JointIntrinsicsPoseStep", "IntrinsicsResult", "solve_intrinsics", "intrinsics_from_theta"]

_NAMES = {"fx": 0, "fy": 1, "cx": 2, "cy": 3}


def intrinsics_from_theta(K0, theta, H, W):
    """[3,3] float32: the ``K`` the kernel writes for ``theta`` -- the four entries evaluated in float64 and rounded once, the
    others ``K0``'s, and an entry whose ``theta`` is exactly 0 with ``K0``'s bits."""
    K0 = np.asarray(K0, dtype=np.float32).reshape(3, 3)
    th = np.asarray(theta, dtype=np.float32).reshape(4).astype(np.float64)
    K = K0.copy()
    k64 = K0.astype(np.float64)
    new = (k64[0, 0] * np.exp(th[0]), k64[1, 1] * np.exp(th[1]), k64[0, 2] + float(W) * th[2], k64[1, 2] + float(H) * th[3])
    for i, (r, c) in enumerate(((0, 0), (1, 1), (0, 2), (1, 2))):
        if th[i] != 0.0:
            K[r, c] = np.float32(new[i])
    return K


def _parse_free(free):
    """(mask [4] of 0/1, tie_focal, canonical names) from names out of "f" (both focal lengths, tied), "fx", "fy", "cx", "cy"."""
    names = [free] if isinstance(free, str) else list(free)
    bad = [n for n in names if n != "f" and n not in _NAMES]
    if bad:
        raise ValueError(f"free intrinsics {bad}: the names are 'f' (both focal lengths, tied), 'fx', 'fy', 'cx', 'cy'")
    if "f" in names and ("fx" in names or "fy" in names):
        raise ValueError("free intrinsics: 'f' ties both focal lengths to one scale and cannot be combined with 'fx' or 'fy'")
    mask = [0, 0, 0, 0]
    if "f" in names:
        mask[0] = mask[1] = 1
    for n in names:
        if n != "f":
            mask[_NAMES[n]] = 1
    order = ["f", "fx", "fy", "cx", "cy"]
    return mask, int("f" in names), sorted(set(names), key=order.index)


class _IntrinsicsGroup:
    """What :class:`IntrinsicsPoseStep` and :class:`JointIntrinsicsPoseStep` share: the refusals, the buffers of the
    parameter group, the launch and the group's part of the state dict.  ``_intr_group`` is the group's index in the state
    dict."""
    _intr_group = 1

    @staticmethod
    def _intr_refuse(batch, kw):
        """The cases the chain cannot express, each with its reason; call before the base constructor."""
        if "starts" in kw:
            raise ValueError("intrinsics refinement is not available for the multi-start step: its hypotheses share one K")
        pg = kw.get("process_group")
        if kw.get("rccl") or kw.get("p2p") or (dist.is_available() and dist.is_initialized() and dist.get_world_size(pg) > 1):
            raise ValueError("intrinsics refinement is not available for a data-parallel job: the intrinsics gradient is not "
                             "exchanged")
        if not _lib.has_intrinsics():
            raise RuntimeError("this libehr_hip.so has no intrinsics kernel (ehr_intrinsics_backward_adam): rebuild it")
        Kb = batch["K"]
        if Kb.dim() != 3 or tuple(Kb.shape[1:]) != (3, 3):
            raise ValueError(f"intrinsics refinement: batch['K'] must be [B,3,3], got {tuple(Kb.shape)}")
        if not bool((Kb == Kb[:1]).all()):
            # FusedPoseStep renders every view with batch["K"][0]
            raise ValueError("intrinsics refinement: batch['K'] differs between views; the chain has one K (per-view "
                             "intrinsics are out of scope)")

    def _intr_init(self, free, intrinsics_lr, intrinsics_weight_decay, init_theta):
        dev = self.dev
        mask, self.tie_focal, self.free_intrinsics = _parse_free(free)
        th0 = np.zeros(4, dtype=np.float32) if init_theta is None else np.asarray(init_theta, dtype=np.float32).reshape(4)
        if self.tie_focal and th0[0] != th0[1]:
            raise ValueError("init_theta: the tied focal lengths ('f') must start from equal theta[0] and theta[1]")
        self.intrinsics_lr = self.lr if intrinsics_lr is None else float(intrinsics_lr)
        self.intrinsics_wd = self.wd if intrinsics_weight_decay is None else float(intrinsics_weight_decay)
        # the intrinsics as given, and the buffer the kernel writes and the chain reads: this object's own, never the caller's
        self.K0 = self.K.detach().clone().contiguous()
        self.K = torch.from_numpy(intrinsics_from_theta(self.K0.cpu().numpy(), th0, self.H, self.W)).to(dev).contiguous()
        self._intr_free = torch.tensor(mask, dtype=torch.int32, device=dev)
        # the group's Adam state: a fresh one unless load_state_dict restores it
        self.theta = torch.from_numpy(th0.copy()).to(dev)
        self.theta_exp_avg = torch.zeros(4, device=dev)
        self.theta_exp_avg_sq = torch.zeros(4, device=dev)
        self.theta_step_t = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.theta_grad = torch.zeros(4, device=dev)

    def _intr_launch(self, stream):
        b1, b2 = self.betas
        _lib.check(_lib.lib().ehr_intrinsics_backward_adam(
            _lib.ptr(self.grad_mvp), _lib.ptr(self.tc_jac), _lib.ptr(self.link_poses), self.B, self.L, self.H, self.W,
            _lib.ptr(self.red), _lib.ptr(self.K0), _lib.ptr(self._intr_free), self.tie_focal, _lib.ptr(self.theta),
            _lib.ptr(self.theta_exp_avg), _lib.ptr(self.theta_exp_avg_sq), _lib.ptr(self.theta_step_t),
            _f(self.intrinsics_lr), _f(b1), _f(b2), _f(self.eps), _f(self.intrinsics_wd), _lib.ptr(self.K),
            _lib.ptr(self.theta_grad), stream), "ehr_intrinsics_backward_adam")

    def intrinsics(self):
        """[3,3] float32 (CPU, a copy): the current ``K``, i.e. the one the next step renders with."""
        return self.K.detach().cpu().clone()

    def _intr_state(self, sd):
        """Adds the group (index ``_intr_group``), ``theta``, ``K0`` and the free set to a state dict."""
        i = self._intr_group
        sd["state"][i] = {"step": self.theta_step_t.float().cpu().reshape(()), "exp_avg": self.theta_exp_avg.cpu().clone(),
                          "exp_avg_sq": self.theta_exp_avg_sq.cpu().clone()}
        g = dict(sd["param_groups"][0])
        g.update(lr=self.intrinsics_lr, weight_decay=self.intrinsics_wd, params=[i])
        sd["param_groups"].append(g)
        sd["intrinsics"] = {"theta": self.theta.cpu().clone(), "K0": self.K0.cpu().clone(),
                            "free": list(self.free_intrinsics), "group": i}
        return sd

    def _intr_check_state(self, sd):
        """Raises where the saved group is not this step's (another free set or tying, other group settings); before
        anything is loaded."""
        it = sd.get("intrinsics")
        if it is None:
            return
        if _parse_free(it["free"])[2] != self.free_intrinsics:
            # the moments of an element that was not free are zero and its theta was never fitted: another set would mix them
            raise ValueError(f"load_state_dict: the state was saved with free intrinsics {list(it['free'])}, this step has "
                             f"{self.free_intrinsics}")
        groups = sd.get("param_groups", [])
        i = int(it.get("group", self._intr_group))
        if i != self._intr_group:
            raise ValueError(f"load_state_dict: the intrinsics' group was saved as group {i}, this step's is {self._intr_group}")
        if len(groups) > i:
            g = groups[i]
            if float(g.get("lr", self.intrinsics_lr)) != self.intrinsics_lr or \
                    float(g.get("weight_decay", self.intrinsics_wd)) != self.intrinsics_wd:
                raise ValueError(f"load_state_dict: the intrinsics' group was saved with lr {g.get('lr')} / weight decay "
                                 f"{g.get('weight_decay')}, this step has {self.intrinsics_lr} / {self.intrinsics_wd}")
        if not torch.equal(torch.as_tensor(it["K0"], dtype=torch.float32).reshape(3, 3), self.K0.cpu()):
            raise ValueError("load_state_dict: the state was saved for other given intrinsics K0 than this step's")

    def _intr_load(self, sd):
        """Restores the group from a state dict that holds one (a pose-only state dict leaves it alone)."""
        it = sd.get("intrinsics")
        if it is None:
            return
        st = sd.get("state", {}).get(self._intr_group)
        if st is not None:
            self.theta_exp_avg.copy_(torch.as_tensor(st["exp_avg"], dtype=torch.float32).reshape(4))
            self.theta_exp_avg_sq.copy_(torch.as_tensor(st["exp_avg_sq"], dtype=torch.float32).reshape(4))
            self.theta_step_t.fill_(int(round(float(torch.as_tensor(st["step"]).reshape(-1)[0]))))
        th = torch.as_tensor(it["theta"], dtype=torch.float32).reshape(4)
        self.theta.copy_(th)
        self.K.copy_(torch.from_numpy(intrinsics_from_theta(self.K0.cpu().numpy(), th.numpy(), self.H, self.W)))


    # -- what both steps override, once: the base class's launches / state first, then this group's -----------------------
    def _enqueue(self, want_mask, stream=None):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        super()._enqueue(want_mask, stream=stream)
        self._intr_launch(stream)   # last: whatever ran before it read K as rendered

    def state_dict(self):
        """The base step's ``state_dict`` with one more parameter group (index ``_intr_group``: the intrinsics' Adam state),
        ``theta``, ``K0`` and the free set."""
        return self._intr_state(super().state_dict())

    def load_state_dict(self, sd):
        """Inverse of :meth:`state_dict`, into a step with the same free set, tying, group settings and ``K0``; a state dict
        without an intrinsics part (``FusedPoseStep``'s, ``JointPoseStep``'s) restores the other groups and leaves this one
        as it is."""
        self._intr_check_state(sd)
        super().load_state_dict(sd)
        self._intr_load(sd)


class IntrinsicsPoseStep(_IntrinsicsGroup, FusedPoseStep):
    def __init__(self, model, batch, *, free=("f",), intrinsics_lr=None, intrinsics_weight_decay=None, init_theta=None, **kw):
        """free: names out of "f" (both focal lengths, tied to one log-scale), "fx", "fy", "cx", "cy"; the default is the
        tied focal length only -- a principal-point shift is nearly a small camera rotation at these fields of view, a gauge
        the masks barely fix.  intrinsics_lr / intrinsics_weight_decay: the group's Adam settings (defaults: the pose's; the
        weight decay is the prior towards the given intrinsics); init_theta [4]: where ``theta`` starts (default 0: ``K`` is
        ``batch["K"][0]`` bit for bit).  Everything else is ``FusedPoseStep``'s."""
        self._intr_refuse(batch, kw)
        super().__init__(model, batch, **kw)
        self._intr_init(free, intrinsics_lr, intrinsics_weight_decay, init_theta)


class JointIntrinsicsPoseStep(_IntrinsicsGroup, JointPoseStep):
    """:class:`easyhec_amd.joint_calib.JointPoseStep` with the intrinsics group (index 2) on top.  The launch order is part
    of the contract: ``ehr_joint_backward_adam`` reads ``K`` as rendered, so the launch that rewrites ``K`` runs last."""
    _intr_group = 2

    def __init__(self, model, batch, robot, qpos=None, *, free_intrinsics=("f",), intrinsics_lr=None,
                 intrinsics_weight_decay=None, init_theta=None, **kw):
        """free_intrinsics: :class:`IntrinsicsPoseStep`'s ``free`` (``free=`` names the free JOINTS here, as in
        ``JointPoseStep``); the other keywords are the two classes'."""
        self._intr_refuse(batch, kw)
        super().__init__(model, batch, robot, qpos, **kw)
        self._intr_init(free_intrinsics, intrinsics_lr, intrinsics_weight_decay, init_theta)


@dataclass
class IntrinsicsResult:
    K: torch.Tensor             # [3,3] fitted intrinsics (float32, CPU)
    theta: torch.Tensor         # [4] fitted parameters (CPU); where an element was not free, where it started
    losses: torch.Tensor        # [num_steps] loss of every effective step, before its update (CPU)
    dof: torch.Tensor           # [6] final camera pose coordinates (CPU); also left in ``model.dof``
    recoveries: list = field(default_factory=list)  # what the chain recovered from, in order
    step: object = None         # the IntrinsicsPoseStep (intrinsics(), state_dict())


def solve_intrinsics(cfg, model, batch, num_steps, capture=True, **kw):
    """``num_steps`` EFFECTIVE steps of the pose + intrinsics solve with the optimiser settings of ``cfg.solver`` (Adam: lr,
    weight decay), from a captured graph, with the loop ``RBSolverTrainer.fit`` uses: a reported step is recovered from and
    taken again.  ``kw``: :class:`IntrinsicsPoseStep`'s keywords."""
    joint_calib._check_solver_settings(cfg, kw)
    st = IntrinsicsPoseStep(model, batch, **kw)
    if capture:
        st.capture()
    kept = []
    for remaining, _ in st.effective_rounds(num_steps, "solve_intrinsics"):
        for _ in range(remaining):  # (a reported step's loss is NaN and is dropped below: num_steps finite ones remain)
            kept.append(st.step().clone())
    torch.cuda.synchronize(st.dev)
    losses = torch.cat(kept).cpu() if kept else torch.zeros(0)
    losses = losses[~torch.isnan(losses)][:num_steps]
    st.release_graph()
    return IntrinsicsResult(st.intrinsics(), st.theta.cpu().clone(), losses, model.dof.detach().cpu().clone(),
                            list(st.recoveries), st)
