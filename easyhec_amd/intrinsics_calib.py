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
solves and the ADAM multi-start step (the multi-start Levenberg-Marquardt solve fits a ``K`` per hypothesis:
:mod:`easyhec_amd.lm_multi`), lens distortion, skew, per-view intrinsics, and the autograd (``use_fused=True``) path."""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .chain_step import check_solver_settings
from .fast import FusedPoseStep, _f, refuse_unsupported
from .joint_calib import JointPoseStep
from .param_group import AdamGroup

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


def _refuse(batch, kw):
    """The cases the chain cannot express, each with its reason; before the step is constructed."""
    refuse_unsupported(
        kw, _lib.has_intrinsics,
        "intrinsics refinement is not available for the multi-start step: its hypotheses share one K",
        "intrinsics refinement is not available for a data-parallel job: the intrinsics gradient is not exchanged",
        "this libehr_hip.so has no intrinsics kernel (ehr_intrinsics_backward_adam): rebuild it")
    Kb = batch["K"]
    if Kb.dim() != 3 or tuple(Kb.shape[1:]) != (3, 3):
        raise ValueError(f"intrinsics refinement: batch['K'] must be [B,3,3], got {tuple(Kb.shape)}")
    if not bool((Kb == Kb[:1]).all()):
        # FusedPoseStep renders every view with batch["K"][0]
        raise ValueError("intrinsics refinement: batch['K'] differs between views; the chain has one K (per-view "
                         "intrinsics are out of scope)")


class _IntrinsicsFinish:
    """The launch after the chain: grad_mvp -> d loss / d theta -> Adam on the free elements -> the ``K`` the next step's
    chain reads; and the group's part of the state dict (parameter group ``index``, ``theta``, ``K0``, the free set).
    Gives ``step`` its own ``K`` and ``K0``; goes LAST among the step's finish launches (the others read ``K`` as rendered)."""
    rewrites_K = True

    def __init__(self, step, index, free, lr, weight_decay, init_theta):
        mask, step.tie_focal, step.free_intrinsics = _parse_free(free)
        th0 = np.zeros(4, dtype=np.float32) if init_theta is None else np.asarray(init_theta, dtype=np.float32).reshape(4)
        if step.tie_focal and th0[0] != th0[1]:
            raise ValueError("init_theta: the tied focal lengths ('f') must start from equal theta[0] and theta[1]")
        self.index, self.free = index, torch.tensor(mask, dtype=torch.int32, device=step.dev)
        self.group = g = AdamGroup(4, step.dev, step.lr if lr is None else float(lr),
                                   step.wd if weight_decay is None else float(weight_decay), th0)
        step.intrinsics_lr, step.intrinsics_wd, step.theta, step.theta_grad = g.lr, g.wd, g.param, g.grad
        step.theta_exp_avg, step.theta_exp_avg_sq, step.theta_step_t = g.exp_avg, g.exp_avg_sq, g.step_t
        # the intrinsics as given, and the buffer the kernel writes and the chain reads: the step's own, never the caller's
        step.K0 = step.K.detach().clone().contiguous()
        step.K = torch.from_numpy(intrinsics_from_theta(step.K0.cpu().numpy(), th0, step.H, step.W)).to(step.dev).contiguous()

    def launch(self, step, stream):
        g, (b1, b2) = self.group, step.betas
        _lib.check(_lib.lib().ehr_intrinsics_backward_adam(
            _lib.ptr(step.grad_mvp), _lib.ptr(step.tc_jac), _lib.ptr(step.link_poses), step.B, step.L, step.H, step.W,
            _lib.ptr(step.red), _lib.ptr(step.K0), _lib.ptr(self.free), step.tie_focal, _lib.ptr(g.param), _lib.ptr(g.exp_avg),
            _lib.ptr(g.exp_avg_sq), _lib.ptr(g.step_t), _f(g.lr), _f(b1), _f(b2), _f(step.eps), _f(g.wd), _lib.ptr(step.K),
            _lib.ptr(g.grad), stream), "ehr_intrinsics_backward_adam")

    def add_state(self, step, sd):
        sd["state"][self.index] = self.group.state_entry()
        sd["param_groups"].append(self.group.param_group(sd["param_groups"][0], self.index))
        sd["intrinsics"] = {"theta": step.theta.cpu().clone(), "K0": step.K0.cpu().clone(),
                            "free": list(step.free_intrinsics), "group": self.index}

    def check_state(self, step, sd):
        """Raises where the saved group is not this step's: another free set or tying, group index, settings or ``K0``."""
        it = sd.get("intrinsics")
        if it is None:
            return
        if _parse_free(it["free"])[2] != step.free_intrinsics:
            # the moments of an element that was not free are zero and its theta was never fitted: another set would mix them
            raise ValueError(f"load_state_dict: the state was saved with free intrinsics {list(it['free'])}, this step has "
                             f"{step.free_intrinsics}")
        i = int(it.get("group", self.index))
        if i != self.index:
            raise ValueError(f"load_state_dict: the intrinsics' group was saved as group {i}, this step's is {self.index}")
        if len(sd.get("param_groups", [])) > i:
            self.group.check_saved(sd["param_groups"][i], "the intrinsics' group", "step")
        if not torch.equal(torch.as_tensor(it["K0"], dtype=torch.float32).reshape(3, 3), step.K0.cpu()):
            raise ValueError("load_state_dict: the state was saved for other given intrinsics K0 than this step's")

    def load_state(self, step, sd):
        """A state dict without an intrinsics part (``FusedPoseStep``'s, ``JointPoseStep``'s) leaves the group as it is."""
        it = sd.get("intrinsics")
        if it is not None:
            self.group.load_state(sd.get("state", {}).get(self.index), it["theta"])
            step.K.copy_(torch.from_numpy(intrinsics_from_theta(step.K0.cpu().numpy(), step.theta.cpu().numpy(), step.H, step.W)))


class IntrinsicsPoseStep(FusedPoseStep):
    def __init__(self, model, batch, *, free=("f",), intrinsics_lr=None, intrinsics_weight_decay=None, init_theta=None, **kw):
        """free: names out of "f" (both focal lengths, tied to one log-scale), "fx", "fy", "cx", "cy"; the default is the
        tied focal length only -- a principal-point shift is nearly a small camera rotation at these fields of view, a gauge
        the masks barely fix.  intrinsics_lr / intrinsics_weight_decay: the group's Adam settings (defaults: the pose's; the
        weight decay is the prior towards the given intrinsics); init_theta [4]: where ``theta`` starts (default 0: ``K`` is
        ``batch["K"][0]`` bit for bit).  Everything else is ``FusedPoseStep``'s."""
        _refuse(batch, kw)
        super().__init__(model, batch, **kw)
        self._after += (_IntrinsicsFinish(self, 1, free, intrinsics_lr, intrinsics_weight_decay, init_theta),)

    def intrinsics(self):
        """[3,3] float32 (CPU, a copy): the current ``K``, i.e. the one the next step renders with."""
        return self.K.detach().cpu().clone()


class JointIntrinsicsPoseStep(JointPoseStep):
    """:class:`easyhec_amd.joint_calib.JointPoseStep` with the intrinsics group (index 2) on top, its finish launch after
    ``ehr_joint_backward_adam``, which reads ``K`` as rendered."""
    intrinsics = IntrinsicsPoseStep.intrinsics

    def __init__(self, model, batch, robot, qpos=None, *, free_intrinsics=("f",), intrinsics_lr=None,
                 intrinsics_weight_decay=None, init_theta=None, **kw):
        """free_intrinsics: :class:`IntrinsicsPoseStep`'s ``free`` (``free=`` names the free JOINTS here, as in
        ``JointPoseStep``); the other keywords are the two classes'."""
        _refuse(batch, kw)
        super().__init__(model, batch, robot, qpos, **kw)
        self._after += (_IntrinsicsFinish(self, 2, free_intrinsics, intrinsics_lr, intrinsics_weight_decay, init_theta),)


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
    st = IntrinsicsPoseStep(model, batch, **{**check_solver_settings(cfg), **kw})
    if capture:
        st.capture()
    losses = st.take_effective_steps(num_steps, "solve_intrinsics")[:num_steps, 0]
    st.release_graph()
    return IntrinsicsResult(st.intrinsics(), st.theta.cpu().clone(), losses, model.dof.detach().cpu().clone(),
                            list(st.recoveries), st)
