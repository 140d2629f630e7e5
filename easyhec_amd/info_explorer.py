"""Information-gain exploration: pick the next joint configuration by the log-determinant it adds (``ehr_information_gain`` /
``ehr_information_pick`` in include/ehr.h, csrc/ehr_explore.hip).

:class:`easyhec_amd.space_explorer.SpaceExplorer` scores a candidate by the variance of its masks under poses drawn from the
optimisation history -- EasyHeC's stand-in for information gain.  This module scores the gain itself.  The information op
forms, per pixel, ``wg = gate * w`` and ``J`` from the rendered job slots alone; the reference mask enters the gradient and the
loss only.  So the matrix a candidate configuration WOULD contribute exists before it is observed: it is the op's ``info`` at
the current estimate with any ``ref``.  The chain

    kinematics  ->  ehr_lm_linearize  ->  ehr_mask_information  ->  [ehr_information_gain -> ehr_information_pick] x k

runs over the candidates in chunks, on contexts and a scene OF THE EXPLORER'S OWN: the step's plan, bound reference, weights,
Adam state and a captured chain are never touched, and a solve that explores half-way ends on the same bits.

The criterion.  With ``A`` = what the frames so far pin plus a prior, a candidate's gain is ``logdet M(A + H_q) - logdet M(A)``,
M the marginal information (Schur complement) of the parameters of interest -- the camera pose by default -- with every other
free parameter (joint offsets, intrinsics) left free to absorb what it can.  Greedy selection of k candidates re-evaluates the
gains after every pick; for ``interest="all"`` the picked gains sum to ``logdet A_final - logdet A_0`` exactly (the chain rule),
and logdet being submodular the greedy set is within 1 - 1/e of the best set of k in that case.  For a marginal (``interest``
a subset) the chain rule still holds, the submodularity guarantee does not.

The prior: ``PRIOR_SIGMA`` are MODELLING DEFAULTS a user overrides (``prior_sigma=``), not measurements.  They exist so that a
gauge direction -- joint 0 against the camera rotation -- leaves ``A`` positive definite instead of making logdet minus
infinity, and they are weighted by the residual variance ``sigma2`` so that prior and frames are in the same units.

HIP only; no fallback."""
import ctypes
import types

import numpy as np
import torch

from . import _lib, dr, fused, information, lm
from .fused import LinkScene
from .joint_calib import joint_forward

__all__ = ["information_gain", "greedy_select", "InformationExplorer", "PRIOR_SIGMA", "interest_indices", "prior_sigmas"]

# one standard deviation per parameter kind: modelling defaults, not measurements (see the module docstring)
PRIOR_SIGMA = {
    "translation": 0.05,  # m      dof[0..2]
    "rotation": 0.1,      # rad    dof[3..5]
    "revolute": 0.05,     # rad    offset[j] of a revolute joint
    "prismatic": 0.01,    # m      offset[j] of a prismatic joint
    "focal": 0.05,        #        theta[f|fx|fy]: log-scale of a focal length
    "principal": 0.02,    #        theta[cx|cy]: fraction of the image size
}


def _missing():
    raise RuntimeError("this libehr_hip.so has no exploration kernels (ehr_information_gain): rebuild it")


# ---- arguments that need no device ------------------------------------------------------------------------------------------
def interest_indices(names, interest):
    """The indices into ``names`` of the parameters of interest: "pose" (``dof[0..5]``), "all", or a list of names."""
    names = list(names)
    if isinstance(interest, str) and interest == "all":
        return list(range(len(names)))
    if isinstance(interest, str) and interest == "pose":
        interest = [f"dof[{i}]" for i in range(6)]
    interest = [interest] if isinstance(interest, str) else list(interest)
    unknown = [nm for nm in interest if nm not in names]
    if unknown or not interest:
        raise ValueError(f"interest {unknown or interest}: 'pose', 'all' or a list out of {names}")
    return sorted({names.index(nm) for nm in interest})


def parameter_kinds(names, joint_kind=None):
    """The ``PRIOR_SIGMA`` kind of every name; ``joint_kind[j]``: 1 revolute, 2 prismatic (``joint_calib.joint_kinds``)."""
    kinds = []
    for nm in names:
        head, arg = nm.split("[")[0], nm.split("[")[1].rstrip("]")
        if head == "dof":
            kinds.append("translation" if int(arg) < 3 else "rotation")
        elif head == "offset":
            kinds.append("prismatic" if joint_kind is not None and int(joint_kind[int(arg)]) == 2 else "revolute")
        elif head == "theta":
            kinds.append("focal" if arg in ("f", "fx", "fy") else "principal")
        else:
            raise ValueError(f"unknown parameter {nm!r}")
    return kinds


def prior_sigmas(names, kinds, prior_sigma=None):
    """[N] float64: the prior's standard deviation of every parameter.  ``prior_sigma``: None (``PRIOR_SIGMA`` per kind), a
    number (every parameter), a dict by name or by kind (the rest: the defaults), or a sequence of N.  Non-positive: ValueError."""
    if prior_sigma is None:
        prior_sigma = {}
    if isinstance(prior_sigma, dict):
        unknown = [k for k in prior_sigma if k not in names and k not in PRIOR_SIGMA]
        if unknown:
            raise ValueError(f"prior_sigma {unknown}: keys are parameter names {list(names)} or kinds {list(PRIOR_SIGMA)}")
        s = np.array([prior_sigma.get(nm, prior_sigma.get(kd, PRIOR_SIGMA[kd])) for nm, kd in zip(names, kinds)], dtype=np.float64)
    else:
        s = np.broadcast_to(np.asarray(prior_sigma, dtype=np.float64), (len(names),)).copy()
    if not (np.isfinite(s) & (s > 0)).all():
        raise ValueError(f"prior_sigma must be finite and > 0 for every parameter, got {s.tolist()}")
    return s


def _mask_of(interest, N):
    if interest is None:
        idx = range(N)
    elif isinstance(interest, (int, np.integer)):
        return int(interest) & 0xffffffff
    else:
        idx = [int(i) for i in interest]
        if any(i < 0 or i >= N for i in idx):
            raise ValueError(f"interest indices {idx}: parameters are 0..{N - 1}")
    return sum(1 << i for i in set(idx))


# ---- the two kernels ----------------------------------------------------------------------------------------------------------
def _flags(x, Q, dev, what):
    if x is None:
        return None
    x = torch.as_tensor(x).to(dev)
    dr._require(x.shape == (Q,), f"{what} must have shape [Q]")
    return (x != 0).to(torch.int32).contiguous()


def _check_matrices(A, info):
    dr._check_dev("A", A, torch.float64)
    dr._check_dev("info", info, torch.float64)
    if info.dim() == 3:
        info = info[:, None]
    N = A.shape[-1]
    dr._require(A.dim() == 2 and A.shape == (N, N) and 1 <= N <= _lib.IG_MAX_PARAMS,
                f"A must have shape [N, N], 1 <= N <= {_lib.IG_MAX_PARAMS}")
    dr._require(info.dim() == 4 and info.shape[0] >= 1 and info.shape[1] >= 1 and tuple(info.shape[2:]) == (N, N),
                "info must have shape [Q, N, N] or [Q, S, N, N]")
    dr._require(info.device == A.device, "A and info must be on one device")
    return info.contiguous()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def information_gain(A, info, valid=None, taken=None, scale=1.0, interest=None):
    """A [N,N] float64 (what is known: prior + frames so far), info [Q,N,N] or [Q,S,N,N] float64 (a candidate: S consecutive
    views), both on the device -> gain [Q] float64 on the device: ``ehr_information_gain`` (include/ehr.h).  ``interest``:
    parameter indices (None: all).  ``valid`` / ``taken`` [Q]: a candidate with valid == 0 or taken != 0 gets -inf.  Never
    synchronises."""
    if not _lib.has_information_gain():
        _missing()
    info = _check_matrices(A, info)
    Q, S, N = info.shape[0], info.shape[1], info.shape[2]
    valid, taken = _flags(valid, Q, A.device, "valid"), _flags(taken, Q, A.device, "taken")
    gain = torch.empty((Q,), dtype=torch.float64, device=A.device)
    A = A.contiguous()
    with torch.cuda.device(A.device):
        _lib.check(_lib.lib().ehr_information_gain(_lib.ptr(A), _lib.ptr(info), _lib.ptr(valid), _lib.ptr(taken), Q,
                                                   S, N, float(scale), _mask_of(interest, N), _lib.ptr(gain), _stream()),
                   "ehr_information_gain")
    return gain


def greedy_select(A, info, k, valid=None, scale=1.0, interest=None):
    """k rounds of gain + pick, 2k stream-ordered launches, never synchronises.  Returns a namespace of device tensors:
    ``picked`` [k] int32 (-1 from the round on in which nothing had a finite gain), ``gains`` [k] float64 (NaN there),
    ``A_final`` [N,N] = A plus the picked candidates' matrices in the order picked, ``taken`` [Q] int32.  ``A`` is not
    written."""
    if not _lib.has_information_gain():
        _missing()
    info = _check_matrices(A, info)
    Q, S, N = info.shape[0], info.shape[1], info.shape[2]
    k = int(k)
    dr._require(k >= 1, "k must be >= 1")
    dev = A.device
    valid = _flags(valid, Q, dev, "valid")
    A_work = A.contiguous().clone()
    taken = torch.zeros((Q,), dtype=torch.int32, device=dev)
    picked = torch.full((k,), -1, dtype=torch.int32, device=dev)
    gains = torch.full((k,), float("nan"), dtype=torch.float64, device=dev)
    gain = torch.empty((Q,), dtype=torch.float64, device=dev)
    mask, lib = _mask_of(interest, N), _lib.lib()
    with torch.cuda.device(dev):
        stream = _stream()
        for r in range(k):
            _lib.check(lib.ehr_information_gain(_lib.ptr(A_work), _lib.ptr(info), _lib.ptr(valid), _lib.ptr(taken), Q, S, N,
                                                float(scale), mask, _lib.ptr(gain), stream), "ehr_information_gain")
            _lib.check(lib.ehr_information_pick(_lib.ptr(gain), _lib.ptr(info), Q, S, N, float(scale), r, _lib.ptr(A_work),
                                                _lib.ptr(taken), _lib.ptr(picked), _lib.ptr(gains), stream),
                       "ehr_information_pick")
    return types.SimpleNamespace(picked=picked, gains=gains, A_final=A_work, taken=taken)


# ---- the explorer -------------------------------------------------------------------------------------------------------------
def _refuse(step):
    """What :func:`easyhec_amd.information.information_of` refuses, a stream that is capturing, and a library without the
    kernels of the chain."""
    information._refuse(step)
    if step.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("InformationExplorer: not available while a graph is being captured: ehr_mask_information sizes "
                           "its scratch on the first call")
    if not _lib.has_information_gain():
        _missing()
    if not _lib.has_lm():
        raise RuntimeError("this libehr_hip.so has no Levenberg-Marquardt kernels (ehr_lm_linearize): rebuild it")
    if not _lib.has_information():
        raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")


def _own_scene(scene):
    """A :class:`LinkScene` with buffers of its own (a plan is tied to the scene's buffers)."""
    own = object.__new__(LinkScene)
    for k, v in vars(scene).items():
        setattr(own, k, v.clone() if torch.is_tensor(v) else (list(v) if isinstance(v, list) else v))
    return own


class InformationExplorer:
    """Scores candidate joint configurations for the solve ``step`` (``FusedPoseStep``, ``JointPoseStep``,
    ``IntrinsicsPoseStep`` or ``JointIntrinsicsPoseStep``) by information gain, at the step's CURRENT parameters (read through
    their device tensors on every call).

    robot: :class:`easyhec_amd.robot.Robot` for the candidates' kinematics where the step has no joint table of its own (a
    step with one runs ``ehr_joint_forward`` at its current offsets).  prior_sigma: see :func:`prior_sigmas` (default
    ``PRIOR_SIGMA`` per kind).  sigma2: the residual variance that weighs the prior (default: the current frames'
    ``loss / max(count - N, 1)``, :meth:`easyhec_amd.information.InformationReport.sigma2`).  interest: "pose" (``dof[0..5]``,
    everything else a nuisance parameter), "all", or a list of ``names``.  chunk_candidates: candidates per call of the
    information op.

    ``names`` are :func:`easyhec_amd.information.information_of`'s: ``dof[0..5]``, ``offset[j]``, ``theta[...]``."""

    def __init__(self, step, robot=None, prior_sigma=None, sigma2=None, interest="pose", chunk_candidates=128):
        _refuse(step)
        self.step, self.dev = step, step.dev
        dev = self.dev
        self.layout = lay = lm.parameter_layout(step)
        self.kin, self.names, self.F, self.N = lay.kin, lay.names, lay.F, lay.N
        kin, free, N = lay.kin, lay.free, lay.N
        self.robot = getattr(step, "robot", None) if robot is None else robot
        if N > _lib.IG_MAX_PARAMS:
            raise ValueError(f"InformationExplorer: the step optimises {N} parameters; the kernels take {_lib.IG_MAX_PARAMS}")
        self.interest = interest_indices(self.names, interest)
        joint_kind = kin.jkind.cpu().numpy() if kin is not None else None
        self.prior_sigma = prior_sigmas(self.names, parameter_kinds(self.names, joint_kind), prior_sigma)
        if sigma2 is not None and not (np.isfinite(sigma2) and sigma2 > 0):
            raise ValueError(f"sigma2 must be finite and > 0, got {sigma2}")
        self.sigma2 = None if sigma2 is None else float(sigma2)
        if kin is None and self.robot is None:
            raise ValueError("InformationExplorer: the step has no joint table: pass robot= for the candidates' kinematics")
        self.chunk = int(chunk_candidates)
        if self.chunk < 1:
            raise ValueError("chunk_candidates must be >= 1")
        self.H, self.W, self.L = step.H, step.W, step.L
        self.free_list = torch.tensor(free, dtype=torch.int32, device=dev) if free else None
        self.prior_diag = torch.from_numpy(np.diag(1.0 / self.prior_sigma ** 2)).to(dev)
        # contexts and a scene of its own: the step's plan, bound reference and weights are never touched.  Two contexts, so
        # that the candidates' plan (a chunk of views) and the current frames' (B views, the step's weights) do not replace
        # each other on every call
        self.glctx = dr.RasterizeCudaContext(device=dev)
        self.glctx_frames = dr.RasterizeCudaContext(device=dev)
        self.scene = _own_scene(step.scene)
        self._zero_ref = None

    # -- the chain's parts ------------------------------------------------------------------------------------------------------
    def kinematics(self, qposes):
        """(link_poses [Q,L,4,4] float32, joint_frames [Q,J,6] float32 or None) of joint vectors [Q, <= dof], on the device:
        ``ehr_joint_forward`` with the step's table at its CURRENT offsets where the step has them, the host's forward
        kinematics (as ``SpaceExplorer.link_poses``) otherwise."""
        q = np.atleast_2d(np.asarray(qposes.detach().cpu() if torch.is_tensor(qposes) else qposes, dtype=np.float64))
        kin, dev = self.kin, self.dev
        if kin is None:
            return torch.as_tensor(self.robot.link_poses_batch(q), dtype=torch.float32).to(dev).contiguous(), None
        qp = np.zeros((q.shape[0], kin.J))
        qp[:, :min(kin.J, q.shape[1])] = q[:, :kin.J]
        return self._joint_forward(torch.from_numpy(qp).to(dev), q.shape[0])

    def _joint_forward(self, qpos_dev, B):
        kin, dev = self.kin, self.dev
        lp = torch.empty((B, self.L, 4, 4), device=dev)
        jf = torch.empty((B, kin.J, 6), device=dev)
        with torch.cuda.device(dev):
            joint_forward(kin.t, kin.N, kin.J, self.L, kin.mount, qpos_dev, self.step.offsets, B, lp, jf, _stream())
        return lp, jf

    def _linearize(self, lp, jf, B):
        """(mvp [B,L,4,4], dmvp [N,B,L,4,4]) of ``ehr_lm_linearize`` at the step's current parameters."""
        dev = self.dev
        mvp = torch.empty((B, self.L, 4, 4), device=dev)
        dmvp = torch.empty((self.N, B, self.L, 4, 4), device=dev)
        with torch.cuda.device(dev):
            lm.launch_linearize(self.step, self.layout, self.free_list, lp, jf, B, mvp, dmvp, _stream())
        return mvp, dmvp

    def _guard(self):
        if self.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("InformationExplorer: not available while a graph is being captured")

    def candidate_information(self, qposes, valid=None, link_poses=None, joint_frames=None):
        """(info [Q,N,N] float64, count [Q] int64) on the device: the matrix every candidate WOULD contribute, at the current
        estimate, before it is observed (the op's ``info`` does not depend on the reference mask: a zero one is passed).  Per
        chunk of ``chunk_candidates``: kinematics, ``ehr_lm_linearize``, ``ehr_mask_information``; a ragged last chunk is
        padded with its last candidate (per-view results do not depend on the batch).  Candidates rejected by ``valid`` [Q]
        are not rendered: their rows are zero.  ``link_poses`` [Q,L,4,4] (with ``joint_frames`` [Q,J,6] where joints are free)
        replaces the kinematics: poses a planner or a test supplies."""
        self._guard()
        dev, N = self.dev, self.N
        if valid is not None:
            keep = np.flatnonzero(np.asarray(valid.cpu() if torch.is_tensor(valid) else valid).reshape(-1) != 0)
            total = len(qposes) if link_poses is None else len(link_poses)
            info = torch.zeros((total, N, N), dtype=torch.float64, device=dev)
            count = torch.zeros((total,), dtype=torch.int64, device=dev)
            if len(keep):
                rows = torch.from_numpy(keep).to(dev)
                part = self.candidate_information(
                    np.asarray(qposes)[keep], None, None if link_poses is None else torch.as_tensor(link_poses).to(dev)[rows],
                    None if joint_frames is None else torch.as_tensor(joint_frames).to(dev)[rows])
                info[rows], count[rows] = part
            return info, count
        if link_poses is None:
            lp, jf = self.kinematics(qposes)
        else:
            lp = torch.as_tensor(link_poses, dtype=torch.float32).to(dev).contiguous()
            jf = None if joint_frames is None else torch.as_tensor(joint_frames, dtype=torch.float32).to(dev).contiguous()
            if self.F and jf is None:
                raise ValueError("candidate_information: link_poses= needs joint_frames= where joints are free")
        Q = lp.shape[0]
        dr._require(Q >= 1 and tuple(lp.shape[1:]) == (self.L, 4, 4), "link poses must have shape [Q, L, 4, 4]")
        C = min(self.chunk, Q)
        info = torch.empty((Q, N, N), dtype=torch.float64, device=dev)
        count = torch.empty((Q,), dtype=torch.int64, device=dev)
        fused._ensure_plan(self.glctx, self.scene, C, self.H, self.W)
        if getattr(self.glctx, "_bound_weight", None) is not None:
            fused.bind_weight(self.glctx, self.scene, None)
        if self._zero_ref is None or self._zero_ref.shape[0] != C:
            self._zero_ref = torch.zeros((C, self.H, self.W), device=dev)
        for lo in range(0, Q, C):
            n = min(C, Q - lo)
            rows = torch.arange(lo, lo + C, device=dev).clamp_(max=Q - 1)
            lp_c = lp[lo:lo + C] if n == C else lp[rows].contiguous()
            jf_c = None if jf is None else (jf[lo:lo + C] if n == C else jf[rows].contiguous())
            mvp, dmvp = self._linearize(lp_c, jf_c, C)
            out = information._outputs(N, C, self.L, dev, False, False)
            information._launch(self.glctx, self.scene, mvp, dmvp, self._zero_ref, out.info, out.grad, out.count, None, None)
            info[lo:lo + n] = out.info[:n]
            count[lo:lo + n] = out.count[:n]
        return info, count

    def current_information(self):
        """The same chain over the step's OWN frames, with ``step.ref`` and the step's weights (bound to the explorer's
        context for the frames, which serves this call alone: the candidates' context never sees them).  A namespace of device tensors: ``H0`` [B,N,N], ``grad`` [B,N], ``loss`` [B], ``count`` [B].
        A step with a joint table gets its kinematics at the CURRENT offsets, into buffers of the explorer's."""
        self._guard()
        st = self.step
        if self.kin is not None:
            lp, jf = self._joint_forward(self.kin.qpos, st.B)
        else:
            lp, jf = st.link_poses, None
        mvp, dmvp = self._linearize(lp, jf, st.B)
        weight = getattr(st, "weight", None)
        out = information.mask_information(self.glctx_frames, self.scene, mvp, dmvp, st.ref, weight=weight, want_loss=True)
        return types.SimpleNamespace(H0=out.info, grad=out.grad, loss=out.loss, count=out.count)

    def prior_matrix(self, current=None):
        """A0 [N,N] float64 on the device: ``sum_b H0[b]`` (in view order) ``+ sigma2 diag(1 / prior_sigma_k^2)``.  Never
        synchronises: the default sigma2 is formed on the device."""
        cur = self.current_information() if current is None else current
        A0 = cur.H0[0].clone()
        for b in range(1, cur.H0.shape[0]):
            A0 += cur.H0[b]
        if self.sigma2 is None:
            s2 = cur.loss.double().sum() / (cur.count.sum() - self.N).clamp(min=1).double()
        else:
            s2 = self.sigma2
        return A0 + s2 * self.prior_diag

    # -- the public methods -----------------------------------------------------------------------------------------------------
    def score(self, qposes, valid=None, **poses):
        """gain [Q] float64 on the device (-inf for candidates rejected by ``valid``, which are not rendered)."""
        info, _ = self.candidate_information(qposes, valid, **poses)
        return information_gain(self.prior_matrix(), info, valid=valid, interest=self.interest)

    def select(self, qposes, k=1, valid=None, **poses):
        """Greedy selection of k candidates.  A namespace: ``picked`` [k] and ``gains`` [k] (device; -1 / NaN once nothing
        is left), ``A0``, ``A_final`` (device), ``info`` / ``count`` of the candidates, and ``report``: the
        :class:`easyhec_amd.information.InformationReport` of ``A_final`` (synchronises)."""
        info, count = self.candidate_information(qposes, valid, **poses)
        A0 = self.prior_matrix()
        sel = greedy_select(A0, info, k, valid=valid, interest=self.interest)
        sel.A0, sel.info, sel.count = A0, info, count
        sel.report = information.InformationReport(sel.A_final.cpu().numpy()[None], self.names)
        return sel

    def forward(self, qposes, valid=None, **poses):
        """The outputs dictionary of ``SpaceExplorer.forward`` with the gain in the variance's place: ``qpos``, ``qpos_idx``,
        ``gain``, ``gain_max`` / ``gain_min`` / ``gain_mean`` (over the candidates with a finite positive gain), ``gains``."""
        gains = self.score(qposes, valid, **poses).cpu()
        ok = torch.isfinite(gains) & (gains > 0)
        if not bool(ok.any()):
            raise RuntimeError("no valid qpos found! Consider to increase the number of sampled qpos, "
                               "or increase the max_dist.")
        tid = torch.where(ok, gains, torch.full_like(gains, -float("inf"))).argmax()
        pos = gains[ok]
        return {"qpos": np.asarray(qposes)[tid], "qpos_idx": tid, "gain": gains[tid], "gain_max": pos.max(),
                "gain_min": pos.min(), "gain_mean": pos.mean(), "gains": gains}
