"""Information matrix of the mask loss: which parameters the views pin (``ehr_mask_information`` in include/ehr.h, DESIGN.md
section 6j).

The solves of this package free more and more parameters -- the camera pose, joint zero offsets, a rig's shared offsets, the
intrinsics -- and the silhouettes cannot tell all of them apart: an offset of joint 0 and a camera rotation explain the same
change, a principal-point shift is nearly a rotation.  :func:`mask_information` returns the Gauss-Newton matrix
``sum_p w_p J_p J_p^T`` of the fused mask loss for ANY parameters, described by their tangents ``d MVP[b,l] / d theta_k``;
the tangent builders make those for every kind of parameter the package optimises, :func:`information_of` assembles them for
a step object at its current parameters, and :class:`InformationReport` turns the matrix into eigenvalues, weak directions
named by parameter, marginal information and a covariance.

The hot part is a HIP kernel beside the composite stage (``vb_info_kernel``); the tangents are built in float64 on the host,
off the hot path.  HIP only; no fallback."""
import ctypes
import types

import numpy as np
import torch

from . import _lib, dr, fused
from .se3 import se3_exp_map

__all__ = ["mask_information", "pose_tangents", "intrinsics_tangents", "joint_tangents", "information_of", "rig_information",
           "InformationReport", "MAX_TANGENTS"]

MAX_TANGENTS = 32
JOINT_STEP = 1e-4  # rad (m for a prismatic joint): the central differences of joint_tangents


# ---- the op ---------------------------------------------------------------------------------------------------------------
def _launch(glctx, scene, mvp, dmvp, ref, info, grad, count, loss, grad_mvp):
    N, B, L = dmvp.shape[0], mvp.shape[0], mvp.shape[1]
    H, W = ref.shape[1], ref.shape[2]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    with torch.cuda.device(glctx.device):
        _lib.check(_lib.lib().ehr_mask_information(
            glctx.handle, _lib.ptr(scene.verts), _lib.ptr(scene.tris), _lib.ptr(scene.tri_link), _lib.ptr(scene.vert_link),
            _lib.ptr(scene.opp), _lib.ptr(mvp), _lib.ptr(dmvp), N, _lib.ptr(ref), B, L, scene.num_verts, scene.num_tris, H, W,
            _lib.ptr(info), _lib.ptr(grad), _lib.ptr(count), _lib.ptr(loss), _lib.ptr(grad_mvp), stream),
            "ehr_mask_information")


def _check_args(scene, mvp, dmvp, ref):
    dr._check_dev("mvp", mvp, torch.float32)
    dr._check_dev("dmvp", dmvp, torch.float32)
    dr._check_dev("ref", ref, torch.float32)
    dr._require(mvp.dim() == 4 and mvp.shape[1] == scene.num_links and mvp.shape[2:] == (4, 4),
                "mvp must have shape [B, num_links, 4, 4]")
    dr._require(ref.dim() == 3 and ref.shape[0] == mvp.shape[0], "ref must have shape [B, H, W]")
    dr._require(dmvp.dim() == 5 and tuple(dmvp.shape[1:]) == tuple(mvp.shape),
                "dmvp must have shape [N, B, num_links, 4, 4]: one tangent d MVP / d theta_k per parameter")
    dr._require(1 <= dmvp.shape[0] <= MAX_TANGENTS, f"dmvp holds {dmvp.shape[0]} tangents: 1 <= N <= {MAX_TANGENTS}")
    dr._require(mvp.device == scene.device and ref.device == scene.device and dmvp.device == scene.device,
                "mvp/dmvp/ref must be on the scene's device")


def _outputs(N, B, L, dev, want_loss, want_grad_mvp):
    return types.SimpleNamespace(
        info=torch.empty((B, N, N), dtype=torch.float64, device=dev), grad=torch.empty((B, N), dtype=torch.float64, device=dev),
        count=torch.empty((B,), dtype=torch.int64, device=dev),
        loss=torch.empty((B,), dtype=torch.float32, device=dev) if want_loss else None,
        grad_mvp=torch.empty((B, L, 4, 4), dtype=torch.float32, device=dev) if want_grad_mvp else None)


def mask_information(glctx, scene, mvp, dmvp, ref, weight=None, want_loss=False, want_grad_mvp=False):
    """mvp [B,L,4,4], ref [B,H,W] and ``weight`` as for :func:`easyhec_amd.fused.render_mask_loss`; dmvp [N,B,L,4,4] float32:
    the tangents ``d MVP[b,l] / d theta_k`` of N <= 32 parameters.  Returns a namespace of device tensors, PER VIEW

        info  [B,N,N] float64   sum_p w_p J_p J_p^T, exactly symmetric
        grad  [B,N]   float64   sum_p 2 w_p e_p J_p: the loss gradient along the tangents
        count [B]     int64     pixels with w_p > 0 and a non-zero J_p
        loss  [B]     float32   (``want_loss``) and grad_mvp [B,L,4,4] (``want_grad_mvp``): ``render_mask_loss``'s, bit for bit

    with ``J_p[k] = gate_p sum_l <d si_l,p / d MVP[b,l], dmvp[k,b,l]>`` (include/ehr.h).  Sums over views, cameras or
    hypotheses are the caller's, in float64.  Deterministic: two calls give identical bits.  A reported call (an overflow of
    the plan, a non-finite sum) returns NaN and count -1; :func:`easyhec_amd.fused.check_status` raises then."""
    _check_args(scene, mvp, dmvp, ref)
    if not _lib.has_information():
        raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")
    B, H, W = ref.shape
    fused._ensure_plan(glctx, scene, B, H, W)
    if weight is not None or getattr(glctx, "_bound_weight", None) is not None:
        if weight is not None:
            dr._check_dev("weight", weight, torch.float32)
            dr._require(weight.dim() == 3 and weight.shape[1:] == ref.shape[1:] and weight.device == scene.device,
                        "weight must have shape [Bv, H, W] on the scene's device")
            weight = weight.contiguous()
        if not fused._same_tensor(weight, getattr(glctx, "_bound_weight", None)):
            fused.bind_weight(glctx, scene, weight, views=B)
    out = _outputs(dmvp.shape[0], B, mvp.shape[1], mvp.device, want_loss, want_grad_mvp)
    _launch(glctx, scene, mvp.detach().contiguous(), dmvp.contiguous(), ref.contiguous(), out.info, out.grad, out.count,
            out.loss, out.grad_mvp)
    return out


# ---- tangents (float64, host) ---------------------------------------------------------------------------------------------
def _projection64(K, H, W, n, f):
    """:func:`easyhec_amd.nvdiffrast_utils.K_to_projection` in float64 (that one rounds K to float32), differentiable."""
    K = torch.as_tensor(K, dtype=torch.float64)
    z, o = torch.zeros((), dtype=torch.float64), torch.ones((), dtype=torch.float64)
    return torch.stack([torch.stack([2 * K[0, 0] / W, z, -2 * K[0, 2] / W + 1, z]),
                        torch.stack([z, 2 * K[1, 1] / H, 2 * K[1, 2] / H - 1, z]),
                        torch.stack([z, z, o * (-(f + n) / (f - n)), o * (-2 * f * n / (f - n))]),
                        torch.stack([z, z, -o, z])])


def _mvp64(K, H, W, dof, link_poses, n, f):
    """:func:`easyhec_amd.fused.mvp_matrices` of the pose ``se3_exp_map(dof)`` in float64 on the host (same association)."""
    Tc = se3_exp_map(dof[None]).permute(0, 2, 1)[0]
    o2b = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))
    return _projection64(K, H, W, n, f) @ (o2b @ (Tc[None, None] @ link_poses))


def _f64(a):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64))


def pose_tangents(K, H, W, dof, link_poses, n=0.001, f=10.0):
    """[6,B,L,4,4] float64: ``d MVP / d dof[i]`` at ``dof`` -- ``torch.autograd.functional.jacobian`` through
    :func:`easyhec_amd.se3.se3_exp_map` and the product :func:`easyhec_amd.fused.mvp_matrices` forms, in float64."""
    K, dof, lp = _f64(K), _f64(dof).reshape(6), _f64(link_poses)
    jac = torch.autograd.functional.jacobian(lambda d: _mvp64(K, H, W, d, lp, n, f), dof)   # [B,L,4,4,6]
    return jac.permute(4, 0, 1, 2, 3).contiguous()


def _K_of_theta(K0, theta, H, W):
    """:func:`easyhec_amd.intrinsics_calib.intrinsics_from_theta`'s four expressions in float64, differentiable (that function
    rounds to float32 and keeps ``K0``'s bits where theta == 0: the same K to 6e-8 relative)."""
    K = K0.clone()
    K[0, 0] = K0[0, 0] * torch.exp(theta[0])
    K[1, 1] = K0[1, 1] * torch.exp(theta[1])
    K[0, 2] = K0[0, 2] + float(W) * theta[2]
    K[1, 2] = K0[1, 2] + float(H) * theta[3]
    return K


def intrinsics_tangents(K0, theta, free, H, W, dof, link_poses, n=0.001, f=10.0):
    """([F,B,L,4,4] float64, names): ``d MVP / d theta`` for the freed entries of ``theta`` (names out of "f", "fx", "fy",
    "cx", "cy" as in :class:`easyhec_amd.intrinsics_calib.IntrinsicsPoseStep`; "f" moves theta[0] and theta[1] together), with
    K(theta) as :func:`easyhec_amd.intrinsics_calib.intrinsics_from_theta` defines it."""
    from .intrinsics_calib import _NAMES, _parse_free
    _, _, names = _parse_free(free)
    K0, th, dof, lp = _f64(K0).reshape(3, 3), _f64(theta).reshape(4), _f64(dof).reshape(6), _f64(link_poses)
    jac = torch.autograd.functional.jacobian(lambda t: _mvp64(_K_of_theta(K0, t, H, W), H, W, dof, lp, n, f), th)
    jac = jac.permute(4, 0, 1, 2, 3)                                                          # [4,B,L,4,4]
    cols = [jac[0] + jac[1] if nm == "f" else jac[_NAMES[nm]] for nm in names]
    return torch.stack(cols).contiguous(), [f"theta[{nm}]" for nm in names]


def joint_tangents(robot, qpos, offsets, free, K, H, W, dof, n=0.001, f=10.0, h=JOINT_STEP):
    """[F,B,L,4,4] float64: ``d MVP / d offset[j]`` for the joints ``free``, by central differences of
    ``UrdfChain.link_poses_batch`` (float64) at ``qpos + offsets``:  (FK(q + h e_j) - FK(q - h e_j)) / 2h.

    Step and error: h = 1e-4.  A link pose is a product of rotations by the joint angles, so the truncation error of the
    central difference is h^2 / 6 = 1.7e-9 of the tangent (third derivative of sin / cos: bounded by the tangent's own
    size), and the rounding error 2^-53 |FK| / h = 1.1e-12 per metre of link position, relative to tangents of the order of a
    metre per radian.  Both are far below the 6e-8 at which the tangents are rounded to float32 for the kernel."""
    q = np.atleast_2d(np.asarray(qpos, dtype=np.float64))
    J = int(robot.chain.dof)
    qp = np.zeros((q.shape[0], J))
    qp[:, :min(J, q.shape[1])] = q[:, :J]
    qp = qp + np.asarray(offsets, dtype=np.float64).reshape(1, J)
    K, dof = _f64(K), _f64(dof).reshape(6)
    out = []
    for j in free:
        e = np.zeros((1, J))
        e[0, int(j)] = h
        dlp = (robot.link_poses_batch(qp + e) - robot.link_poses_batch(qp - e)) / (2.0 * h)
        Tc = se3_exp_map(dof[None]).permute(0, 2, 1)[0]
        o2b = torch.diag(torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64))
        out.append(_projection64(K, H, W, n, f) @ (o2b @ (Tc[None, None] @ torch.from_numpy(dlp))))
    return torch.stack(out).contiguous() if out else torch.zeros((0, q.shape[0], len(robot.use_links), 4, 4), dtype=torch.float64)


# ---- the report -----------------------------------------------------------------------------------------------------------
class InformationReport:
    """What an information matrix says about a set of named parameters.

    H_views [B,N,N] (one matrix per view, or per camera of a rig), H their sum, ``names``; eigenvalues (ascending) and
    eigenvectors (columns) of the SCALED matrix ``D^-1/2 H D^-1/2``, D = diag H -- the parameters have different units
    (metres, radians, log-focal-length), and the scaled matrix is the correlation structure, free of them.  A parameter whose
    row and column are all zero is listed in ``no_information`` and left out of the scaling (its eigenvector components are 0).
    ``condition`` = largest / smallest eigenvalue of the scaled matrix (inf where the smallest is <= 0).

    The covariance, read with care: ``covariance()`` = sigma2 pinv(H), sigma2 = sum(loss) / max(sum(count) - N, 1), is the
    covariance of the SOLVER'S OWN antialiasing model -- J is the derivative the optimiser descends along, which exists only
    on the pixels where a blended pair was written.  At sub-pixel triangles that model sees about a tenth of the silhouette
    (DESIGN.md section 3), so the absolute sigmas are conservative guides, not error bars.  The directions and the RATIOS --
    which combination of parameters is weak, and by how much next to the others -- are the product."""

    def __init__(self, H_views, names, grad_views=None, count=None, loss=None):
        self.H_views = np.asarray(H_views, dtype=np.float64)
        self.H = self.H_views.sum(axis=0)
        self.names = list(names)
        N = len(self.names)
        assert self.H.shape == (N, N)
        self.grad = None if grad_views is None else np.asarray(grad_views, dtype=np.float64).sum(axis=0)
        self.count = None if count is None else int(np.asarray(count).sum())
        self.loss = None if loss is None else float(np.asarray(loss, dtype=np.float64).sum())
        d = np.diag(self.H)
        self.live = d > 0
        self.no_information = [nm for nm, ok in zip(self.names, self.live) if not ok]
        s = np.sqrt(d[self.live])
        Hs = self.H[np.ix_(self.live, self.live)] / np.outer(s, s)
        self.scaled = 0.5 * (Hs + Hs.T)
        if self.live.any():
            w, v = np.linalg.eigh(self.scaled)
        else:
            w, v = np.zeros(0), np.zeros((0, 0))
        self.eigenvalues = w
        self.eigenvectors = np.zeros((N, len(w)))
        self.eigenvectors[self.live] = v
        self.condition = float(w[-1] / w[0]) if len(w) and w[0] > 0 else float("inf")

    def direction(self, i):
        """Eigenvector i (ascending eigenvalues) as a list of (name, component), largest magnitude first."""
        v = self.eigenvectors[:, i]
        return [(self.names[k], float(v[k])) for k in np.argsort(-np.abs(v)) if v[k] != 0.0]

    def weak_directions(self, rtol=1e-3):
        """The directions of the scaled matrix whose eigenvalue is below ``rtol`` times the largest: a list of
        ``(eigenvalue, [(name, component), ...])``, weakest first.  Components refer to the scaled parameters
        ``sqrt(H_kk) theta_k``."""
        w = self.eigenvalues
        return [(float(w[i]), self.direction(i)) for i in range(len(w)) if w[i] < rtol * w[-1]]

    def marginal_information(self, names):
        """The Schur complement ``H_aa - H_ab pinv(H_bb) H_ba`` for the parameters ``names``: what the views say about them
        once every other parameter is left free to absorb what it can."""
        names = [names] if isinstance(names, str) else list(names)
        a = [self.names.index(nm) for nm in names]
        b = [k for k in range(len(self.names)) if k not in a]
        Haa = self.H[np.ix_(a, a)]
        if not b:
            return Haa
        Hab = self.H[np.ix_(a, b)]
        return Haa - Hab @ np.linalg.pinv(self.H[np.ix_(b, b)], hermitian=True) @ Hab.T

    def sigma2(self):
        if self.loss is None or self.count is None:
            raise ValueError("covariance(): the report was built without loss and count")
        return self.loss / max(self.count - len(self.names), 1)

    def covariance(self, rcond=1e-10):
        """``sigma2 pinv(H)``: the covariance of the solver's own antialiasing model (see the class docstring).  The
        pseudo-inverse is taken on the scaled matrix: directions whose eigenvalue is below ``rcond`` times the largest -- a
        gauge: no information at all -- and parameters without information are left out (zero rows and columns), not
        reported with a huge variance."""
        w, v = self.eigenvalues, self.eigenvectors
        keep = w > rcond * (w[-1] if len(w) else 1.0)
        d = np.where(self.live, np.diag(self.H), 1.0)
        P = (v[:, keep] / w[keep]) @ v[:, keep].T
        return self.sigma2() * P / np.sqrt(np.outer(d, d))

    def summary(self):
        lines = [f"{len(self.names)} parameters, condition {self.condition:.3g}"]
        if self.no_information:
            lines.append("no information: " + ", ".join(self.no_information))
        for i, w in enumerate(self.eigenvalues):
            top = ", ".join(f"{nm} {c:+.2f}" for nm, c in self.direction(i)[:4])
            lines.append(f"  {w:10.3e}  {top}")
        return "\n".join(lines)


# ---- steps ----------------------------------------------------------------------------------------------------------------
def _refuse(step):
    from .multistart import MultiStartPoseStep
    from .rig_calib import RigJointStep
    if isinstance(step, MultiStartPoseStep):
        raise ValueError("information_of: not available for the multi-start step: its hypotheses are separate solves (an "
                         "information matrix across hypotheses is out of scope); ask for the winner's FusedPoseStep")
    if isinstance(step, RigJointStep):
        raise ValueError("information_of: a rig has one system over all cameras: use rig_information(rig_step)")
    if getattr(step, "distributed", False) or getattr(step, "rccl", False) or getattr(step, "p2p", False):
        raise ValueError("information_of: not available for a data-parallel job: each rank holds its own views, and the "
                         "matrices are not exchanged")
    for attr in ("glctx", "scene", "ref", "link_poses", "K", "model"):
        if not hasattr(step, attr):
            raise TypeError(f"information_of: {type(step).__name__} is not a launch-chain step (FusedPoseStep, JointPoseStep, "
                            "IntrinsicsPoseStep, JointIntrinsicsPoseStep)")


def _step_system(step):
    """(mvp float32 device, tangents [N,B,L,4,4] float64 host, names) at the step's CURRENT parameters."""
    dof = _f64(step.model.dof.data)
    K = _f64(step.K)
    H, W, n, f = step.H, step.W, step.near, step.far
    kin = getattr(step, "kinematics", None)
    if kin is not None:   # the link poses at the current offsets, in float64 (the forward kernel's own arithmetic)
        qp = kin.qpos.cpu().numpy() + step.offsets.detach().cpu().double().numpy()[None]
        lp = torch.from_numpy(step.robot.link_poses_batch(qp))
    else:
        lp = _f64(step.link_poses)
    tang, names = [pose_tangents(K, H, W, dof, lp, n, f)], [f"dof[{i}]" for i in range(6)]
    if kin is not None and len(step.free_joints):
        tang.append(joint_tangents(step.robot, kin.qpos.cpu().numpy(), step.offsets.detach().cpu().numpy(), step.free_joints,
                                   K, H, W, dof, n, f))
        names += [f"offset[{j}]" for j in step.free_joints]
    if hasattr(step, "free_intrinsics"):
        t, nm = intrinsics_tangents(_f64(step.K0), step.theta.detach(), step.free_intrinsics, H, W, dof, lp, n, f)
        tang.append(t)
        names += nm
    mvp = _mvp64(K, H, W, dof, lp, n, f).to(torch.float32).to(step.dev).contiguous()
    return mvp, torch.cat(tang), names


def _step_call(step):
    """One ``ehr_mask_information`` on the step's own context, plan, bound reference and weights; nothing of the step is
    written, no plan or binding changes."""
    _refuse(step)
    if not _lib.has_information():
        raise RuntimeError("this libehr_hip.so has no information kernel (ehr_mask_information): rebuild it")
    plan = getattr(step.glctx, "_plan", None)
    if plan is None or plan.key != fused._plan_key(step.scene, step.B, step.H, step.W):
        raise RuntimeError("information_of: the step's context holds another plan (somebody else rendered with it): take a "
                           "step first, which plans and binds again")
    if getattr(step.glctx, "_bound_weight", None) is not getattr(step, "weight", None):
        raise RuntimeError("information_of: the weights bound to the step's context are not the step's (somebody else used "
                           "the context): take a step first, which binds them again")
    mvp, tang, names = _step_system(step)
    if len(names) > MAX_TANGENTS:
        raise ValueError(f"information_of: the step optimises {len(names)} parameters; the op takes {MAX_TANGENTS}")
    dmvp = tang.to(torch.float32).to(step.dev).contiguous()
    out = _outputs(len(names), step.B, step.L, step.dev, True, False)
    _launch(step.glctx, step.scene, mvp, dmvp, step.ref, out.info, out.grad, out.count, out.loss, None)
    return out, names


def information_of(step):
    """The :class:`InformationReport` of the parameters ``step`` actually optimises, at their CURRENT values: ``dof[0..5]``,
    then ``offset[j]`` for the free joints, then ``theta[f|fx|fy|cx|cy]`` for the free intrinsics.  Accepts ``FusedPoseStep``,
    ``JointPoseStep``, ``IntrinsicsPoseStep`` and ``JointIntrinsicsPoseStep``; refuses, with the reason, the multi-start step
    and data-parallel jobs.  It does not disturb the step: a solve that calls it half-way ends on the same bits (captured
    graph included).  Synchronises (the result comes to the host)."""
    out, names = _step_call(step)
    torch.cuda.synchronize(step.dev)
    return InformationReport(out.info.cpu().numpy(), names, out.grad.cpu().numpy(), out.count.cpu().numpy(),
                             out.loss.cpu().numpy())


def rig_information(rig_step):
    """The report of the ``6 C + F`` system :class:`easyhec_amd.rig_calib.RigJointStep` optimises: one call per camera, each
    camera's ``(6 + F)`` matrix embedded with the offsets shared -- ``cam0.dof[0..5]``, ``cam1.dof[0..5]``, ...,
    ``offset[j]`` -- and summed.  ``H_views`` holds one matrix per CAMERA (its views summed)."""
    from .rig_calib import RigJointStep
    if not isinstance(rig_step, RigJointStep):
        raise TypeError("rig_information: expects a RigJointStep")
    C, F = rig_step.C, len(rig_step.free_joints)
    names = [f"cam{c}.dof[{i}]" for c in range(C) for i in range(6)] + [f"offset[{j}]" for j in rig_step.free_joints]
    N = 6 * C + F
    Hc, gc, count, loss = np.zeros((C, N, N)), np.zeros((C, N)), 0, 0.0
    for c, cam in enumerate(rig_step.cameras):
        out, _ = _step_call(cam)
        torch.cuda.synchronize(cam.dev)
        idx = list(range(6 * c, 6 * c + 6)) + list(range(6 * C, N))
        Hc[c][np.ix_(idx, idx)] = out.info.cpu().numpy().sum(axis=0)
        gc[c][idx] = out.grad.cpu().numpy().sum(axis=0)
        count += int(out.count.sum().item())
        loss += float(out.loss.double().sum().item())
    return InformationReport(Hc, names, gc, [count], [loss])
