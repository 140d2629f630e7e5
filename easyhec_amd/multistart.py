"""Multi-start pose solve: P start poses of ONE calibration problem advance together, one ``ehr_solver_step_multi`` launch
chain per step whatever P is (include/ehr.h).

The solve of :class:`easyhec_amd.fast.FusedPoseStep` is local -- the reference's tools/manual_tune_franka_init.py exists
because somebody has to find a start it converges from -- and at small view counts it leaves most of the GPU idle.  Here
hypothesis p on real view j is virtual view ``p * Bv + j`` of a P x Bv-view plan; images, link poses and intrinsics are
shared, never copied, and every hypothesis reproduces its solo ``FusedPoseStep`` solve bit for bit
(tests/test_gpu_multistart.py).  HIP only: CPU tensors or a missing device raise, there is no fallback."""
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .chain_step import _ChainStep, check_solver_settings
from .fast import _f, _hip_device, _private_weight
from .se3 import se3_log_map
from .synthetic import perturb_pose

__all__ = ["MultiStartPoseStep", "MultiStartResult", "sample_starts", "rank_losses", "solve_multistart"]


def sample_starts(Tc_init, P, trans_sigma_m=0.03, rot_sigma_deg=4.0, seed=0):
    """[P,4,4] float64 start poses around ``Tc_init``: start 0 is ``Tc_init`` itself, start p > 0 is
    ``Tc_init @ exp([dt, drot])`` (:func:`easyhec_amd.synthetic.perturb_pose`) with dt ~ N(0, trans_sigma_m) metres and
    drot ~ N(0, rot_sigma_deg) degrees per axis.  Deterministic: ``numpy.random.default_rng(seed)``, six normals per start
    in order, so the first P starts of a larger draw are the same poses."""
    Tc_init = np.asarray(Tc_init, dtype=np.float64)
    if Tc_init.shape != (4, 4) or P < 1:
        raise ValueError("sample_starts: Tc_init must be a 4x4 pose and P >= 1")
    rng = np.random.default_rng(seed)
    out = [Tc_init.copy()]
    for _ in range(P - 1):
        z = rng.standard_normal(6)
        out.append(perturb_pose(Tc_init, dt=z[:3] * trans_sigma_m, drot_deg=z[3:] * rot_sigma_deg))
    return np.stack(out)


def rank_losses(values):
    """Indices of ``values`` from best to worst: ascending, NaN last, ties by index."""
    v = [float(x) for x in np.asarray(values, dtype=np.float64).reshape(-1)]
    return sorted(range(len(v)), key=lambda i: (v[i] != v[i], 0.0 if v[i] != v[i] else v[i], i))


def _starts_to_dof(starts):
    """[P,4,4] poses or [P,6] dofs -> [P,6] float32 (CPU).  A pose goes through the conversion RBSolver applies to
    ``init_Tc_c2b``, one pose at a time, so that start p is bit for bit the dof a solver built on that pose starts from."""
    s = torch.as_tensor(np.asarray(starts.detach().cpu() if torch.is_tensor(starts) else starts))
    if s.dim() == 2 and s.shape[1] == 6:
        return s.to(torch.float32).contiguous()
    if s.dim() == 3 and s.shape[1:] == (4, 4):
        return torch.stack([se3_log_map(T.to(torch.float32)[None].permute(0, 2, 1), eps=1e-5, backend="opencv")[0]
                            for T in s]).contiguous()
    raise ValueError("starts must be [P,4,4] poses or [P,6] dofs")


class MultiStartPoseStep(_ChainStep):
    """:class:`easyhec_amd.fast.FusedPoseStep` for P hypotheses, on the same :class:`easyhec_amd.chain_step._ChainStep`
    (``step`` returns the [P] losses: NaN for a hypothesis that is frozen, all NaN for a reported step -- the conditions
    are step-wide).  State lives in this object (``dof``, ``exp_avg``, ``exp_avg_sq`` [P,6]; ``step_t``, ``hist_row`` [P];
    ``history`` [P,rows,6], every hypothesis starting from a copy of the model's ``history_ops``); the model is only read
    (meshes, image size, history) until :func:`solve_multistart` writes the winner into it.  Single process: hypotheses are
    not exchanged across ranks."""

    def __init__(self, model, batch, starts, lr=0.003, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0005, near=0.001,
                 far=10.0, slack=None):
        dev = _hip_device("MultiStartPoseStep", model, batch)
        if not _lib.has_multistart():
            raise RuntimeError("libehr_hip.so has no ehr_solver_step_multi: rebuild it (python -m easyhec_amd.build)")
        self.model = model
        self.renderer = model._ensure_renderer()
        self.scene = model._ensure_scene()
        self.glctx = self.renderer.glctx
        self.dev = dev
        self.H, self.W = model.H, model.W
        self.ref = batch["mask"].to(dev, torch.float32).contiguous().clone()  # private: its cached sums must not go stale
        self.weight = _private_weight(batch, dev)  # optional per-pixel weights [Bv,H,W], shared by the hypotheses like ref
        self.link_poses = batch["link_poses"].to(dev, torch.float32).contiguous()
        self.K = batch["K"][0].to(dev, torch.float32).contiguous()
        self.Bv, self.L = self.link_poses.shape[0], self.link_poses.shape[1]
        assert self.L == self.scene.num_links and self.ref.shape == (self.Bv, self.H, self.W)
        assert self.weight is None or self.weight.shape == self.ref.shape
        self.dof = _starts_to_dof(starts).to(dev)
        self.P = self.dof.shape[0]
        self.B = self.P * self.Bv  # virtual views
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.near, self.far = near, far
        P, B = self.P, self.B
        self.exp_avg = torch.zeros((P, 6), device=dev)
        self.exp_avg_sq = torch.zeros((P, 6), device=dev)
        self.step_t = torch.zeros((P,), dtype=torch.int32, device=dev)
        self.hist_row = torch.full((P,), int(model.history_cursor()), dtype=torch.int32, device=dev)
        self.history = model.history_ops.detach().to(dev)[None].repeat(P, 1, 1).contiguous()
        self.mvp = torch.empty((B, self.L, 4, 4), device=dev)
        self.grad_mvp = torch.empty((B, self.L, 4, 4), device=dev)
        self.tc_jac = torch.empty((P, 7, 16), device=dev)
        self.loss_b = torch.empty((B,), device=dev)
        self.red = torch.empty((P, 8), device=dev)
        self.loss = torch.zeros((P,), device=dev)
        self.grad = torch.zeros((P, 6), device=dev)
        self.mask = None  # [B,H,W], allocated by the first step that asks for masks
        self._init_chain(slack)  # (job slots per VIRTUAL view)

    def _enqueue(self, want_mask, stream=None):
        if stream is None:
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if want_mask and self.mask is None:
            self.mask = torch.empty((self.B, self.H, self.W), device=self.dev)
        sc = self.scene
        # one C call = 4 launches whatever P is: vertex (+ P pose heads), jobs, composite, finish (a workgroup per hypothesis)
        _lib.check(_lib.lib().ehr_solver_step_multi(
            self.glctx.handle, _lib.ptr(sc.verts), _lib.ptr(sc.tris), _lib.ptr(sc.tri_link), _lib.ptr(sc.vert_link),
            _lib.ptr(sc.opp), _lib.ptr(self.K), _lib.ptr(self.link_poses), _lib.ptr(self.ref), self.P, self.Bv, self.L,
            sc.num_verts, sc.num_tris, self.H, self.W, _f(self.near), _f(self.far), _lib.ptr(self.dof),
            _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self.step_t), _lib.ptr(self.history),
            self.history.shape[1], _lib.ptr(self.hist_row), _f(self.lr), _f(self.betas[0]), _f(self.betas[1]), _f(self.eps),
            _f(self.wd), _lib.ptr(self.mvp), _lib.ptr(self.tc_jac), _lib.ptr(self.mask if want_mask else None),
            _lib.ptr(self.loss_b), _lib.ptr(self.grad_mvp), _lib.ptr(self.red), _lib.ptr(self.loss), _lib.ptr(self.grad),
            stream), "ehr_solver_step_multi")

    @property
    def steps_done(self):
        """Effective steps of the hypothesis that has taken most (a frozen hypothesis stops counting; a reported step
        counts for nobody).  Synchronises."""
        return int(self.step_t.max().item())

    def state_dict(self):
        rows = int(self.hist_row.max().item())
        return {"dof": self.dof.cpu().clone(), "exp_avg": self.exp_avg.cpu().clone(), "exp_avg_sq": self.exp_avg_sq.cpu().clone(),
                "step": self.step_t.cpu().clone(), "hist_row": self.hist_row.cpu().clone(),
                "history": self.history[:, :rows].cpu().clone(),
                "param_groups": [{"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.wd}]}

    def load_state_dict(self, sd):
        if tuple(sd["dof"].shape) != (self.P, 6):
            raise ValueError(f"load_state_dict: the state holds {sd['dof'].shape[0]} hypotheses, this solve {self.P}")
        self.dof.copy_(sd["dof"])
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.step_t.copy_(sd["step"])
        self.hist_row.copy_(sd["hist_row"])
        h = sd["history"]
        self.history.zero_()
        self.history[:, :h.shape[1]].copy_(h)


@dataclass
class MultiStartResult:
    dofs: torch.Tensor          # [P,6] final dof of every hypothesis (CPU)
    losses: torch.Tensor        # [P] mean of each hypothesis's last `tail` losses (float64, CPU; NaN: frozen)
    ranking: list               # hypothesis indices, best first (NaN last, ties by index)
    winner: int
    loss_history: torch.Tensor  # [steps,P] loss of every effective step (CPU)
    steps: int
    recoveries: list = field(default_factory=list)


def solve_multistart(cfg, model, batch, starts, num_steps, tail=20, slack=None):
    """Runs ``num_steps`` effective steps of every start from a captured graph, with the recovery loop
    ``RBSolverTrainer.fit`` uses (a reported step is recovered from and run again), ranks the hypotheses by the mean of their
    last ``tail`` losses and writes the winner's pose into ``model.dof`` and its rows into ``model.history_ops`` -- so
    SpaceExplorer and checkpoints see an ordinary solve."""
    ms = MultiStartPoseStep(model, batch, starts, slack=slack, **check_solver_settings(cfg))
    ms.capture()
    hist = ms.take_effective_steps(num_steps, "solve_multistart")
    means = hist[-tail:].double().mean(dim=0) if hist.shape[0] > 0 else torch.full((ms.P,), float("nan"), dtype=torch.float64)
    ranking = rank_losses(means.numpy())
    w = ranking[0]
    with torch.no_grad():
        model.dof.data.copy_(ms.dof[w])
        model.history_ops.copy_(ms.history[w])
    model._hist_n = None
    ms.release_graph()
    return MultiStartResult(dofs=ms.dof.cpu().clone(), losses=means, ranking=ranking, winner=w, loss_history=hist,
                            steps=hist.shape[0], recoveries=list(ms.recoveries))
