"""The online calibration loop of /root/reference/easyhec/trainer/rbsolve_iter.py:157-167 (``fit``) with the hardware
replaced by callbacks: per exploration round ``capture_data`` (robot + camera + segmentation -> one more (mask, qpos)
frame), ``rebuild`` (a fresh RBSolver from the configured initial pose over ALL frames so far, rbsolve_iter.py:277-285),
``do_fit`` (``num_epochs`` Adam iterations -- one ``ehr_solver_step`` launch chain each), ``explore_next_state``
(space_explorer.py:87-96,152-185: sample camera poses from this round's optimisation history, score the candidate joint
configurations by summed mask variance -- one ``ehr_mask_variance`` call --, move to the best; or, with
``explore="information"``, by the information gain of easyhec_amd/info_explorer.py).

Robot drivers, RealSense capture, PointRend / SAM segmentation and motion planning are the parts of the reference that
stay outside this package; they enter as ``capture`` and ``candidates`` callables."""
import time

import numpy as np
import torch

from .config import Cfg
from .info_explorer import InformationExplorer
from .rb_solver import RBSolver
from .space_explorer import SpaceExplorer
from .trainer import RBSolverTrainer

__all__ = ["OnlineCalibration"]


class OnlineCalibration:
    def __init__(self, robot, K, H, W, init_Tc_c2b, capture, candidates, device="cuda:0", num_epochs=1000,
                 explore_iters=5, sample=10, start=200, lr=0.003, seed=0, explore="variance", feasible=None):
        """capture(qpos) -> bool/float mask [H,W] of the robot as the camera sees it at that joint configuration;
        candidates(round) -> (qposes [Q,dof], valid [Q] bool or None): the joint configurations the planner would
        accept this round (space_explorer.py:98-150 decides that with pymp / SAPIEN in the reference).
        explore: "variance" (the reference's mask-variance score, ``SpaceExplorer``) or "information" (the log-det information
        gain of :class:`easyhec_amd.info_explorer.InformationExplorer`, built each round on that round's solve; it needs no
        optimisation history, so ``sample`` and ``start`` are not used).
        feasible: a :class:`easyhec_amd.feasibility.FeasibilityFilter`, or None.  With a filter, the callback's ``valid`` is
        AND-ed with the filter's verdict on the candidates and on the straight joint-space segment from the last captured
        configuration to each (``feasible.path_steps`` configurations, 1 by default), and the round's log record gains
        ``rejected_self`` / ``rejected_env`` / ``rejected_reach``, the candidates each test turned down (and, for a filter
        built with ``exact=True``, ``rejected_mode = "exact"``: the meshes turned them down, not the proxies).  A filter built
        with ``swept=True`` judges the WHOLE segment instead (``check_swept``): the record then has ``rejected_mode = "swept"``
        and ``undecided``, the candidates the certificate's budget could not decide (they count as turned down).  A filter built
        with ``detour_hops >= 2`` replaces a move that is turned down by a detour over the other candidates (``plan``): a
        candidate is valid if a path of certified moves reaches it; the ``rejected_*`` and ``undecided`` counts stay those of
        the direct moves, ``rejected_mode`` is ``"roadmap"``, ``detours`` counts the candidates only a detour reaches,
        ``roadmap_edges`` the edges searched, and ``hops`` and ``path`` (the waypoints, lists of joint values, the current
        configuration first) describe the way to the chosen candidate.  When it turns all of
        them down, the explorers' "no valid qpos found" error is what the caller sees."""
        if explore not in ("variance", "information"):
            raise ValueError(f"explore={explore!r}: 'variance' or 'information'")
        self.explore, self.feasible = explore, feasible
        self.robot, self.K, self.H, self.W = robot, np.asarray(K, dtype=np.float64), int(H), int(W)
        self.init_Tc_c2b = np.asarray(init_Tc_c2b, dtype=np.float64)
        self.capture, self.candidates = capture, candidates
        self.device = torch.device(device)
        self.num_epochs, self.explore_iters, self.sample, self.start, self.lr = num_epochs, explore_iters, sample, start, lr
        self.gen = torch.Generator().manual_seed(seed)
        self.explorer = SpaceExplorer(robot, self.K, self.H, self.W, device=self.device)
        self.qposes, self.masks = [], []
        self.model = None
        self.log = []

    def _batch(self):
        lp = np.stack([self.robot.link_poses(q) for q in self.qposes]).astype(np.float32)
        n = len(self.qposes)
        return {"mask": torch.as_tensor(np.stack(self.masks), dtype=torch.float32, device=self.device),
                "link_poses": torch.as_tensor(lp, device=self.device),
                "K": torch.as_tensor(self.K, dtype=torch.float32, device=self.device)[None].repeat(n, 1, 1)}

    def fit(self, first_qpos):
        """Returns the final Tc_c2b [4,4] (numpy).  ``self.log`` holds one record per exploration round."""
        qpos = np.asarray(first_qpos, dtype=np.float64)
        for it in range(self.explore_iters):
            t0 = time.perf_counter()
            self.qposes.append(qpos)                                      # capture_data (rbsolve_iter.py:169-262)
            self.masks.append(np.asarray(self.capture(qpos), dtype=np.float32))
            cfg = Cfg()                                                   # rebuild (rbsolve_iter.py:277-285)
            cfg.model.rbsolver.H, cfg.model.rbsolver.W = self.H, self.W
            cfg.model.rbsolver.init_Tc_c2b = self.init_Tc_c2b.tolist()
            cfg.solver.max_lr = self.lr
            self.model = RBSolver(cfg, meshes=self.robot.meshes).to(self.device)
            trainer = RBSolverTrainer(cfg, self.model, self._batch(), fast=True)
            # do_fit (rbsolve_iter.py:139-155): exactly num_epochs effective steps -- a step the chain reports instead of
            # taking (a close-up view the slot-limited plan cannot hold) is recovered from and run again by fit()
            trainer.fit(self.num_epochs)
            loss = trainer.last_loss
            torch.cuda.synchronize(self.device)
            if not np.isfinite(float(loss)):
                raise RuntimeError(f"round {it}: the solve ended on a reported step (mask_loss NaN)")
            t1 = time.perf_counter()
            rec = {"round": it, "frames": len(self.qposes), "mask_loss": float(loss), "solve_s": t1 - t0}
            if it + 1 < self.explore_iters:                               # explore_next_state (rbsolve_iter.py:263-275)
                cand, valid = self.candidates(it)
                rejected = {}
                if self.feasible is not None:
                    swept = getattr(self.feasible, "swept", False)
                    roadmap = self.feasible.plan(cand, qpos) if getattr(self.feasible, "detour_hops", 0) >= 2 else None
                    if roadmap is not None:                               # a path of certified moves, not the direct one alone
                        fc = roadmap.direct
                    elif swept:
                        fc = self.feasible.check_swept(cand, qpos)
                    else:
                        fc = self.feasible.check(cand, current_qpos=qpos, path_steps=self.feasible.path_steps or 1)
                    ok = (fc.valid if roadmap is None else roadmap.reachable).cpu().numpy()
                    valid = ok if valid is None else (np.asarray(valid.cpu() if torch.is_tensor(valid) else valid) != 0) & ok
                    rejected = {f"rejected_{k}": int((~getattr(fc, f"{k}_ok")).sum()) for k in ("self", "env", "reach")}
                    if getattr(self.feasible, "exact", False):            # (a proxy filter's record keeps today's keys)
                        rejected["rejected_mode"] = "exact"
                    if swept:                                             # the whole segment, certified or turned down
                        rejected["rejected_mode"] = "swept"
                        rejected["undecided"] = int((fc.status >= 2).sum())
                    if roadmap is not None:
                        rejected.update(rejected_mode="roadmap", detours=int(roadmap.detour.sum()),
                                        roadmap_edges=int((roadmap.edges[:, 0] >= 0).sum()))
                if self.explore == "information":
                    out = InformationExplorer(trainer.fast, robot=self.robot).forward(cand, valid=valid)
                    scores = {"info_gain": float(out["gain"]), "gain_mean": float(out["gain_mean"])}
                else:
                    out = self.explorer.forward(cand, self.model.history_ops.detach().cpu(), start=self.start,
                                                sample=self.sample, valid=valid, generator=self.gen)
                    scores = {"variance": float(out["variance"]), "var_mean": float(out["var_mean"])}
                torch.cuda.synchronize(self.device)
                qpos = np.asarray(out["qpos"], dtype=np.float64)
                if self.feasible is not None and roadmap is not None:      # how the arm gets there: the path's corners
                    i = int(out["qpos_idx"])
                    h = int(roadmap.hops[i])
                    rejected.update(hops=h, path=roadmap.waypoints[i, :h + 1].cpu().numpy().tolist())
                rec.update(explore_s=time.perf_counter() - t1, **scores, candidates=int(len(cand)), **rejected)
            self.log.append(rec)
        return self.model.Tc_c2b().detach().cpu().numpy()
