"""Cost of one exploration round by information gain (easyhec_amd/info_explorer.py) next to the mask-variance score:
    python tools/info_explorer_bench.py [--candidates 1000] [--reps 20] [--online]
Workload: xArm7, 4 frames at 640x360 (masks rendered at the true pose, the pose perturbed), 1000 candidate joint vectors
~ U(0.9 x limits); pose only (N = 6) and with six free joint offsets (N = 12).  Per N, the median of `--reps` host-clock
windows that end in ONE device synchronise, after 3 warm-up runs, of
    kinematics + linearize | the information op over all chunks | gain + pick, k = 5 | the whole select()
and of the same greedy selection in numpy on the host, the device-to-host copy of the matrices included.  Beside them
`SpaceExplorer.score` of the same candidates under 10 sampled poses.  --online adds, on the online test's problem (120x160,
12 candidates, two invalid), whether the information pick and the variance pick of a round agree.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, sync):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def host_greedy(A, info, k, interest):
    """Greedy log-det selection in numpy float64 (batched slogdet), the contract of the two kernels."""
    N = A.shape[0]
    rest = [i for i in range(N) if i not in interest]

    def m(X):
        ld = np.linalg.slogdet(X)[1]
        return ld - np.linalg.slogdet(X[..., rest, :][..., :, rest])[1] if rest else ld
    A, taken, picked = A.copy(), np.zeros(len(info), dtype=bool), []
    for _ in range(k):
        g = m(A[None] + info) - m(A)
        g[taken] = -np.inf
        q = int(np.argmax(g))
        picked.append(q)
        taken[q] = True
        A = A + info[q]
    return picked


def problem(rb, B, H, W, scale, dev):
    import torch
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    K = scaled_K(XARM7_K_1280x720, scale, W, H, True)
    q, lp = make_views(rb, B, seed=0)
    qp = np.zeros((B, rb.chain.dof))
    qp[:, :q.shape[1]] = q
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=rb.meshes).to(dev)
    m0 = make()
    Kt, lpt = torch.tensor(K, dtype=torch.float32, device=dev), torch.tensor(lp, dtype=torch.float32, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((B, H, W), device=dev))
    return make, {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(B, 1, 1)}, qp, K, Tc


def explorer_times(ex, cand, reps, sync):
    import torch
    from easyhec_amd import fused, information, info_explorer
    out = {"N": ex.N}
    kin = {}

    def kinematics():
        kin["lp"], kin["jf"] = ex.kinematics(cand)
        Q, C = kin["lp"].shape[0], min(ex.chunk, kin["lp"].shape[0])
        kin["lin"] = []
        for lo in range(0, Q, C):  # (a ragged last chunk is padded with its last candidate, as candidate_information does)
            rows = torch.arange(lo, lo + C, device=ex.dev).clamp_(max=Q - 1)
            kin["lin"].append(ex._linearize(kin["lp"][rows].contiguous(), None if kin["jf"] is None else kin["jf"][rows].contiguous(), C))
    out["kinematics + linearize"] = median_ms(kinematics, reps, sync)
    C = min(ex.chunk, len(cand))
    fused._ensure_plan(ex.glctx, ex.scene, C, ex.H, ex.W)
    zero = torch.zeros((C, ex.H, ex.W), device=ex.dev)
    outs = information._outputs(ex.N, C, ex.L, ex.dev, False, False)

    def op():
        for mvp, dmvp in kin["lin"]:
            information._launch(ex.glctx, ex.scene, mvp, dmvp, zero, outs.info, outs.grad, outs.count, None, None)
    out["information op, all chunks"] = dict(median_ms(op, reps, sync), chunks=len(kin["lin"]), chunk_candidates=C)
    info, count = ex.candidate_information(cand)
    A0 = ex.prior_matrix()
    out["gain + pick, k=5"] = median_ms(lambda: info_explorer.greedy_select(A0, info, 5, interest=ex.interest), reps, sync)
    out["select(k=5), whole"] = median_ms(lambda: ex.select(cand, k=5), reps, sync)
    out["prior_matrix (the current frames)"] = median_ms(ex.prior_matrix, reps, sync)
    host = {}

    def on_host():
        host["picked"] = host_greedy(A0.cpu().numpy(), info.cpu().numpy(), 5, ex.interest)
    out["numpy greedy on the host, copy included"] = median_ms(on_host, reps, sync)
    sel = info_explorer.greedy_select(A0, info, 5, interest=ex.interest)
    out["picked"] = sel.picked.cpu().tolist()
    out["gains"] = [round(g, 4) for g in sel.gains.cpu().tolist()]
    out["host picked"] = host["picked"]
    out["candidates with pixels"] = int((count > 0).sum().item())
    return out


def online_agreement(rb, dev):
    """The online test's problem: per exploring round, the index the information explorer asked for and the index the
    variance score of that round's optimisation history would have asked for, on the same candidates."""
    import torch
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    rng = np.random.default_rng(1)
    rounds, asked = [], []

    def capture(qpos):
        asked.append(np.array(qpos))
        return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

    def candidates(_round):
        cand, valid = rb.sample_qpos(12, rng, scale=0.9), np.ones(12, dtype=bool)
        valid[[2, 7]] = False
        var = loop.explorer.forward(cand, loop.model.history_ops.detach().cpu(), start=10, sample=4, valid=valid,
                                    generator=torch.Generator().manual_seed(0))
        rounds.append({"cand": cand, "variance_pick": int(var["qpos_idx"])})
        return cand, valid

    loop = OnlineCalibration(rb, K, H, W, perturb_pose(Tc_gt), capture, candidates, num_epochs=60, explore_iters=4,
                             explore="information", device=dev)
    loop.fit(np.zeros(7))
    out = []
    for r, a in zip(rounds, asked[1:]):
        i = int(np.flatnonzero((r["cand"] == a).all(axis=1))[0])
        out.append({"information_pick": i, "variance_pick": r["variance_pick"], "agree": i == r["variance_pick"]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--online", action="store_true")
    a = ap.parse_args()
    import torch
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.info_explorer import InformationExplorer
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.robot import load_robot
    from easyhec_amd.space_explorer import SpaceExplorer
    from easyhec_amd.synthetic import perturb_pose
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rb = load_robot("xarm7")
    H, W, B = 360, 640, 4
    make, batch, qp, K, Tc = problem(rb, B, H, W, 0.5, dev)
    cand = rb.sample_qpos(a.candidates, np.random.default_rng(0), scale=0.9)
    res = {"workload": f"xArm7, {B} frames {W}x{H}, {a.candidates} candidates, median of {a.reps}"}
    res["pose only"] = explorer_times(InformationExplorer(FusedPoseStep(make(), batch), robot=rb), cand, a.reps, sync)
    res["pose + six offsets"] = explorer_times(InformationExplorer(JointPoseStep(make(), batch, rb, qp)), cand, a.reps, sync)
    se = SpaceExplorer(rb, K, H, W, device=dev)
    rng = np.random.default_rng(1)
    poses = np.stack([perturb_pose(Tc, dt=rng.normal(0, 0.02, 3), drot_deg=rng.normal(0, 2.0, 3)) for _ in range(10)])
    res["SpaceExplorer.score, sample=10"] = median_ms(lambda: se.score(cand, poses), a.reps, sync)
    res["SpaceExplorer pick"] = int(se.score(cand, poses).argmax().item())
    if a.online:
        res["online rounds"] = online_agreement(rb, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
