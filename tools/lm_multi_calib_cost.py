"""Cost of the multi-start Levenberg-Marquardt solve with joint offsets and intrinsics per hypothesis (easyhec_amd/lm_multi.py,
DESIGN.md section 6q) next to P sequential solo solves; the figures of profiles/lm_multi_calib.md:
    python tools/lm_multi_calib_cost.py [--iters 20] [--rounds 5] [--out FILE.json] [--skip-timing] [--skip-demo]
Prints one JSON line per measurement:

* timing: two scenes, xArm7: 8 views 1280x720 (the flagship shape of bench.py) and 2 views 120x160; P in {1, 4, 16}; layout
  "6 offsets + f" (the default free joints 1..6 and the tied focal length: N = 13); the starts are sample_starts around the
  scene's start pose.  Milliseconds per ``MultiStartLM.iterate(1)`` of all P hypotheses against P sequential
  ``LevenbergMarquardt.iterate(1)`` on P ``JointIntrinsicsPoseStep`` objects (each on a solver and a context of its own) in one
  process -- a host clock around ``--iters`` iterations that end in ONE device synchronise, after 2 warm-up iterations, the
  two forms ALTERNATING for ``--rounds`` rounds; median, min and max.  ftol = 0 and lambda_max = 1e300, so that nobody stops
  by those rules during the timed iterations.  Also: whether every hypothesis's state block still equals its solo solve's.
* demo: the demonstration problem of tests/test_gpu_lm_multi_calib.py -- ``soft_problem`` (2 views 120x160, zoom 2) seen
  through encoders whose joint 1 reads one degree low and a focal length given 2 % short; ``solve_global_lm`` with Q = 16,
  P = 3, free joints 1 and 3 and the tied focal length under the default prior -- the recovered offset, focal and pose errors
  of the winner and of hypothesis 0 (the plain solve), for ``--demo-iters`` iterations."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES = (("8 x 1280x720", 8, 720, 1280, 1.0), ("2 x 120x160", 2, 120, 160, 0.125))


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--demo-iters", type=int, nargs="+", default=[12, 50])
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--skip-demo", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from easyhec_amd import lm, lm_multi
    from easyhec_amd.intrinsics_calib import JointIntrinsicsPoseStep
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.robot import load_robot
    from easyhec_amd.se3 import se3_exp_map
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose
    from test_gpu_fast import problem

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / a.iters

    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    xarm7 = load_robot("xarm7")
    dev = torch.device("cuda:0")
    for name, Bv, H, W, scale in (() if a.skip_timing else SCENES):
        cfg, make, batch = problem(xarm7, Bv, H, W, scale)
        q, _ = make_views(xarm7, Bv, seed=0)
        Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
        for P in (1, 4, 16):
            starts = sample_starts(Tc_init, P, 0.002, 0.3, seed=2)
            kw = dict(ftol=0.0, lambda_max=1e300)
            ms = lm_multi.MultiStartLM(make(), batch, starts, robot=xarm7, qpos=q, free_intrinsics=("f",), **kw)
            solos = []
            for p in range(P):
                cfg.model.rbsolver.init_Tc_c2b = np.asarray(starts[p]).tolist()
                solos.append(lm.LevenbergMarquardt(JointIntrinsicsPoseStep(make(), batch, xarm7, q, free_intrinsics=("f",)), **kw))
            cfg.model.rbsolver.init_Tc_c2b = Tc_init.tolist()
            ms.iterate(2)
            for o in solos:
                o.iterate(2)
            tb, ts = [], []
            for _ in range(a.rounds):
                tb.append(timed(lambda: ms.iterate(a.iters)))
                ts.append(timed(lambda: [o.iterate(a.iters) for o in solos]))
            S = ms.state()
            equal = all(ms.state_block[p].cpu().numpy().tobytes() == solos[p].state_block.cpu().numpy().tobytes()
                        for p in range(P))
            emit({"what": "timing", "scene": name, "layout": ms.names[6:], "N": ms.N, "P": P, "batched_ms": stats(tb),
                  "sequential_ms": stats(ts), "sequential_over_batched": round(statistics.median(ts) / statistics.median(tb), 3),
                  "done": sum(s.done for s in S), "reported": sum(s.reported for s in S), "state_blocks_equal_solo": equal,
                  "memory_bytes": ms.memory_bytes()})
            del ms, solos
            torch.cuda.empty_cache()
    if not a.skip_demo:
        from test_gpu_lm import soft_problem
        make, batch, qp = soft_problem(xarm7)
        qbad = qp.copy()
        qbad[:, 1] -= np.radians(1.0)
        Kbad = batch["K"].clone()
        Kbad[:, 0, 0] /= 1.02
        Kbad[:, 1, 1] /= 1.02
        seen = dict(batch, K=Kbad, link_poses=torch.from_numpy(xarm7.link_poses_batch(qbad)).float().to(dev))
        Tc_true = camera_Tc_c2b()
        Tc_init = perturb_pose(Tc_true)
        f_true = batch["K"][0, 0, 0].item()

        def errors(res, p):
            Tc = se3_exp_map(res.dofs[p].double()[None]).permute(0, 2, 1)[0].numpy()
            D = np.linalg.inv(Tc_true) @ Tc
            rot = np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1)))
            return {"hypothesis": int(p), "loss": round(float(res.losses[p]), 4), "iterations": res.iterations[p], "why": res.why[p],
                    "offset1_deg": round(float(np.degrees(res.offsets[p][1].item())), 4),
                    "offset3_deg": round(float(np.degrees(res.offsets[p][3].item())), 4),
                    "focal_error_percent": round(100 * (res.Ks[p][0, 0].item() / f_true - 1), 4),
                    "pose_error_mm": round(1e3 * float(np.linalg.norm(D[:3, 3])), 3), "pose_error_deg": round(float(rot), 4)}

        D0 = np.linalg.inv(Tc_true) @ Tc_init
        for iters in a.demo_iters:
            torch.cuda.synchronize()
            t = time.perf_counter()
            _, res = lm_multi.solve_global_lm(make(), seen, Tc_init, 16, 3, max_iters=iters, robot=xarm7, qpos=qbad, free=[1, 3],
                                              free_intrinsics=("f",), prior_sigma="default", sigma2=0.05)
            torch.cuda.synchronize()
            emit({"what": "demo", "max_iters": iters, "planted": {"offset1_deg": 1.0, "offset3_deg": 0.0, "focal_error_percent":
                  round(100 * (1 / 1.02 - 1), 4), "pose_error_mm": round(1e3 * float(np.linalg.norm(D0[:3, 3])), 3)},
                  "winner": errors(res, res.winner), "plain": errors(res, 0), "losses": [round(x, 3) for x in res.losses.tolist()],
                  "basins": res.basins, "wall_ms": round(1e3 * (time.perf_counter() - t), 1)})
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
