"""Step time of the camera rig (easyhec_amd/rig_calib.py) against two separate JointPoseStep steps, eager launches:
    python tools/rig_step_bench.py [--parent-lib PATH] [--reps 3] [--steps 400] [--windows 5] [--warmup 100]
Workload: xArm7, 2 cameras x 4 views 320x240 (azimuth 20 and 110 degrees), joint zero errors of +2, -1.5, +2, -2 degrees on
joints 1, 2, 3, 5 rendered into the masks, both poses perturbed, joints 1..6 free.
    rig   one RigJointStep.step(): per camera the forward kernel and the chain, then ONE ehr_rig_backward_adam
    pair  JointPoseStep.step() of camera A, then of camera B: two forward kernels, two chains, two ehr_joint_backward_adam
Every figure is a host clock around `--steps` eager steps that end in a device synchronise, after `--warmup` steps, `--windows`
windows per process.  A process per variant, the variants alternating `--reps` times, so that drift of the machine shows as
spread.  --parent-lib: a libehr_hip.so built from the parent commit's easyhec_amd/csrc (loaded through EHR_LIB; it has no rig
kernel, so it runs `pair` only); without it `pair` runs on this tree's library alone.  Prints one JSON line per process."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera(robot, truth, theta_deg, seed, H=240, W=320, B=4):
    import numpy as np
    import torch
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    K = scaled_K(XARM7_K_1280x720, 0.25, W, H, True)
    q, _ = make_views(robot, B, seed=seed)
    qp = np.zeros((B, robot.chain.dof))
    qp[:, :q.shape[1]] = q
    Tc = camera_Tc_c2b(theta_deg=theta_deg)
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    model = RBSolver(cfg, meshes=robot.meshes).to(dev)
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lp_true = torch.tensor(robot.link_poses_batch(qp + truth[None]), dtype=torch.float32, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(model._ensure_renderer().glctx, model._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lp_true), torch.zeros((B, H, W), device=dev))
    batch = {"mask": (gt > 0.5).float(), "K": Kt[None].repeat(B, 1, 1),
             "link_poses": torch.tensor(robot.link_poses_batch(qp), dtype=torch.float32, device=dev)}
    return cfg, model, batch, qp


def child(a):
    from easyhec_amd import _lib
    if os.environ.get("EHR_LIB"):
        _lib.SIGNATURES.pop("ehr_rig_backward_adam")   # the parent's library predates it
    import numpy as np
    import torch
    from easyhec_amd.robot import load_robot
    robot = load_robot("xarm7")
    truth = np.zeros(robot.chain.dof)
    truth[[1, 2, 3, 5]] = np.radians([2.0, -1.5, 2.0, -2.0])
    (cfg, ma, ba, qa), (_, mb, bb, qb) = camera(robot, truth, 20.0, 0), camera(robot, truth, 110.0, 1)
    kw = dict(lr=cfg.solver.max_lr, weight_decay=cfg.solver.weight_decay)
    if a.mode == "rig":
        from easyhec_amd.rig_calib import RigJointStep
        step = RigJointStep([ma, mb], [ba, bb], robot, [qa, qb], **kw).step
    else:
        from easyhec_amd.joint_calib import JointPoseStep
        ja, jb = JointPoseStep(ma, ba, robot, qa, **kw), JointPoseStep(mb, bb, robot, qb, **kw)

        def step():
            ja.step()
            jb.step()
    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    us = []
    for _ in range(a.windows):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        us.append(round((time.perf_counter() - t0) / a.steps * 1e6, 1))
    print(json.dumps({"mode": a.mode, "lib": "parent" if os.environ.get("EHR_LIB") else "this tree", "us_per_step": us}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["rig", "pair"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=100)
    a = ap.parse_args()
    if a.mode:
        child(a)
        sys.exit(0)
    variants = [("rig", None), ("pair", None)] + ([("pair", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
    common = ["--steps", str(a.steps), "--windows", str(a.windows), "--warmup", str(a.warmup)]
    for _ in range(a.reps):
        for mode, lib in variants:
            env = dict(os.environ)
            env.pop("EHR_LIB", None)
            if lib:
                env["EHR_LIB"] = lib
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode] + common, env=env, timeout=120).returncode
            if rc != 0:   # (a fault ends the run: nothing more is started on the device)
                sys.exit(rc)
