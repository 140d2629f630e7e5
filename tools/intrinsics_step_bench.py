"""Cost of the intrinsics launch per step: IntrinsicsPoseStep against FusedPoseStep, eager launches:
    python tools/intrinsics_step_bench.py [--parent-lib PATH] [--reps 3] [--steps 200] [--windows 5] [--warmup 50]
Workload: xArm7, 8 views 1280x720 (the flagship shape of bench.py), masks rendered at the true pose, the pose perturbed.
    pose        one FusedPoseStep.step(): the three-launch chain
    intrinsics  one IntrinsicsPoseStep.step() with free=("f",): the same chain, then ONE ehr_intrinsics_backward_adam
Every figure is a host clock around `--steps` eager steps that end in a device synchronise, after `--warmup` steps, `--windows`
windows per process.  A process per variant, the variants alternating `--reps` times, so that drift of the machine shows as
spread.  --parent-lib: a libehr_hip.so built from the parent commit's easyhec_amd/csrc (loaded through EHR_LIB; it has no
intrinsics kernel, so it runs `pose` only); without it `pose` runs on this tree's library alone, whose chain is the parent's
source byte for byte.  Prints one JSON line per process."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(robot, B=8, H=720, W=1280):
    import torch
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    K = scaled_K(XARM7_K_1280x720, 1.0, W, H, False)
    _, lp = make_views(robot, B, seed=0)
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    model = RBSolver(cfg, meshes=robot.meshes).to(dev)
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lpt = torch.tensor(lp, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(model._ensure_renderer().glctx, model._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((B, H, W), device=dev))
    return cfg, model, {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(B, 1, 1)}


def child(a):
    from easyhec_amd import _lib
    if os.environ.get("EHR_LIB"):
        _lib.SIGNATURES.pop("ehr_intrinsics_backward_adam")   # the parent's library predates it
    import torch
    from easyhec_amd.robot import load_robot
    cfg, model, batch = problem(load_robot("xarm7"))
    kw = dict(lr=cfg.solver.max_lr, weight_decay=cfg.solver.weight_decay)
    if a.mode == "intrinsics":
        from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep
        step = IntrinsicsPoseStep(model, batch, **kw).step
    else:
        from easyhec_amd.fast import FusedPoseStep
        step = FusedPoseStep(model, batch, **kw).step
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
    ap.add_argument("--mode", choices=["pose", "intrinsics"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    if a.mode:
        child(a)
        sys.exit(0)
    variants = [("intrinsics", None), ("pose", None)] + ([("pose", os.path.abspath(a.parent_lib))] if a.parent_lib else [])
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
