"""Everything the five steppers compute on one small scene, written out for a byte-for-byte comparison between two builds:
    python tools/calib_dump.py --out DIR
Scene: xArm7, 2 views 160x120 (the calibration tests' `problem(xarm7, 2, 120, 160, 0.125)`), masks rendered at the true pose,
the pose perturbed.  FusedPoseStep, JointPoseStep (joints 1..6 free), IntrinsicsPoseStep (free=("f","cx")),
JointIntrinsicsPoseStep (both) and a two-camera RigJointStep each take 32 eager steps and then 32 steps replayed from the
captured graph (the rig has no graph: 64 eager steps).  Per stepper DIR gets `<name>.<what>.npy` -- the loss of every step, the
final dof, offsets, theta, K, every moment and counter, every tensor of the state dict -- and `<name>.state_dict.json` with the
rest of the state dict.  Only public classes and attributes are used, so the same file runs on an older commit's tree; two runs
agree when `diff -r` of their DIRs is empty."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ATTRS = ("offsets", "offset_exp_avg", "offset_exp_avg_sq", "offset_step_t", "offset_grad", "theta", "theta_exp_avg",
         "theta_exp_avg_sq", "theta_step_t", "theta_grad", "K", "K0", "exp_avg", "exp_avg_sq", "step_t", "grad", "link_poses",
         "joint_frames")


def problem(robot, B=2, H=120, W=160, scale=0.125):
    from easyhec_amd import fused
    from easyhec_amd.config import XARM7_K_1280x720, Cfg
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K
    dev = torch.device("cuda:0")
    K = scaled_K(XARM7_K_1280x720, scale, W, H, True)
    q, lp = make_views(robot, B, seed=0)
    qp = np.zeros((B, robot.chain.dof))
    qp[:, :q.shape[1]] = q
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=robot.meshes).to(dev)
    m0 = make()
    Kt = torch.tensor(K, dtype=torch.float32, device=dev)
    lpt = torch.tensor(lp, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((B, H, W), device=dev))
    return make, {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(B, 1, 1)}, qp


def flatten(x, path, arrays):
    """Tensors of a state dict into ``arrays[path]``; returns the JSON-able rest."""
    if torch.is_tensor(x):
        arrays[path] = x
        return f"<{path}.npy>"
    if isinstance(x, dict):
        return {str(k): flatten(v, f"{path}.{k}", arrays) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [flatten(v, f"{path}.{i}", arrays) for i, v in enumerate(x)]
    return x


def dump(out, name, step, models, eager, replayed):
    losses = [step.step().clone() for _ in range(eager)]
    if replayed:
        step.capture()
        losses += [step.step().clone() for _ in range(replayed)]
    torch.cuda.synchronize()
    if replayed:
        step.release_graph()
    arrays = {"loss": torch.stack(losses), "dof": torch.stack([m.dof.detach() for m in models]),
              "history": torch.stack([m.history_ops[:eager + replayed + 1] for m in models])}
    for who, obj in [("", step)] + [(f"camera{c}.", cam) for c, cam in enumerate(getattr(step, "cameras", []))]:
        for a in ATTRS:
            if torch.is_tensor(getattr(obj, a, None)):
                arrays[who + a] = getattr(obj, a)
    rest = flatten(step.state_dict(), "state_dict", arrays)
    for k, t in arrays.items():
        np.save(os.path.join(out, f"{name}.{k}.npy"), t.detach().cpu().numpy())
    with open(os.path.join(out, f"{name}.state_dict.json"), "w") as f:
        json.dump(rest, f, indent=1, sort_keys=True)
    print(f"{name}: {len(arrays)} arrays, last loss {losses[-1].tolist()}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--steps", type=int, default=32, help="eager steps, and as many replayed ones")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.intrinsics_calib import IntrinsicsPoseStep, JointIntrinsicsPoseStep
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.rig_calib import RigJointStep
    from easyhec_amd.robot import load_robot
    robot = load_robot("xarm7")
    make, batch, qp = problem(robot)
    free_j, free_i, n = [1, 2, 3, 4, 5, 6], ("f", "cx"), a.steps
    m = make()
    dump(a.out, "pose", FusedPoseStep(m, batch), [m], n, n)
    m = make()
    dump(a.out, "joint", JointPoseStep(m, batch, robot, qp, free=free_j), [m], n, n)
    m = make()
    dump(a.out, "intrinsics", IntrinsicsPoseStep(m, batch, free=free_i), [m], n, n)
    m = make()
    dump(a.out, "joint_intrinsics", JointIntrinsicsPoseStep(m, batch, robot, qp, free=free_j, free_intrinsics=free_i), [m], n, n)
    ms = [make(), make()]
    dump(a.out, "rig", RigJointStep(ms, [batch, batch], robot, [qp, qp], free=free_j), ms, 2 * n, 0)
