"""Stage timings of the solver step (the chain bench.py times) on a bench workload, without the CPU baseline:
    [EHR_LIB=ab/libehr_x.so] python tools/step_bench.py [workload] [steps] [--weight] [--joints]
--joints: the step of easyhec_amd.joint_calib.JointPoseStep (the same chain between ehr_joint_forward and
ehr_joint_backward_adam, arm joints 1..6 free); the stage timings are the chain's, the two extra launches show in us/step.
--weight: the same step with per-pixel weights bound (ehr_fused_bind_weight; uniform in [0, 2], a fifth of them zero): the
composite stage then runs its weighted instantiation."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import time
import torch
import bench
from easyhec_amd import fused
weighted = "--weight" in sys.argv
joints = "--joints" in sys.argv
args = [a for a in sys.argv[1:] if a not in ("--weight", "--joints")]
wl = args[0] if len(args) > 0 else bench.WORKLOAD
steps = int(args[1]) if len(args) > 1 else 200
dev = torch.device("cuda", 0)
p = bench.build_problem(0, 1, dev, graph=False, workload=wl)
tr = p["trainer"]
if weighted:
    g = torch.Generator(device="cpu").manual_seed(0)
    w = torch.rand(tuple(tr.fast.ref.shape), generator=g) * 2
    w[torch.rand(tuple(w.shape), generator=g) < 0.2] = 0
    tr.fast.weight = w.to(dev).contiguous()
    tr.fast._plan_and_bind()  # weights, then the reference (its cached sums are sums of w ref^2)
if joints:
    import numpy as np
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.robot import load_robot
    from easyhec_amd.synthetic import WORKLOADS, make_views
    rb = load_robot(WORKLOADS[wl]["robot"])
    f = tr.fast
    q, lp = make_views(rb, f.B, seed=0)  # (bench.build_problem's views: the same link poses, now from the device's kinematics)
    assert np.abs(lp - f.link_poses.cpu().numpy()).max() <= 1e-6, "bench views are not make_views(seed=0)"
    batch = {"mask": f.ref, "link_poses": f.link_poses, "K": f.K[None].repeat(f.B, 1, 1)}
    tr.fast = JointPoseStep(tr.model, batch, rb, q, lr=f.lr, weight_decay=f.wd)
for _ in range(20):
    tr.step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    tr.step()
torch.cuda.synchronize()
el = time.perf_counter() - t0
fused.check_status(p["glctx"])
fused.set_timing(p["glctx"], True)
for _ in range(steps):
    tr.step()
ms, n = fused.read_timing(p["glctx"])
print(os.environ.get("EHR_LIB", "default"), wl, "weighted" if weighted else "unweighted", "joints" if joints else "pose-only", f"{el / steps * 1e6:.1f} us/step {p['n_views'] * steps / el:.0f} frames/s",
      {k: round(v / n * 1e3, 1) for k, v in ms.items() if not k.startswith("unused")}, "loss", float(tr.last_loss), flush=True)
