"""Pose search against the scoring op it shares its render with (profiles/pose_search.md):
    python tools/pose_search_bench.py [--Q 4096] [--S 8] [--calls 12] [--warmup 2] [--out FILE.json]

xArm7 at 1280x720: Q candidate camera poses (sample_starts around a perturbed pose) seen in S real views.  Two legs on the
SAME [Q,S,L,4,4] matrices, hence the same Q x S renders through the same vertex and job kernels:
  overlap   one ehr_mask_overlap call   (pose_search.mask_overlap: integers against the S observed masks)
  variance  one ehr_mask_variance call  (space_explorer.mask_variance: the variance count over the S renders)
The legs alternate; each call is timed with device events around the whole call (both synchronise inside), every leg is
warmed first, and the value is the median over the calls.  Under `rocprofv3 --kernel-trace --stats` the per-kernel
averages give the count stages' shares."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyhec_amd import dr, fused, pose_search, space_explorer  # noqa: E402
from easyhec_amd.config import XARM7_K_1280x720  # noqa: E402
from easyhec_amd.multistart import sample_starts  # noqa: E402
from easyhec_amd.robot import load_robot  # noqa: E402
from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K  # noqa: E402

H, W = 720, 1280


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Q", type=int, default=4096)
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_search_bench needs a HIP device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    rb = load_robot("xarm7")
    ctx = dr.RasterizeCudaContext(dev)
    scene = fused.LinkScene([v for v, _ in rb.meshes], [f for _, f in rb.meshes], dev)
    K = torch.tensor(scaled_K(XARM7_K_1280x720, 1.0, W, H, False), dtype=torch.float32, device=dev)
    _, lp = make_views(rb, a.S, seed=0)
    lp = torch.tensor(lp, device=dev)
    Tc = camera_Tc_c2b()
    cands = sample_starts(perturb_pose(Tc), a.Q, 0.03, 4.0, seed=0)
    mvp = pose_search.candidate_mvps(K, H, W, torch.tensor(cands, dtype=torch.float32, device=dev), lp).contiguous()
    mvp_gt = pose_search.candidate_mvps(K, H, W, torch.tensor(Tc[None], dtype=torch.float32, device=dev), lp)[0]
    _, _, counts = space_explorer.mask_variance(ctx, scene, mvp_gt[:, None].contiguous(), H, W, return_counts=True)
    ref = counts.float()

    legs = {"overlap": lambda: pose_search.mask_overlap(ctx, scene, mvp, ref),
            "variance": lambda: space_explorer.mask_variance(ctx, scene, mvp, H, W)}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(a.calls):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    inter, area, ref_area = legs["overlap"]()
    xor, iou = pose_search.overlap_scores(inter, area, ref_area)
    renders = a.Q * a.S
    out = {"Q": a.Q, "S": a.S, "H": H, "W": W, "renders_per_call": renders, "calls": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"median_s": med, "min_s": min(t), "max_s": max(t), "renders_per_s": renders / med}
    out["overlap_over_variance"] = out["overlap"]["median_s"] / out["variance"]["median_s"]
    out["best_candidate"] = int(torch.argmin(xor))
    out["best_iou"] = float(iou[int(torch.argmin(xor))])
    out["covered_fraction"] = float(area.double().mean()) / (H * W)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
