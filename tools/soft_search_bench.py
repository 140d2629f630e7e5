"""The soft pose search against the overlap search it extends (profiles/soft_search.md):
    python tools/soft_search_bench.py [--Q 1000] [--S 10] [--cap 320] [--calls 12] [--warmup 2] [--out FILE.json]

xArm7 at 1280x720: Q candidate camera poses (sample_starts around a perturbed pose, the draw of pose_search_bench.py)
seen in S real views, the observed masks the ground-truth pose's own renders.  Legs on the SAME [Q,S,L,4,4] matrices:
  overlap    one ehr_mask_overlap call                      (pose_search.mask_overlap)
  distance   one ehr_mask_distance call, cap_px = --cap     (pose_search.mask_distance)
  costs      the torch expression that turns d2 into the cost images [fg, k]   (pose_search.soft_costs)
  cost       one ehr_mask_cost call with those C = 2 images (pose_search.mask_cost)
The legs alternate; each call is timed with device events around the whole call and a synchronisation after it (the way
pose_search_bench.py times), every leg is warmed first, and the value is the median over the calls.  soft = distance +
costs + cost is what search_starts(score="soft") adds up to on the device; soft_over_overlap is its ratio to overlap."""
import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--Q", type=int, default=1000)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--cap", type=int, default=320)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("soft_search_bench needs a HIP device: a timing taken anywhere else says nothing")
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
    d2 = pose_search.mask_distance(ctx, ref, a.cap)
    cost = pose_search.soft_costs(d2, a.cap)

    legs = {"overlap": lambda: pose_search.mask_overlap(ctx, scene, mvp, ref),
            "distance": lambda: pose_search.mask_distance(ctx, ref, a.cap),
            "costs": lambda: pose_search.soft_costs(d2, a.cap),
            "cost": lambda: pose_search.mask_cost(ctx, scene, mvp, cost)}
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    times = {k: [] for k in legs}
    for _ in range(a.calls):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    inter, area, ref_area = legs["overlap"]()
    area_c, sums = legs["cost"]()
    assert torch.equal(area_c, area) and torch.equal(sums[..., 0], inter), "ehr_mask_cost and ehr_mask_overlap disagree"
    soft = pose_search.soft_iou_scores(area, inter, sums[..., 1], ref_area, a.cap)
    renders = a.Q * a.S
    out = {"Q": a.Q, "S": a.S, "H": H, "W": W, "cap_px": a.cap, "C": 2, "renders_per_call": renders, "calls": a.calls,
           "device": torch.cuda.get_device_name(0)}
    for k, t in times.items():
        med = statistics.median(t)
        out[k] = {"median_s": med, "min_s": min(t), "max_s": max(t)}
    out["soft_s"] = out["distance"]["median_s"] + out["costs"]["median_s"] + out["cost"]["median_s"]
    out["soft_over_overlap"] = out["soft_s"] / out["overlap"]["median_s"]
    out["cost_over_overlap"] = out["cost"]["median_s"] / out["overlap"]["median_s"]
    out["best_candidate"] = int(torch.argmax(soft))
    out["best_soft"] = float(soft.max())
    out["covered_fraction"] = float(area.double().mean()) / (H * W)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
