"""Cost of one ehr_mask_information call next to one ehr_render_mask_loss call:
    python tools/information_cost.py [--calls 50] [--windows 3]
Workload: xArm7, 8 views 1280x720 (the flagship shape of bench.py), masks rendered at the true pose, the pose perturbed,
N = 6 pose tangents and N = 17 (the pose, six joint offsets, five intrinsics-sized random tangents).  Every figure is a host
clock around `--calls` calls that end in a device synchronise, after 10 warm-up calls, `--windows` windows; the best window
is reported beside all of them.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from easyhec_amd import fused, information
    from easyhec_amd.robot import load_robot
    from tools.intrinsics_step_bench import problem
    rb = load_robot("xarm7")
    cfg, model, batch = problem(rb)
    dev = model.dof.device
    ctx, scene = model._ensure_renderer().glctx, model._ensure_scene()
    B, H, W = batch["mask"].shape
    K, lp, ref = batch["K"][0], batch["link_poses"], batch["mask"].contiguous()
    T6 = information.pose_tangents(K, H, W, model.dof.data, lp)
    rng = np.random.default_rng(0)
    extra = torch.from_numpy(rng.normal(size=(11,) + tuple(T6.shape[1:]))) * T6.abs().amax(dim=(0, 3, 4))[None, :, :, None, None]
    D = {6: T6.float().to(dev).contiguous(), 17: torch.cat([T6, extra]).float().to(dev).contiguous()}
    mvp = information._mvp64(information._f64(K), H, W, information._f64(model.dof.data), information._f64(lp), 0.001, 10.0)
    mvp = mvp.float().to(dev).contiguous()
    fused._ensure_plan(ctx, scene, B, H, W)
    loss, grad = torch.empty((B,), device=dev), torch.empty((B, scene.num_links, 4, 4), device=dev)

    def render():
        fused._launch(ctx, scene, mvp, ref, None, loss, grad)

    outs = {n: information._outputs(n, B, scene.num_links, dev, True, True) for n in D}

    def info(n):
        o = outs[n]
        information._launch(ctx, scene, mvp, D[n], ref, o.info, o.grad, o.count, o.loss, o.grad_mvp)

    res = {}
    for name, fn in (("render_mask_loss", render), ("information N=6", lambda: info(6)), ("information N=17", lambda: info(17))):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        ws = []
        for _ in range(a.windows):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            ws.append(1e6 * (time.perf_counter() - t0) / a.calls)
        res[name] = {"us_per_call": round(min(ws), 1), "windows_us": [round(w, 1) for w in ws]}
    fused.check_status(ctx)
    res["count"] = outs[17].count.cpu().tolist()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
