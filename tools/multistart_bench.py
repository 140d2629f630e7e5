"""Multi-start solve against P solo solves, one after another (profiles/multistart.md):
    python tools/multistart_bench.py [--P 1 4 16 64] [--Bv 1 4] [--steps 2000] [--repeats 5] [--out FILE.json]
    python tools/multistart_bench.py --study [--out FILE.json]        (the convergence table, not a timing)

xArm7 at 640x480.  Both legs replay captured graphs, are warmed, and are timed with events around the whole leg:
  batched     one MultiStartPoseStep, `steps` replays of ehr_solver_step_multi          = P x steps hypothesis-steps
  sequential  the same P solves one after another through ONE FusedPoseStep's graph      = P x steps hypothesis-steps
              (between two solves its state is reset on the device: a few copies, inside the timed region -- the
              parent's API offers nothing cheaper)
The legs alternate and every pair is repeated; values are hypothesis-steps per second.  Stage times come from a separate
eager pass with ehr_fused_timing (events cannot be recorded under capture)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from easyhec_amd import fused  # noqa: E402
from easyhec_amd.config import XARM7_K_1280x720, Cfg  # noqa: E402
from easyhec_amd.fast import FusedPoseStep  # noqa: E402
from easyhec_amd.multistart import MultiStartPoseStep, _starts_to_dof, sample_starts, solve_multistart  # noqa: E402
from easyhec_amd.rb_solver import RBSolver  # noqa: E402
from easyhec_amd.robot import load_robot  # noqa: E402
from easyhec_amd.se3 import se3_exp_map  # noqa: E402
from easyhec_amd.synthetic import camera_Tc_c2b, make_views, perturb_pose, scaled_K  # noqa: E402

H, W = 480, 640


def build(rb, Bv, dev):
    K = scaled_K(XARM7_K_1280x720, 0.5, W, H, True)
    _, lp = make_views(rb, Bv, seed=0)
    Tc = camera_Tc_c2b()
    cfg = Cfg()
    cfg.model.rbsolver.H, cfg.model.rbsolver.W = H, W
    cfg.model.rbsolver.init_Tc_c2b = perturb_pose(Tc).tolist()
    make = lambda: RBSolver(cfg, meshes=rb.meshes).to(dev)
    m0 = make()
    Kt, lpt = torch.tensor(K, dtype=torch.float32, device=dev), torch.tensor(lp, device=dev)
    with torch.no_grad():
        gt, _ = fused.render_mask_loss(m0._ensure_renderer().glctx, m0._ensure_scene(), fused.mvp_matrices(
            Kt, H, W, torch.tensor(Tc, dtype=torch.float32, device=dev), lpt), torch.zeros((Bv, H, W), device=dev))
    return cfg, make, {"mask": (gt > 0.5).float(), "link_poses": lpt, "K": Kt[None].repeat(Bv, 1, 1)}, Tc


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def pose_error(T, Tgt):
    D = np.linalg.inv(Tgt) @ T
    return float(np.linalg.norm(D[:3, 3]) * 1000.0), float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))))


def bench_one(rb, P, Bv, steps, repeats, warmup, dev):
    cfg, make, batch, Tc = build(rb, Bv, dev)
    starts = sample_starts(np.asarray(cfg.model.rbsolver.init_Tc_c2b), P, 0.03, 4.0, seed=0)
    dofs = _starts_to_dof(starts).to(dev)
    ms = MultiStartPoseStep(make(), batch, starts)
    ms.check_every = 1 << 30  # (no host look at the loss inside a timed leg, in either leg)
    ms.capture()
    solo_model = make()
    fs = FusedPoseStep(solo_model, batch)
    fs.check_every = 1 << 30
    fs.capture()

    def reset_multi():
        ms.dof.copy_(dofs)
        for t in (ms.exp_avg, ms.exp_avg_sq, ms.step_t, ms.hist_row):
            t.zero_()

    def batched():
        reset_multi()
        for _ in range(steps):
            ms.step()

    def sequential():
        for p in range(P):
            solo_model.dof.data.copy_(dofs[p])
            for t in (fs.exp_avg, fs.exp_avg_sq, fs.step_t, fs.hist_row):
                t.zero_()
            for _ in range(steps):
                fs.step()

    reset_multi()
    for _ in range(warmup):
        ms.step()
        fs.step()
    tb, tq = [], []
    for _ in range(repeats):
        tb.append(P * steps / timed(batched))
        tq.append(P * steps / timed(sequential))
    assert bool(torch.isfinite(ms.loss).all()) and bool(torch.isfinite(fs.loss).all())
    # stage times of the batched step: an eager pass with events around every launch
    ms.release_graph()
    reset_multi()
    fused.set_timing(ms.glctx, True)
    for _ in range(200):
        ms.step()
    st, n = fused.read_timing(ms.glctx)
    fused.set_timing(ms.glctx, False)
    fused.check_status(ms.glctx)
    stage_us = {"vertex": st["vertex"] / n * 1e3, "job": st["job"] / n * 1e3, "composite": st["composite"] / n * 1e3,
                "finish": st["unused5"] / n * 1e3, "event_pair": st["resolve"] / n * 1e3}
    r = {"P": P, "Bv": Bv, "steps": steps, "batched": tb, "sequential": tq,
         "batched_median": statistics.median(tb), "sequential_median": statistics.median(tq),
         "sequential_spread": max(tq) - min(tq), "batched_spread": max(tb) - min(tb),
         "speedup": statistics.median(tb) / statistics.median(tq), "stage_us": stage_us}
    print(json.dumps(r), flush=True)
    return r


def study(rb, dev, num_steps=200, tail=20):
    """Config 2 (1 view) and the 4-view problem, 16 starts at two spreads: where every start ends, and the winner."""
    rows = []
    for Bv in (1, 4):
        cfg, make, batch, Tc = build(rb, Bv, dev)
        for ts, rs in ((0.03, 4.0), (0.06, 8.0)):
            starts = sample_starts(np.asarray(cfg.model.rbsolver.init_Tc_c2b), 16, ts, rs, seed=0)
            res = solve_multistart(cfg, make(), batch, starts, num_steps, tail=tail)
            ends = [pose_error(se3_exp_map(d[None]).permute(0, 2, 1)[0].numpy().astype(np.float64), Tc) for d in res.dofs]
            begins = [pose_error(T, Tc) for T in starts]
            r = {"Bv": Bv, "trans_sigma_m": ts, "rot_sigma_deg": rs, "start_err_mm_deg": begins, "end_err_mm_deg": ends,
                 "tail_loss": [float(x) for x in res.losses], "ranking": res.ranking, "winner": res.winner,
                 "winner_err_mm_deg": ends[res.winner], "recoveries": res.recoveries}
            print(json.dumps(r), flush=True)
            rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--Bv", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--study", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/multistart_bench.py needs a HIP device")
    dev = torch.device("cuda:0")
    rb = load_robot("xarm7")
    if a.study:
        out = {"study": study(rb, dev)}
    else:
        out = {"bench": [bench_one(rb, P, Bv, a.steps, a.repeats, a.warmup, dev) for Bv in a.Bv for P in a.P]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
