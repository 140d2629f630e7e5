"""Cost of the multi-start Levenberg-Marquardt solve (easyhec_amd/lm_multi.py) next to P sequential solo solves:
    python tools/lm_multi_cost.py [--iters 40] [--rounds 7] [--out FILE.json]
Two scenes, xArm7: 8 views 1280x720 (the flagship shape of bench.py) and 2 views 120x160; P in {1, 4, 16}; the starts are
sample_starts around the scene's start pose.  Prints one JSON line per measurement:

* timing: milliseconds per ``MultiStartLM.iterate(1)`` against P sequential ``LevenbergMarquardt.iterate(1)`` on P plain steps
  (each on a solver and a context of its own) -- a host clock around ``--iters`` iterations that end in ONE device
  synchronise, after 2 warm-up iterations, the two forms ALTERNATING for ``--rounds`` rounds; median, min and max.  ftol = 0
  and lambda_max = 1e300, so that nobody stops by those rules during the timed iterations.  Also: whether every
  hypothesis's state block still equals its solo solve's, and the device memory (``ehr_ctx_scratch_bytes`` of the solve's
  context, the tiled reference, a solo context).
* solve: a whole ``solve_lm_multi`` at P = 16 -- iterations per hypothesis, why each stopped, the basins, the wall time, and
  the share of rendered views that belonged to hypotheses that were already done, ``sum_p (calls - iterations[p]) / (calls P)``:
  the cost of not retiring them."""
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
SOLVES = (("0.002 m / 0.3 deg", 0.002, 0.3, 2, 50), ("0.03 m / 4 deg", 0.03, 4.0, 0, 50),
          ("0.002 m / 0.3 deg", 0.002, 0.3, 2, 300), ("0.03 m / 4 deg", 0.03, 4.0, 0, 300))   # sigma_t, sigma_r, seed, max_iters


def stats(x):
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch
    from easyhec_amd import lm, lm_multi
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.multistart import sample_starts
    from easyhec_amd.robot import load_robot
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
    for name, Bv, H, W, scale in SCENES:
        cfg, make, batch = problem(xarm7, Bv, H, W, scale)
        Tc_init = np.asarray(cfg.model.rbsolver.init_Tc_c2b, dtype=np.float64)
        for P in (1, 4, 16):
            starts = sample_starts(Tc_init, P, 0.002, 0.3, seed=2)
            kw = dict(ftol=0.0, lambda_max=1e300)
            ms = lm_multi.MultiStartLM(make(), batch, starts, **kw)
            solos = []
            for p in range(P):
                cfg.model.rbsolver.init_Tc_c2b = np.asarray(starts[p]).tolist()
                solos.append(lm.LevenbergMarquardt(FusedPoseStep(make(), batch), **kw))
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
            emit({"what": "timing", "scene": name, "P": P, "batched_ms": stats(tb), "sequential_ms": stats(ts),
                  "sequential_over_batched": round(statistics.median(ts) / statistics.median(tb), 3),
                  "done": sum(s.done for s in S), "reported": sum(s.reported for s in S), "state_blocks_equal_solo": equal,
                  "ctx_scratch_bytes": ms.glctx.scratch_bytes(), "tiled_ref_bytes": ms.ref.numel() * 4,
                  "solo_ctx_scratch_bytes": solos[0].step.glctx.scratch_bytes()})
            del ms, solos
            torch.cuda.empty_cache()
        for what, ts_m, rs_deg, seed, max_iters in SOLVES:
            P = 16
            starts = sample_starts(Tc_init, P, ts_m, rs_deg, seed=seed)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = lm_multi.solve_lm_multi(make(), batch, starts, max_iters=max_iters)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t
            calls = res.lm.calls
            emit({"what": "solve", "scene": name, "starts": what, "max_iters": max_iters, "P": P, "calls": calls,
                  "iterations": res.iterations, "why": res.why,
                  "done_view_share": round(sum(calls - it for it in res.iterations) / (calls * P), 4),
                  "losses": [round(x, 2) for x in res.losses.tolist()], "basins": res.basins, "winner": res.winner,
                  "wall_ms": round(1e3 * wall, 2), "memory_bytes": res.lm.memory_bytes()})
            del res
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
