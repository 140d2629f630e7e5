"""Cost of one Levenberg-Marquardt iteration (easyhec_amd/lm.py) next to one Adam step and one ehr_mask_information call:
    python tools/lm_cost.py [--iters 50] [--windows 3] [--gauge]
Workload: xArm7, 8 views 1280x720 (the flagship shape of bench.py), masks rendered at the true pose, the pose perturbed, pose
only (N = 6).  Every figure is a host clock around `--iters` iterations that end in ONE device synchronise, after 10 warm-up
iterations, `--windows` windows; every window starts from the same pose and a cleared state block, so the windows run the same
iterations; the best window is reported beside all of them.  --gauge adds the wall time of solve_lm against the 400-step Adam
solve on the gauge problem of tests/information_reference.py (4 views 120x160; needs the oracle).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, reset, n, nwin, sync):
    ws = []
    for _ in range(nwin):
        reset()
        sync()
        t0 = time.perf_counter()
        fn(n)
        sync()
        ws.append(1e6 * (time.perf_counter() - t0) / n)
    return {"us_per_iteration": round(min(ws), 1), "windows_us": [round(w, 1) for w in ws]}


def gauge_times():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import information_reference as IR
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.lm import solve_lm
    from easyhec_amd.rb_solver import RBSolver
    from easyhec_amd.robot import load_robot
    from oracle import oracle
    oracle.lib()
    dev = torch.device("cuda:0")
    p = IR.gauge_problem(oracle, load_robot("xarm7"), base=True)
    out = {}
    for name in ("lm", "adam", "lm", "adam"):          # (the first pair warms everything up; the constructor plans and binds)
        cfg, batch, _ = IR.gauge_batch(p, dev)
        st = FusedPoseStep(RBSolver(cfg, meshes=p.rb.meshes).to(dev), batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "lm":
            res = solve_lm(st, max_iters=12)
            torch.cuda.synchronize()
            out["solve_lm"] = {"ms": round(1e3 * (time.perf_counter() - t0), 2), "iterations": res.iterations,
                               "accepted": res.accepted, "summed_loss": round(res.loss, 2), "stopped_by": res.why}
        else:
            st.capture()
            losses = st.take_effective_steps(400, "lm_cost")[:400, 0].double().numpy() * st.B
            torch.cuda.synchronize()
            out["adam_400_captured"] = {"ms": round(1e3 * (time.perf_counter() - t0), 2), "last_summed_loss": round(float(losses[-1]), 2),
                                        "best_summed_loss": round(float(losses.min()), 2),
                                        "first_step_below_200": int(np.argmax(losses < 200.0)) if (losses < 200.0).any() else -1}
            st.release_graph()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--gauge", action="store_true")
    a = ap.parse_args()
    import torch
    from easyhec_amd import fused, information
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.lm import LevenbergMarquardt
    from easyhec_amd.robot import load_robot
    from tools.intrinsics_step_bench import problem
    rb = load_robot("xarm7")
    cfg, model, batch = problem(rb)
    st = FusedPoseStep(model, batch)
    lm = LevenbergMarquardt(st, log_rows=a.iters + 16)
    dof0, state0 = model.dof.data.clone(), lm.state_block.clone()
    sync = torch.cuda.synchronize

    def reset():
        model.dof.data.copy_(dof0)
        lm.state_block.copy_(state0)

    res = {}
    lm.iterate(10)
    res["lm_iteration N=6"] = windows(lm.iterate, reset, a.iters, a.windows, sync)
    s = lm.state()
    res["lm_state"] = {"accepted": s.accepted, "rejected": s.rejected, "reported": s.reported, "done": s.done,
                       "summed_loss": round(s.F_acc, 1)}

    def info(n):
        for _ in range(n):
            information._launch(st.glctx, st.scene, lm.mvp, lm.dmvp, st.ref, lm.out.info, lm.out.grad, lm.out.count, lm.out.loss, None)

    res["information N=6"] = windows(info, reset, a.iters, a.windows, sync)

    def lin_upd(n):
        import ctypes
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for _ in range(n):
            lm._linearize(stream)
            lm._update(stream)

    res["linearize + update alone"] = windows(lin_upd, reset, a.iters, a.windows, sync)
    reset()

    def adam(n):
        for _ in range(n):
            st.step()

    adam(10)
    res["adam_step eager"] = windows(adam, reset, a.iters, a.windows, sync)
    st.capture()
    adam(10)
    res["adam_step captured"] = windows(adam, reset, a.iters, a.windows, sync)
    st.release_graph()
    fused.check_status(st.glctx)
    if a.gauge:
        res["gauge"] = gauge_times()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
