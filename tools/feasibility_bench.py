"""Cost of the feasibility filter (easyhec_amd/feasibility.py) next to the scoring it stands in front of:
    python tools/feasibility_bench.py [--candidates 1000] [--path-steps 8] [--reps 20]
Workload: xArm7, 1000 candidate joint vectors ~ U(0.9 x limits), each judged at 8 configurations of the straight segment from
the zero configuration; leaf_triangles 64, margin 0.01, the reference's workspace box with the table at z = 0.  Median of
`--reps` host-clock windows that end in ONE device synchronise, after 3 warm-up runs, of
    the path table (host) | kinematics (upload + ehr_joint_forward) | the clearance kernel | check(), whole
and, on the problem of tools/info_explorer_bench.py (4 frames at 640x360), `InformationExplorer.score` of the same candidates
without a filter and with the filter's ``valid``.  Then the same candidates through ``FeasibilityFilter(exact=True)``
(``ehr_mesh_clearance``): the mesh kernel whole, its two phases alone (the arm against itself; planes), and
``check()``.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--path-steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from info_explorer_bench import median_ms, problem
    from easyhec_amd import feasibility as F
    from easyhec_amd.fast import FusedPoseStep
    from easyhec_amd.info_explorer import InformationExplorer
    from easyhec_amd.joint_calib import JointPoseStep
    from easyhec_amd.robot import load_robot
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rb = load_robot("xarm7")
    cand = rb.sample_qpos(a.candidates, np.random.default_rng(0), scale=0.9)
    cur = np.zeros(7)
    lo, hi = F.REFERENCE_WORKSPACE
    flt = F.FeasibilityFilter(rb, leaf_triangles=64, margin=0.01, planes=F.box_planes((lo[0], lo[1], 0.0), hi), device=dev)
    n_i = np.diff(flt.sphere_offsets)
    pairs_per_config = int(sum(int(n_i[i]) * int(n_i[j]) for i, j in flt.pairs))
    res = {"workload": f"xArm7, {a.candidates} candidates x {a.path_steps} path steps, median of {a.reps}",
           "spheres": int(flt.sphere_offsets[-1]), "link pairs": len(flt.pairs), "sphere pairs per configuration": pairs_per_config,
           "planes": 6}
    box = {}

    def table():
        box["table"], _ = flt.path_table(cand, cur, a.path_steps)
    res["path table (host)"] = median_ms(table, a.reps, sync)

    def kin():
        box["lp"] = flt.kinematics(box["table"])
    res["kinematics"] = median_ms(kin, a.reps, sync)
    res["clearance kernel"] = median_ms(lambda: flt.clearance(box["lp"]), a.reps, sync)
    k_ms = res["clearance kernel"]["median_ms"]
    res["clearance kernel"]["sphere pairs before culling, 1e9/s"] = round(pairs_per_config * box["lp"].shape[0] / k_ms / 1e6, 2)
    res["check(), whole"] = median_ms(lambda: flt.check(cand, current_qpos=cur, path_steps=a.path_steps), a.reps, sync)
    res["check(), candidates alone"] = median_ms(lambda: flt.check(cand), a.reps, sync)
    out = flt.check(cand, current_qpos=cur, path_steps=a.path_steps)
    valid = out.valid.cpu().numpy()
    res["accepted"] = int(valid.sum())
    res["rejected self / env / reach"] = [int((~getattr(out, k)).sum()) for k in ("self_ok", "env_ok", "reach_ok")]
    res["accepted, candidates alone"] = int(flt.check(cand).valid.sum())
    # the scoring the filter stands in front of (these modules are not edited by the filter: the parent commit's figures)
    H, W, B = 360, 640, 4
    make, batch, qp, K, Tc = problem(rb, B, H, W, 0.5, dev)
    for name, ex in (("pose only", InformationExplorer(FusedPoseStep(make(), batch), robot=rb)),
                     ("pose + six offsets", InformationExplorer(JointPoseStep(make(), batch, rb, qp)))):
        res[f"InformationExplorer.score, {name}"] = median_ms(lambda: ex.score(cand), a.reps, sync)
        res[f"InformationExplorer.score, {name}, the filter's valid"] = median_ms(lambda: ex.score(cand, valid), a.reps, sync)
    # the meshes behind the proxies: the same candidates, path and box
    ex = F.FeasibilityFilter(rb, leaf_triangles=64, margin=0.01, planes=F.box_planes((lo[0], lo[1], 0.0), hi), device=dev, exact=True)
    res["exact: triangles"], res["exact: mesh pairs"], res["exact: cutoff"] = int(ex.triangles.shape[0]), len(ex.mesh_pairs), ex.exact_cutoff
    lp = box["lp"]
    none = torch.zeros((ex.L,), dtype=torch.int32, device=dev)
    mesh = lambda pairs, planes, env: F.mesh_clearance(lp, ex._spheres, ex.sphere_offsets, ex._bounds, pairs, ex._triangles,
                                                       ex._tri_offsets, planes, None, env, ex.exact_cutoff)
    res["mesh kernel, whole"] = median_ms(lambda: ex.mesh_clearance(lp), a.reps, sync)
    res["mesh kernel, the arm against itself alone"] = median_ms(lambda: mesh(ex._mesh_enable, None, 0), a.reps, sync)
    res["mesh kernel, the planes alone"] = median_ms(lambda: mesh(none, ex._planes, ex.env_mask), a.reps, sync)
    res["check(exact), whole"] = median_ms(lambda: ex.check(cand, current_qpos=cur, path_steps=a.path_steps), a.reps, sync)
    res["check(exact), candidates alone"] = median_ms(lambda: ex.check(cand), a.reps, sync)
    eo = ex.check(cand, current_qpos=cur, path_steps=a.path_steps)
    res["exact: accepted"] = int(eo.valid.sum())
    res["exact: rejected self / env / reach"] = [int((~getattr(eo, k)).sum()) for k in ("self_ok", "env_ok", "reach_ok")]
    res["exact: accepted, candidates alone"] = int(ex.check(cand).valid.sum())
    res["exact: accepted that the proxies reject"] = int((eo.valid.cpu().numpy() & ~valid).sum())
    res["exact: rejected that the proxies accept"] = int((~eo.valid.cpu().numpy() & valid).sum())
    raw = ex.mesh_clearance(lp)
    res["exact: configurations at distance 0 / below cutoff"] = [int((raw.mesh_clear == 0).sum()), int((raw.mesh_clear < ex.exact_cutoff).sum())]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
