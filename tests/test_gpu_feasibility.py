"""The feasibility kernel (csrc/ehr_feasible.hip) and easyhec_amd/feasibility.py on the GPU, against the brute-force float64
reference of tests/feasibility_reference.py: the three clearances bit for bit and the pair equal over sphere counts 0..257 per
link, 1..32 links (4096 spheres at 32), 1..70 configurations, planes, obstacles, reach, masks, a NaN pose, culling and the
refusals; the packaged xArm7 on sampled configurations; ``check`` over a path; the online loop.  tests/
test_feasibility_reference.py pins the reference on the CPU.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import feasibility_reference as FR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, feasibility
    assert _lib.has_feasibility()
    return feasibility


def dev64(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(F, case, link_poses=None):
    lp = case["link_poses"] if link_poses is None else link_poses
    out = F.config_clearance(torch.tensor(lp, device=DEV), dev64(case["spheres"]), case["offsets"], dev64(case["bounds"]),
                             torch.tensor(case["pair_enable"].view(np.int32), device=DEV), dev64(case["planes"]),
                             dev64(case["obstacles"]), case["env_links"], dev64(case["reach"]), case["cutoff"])
    return host(out.self_clear), host(out.self_pair), host(out.env_clear), host(out.reach_clear)


def assert_same(what, got, ref):
    """The clearances bit for bit (NaN against NaN), the pair equal."""
    bad = []
    for name, g, r in zip(("self_clear", "self_pair", "env_clear", "reach_clear"), got, ref):
        same = (g == r) if name == "self_pair" else ((bits(g) == bits(r)) | (np.isnan(g) & np.isnan(r)))
        print(f"[feasibility] {what}: {name} differs in {int((~same).sum())} of {same.size}"
              + ("" if same.all() else f" (first: got {g[~same][0]!r}, reference {r[~same][0]!r})"))
        bad += [] if same.all() else [name]
    assert not bad, (what, bad)


# counts per link, n, planes, obstacles, reach, pairs, spread
CASES = {
    "L1": dict(counts=[65], n=1, n_planes=1, n_obstacles=1, with_reach=True),
    "L2-n70": dict(counts=[257, 63], n=70),
    "L9-ragged": dict(counts=[0, 1, 63, 64, 65, 257, 1, 0, 64], n=3, n_planes=6, n_obstacles=300, with_reach=True, pairs="random"),
    "L9-mask-off": dict(counts=[64, 1, 63, 0, 65, 2, 1, 7, 64], n=3, n_planes=1, pairs="none"),
    "L32-S4096": dict(counts=[128] * 32, n=3, n_planes=1, n_obstacles=1, spread=1.2),
}
_BUILT = {}


def built(name):
    """A case and its reference, computed once and shared (never written to)."""
    if name not in _BUILT:
        case = FR.make_case(list(CASES).index(name) + 11, **CASES[name])
        _BUILT[name] = (case, FR.reference_of(case))
    return _BUILT[name]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_the_reference(F, name):
    case, ref = built(name)
    sc, sp, ec, rc = ref
    cut = case["cutoff"]
    print(f"[feasibility] {name}: S = {int(case['offsets'][-1])}, reference self_clear {sc.min():.4f}..{sc.max():.4f} "
          f"({int((sc < cut).sum())} of {sc.size} below cutoff), env {ec.min():.4f}..{ec.max():.4f}, reach {rc.min():.4f}..{rc.max():.4f}")
    got = run(F, case)
    assert_same(name, got, ref)
    assert_same(name + " again", run(F, case), got)                                  # two runs: the same bits
    if name == "L32-S4096":
        assert int(case["offsets"][-1]) == 4096
    if name == "L9-mask-off":
        assert (got[0] == cut).all() and (got[1] == -1).all() and (got[3] == cut).all()   # no pairs, reach NULL: cutoff
    if name == "L1":
        assert (got[0] == cut).all() and (got[1] == -1).all() and (got[3] < cut).all()   # one link: nothing to pair


def test_a_nan_pose_leaves_its_neighbours_alone(F):
    case, ref = built("L9-ragged")
    lp = case["link_poses"].copy()
    lp[1, 4, 1, 2] = np.nan
    got = run(F, case, lp)
    assert np.isnan([got[0][1], got[2][1], got[3][1]]).all() and got[1][1] == -1
    assert_same("NaN pose", got, FR.clearance(lp, case["spheres"], case["offsets"], case["pair_enable"], case["planes"],
                                              case["obstacles"], case["env_links"], case["reach"], case["cutoff"]))
    for k in (0, 2):                                                                 # the neighbours: what they were
        assert all(g[k] == r[k] for g, r in zip(got, ref))
    lp[1, 4, 1, 2], lp[1, 8, 3, 0] = case["link_poses"][1, 4, 1, 2], np.inf          # ... and an infinite entry, in the last row
    got = run(F, case, lp)
    assert np.isnan([got[0][1], got[2][1], got[3][1]]).all() and got[1][1] == -1


def test_culling_changes_nothing(F):
    """Two links whose bounds lie beyond cutoff (culled), inside the slack of 1e-6 above it (not culled), just inside and well
    inside; a plane and obstacles that the bounds clear in the first and reach in the last."""
    cut = 0.25
    case = FR.make_case(5, [64, 65], 1, cutoff=cut)
    b = case["bounds"]
    delta = b[1, :3] - b[0, :3]
    targets = [cut + 1e-3, cut + 5e-7, cut - 1e-3, 0.05]
    lp = np.zeros((len(targets), 2, 4, 4), dtype=np.float32)
    lp[:, :, range(4), range(4)] = 1.0
    for k, t in enumerate(targets):
        T = t + b[0, 3] + b[1, 3]
        lp[k, 1, 0, 3] = np.sqrt(T * T - delta[1] ** 2 - delta[2] ** 2) - delta[0]
    case["link_poses"] = lp
    x1 = lp[:, 1, 0, 3].astype(np.float64)
    # a wall beyond link 1 at its nearest (k = 3) + 0.1 m; obstacles along the x axis beyond the farthest position
    case["planes"] = np.array([[-1.0, 0.0, 0.0, x1[3] + b[1, 0] + b[1, 3] + 0.1]])
    case["obstacles"] = np.array([[x1[0] + 0.6, 0.0, 0.0, 0.05], [x1[0] + 2.0, 0.0, 0.0, 0.05]])
    case["env_links"] = 3
    bound_gap = np.linalg.norm((b[1, :3] + np.stack([x1, 0 * x1, 0 * x1], axis=1)) - b[0, :3], axis=1) - (b[0, 3] + b[1, 3])
    print(f"[feasibility] culling: bound gaps - cutoff {(bound_gap - cut).tolist()}")
    assert bound_gap[0] > cut + 1e-6 and cut < bound_gap[1] < cut + 1e-6 and bound_gap[2] < cut
    ref = FR.reference_of(case)
    print(f"[feasibility] culling: reference self {ref[0].tolist()} pair {ref[1].tolist()} env {ref[2].tolist()}")
    assert ref[0][0] == cut and ref[1][0] == -1 and ref[0][3] < cut and ref[1][3] == 1
    assert ref[2][0] < ref[2][3] or ref[2][3] < cut                                  # the environment is in play somewhere
    assert_same("culling", run(F, case), ref)


def test_sizes_outside_the_limits_are_refused(F):
    case, _ = built("L1")
    sph, bnd = dev64(case["spheres"]), dev64(np.zeros((33, 4)))
    pe = lambda L: torch.zeros((L,), dtype=torch.int32, device=DEV)
    lp = lambda n, L: torch.zeros((n, L, 4, 4), device=DEV)
    big = dev64(np.zeros((4097, 4)))
    for match, call in (
            ("1 <= L <= 32", lambda: F.config_clearance(lp(1, 33), sph, np.zeros(34, dtype=np.int32), bnd, pe(33))),
            ("n 0 >= 1", lambda: F.config_clearance(lp(0, 1), sph, case["offsets"], bnd, pe(1))),
            ("S 4097 <= 4096", lambda: F.config_clearance(lp(1, 1), big, np.array([0, 4097], dtype=np.int32), bnd, pe(1))),
            ("ascend from 0", lambda: F.config_clearance(lp(1, 2), sph, np.array([0, 9, 3], dtype=np.int32), bnd, pe(2))),
            ("planes <= 16", lambda: F.config_clearance(lp(1, 1), sph, case["offsets"], bnd, pe(1), planes=dev64(np.zeros((17, 4))))),
            ("obstacles <= 1024", lambda: F.config_clearance(lp(1, 1), sph, case["offsets"], bnd, pe(1), obstacles=dev64(np.zeros((1025, 4))))),
            ("finite and > 0", lambda: F.config_clearance(lp(1, 1), sph, case["offsets"], bnd, pe(1), cutoff=0.0)),
            ("finite and > 0", lambda: F.config_clearance(lp(1, 1), sph, case["offsets"], bnd, pe(1), cutoff=float("nan"))),
            ("CUDA/HIP tensor", lambda: F.config_clearance(torch.zeros((1, 1, 4, 4)), sph, case["offsets"], bnd, pe(1)))):
        with pytest.raises(RuntimeError, match=match):
            call()
    # the limits themselves pass: 16 planes and 1024 obstacles
    c = FR.make_case(3, [5, 4], 2, n_planes=16, n_obstacles=1024)
    assert_same("at the limits", run(F, c), FR.reference_of(c))


# ---- the packaged arm -------------------------------------------------------------------------------------------------------
def reference_of_filter(flt, link_poses):
    return FR.clearance(link_poses, flt.spheres, flt.sphere_offsets, F_words(flt), flt.planes, flt.obstacles, flt.env_mask,
                        flt.reach, flt.cutoff)


def F_words(flt):
    from easyhec_amd.feasibility import pair_words
    return pair_words(flt.pairs, flt.L)


def test_xarm7_sampled_configurations(F, xarm7):
    flt = F.FeasibilityFilter(xarm7, leaf_triangles=64, margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]])
    assert sorted(d["pair"] for d in flt.ignored if d["reason"] == "settle") == [(1, 5), (2, 4), (2, 5)]
    assert flt.env_links == list(range(1, 8))                                        # the base stands on the table
    q = xarm7.sample_qpos(128, np.random.default_rng(1), scale=1.0)
    table, steps = flt.path_table(q)
    lp = host(flt.kinematics(table))
    fk = xarm7.link_poses_batch(table)
    print(f"[feasibility xarm7] device kinematics against the host's float64: max |diff| {np.abs(lp - fk).max():.2e}")
    assert steps == 1 and np.abs(lp - fk).max() <= 1e-6
    sc, sp, ec, rc = ref = reference_of_filter(flt, lp)
    ok = FR.validity(sc, ec, rc, flt.margin)
    near = min(np.abs(sc - flt.margin).min(), np.abs(ec - flt.margin).min())
    print(f"[feasibility xarm7] the reference accepts {int(ok.sum())} of 128 (self {int((sc > flt.margin).sum())}, env "
          f"{int((ec > flt.margin).sum())}); nearest clearance to its threshold {near:.2e} m")
    assert 0.1 * 128 <= ok.sum() <= 0.9 * 128                                        # (on the reference alone)
    assert near > 1e-9
    out = flt.check(q)
    got = (host(out.self_clear), host(out.self_pair), host(out.env_clear), host(out.reach_clear))
    assert_same("xarm7", got, ref)
    assert (host(out.valid) == ok).all() and (host(out.worst_step) == 0).all()
    assert (got[3] == flt.cutoff).all() and host(out.reach_ok).all()                 # no reach constraint


def sweep_problem(F, xarm7):
    """A bent arm that turns about its base through an obstacle: clear at both ends, not along the way."""
    cur = np.array([0.0, 0.3, 0.0, 1.2, 0.0, 0.9, 0.0])
    swept = cur.copy()
    swept[0] = 2.0
    mid = cur.copy()
    mid[0] = 1.0
    ob = xarm7.link_poses(mid)[6][:3, 3]
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=F.box_planes((-1.0, -1.0, 0.0), (1.0, 1.0, 1.5)),
                              obstacles=[[ob[0], ob[1], ob[2], 0.03]], reach=[0.0, 0.0, 0.2, 0.75])
    cand = np.concatenate([xarm7.sample_qpos(12, np.random.default_rng(4), scale=0.8), swept[None]])
    return flt, cur, cand


def test_check_over_a_path(F, xarm7):
    flt, cur, cand = sweep_problem(F, xarm7)
    table, steps = flt.path_table(cand, cur, 4)
    assert steps == 4 and table.shape == (52, flt.J) and (table[3::4, :7] == cand).all()
    assert np.allclose(table[48, :7], cur + 0.25 * (cand[12] - cur), rtol=0, atol=1e-15)
    lp = host(flt.kinematics(table))
    raw = reference_of_filter(flt, lp)
    ref = FR.reduce_steps(*raw, 4, flt.margin)
    end = FR.validity(*(np.asarray(a)[3::4] for a in (raw[0], raw[2], raw[3])), flt.margin)
    print(f"[feasibility check] reference: valid {ref['valid'].astype(int).tolist()}, at the end alone {end.astype(int).tolist()}, "
          f"worst steps {ref['worst_step'].tolist()}, reach ok {ref['reach_ok'].astype(int).tolist()}")
    assert end[12] and not ref["valid"][12] and not ref["env_ok"][12] and ref["worst_step"][12] == 1   # (on the reference alone)
    assert 0 < ref["valid"].sum() < 13
    out = flt.check(cand, current_qpos=cur, path_steps=4)
    for k in ("valid", "self_ok", "env_ok", "reach_ok", "self_pair", "worst_step"):
        assert (host(getattr(out, k)) == ref[k]).all(), k
    for k in ("self_clear", "env_clear", "reach_clear"):
        assert (bits(host(getattr(out, k))) == bits(ref[k])).all(), k
    ends = flt.check(cand)                                                           # at its end alone the sweep passes
    assert (host(ends.valid) == end).all() and bool(host(ends.valid)[12])
    # a configuration that cannot be judged is not valid, whatever the step
    bad = cand.copy()
    bad[5, 2] = np.nan
    out = flt.check(bad, current_qpos=cur, path_steps=4)
    assert not host(out.valid)[5] and np.isnan(host(out.self_clear)[5]) and host(out.self_pair)[5] == -1
    assert (np.delete(host(out.valid), 5) == np.delete(ref["valid"], 5)).all()
    # offsets: a step's tensor is read on every call
    off = torch.zeros((flt.J,), device=DEV)
    flt2 = F.FeasibilityFilter(xarm7, margin=0.01, offsets=off)
    a = host(flt2.check(cand).self_clear)
    off[1] = 0.3
    b = host(flt2.check(cand).self_clear)
    shifted = cand.copy()
    shifted[:, 1] += np.float64(np.float32(0.3))
    off[1] = 0.0
    assert (a != b).any()
    assert (bits(host(flt2.check(shifted).self_clear)) == bits(b)).all()


# ---- the online loop --------------------------------------------------------------------------------------------------------
def test_online_loop_with_a_filter(F, xarm7):
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    init = perturb_pose(Tc_gt)
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]], path_steps=2)
    under = np.array([[0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 0.0], [1.0, 1.9, 0.0, 0.2, 0.0, 0.3, 0.0]])   # folded below the table
    cand = np.concatenate([xarm7.sample_qpos(10, np.random.default_rng(1), scale=0.6), under])
    given = np.ones(12, dtype=bool)
    given[3] = False
    first = np.zeros(7)
    table, _ = flt.path_table(cand, first, 2)
    raw = reference_of_filter(flt, host(flt.kinematics(table)))
    ref = FR.reduce_steps(*raw, 2, flt.margin)
    print(f"[feasibility online] the reference accepts {ref['valid'].astype(int).tolist()}")
    assert not ref["valid"][10:].any() and 2 <= (~ref["valid"]).sum() < 11 and ref["valid"][:10].sum() >= 2
    asked = []

    def capture(qpos):
        asked.append(np.array(qpos))
        return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

    logs = {}
    for name, feasible in (("filter", flt), ("none", None)):
        asked.clear()
        loop = OnlineCalibration(xarm7, K, H, W, init, capture, lambda _r: (cand, given), num_epochs=60, explore_iters=2,
                                 explore="information", feasible=feasible)
        loop.fit(first)
        logs[name] = loop.log
        print(f"[feasibility online] {name}: {loop.log}")
        hit = [i for i in range(12) if (cand[i] == asked[1]).all()]
        assert len(hit) == 1 and given[hit[0]] and (feasible is None or ref["valid"][hit[0]])
    today = ["round", "frames", "mask_loss", "solve_s", "explore_s", "info_gain", "gain_mean", "candidates"]
    assert sorted(logs["none"][0]) == sorted(today)                                  # feasible=None: the keys it has today
    assert sorted(logs["filter"][0]) == sorted(today + ["rejected_self", "rejected_env", "rejected_reach"])
    r = logs["filter"][0]
    assert (r["rejected_self"], r["rejected_env"], r["rejected_reach"]) == (
        int((~ref["self_ok"]).sum()), int((~ref["env_ok"]).sum()), int((~ref["reach_ok"]).sum()))
    assert r["rejected_env"] >= 2 and r["rejected_reach"] == 0
    assert sorted(logs["filter"][1]) == sorted(logs["none"][1]) == sorted(["round", "frames", "mask_loss", "solve_s"])
    # every candidate rejected: the explorers' own error
    for explore in ("information", "variance"):
        loop = OnlineCalibration(xarm7, K, H, W, init, capture, lambda _r: (under, None), num_epochs=60, explore_iters=2,
                                 sample=4, start=10, explore=explore, feasible=flt)
        with pytest.raises(RuntimeError, match="no valid qpos found"):
            loop.fit(first)
