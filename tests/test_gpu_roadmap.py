"""The roadmap kernels on the GPU: ``ehr_edge_clearance`` against one-candidate ``segment_clearance`` calls (which
tests/test_gpu_segment_clearance.py pins on the numpy mirror) BIT FOR BIT through the trace, ``ehr_roadmap_paths`` and
``roadmap_edges`` against the mirrors of tests/roadmap_reference.py bit for bit, ``FeasibilityFilter.plan`` on the xArm7 and
the online loop with detours.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import feasibility_reference as FR
import roadmap_reference as RR
from test_gpu_segment_clearance import (BENT, DEV, FLOATS, INTS, built, dev, joint_forward, same, swept_outputs, table_tensors,
                                        words)

pytestmark = pytest.mark.gpu

EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (3, 1), (2, 2))
TRACES = ("trace_t", "trace_val")
VIA = (0, 0.5, 0, 1.6, 0, 0, 0)


@pytest.fixture(scope="module")
def F():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from easyhec_amd import _lib, feasibility
    assert _lib.has_roadmap(), "libehr_hip.so must export ehr_edge_clearance and ehr_roadmap_paths"
    return feasibility


@pytest.fixture(scope="module")
def xarm7():
    from easyhec_amd.robot import load_robot
    return load_robot("xarm7")


def numpy_of(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in vars(out).items() if torch.is_tensor(v)}


def proxy_args(c):
    return (dev(c["offset"], np.float32), dev(c["spheres"]), c["offsets"], dev(c["bounds"]), words(c["pair_enable"]),
            words(c["table"]["upstream"]), words(c["below"]), dev(c["W"]), dev(c["planes"]), dev(c["obstacles"]), c["env_links"],
            dev(c["reach"]), c["cutoff"], c["margin"], c["depth"], c["max_evals"])


def launch_edges(F, case, nodes, edges, **over):
    c = dict(case, **over)
    e = np.asarray(edges, dtype=np.int32).reshape(-1, 2)
    return numpy_of(F.edge_clearance(table_tensors(c["table"]), dev(nodes), dev(e[:, 0], np.int32), dev(e[:, 1], np.int32),
                                     *proxy_args(c), trace=True))


def launch_single(F, case, q0, q1, **over):
    c = dict(case, **over)
    return numpy_of(F.segment_clearance(table_tensors(c["table"]), dev(q0), dev(q1[None]), *proxy_args(c), trace=True))


def equal_entry(got, e, ref, b=0):
    return [k for k in FLOATS + TRACES if not same(got[k][e], ref[k][b]).all()] + [k for k in INTS if got[k][e] != ref[k][b]]


def case_nodes(case):
    return np.concatenate([case["q0"][None], case["q1"][:3]])


# ---- ehr_edge_clearance -----------------------------------------------------------------------------------------------------------------
def test_edges_against_single_calls(F):
    splits = []
    for name in ("L1", "L2-J1", "prismatic-empty-link", "tree"):
        case = built(name)
        nodes = case_nodes(case)
        got = launch_edges(F, case, nodes, EDGES)
        for e, (a, b) in enumerate(EDGES):
            ref = launch_single(F, case, nodes[a], nodes[b])
            print(f"[roadmap] {name} edge {e} ({a}, {b}): status {int(got['status'][e])} after {int(got['evals'][e])} evaluations, "
                  f"t_free {got['t_free'][e]}, length {float(got['length'][e])!r}; single call: status {int(ref['status'][0])} after "
                  f"{int(ref['evals'][0])}")
            assert not equal_entry(got, e, ref), (name, e, equal_entry(got, e, ref))
            assert same(got["length"][e], RR.length(nodes[a], nodes[b])).all(), (name, e)
            if a != 0 and int(got["evals"][e]) > 2 ** case["depth"][0]:
                splits.append((name, e))
        again = launch_edges(F, case, nodes, EDGES)
        assert all(same(got[k], again[k]).all() for k in FLOATS + TRACES + ("length",)) and \
            all((got[k] == again[k]).all() for k in INTS), "two runs: the same bits"
        assert got["length"][5] == 0.0, "a node to itself"
    print(f"[roadmap] edges not from node 0 that split an interval: {splits}")
    assert splits, "an edge that does not start at node 0 must split an interval"


def test_bad_indices_and_a_nan_node(F):
    case = built("tree")
    q = case_nodes(case)
    nodes = np.stack([q[0], q[1], np.full_like(q[0], np.nan), q[2]])
    nodes[2, 1:] = q[3, 1:]                                                            # one NaN entry is enough
    V = nodes.shape[0]
    edges = [(0, 1), (-1, 1), (0, 3), (1, V), (0, 2), (2, 3), (1, 3), (-1, -1)]
    good = [0, 2, 6]
    got = launch_edges(F, case, nodes, edges)
    alone = launch_edges(F, case, nodes, [edges[e] for e in good])
    print(f"[roadmap] status {got['status'].tolist()}, evals {got['evals'].tolist()}, length {got['length'].tolist()}")
    for e in (1, 3, 4, 5, 7):
        assert (got["status"][e], got["evals"][e], got["stop_pair"][e], got["t_free"][e]) == (3, 0, -1, 0.0), e
        assert np.isnan([got["stop_self"][e], got["stop_env"][e], got["stop_reach"][e], got["length"][e]]).all()
        assert got["cert_self"][e] == got["cert_env"][e] == got["cert_reach"][e] == case["cutoff"]
        assert np.isnan(got["trace_t"][e]).all() and np.isnan(got["trace_val"][e]).all(), "the trace rows are untouched"
    for k, e in enumerate(good):
        assert not equal_entry(got, e, alone, k) and same(got["length"][e], alone["length"][k]).all(), e
        assert got["status"][e] != 3 or got["evals"][e] > 0
    inf = nodes.copy()
    inf[2] = q[3]
    inf[2, 0] = np.inf
    assert launch_edges(F, case, inf, edges)["status"].tolist() == got["status"].tolist()


def test_one_evaluation_and_depth_zero(F):
    case = built("prismatic-empty-link")
    nodes = case_nodes(case)
    for over in (dict(max_evals=1), dict(depth=(0, 0))):
        got = launch_edges(F, case, nodes, EDGES, **over)
        print(f"[roadmap] {over}: status {got['status'].tolist()}, evals {got['evals'].tolist()}, t_free {got['t_free'].tolist()}")
        for e, (a, b) in enumerate(EDGES):
            assert not equal_entry(got, e, launch_single(F, case, nodes[a], nodes[b], **over)), (over, e)
        assert (got["evals"] == 1).all()
        assert np.isnan(got["trace_t"][:, 1:]).all()


def test_refusals(F):
    from easyhec_amd import _lib
    case = built("L2-J1")
    nodes = case_nodes(case)
    for over, msg in ((dict(depth=(5, 3)), "ehr_edge_clearance: bad budget"), (dict(max_evals=0), "bad budget"),
                      (dict(margin=0.3), "margin"), (dict(cutoff=float("inf")), "cutoff")):
        with pytest.raises(RuntimeError, match=msg):
            launch_edges(F, case, nodes, EDGES, **over)
    with pytest.raises(RuntimeError, match="V 0"):
        launch_edges(F, case, nodes[:0], EDGES)
    with pytest.raises(RuntimeError, match="ascend"):
        launch_edges(F, dict(case, offsets=np.array([0, 33, 20], np.int32)), nodes, EDGES)
    t = table_tensors(case["table"])
    p = _lib.ptr
    z = torch.zeros(64, dtype=torch.float64, device=DEV)
    args = [p(x) for x in t] + [2, 1, 2, p(z), 1, p(z), p(z), p(z), 1, p(z), case["offsets"].ctypes.data_as(ctypes.c_void_p), p(z),
                                p(z), None, 0, None, 0, 0, None, 0.25, p(z), p(z), p(z), 0.01, 3, 9, 96] + [p(z)] * 11 + \
        [None, None, None]
    assert len(args) == len(_lib.SIGNATURES["ehr_edge_clearance"][1])
    for k in (0, 9, 11, 12, 13, 17, 28, 33, 43):                                       # 9: nodes, 11, 12: the indices, 43: length
        bad = list(args)
        bad[k] = None
        assert _lib.lib().ehr_edge_clearance(*bad) != 0 and b"NULL" in _lib.lib().ehr_last_error(), k
    bad = list(args)
    bad[10] = 0
    assert _lib.lib().ehr_edge_clearance(*bad) != 0 and b"V 0" in _lib.lib().ehr_last_error()
    # ehr_roadmap_paths
    g = RR.hand_graphs()["chain"]
    for over, msg in ((dict(hops=0), "bad sizes"), (dict(hops=9), "bad sizes"), (dict(source=5), "source"), (dict(source=-1), "source")):
        with pytest.raises(RuntimeError, match="ehr_roadmap_paths: " + msg):
            launch_paths(F, g, **dict(dict(hops=2), **over))
    with pytest.raises(RuntimeError, match="bad sizes"):
        F.roadmap_paths(torch.zeros(_lib.ROADMAP_MAX_NODES + 2, dtype=torch.int32, device=DEV), dev([], np.int32), dev([], np.int32),
                        dev([], np.int32), dev([]), 0, 2)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    args = [p(zi), p(zi), p(zi), 2, p(zi), p(z), 2, 1, 0, 2] + [p(z)] + [p(zi)] * 6 + [None]
    assert len(args) == len(_lib.SIGNATURES["ehr_roadmap_paths"][1])
    for k in (0, 1, 2, 4, 5, 10, 11, 13, 16):
        bad = list(args)
        bad[k] = None
        assert _lib.lib().ehr_roadmap_paths(*bad) != 0 and b"NULL" in _lib.lib().ehr_last_error(), k
    from easyhec_amd.robot import load_robot
    robot = load_robot("xarm7")
    for kw in (dict(swept=True, detour_hops=1), dict(swept=True, detour_hops=9), dict(swept=True, detour_hops=-2),
               dict(detour_hops=3), dict(swept=True, detour_hops=2, detour_neighbours=-1)):
        with pytest.raises(ValueError, match="detour"):
            F.FeasibilityFilter(robot, **kw)
    flt = F.FeasibilityFilter(robot, swept=True, detour_hops=2)
    with pytest.raises(ValueError, match="4097 nodes"):
        flt.plan(np.zeros((4096, 7)), BENT)
    with pytest.raises(RuntimeError, match="detour_hops=0"):
        F.FeasibilityFilter(robot, swept=True).plan(np.zeros((2, 7)), BENT)


# ---- ehr_roadmap_paths ------------------------------------------------------------------------------------------------------------------
def launch_paths(F, g, hops, source=None):
    return numpy_of(F.roadmap_paths(dev(g["adj_start"], np.int32), dev(g["adj_node"], np.int32), dev(g["adj_edge"], np.int32),
                                    dev(g["status"], np.int32), dev(g["length"]), g["source"] if source is None else source, hops))


def assert_paths(what, got, g, H):
    ref = RR.paths(g["adj_start"], g["adj_node"], g["adj_edge"], g["status"], g["length"], g["V"], g["source"], H)
    bad = [k for k in ("pred_node", "pred_edge", "hops", "path", "path_edge", "changed") if not (got[k] == ref[k]).all()]
    bad += ["dist"] if not same(got["dist"], ref["dist"]).all() else []
    print(f"[roadmap] {what} H {H}: {int((ref['hops'] >= 0).sum())} of {g['V']} nodes reached, changed {ref['changed'].tolist()}, "
          f"kernel changed {got['changed'].tolist()}")
    assert not bad, (what, H, bad)
    return ref


def test_paths_on_the_hand_graphs(F):
    for name, g in RR.hand_graphs().items():
        for H in (1, 2, 3, 4, 8):
            assert_paths(name, launch_paths(F, g, H), g, H)


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 4096])
def test_paths_on_random_graphs(F, V):
    g = RR.random_graph(V, 0 if V == 1 else 3 * V, seed=V)
    for H in (1, 8):
        ref = assert_paths(f"random V {V}", launch_paths(F, g, H), g, H)
    if V > 2:
        assert (ref["hops"] > 2).any() and (ref["hops"] < 0).any() == (ref["dist"][8] == np.inf).any()


# ---- roadmap_edges ------------------------------------------------------------------------------------------------------------------------
def test_roadmap_edges_against_the_mirror(F):
    """The node sets of tests/test_roadmap_reference.py's ``test_edge_list`` through the device code: coincident nodes, nodes
    without ``ok``, too few with it, fewer other nodes than K, V = 2 and V = 1, a NaN row, K = 0, and more rows than a block."""
    rng = np.random.default_rng(5)
    V, J, K = 12, 4, 3
    nodes = rng.normal(size=(V, J))
    nodes[7] = nodes[3]
    nodes[9] = nodes[3]
    some, few = np.ones(V, bool), np.zeros(V, bool)
    some[[4, 10]] = False
    few[[0, 2, 6]] = True
    nan = nodes.copy()
    nan[5, 2] = np.nan
    big = np.random.default_rng(6).normal(size=(300, 7))
    big[17] = big[200]
    big_ok = np.random.default_rng(7).random(300) < 0.6
    cases = [("ties", nodes, some, K), ("few ok", nodes, few, K), ("none ok", nodes, np.zeros(V, bool), K),
             ("K > others", nodes[:3], np.ones(3, bool), 3), ("V = 2", nodes[:2], np.ones(2, bool), 3),
             ("V = 1", nodes[:1], np.ones(1, bool), 3), ("a NaN row", nan, some, K), ("K = 0", nodes, some, 0),
             ("K = 1", nodes, some, 1), ("K = V", nodes, some, V), ("V = 300", big, big_ok, 8)]
    for what, x, ok, k in cases:
        got = F.roadmap_edges(dev(x), torch.tensor(ok, device=DEV), k)
        torch.cuda.synchronize()
        ref = RR.edges(x, ok, k)
        bad = [n for n, g, r in zip(("edge_a", "edge_b", "adj_start", "adj_node", "adj_edge"), got, ref)
               if g.dtype != torch.int32 or g.shape != r.shape or not (g.cpu().numpy() == r).all()]
        print(f"[roadmap] edges, {what}: {int((ref[0] >= 0).sum())} of {len(ref[0])} kept, adjacency {int(ref[2][-1])} slots")
        assert not bad, (what, bad)


# ---- plan on the packaged arm -----------------------------------------------------------------------------------------------------------
def test_plan_finds_the_detour_around_the_tunnelling_obstacle(F, xarm7):
    q0, q1 = np.array([-1.5, 0.8, 0, 1.6, 0, 0, 0.0]), np.array([1.5, 0.8, 0, 1.6, 0, 0, 0.0])
    probe = F.FeasibilityFilter(xarm7, margin=0.01)
    lp, _ = joint_forward(probe._t, probe.path_table((q0 + 9 / 16 * (q1 - q0))[None])[0], probe.offsets)
    last = FR.world_spheres(lp[0], probe.spheres, probe.sphere_offsets)[probe.sphere_offsets[-2]:]
    far = int(np.argmax(np.hypot(last[:, 0], last[:, 1])))
    flt = F.FeasibilityFilter(xarm7, margin=0.01, obstacles=[[last[far, 0], last[far, 1], last[far, 2], 0.01]], swept=True,
                              detour_hops=2, detour_neighbours=1)
    plan = flt.plan(q1[None], q0, via=[VIA])
    got, direct = numpy_of(plan), numpy_of(plan.direct)
    print(f"[roadmap] tunnelling: direct status {direct['status'].tolist()} t_free {direct['t_free'].tolist()}, edges "
          f"{got['edges'].tolist()} status {got['edge_status'].tolist()} evals {got['edge_evals'].tolist()}, path "
          f"{got['path_nodes'].tolist()}, length {got['length'].tolist()}, path_cert {got['path_cert'].tolist()}")
    assert got["edges"].tolist() == [[0, 1], [0, 2], [1, 2], [-1, -1]]
    assert direct["status"][0] == 1 and 0.5 <= direct["t_free"][0] and not direct["valid"][0] and not direct["env_ok"][0]
    assert got["edge_status"].tolist() == [1, 0, 0, 3]
    assert got["reachable"][0] and got["detour"][0] and got["hops"][0] == 2 and got["path_nodes"][0].tolist() == [0, 2, 1]
    assert got["waypoints"].shape == (1, 3, flt.J)                                     # (the gripper's joints ride along at 0)
    assert (got["waypoints"][0, :, :7] == np.stack([q0, np.array(VIA, dtype=np.float64), q1])).all()
    assert (got["waypoints"][0, :, 7:] == 0).all()
    assert same(got["length"][0], RR.length(q0, VIA) + RR.length(q1, VIA)).all()
    assert flt.margin < got["path_cert"][0] <= flt.cutoff
    swept = swept_outputs(flt.check_swept(q1[None], q0))
    assert all(same(direct[k], swept[k]).all() for k in FLOATS) and all((direct[k] == swept[k]).all() for k in INTS)


def test_plan_from_the_bent_start(F, xarm7):
    K, H = 6, 4
    flt = F.FeasibilityFilter(xarm7, margin=0.01, planes=F.box_planes(*F.REFERENCE_WORKSPACE), swept=True, detour_hops=H,
                              detour_neighbours=K)
    cand = xarm7.sample_qpos(40, np.random.default_rng(0), scale=0.5)
    Q = len(cand)
    plan = flt.plan(cand, BENT)
    got, direct = numpy_of(plan), numpy_of(plan.direct)
    swept = swept_outputs(flt.check_swept(cand, BENT))
    print(f"[roadmap] bent start: {int(direct['valid'].sum())} direct, {int(got['reachable'].sum())} reachable, "
          f"{int(got['detour'].sum())} by a detour only, {int(got['end_valid'][1:].sum())} end-point valid, "
          f"{int((got['edges'][:, 0] >= 0).sum())} edges of {len(got['edges'])}, {int(got['edge_evals'].sum())} evaluations, "
          f"changed {got['changed'].tolist()}")
    for k in FLOATS + INTS + ("valid", "self_ok", "env_ok", "reach_ok"):
        assert same(direct[k], swept[k]).all() if k in FLOATS else (direct[k] == swept[k]).all(), k
    # the edge list and the adjacency are the mirror's, on the kernel's own end-point verdicts
    nodes = got["nodes"]
    assert (nodes[0, :7] == BENT).all() and (nodes[1:, :7] == cand).all() and (nodes[:, 7:] == 0).all()
    assert nodes.shape == (Q + 1, flt.J)
    assert (got["end_valid"][1:] == numpy_of(flt.check(cand))["valid"]).all() and got["end_valid"][0]
    ea, eb, start, node, edge = RR.edges(nodes, got["end_valid"], K)
    assert (got["edges"][:, 0] == ea).all() and (got["edges"][:, 1] == eb).all()
    dev_edges = F.roadmap_edges(plan.nodes, plan.end_valid, K)
    torch.cuda.synchronize()
    for mine, ref in zip(dev_edges, (ea, eb, start, node, edge)):
        assert mine.dtype == torch.int32 and (mine.cpu().numpy() == ref).all()
    # eight edges against single calls
    W = F.reach_radii(flt._table, flt.link_bounds, np.zeros(flt.J))
    kept = np.flatnonzero(ea >= 0)
    for e in kept[np.linspace(0, len(kept) - 1, 8).astype(int)]:
        one = numpy_of(F.segment_clearance(flt._t, plan.nodes[int(ea[e])], plan.nodes[int(eb[e])][None], flt.offsets, flt._spheres,
                                           flt.sphere_offsets, flt._bounds, flt._pair_enable, flt._upstream, flt._below, dev(W),
                                           flt._planes, flt._obstacles, flt.env_mask, flt._reach, flt.cutoff, flt.margin,
                                           flt.swept_depth, flt.swept_evals))
        assert (got["edge_status"][e], got["edge_evals"][e]) == (one["status"][0], one["evals"][0]), e
        assert same(got["edge_length"][e], RR.length(nodes[ea[e]], nodes[eb[e]])).all()
    assert (got["edge_status"][ea < 0] == 3).all() and np.isnan(got["edge_length"][ea < 0]).all()
    # the paths are the mirror's on the kernel's own edge results
    ref = RR.paths(start, node, edge, got["edge_status"], got["edge_length"], Q + 1, 0, H)
    assert (got["hops"] == ref["hops"][1:]).all() and (got["reachable"] == (ref["hops"][1:] >= 0)).all()
    assert (got["path_nodes"] == ref["path"][1:]).all() and same(got["length"], ref["dist"][H, 1:]).all()
    assert (got["changed"] == ref["changed"]).all() and (got["detour"] == (got["reachable"] & ~direct["valid"])).all()
    assert (got["hops"][direct["valid"]] == 1).all() and got["end_valid"][1:][got["reachable"]].all()
    found, every = numpy_of(plan.paths), numpy_of(plan.edge_clearance)
    assert (found["path_edge"] == ref["path_edge"]).all()
    least = np.minimum(every["cert_self"], every["cert_env"])
    for i in range(Q):
        h = int(got["hops"][i])
        assert np.isnan(got["waypoints"][i, h + 1:]).all()
        if h < 0:
            assert np.isnan(got["path_cert"][i]) and got["length"][i] == np.inf
            continue
        assert (got["waypoints"][i, :h + 1] == nodes[got["path_nodes"][i, :h + 1]]).all()
        assert got["path_cert"][i] == least[ref["path_edge"][i + 1, :h]].min() > flt.margin
    # via nodes come from the filter's own generator, seeded once
    a = F.FeasibilityFilter(xarm7, margin=0.01, swept=True, detour_hops=2, detour_via=3, detour_seed=7)
    b = F.FeasibilityFilter(xarm7, margin=0.01, swept=True, detour_hops=2, detour_via=3, detour_seed=7)
    pa, pa2, pb = a.plan(cand[:2], BENT), a.plan(cand[:2], BENT), b.plan(cand[:2], BENT)
    torch.cuda.synchronize()
    assert pa.nodes.shape == (6, a.J) and (pa.nodes == pb.nodes).all() and not (pa.nodes[3:] == pa2.nodes[3:]).all()
    assert pa.hops.shape == (2,) and pa.path_nodes.shape == (2, 3) and pa.waypoints.shape == (2, 3, a.J)


# ---- the online loop ----------------------------------------------------------------------------------------------------------------------
def test_online_loop_with_detours(F, xarm7):
    from easyhec_amd import render_api
    from easyhec_amd.config import XARM7_K_1280x720
    from easyhec_amd.online import OnlineCalibration
    from easyhec_amd.synthetic import camera_Tc_c2b, perturb_pose, scaled_K
    H, W = 120, 160
    K = np.array(scaled_K(XARM7_K_1280x720, 0.125, W, H, True), dtype=np.float64)
    Tc_gt = camera_Tc_c2b()
    kw = dict(margin=0.01, planes=[[0.0, 0.0, 1.0, 0.0]], swept=True, swept_depth=(3, 7), swept_evals=40)
    under = np.array([[0.0, 2.0, 0.0, 0.3, 0.0, 0.0, 0.0]])                             # folded below the table
    cand = np.concatenate([xarm7.sample_qpos(7, np.random.default_rng(1), scale=0.6), under])
    records = {}
    for hops in (3, 0):
        flt = F.FeasibilityFilter(xarm7, detour_hops=hops, detour_neighbours=3, **kw)
        asked = []

        def capture(qpos):
            asked.append(np.array(qpos))
            return render_api.nvdiffrast_render_xarm_api(None, Tc_gt, qpos, H, W, K)

        loop = OnlineCalibration(xarm7, K, H, W, perturb_pose(Tc_gt), capture, lambda _r: (cand, None), num_epochs=60,
                                 explore_iters=2, explore="information", feasible=flt)
        loop.fit(BENT)
        records[hops] = r = loop.log[0]
        print(f"[roadmap online] detour_hops {hops}: { {k: v for k, v in r.items() if k != 'path'} }")
        if hops:
            plan = flt.plan(cand, BENT)
            got, direct = numpy_of(plan), numpy_of(plan.direct)
            hit = [i for i in range(len(cand)) if (cand[i] == asked[1]).all()]
            assert len(hit) == 1 and got["reachable"][hit[0]] and not got["reachable"][-1]
            assert r["rejected_mode"] == "roadmap" and r["detours"] == int(got["detour"].sum())
            assert r["roadmap_edges"] == int((got["edges"][:, 0] >= 0).sum()) and r["undecided"] == int((direct["status"] >= 2).sum())
            for k in ("self", "env", "reach"):
                assert r["rejected_" + k] == int((~direct[k + "_ok"]).sum())
            assert r["hops"] == int(got["hops"][hit[0]]) >= 1 and len(r["path"]) == r["hops"] + 1
            assert r["path"][0][:7] == list(BENT) and r["path"][-1][:7] == asked[1].tolist()
            assert all(len(q) == flt.J and q[7:] == [0.0] * (flt.J - 7) for q in r["path"])
            assert "rejected_mode" not in loop.log[1]
    today = {"round", "frames", "mask_loss", "solve_s", "explore_s", "info_gain", "gain_mean", "candidates", "rejected_self",
             "rejected_env", "rejected_reach", "rejected_mode", "undecided"}
    assert set(records[0]) == today and records[0]["rejected_mode"] == "swept"
    assert set(records[3]) == today | {"detours", "roadmap_edges", "hops", "path"}
