"""The numpy mirrors of tests/roadmap_reference.py, pinned on the CPU: the layered shortest paths against brute force over all
simple paths and on hand graphs, the edge list of ``roadmap_edges``, and the roadmap itself on the xArm7 with the host's
kinematics and ``segment_clearance_reference.search`` -- the detour around the tunnelling obstacle, and 40 candidates from the
bent start.  tests/test_gpu_roadmap.py holds the kernels against these mirrors bit for bit."""
import numpy as np
import pytest

import feasibility_reference as F
import joint_reference as JR
import roadmap_reference as RR
import segment_clearance_reference as SR
from test_segment_clearance_reference import BENT, CUTOFF, MARGIN, arm, padded, tunnelling_case

INF = float("inf")


def run(g, H):
    return RR.paths(g["adj_start"], g["adj_node"], g["adj_edge"], g["status"], g["length"], g["V"], g["source"], H)


def consistent(g, out, H):
    """What holds on every graph: dist[H] is the sum along path_edge, the path is made of usable edges between its nodes, hops
    counts them, layers never grow and ``changed`` counts the nodes that fell."""
    V = g["V"]
    for v in range(V):
        h = int(out["hops"][v])
        if h < 0:
            assert out["dist"][H, v] == INF and (out["path"][v] == -1).all() and (out["path_edge"][v] == -1).all()
            continue
        assert out["path"][v, 0] == g["source"] and out["path"][v, h] == v and (out["path"][v, h + 1:] == -1).all()
        assert (out["path_edge"][v, h:] == -1).all() and 0 <= h <= H
        assert out["dist"][H, v] == RR.sum_along(out["path_edge"][v], g["length"])
        for k in range(h):
            e, a, b = int(out["path_edge"][v, k]), int(out["path"][v, k]), int(out["path"][v, k + 1])
            assert RR.usable(int(g["status"][e]), g["length"][e]) and {int(g["ea"][e]), int(g["eb"][e])} == {a, b}
    assert out["hops"][g["source"]] == 0
    for r in range(1, H + 1):
        assert (out["dist"][r] <= out["dist"][r - 1]).all()
        assert out["changed"][r - 1] == int((out["dist"][r] < out["dist"][r - 1]).sum()) == int((out["pred_node"][r - 1] >= 0).sum())


# ---- ehr_roadmap_paths' mirror ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(40))
def test_paths_mirror_against_brute_force(seed):
    rng = np.random.default_rng(1000 + seed)
    V = int(rng.integers(1, 8))
    g = RR.random_graph(V, int(rng.integers(0, 13)), seed, bad=0.35)
    for H in (1, 2, 3, 4):
        out = run(g, H)
        want = RR.brute_force(V, g["ea"], g["eb"], g["status"], g["length"], g["source"], H)
        assert (out["dist"][H] == want).all(), (seed, H, out["dist"][H].tolist(), want.tolist())
        consistent(g, out, H)


def test_hand_graphs():
    G = RR.hand_graphs()
    g = G["chain"]
    two, four = run(g, 2), run(g, 4)
    assert two["hops"].tolist() == [0, 1, 2, -1, -1] and two["dist"][2, 3] == INF
    assert four["hops"].tolist() == [0, 1, 2, 3, 4] and four["path"][4].tolist() == [0, 1, 2, 3, 4]
    assert four["dist"][4, 4] == ((0.1 + 0.2) + 0.3) + 0.4 and four["path_edge"][4].tolist() == [0, 1, 2, 3]
    assert two["changed"].tolist() == [1, 1] and four["changed"].tolist() == [1, 1, 1, 1]
    assert run(g, 8)["changed"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]

    g = G["short-3-against-long-1"]                      # the answer changes with H
    for H, path, d in ((1, [0, 3], 1.0), (2, [0, 3], 1.0), (3, [0, 1, 2, 3], (0.1 + 0.2) + 0.3)):
        out = run(g, H)
        assert out["path"][3, :len(path)].tolist() == path and out["dist"][H, 3] == d and out["hops"][3] == len(path) - 1
        consistent(g, out, H)
    # a path found early and improved late: rounds 1 and 3 record node 3, round 2 carries it
    assert run(g, 3)["pred_node"][:, 3].tolist() == [0, -1, 2]

    g = G["two-equal-routes"]                            # node 3's slots: edge 2 (from node 2) before edge 3 (from node 1)
    out = run(g, 2)
    assert out["path"][3].tolist() == [0, 2, 3] and out["path_edge"][3].tolist() == [1, 2] and out["dist"][2, 3] == 0.75
    consistent(g, out, 2)

    g = G["unusable"]                                    # status 1, 2, 3, NaN, negative, infinite: skipped
    out = run(g, 3)
    assert out["hops"].tolist() == [0, -1, 1] and out["dist"][3].tolist() == [0.0, INF, 2.0] and out["changed"].tolist() == [1, 0, 0]
    consistent(g, out, 3)

    g = G["indices-out-of-range"]
    out = run(g, 2)
    assert out["dist"][2].tolist() == [0.0, 1.0, 5.0] and out["path_edge"][2].tolist() == [2, -1]

    out = run(G["isolated-source"], 2)
    assert out["hops"].tolist() == [0, -1, -1] and out["changed"].tolist() == [0, 0] and out["path"][0].tolist() == [0, -1, -1]

    out = run(G["one-node"], 1)
    assert out["hops"].tolist() == [0] and out["dist"].tolist() == [[0.0], [0.0]] and out["path"].tolist() == [[0, -1]]

    g = G["duplicates"]                                  # the shorter copy; of two equal copies the lower slot
    out = run(g, 2)
    assert out["path_edge"][1].tolist() == [1, -1] and out["path_edge"][2].tolist() == [1, 2] and out["dist"][2, 2] == 4.0
    consistent(g, out, 2)

    g = G["source-2"]
    out = run(g, 2)
    assert out["hops"].tolist() == [2, 1, 0, 1] and out["path"][0].tolist() == [2, 1, 0] and out["dist"][2, 0] == 3.0
    consistent(g, out, 2)


# ---- roadmap_edges' mirror ------------------------------------------------------------------------------------------------------------
def test_edge_list():
    rng = np.random.default_rng(5)
    V, J, K = 12, 4, 3
    nodes = rng.normal(size=(V, J))
    nodes[7] = nodes[3]                                  # exact ties: 3, 7 and 9 coincide
    nodes[9] = nodes[3]
    ok = np.ones(V, bool)
    ok[[4, 10]] = False
    ea, eb, start, node, edge = RR.edges(nodes, ok, K)
    E = (V - 1) * (1 + K)
    assert ea.shape == eb.shape == (E,) and ea[:V - 1].tolist() == [0] * (V - 1) and eb[:V - 1].tolist() == list(range(1, V))
    kept = [(int(a), int(b)) for a, b in zip(ea[V - 1:], eb[V - 1:]) if a >= 0]
    assert len(set(kept)) == len(kept) and all(1 <= a < b for a, b in kept), "no undirected pair twice"
    assert all(ok[a] and ok[b] for a, b in kept) and ((ea < 0) == (eb < 0)).all() and set(ea[ea < 0].tolist()) <= {-1}
    assert (ea[V - 1:] < 0).any() and not any(4 in p or 10 in p for p in kept)
    # every node with ok is joined to each of its K nearest nodes with ok (they come before the others), by its own slot or
    # the partner's
    d2 = ((nodes[:, None] - nodes[None]) ** 2).sum(axis=2)
    for v in np.flatnonzero(ok[1:]) + 1:
        others = [u for u in range(1, V) if u != v and ok[u]]
        for u in sorted(others, key=lambda u: d2[v, u])[:K]:
            assert (min(u, v), max(u, v)) in kept, (v, u)
    # too few nodes with ok: the others fill the list and their slots are skipped
    few = np.zeros(V, bool)
    few[[0, 2, 6]] = True
    fa, fb, *_ = RR.edges(nodes, few, K)
    assert [(int(a), int(b)) for a, b in zip(fa[V - 1:], fb[V - 1:]) if a >= 0] == [(2, 6)]
    # ties go to the lower index: 3, 7 and 9 coincide, so 3 lists 7 then 9, 7 lists 3 then 9, 9 lists 3 then 7
    slot = lambda v, k: (int(ea[V - 1 + (v - 1) * K + k]), int(eb[V - 1 + (v - 1) * K + k]))
    assert [slot(3, 0), slot(3, 1)] == [(3, 7), (3, 9)]
    assert [slot(7, 0), slot(7, 1)] == [(-1, -1), (7, 9)] and [slot(9, 0), slot(9, 1)] == [(-1, -1), (-1, -1)]
    # the adjacency: both directions, ascending edge index per node, skipped edges past adj_start[V]
    assert start[0] == 0 and start[V] == 2 * int((ea >= 0).sum()) and node.shape == edge.shape == (2 * E,)
    for v in range(V):
        sl = slice(start[v], start[v + 1])
        assert (np.diff(edge[sl]) > 0).all()
        assert [(int(u), int(e)) for u, e in zip(node[sl], edge[sl])] == \
            [(int(eb[e] if ea[e] == v else ea[e]), e) for e in range(E) if v in (ea[e], eb[e])]
    assert (node[start[V]:] == -1).all() and sorted(edge[start[V]:].tolist()) == sorted(2 * np.flatnonzero(ea < 0).tolist())
    # fewer other nodes than K: the slots that have no neighbour are skipped
    ea2, eb2, *_ = RR.edges(nodes[:3], np.ones(3, bool), 3)
    assert list(zip(ea2.tolist(), eb2.tolist())) == [(0, 1), (0, 2), (1, 2), (-1, -1), (-1, -1), (-1, -1), (-1, -1), (-1, -1)]
    assert RR.edges(nodes[:1], np.ones(1, bool), 3)[0].shape == (0,)


# ---- the roadmap on the xArm7, host kinematics ------------------------------------------------------------------------------------------
def end_valid(table, parts, tab, nodes):
    _, lp, _ = JR.fk(table, nodes)
    raw = F.clearance(lp.astype(np.float32), parts["spheres"], parts["offsets"], parts["pair_enable"], tab["planes"], tab["obstacles"],
                      parts["env_links"], tab["reach"], CUTOFF)
    return F.reduce_steps(*raw, 1, MARGIN)["valid"]


def test_detour_around_the_tunnelling_obstacle():
    from easyhec_amd import _lib
    assert _lib.has_roadmap(), "libehr_hip.so must export ehr_edge_clearance and ehr_roadmap_paths"
    robot, table, q0, q1, obstacle = tunnelling_case()
    _, tab, parts = SR.robot_case(robot, obstacles=obstacle)
    nodes = np.stack([q0, q1, padded(robot, (0, 0.5, 0, 1.6, 0, 0, 0))])
    ok = np.concatenate([[True], end_valid(table, parts, tab, nodes[1:])])
    assert ok.all()
    ea, eb, res, out = RR.roadmap(table, tab, nodes, ok, 1, 2, MARGIN, (3, 9), 96)
    assert list(zip(ea.tolist(), eb.tolist())) == [(0, 1), (0, 2), (1, 2), (-1, -1)]
    print(f"[roadmap] tunnelling: direct status {res[0]['status']} after {res[0]['evals']} evaluations, t_free {res[0]['t_free']}; "
          f"legs {[(r['status'], r['evals']) for r in res[1:3]]}")
    assert res[0]["status"] == 1 and 0.5 <= res[0]["t_free"]
    assert res[1]["status"] == 0 and res[2]["status"] == 0 and res[3] is None
    assert out["path"][1].tolist() == [0, 2, 1] and out["hops"][1] == 2 and out["path_edge"][1].tolist() == [1, 2]
    assert out["hops"][1] >= 0 and res[0]["status"] != 0, "reachable, and only by a detour"
    assert out["dist"][2, 1] == RR.length(nodes[0], nodes[2]) + RR.length(nodes[1], nodes[2])


def test_forty_candidates_from_the_bent_start():
    """Here: 8 direct, 10 reachable, 13 end-point valid, 86 edges."""
    robot, table, tab, parts = arm("xarm7")
    cand = robot.sample_qpos(40, np.random.default_rng(0), scale=0.5)
    nodes = np.stack([padded(robot, BENT)] + [padded(robot, c) for c in cand])
    ok = np.concatenate([[True], end_valid(table, parts, tab, nodes[1:])])
    H = 4
    ea, eb, res, out = RR.roadmap(table, tab, nodes, ok, 6, H, MARGIN, (3, 9), 96)
    status = np.array([3 if r is None else r["status"] for r in res])
    direct, hops = status[:40] == 0, out["hops"][1:]
    reachable = hops >= 0
    print(f"[roadmap] bent start: {int(direct.sum())} direct, {int(reachable.sum())} reachable, {int(ok[1:].sum())} end-point valid, "
          f"{int((ea >= 0).sum())} edges, {sum(r['evals'] for r in res if r)} evaluations, changed {out['changed'].tolist()}")
    assert ok[1:][reachable].all(), "every reachable candidate is end-point valid"
    assert (hops[direct] == 1).all(), "every directly clear candidate is reachable with 1 hop"
    assert (reachable & ~direct).any(), "a candidate only a detour reaches"
    assert out["changed"][3] == 0
    for v in np.flatnonzero(reachable) + 1:
        assert out["dist"][H, v] == RR.sum_along(out["path_edge"][v], [RR.length(nodes[a], nodes[b]) if a >= 0 else np.nan
                                                                     for a, b in zip(ea, eb)])
