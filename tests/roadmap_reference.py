"""Numpy restatements of ``feasibility.roadmap_edges`` (with its adjacency) and of ``ehr_roadmap_paths`` (include/ehr.h,
csrc/ehr_roadmap.hip), operation by operation, and the roadmap of one round on the host: the edge search itself is
``segment_clearance_reference.search``.  Every sum runs left to right in float64, so the kernels are compared bit for bit.
``hand_graphs`` are the small graphs both tests/test_roadmap_reference.py and tests/test_gpu_roadmap.py walk.  CPU only, numpy."""
import numpy as np

INF = float("inf")


# ---- roadmap_edges ------------------------------------------------------------------------------------------------------------------
def adjacency(V, ea, eb):
    """(adj_start [V+1], adj_node [2E], adj_edge [2E]) int32: both directions of every edge (a, b) with a >= 0, each node's slots
    in ascending edge index; the two slots of every skipped edge follow, in edge order, with node -1."""
    E = len(ea)
    slots = [[] for _ in range(V)]
    for e in range(E):
        if ea[e] >= 0:
            slots[ea[e]].append((eb[e], e))
            slots[eb[e]].append((ea[e], e))
    start, node, edge = [0], [], []
    for v in range(V):
        node += [u for u, _ in slots[v]]
        edge += [e for _, e in slots[v]]
        start.append(len(node))
    for e in range(E):
        if ea[e] < 0:
            node += [-1, -1]
            edge += [e, e]
    return np.array(start, np.int32), np.array(node, np.int32).reshape(-1), np.array(edge, np.int32).reshape(-1)


def edges(nodes, ok, K):
    """``feasibility.roadmap_edges`` on the host: (edge_a, edge_b, adj_start, adj_node, adj_edge)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    V, J = nodes.shape
    M = V - 1
    x = nodes[1:]
    near = []
    for v in range(M):
        others = np.array([u for u in range(M) if u != v], dtype=np.int64)
        acc = np.zeros(others.shape[0])
        for j in range(J):
            d = x[others, j] - x[v, j]
            acc = acc + d * d
        by_distance = others[np.argsort(acc, kind="stable")]
        ok_first = by_distance[np.argsort(~np.asarray(ok, dtype=bool)[by_distance + 1], kind="stable")]
        near.append([int(u) for u in ok_first[:K]])
    ea, eb = [0] * M, list(range(1, V))
    for v in range(M):
        for k in range(K):
            good = k < len(near[v])
            if good:
                u = near[v][k]
                good = bool(ok[v + 1]) and bool(ok[u + 1]) and not (u < v and v in near[u])
            ea.append(min(u, v) + 1 if good else -1)
            eb.append(max(u, v) + 1 if good else -1)
    return (np.array(ea, np.int32), np.array(eb, np.int32)) + adjacency(V, ea, eb)


def length(a, b):
    """sqrt(sum_j d_j d_j), j ascending from 0.0; NaN where an entry of either node is not finite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float("nan")
    acc = np.float64(0.0)
    for j in range(a.shape[0]):
        d = b[j] - a[j]
        acc = acc + d * d
    return float(np.sqrt(acc))


# ---- ehr_roadmap_paths ----------------------------------------------------------------------------------------------------------------
def usable(status, w):
    return status == 0 and np.isfinite(w) and w >= 0


def paths(adj_start, adj_node, adj_edge, edge_status, edge_length, V, source, H):
    """The layers, predecessors, ``changed`` and the paths, as the kernel computes them.  Returns a dict of numpy arrays."""
    A, E = len(adj_node), len(edge_status)
    w = np.asarray(edge_length, dtype=np.float64)
    dist = np.full((H + 1, V), INF)
    dist[0, source] = 0.0
    pn, pe = np.full((H, V), -1, np.int32), np.full((H, V), -1, np.int32)
    changed = np.zeros(H, np.int32)
    for r in range(1, H + 1):
        for v in range(V):
            best, bn, be = dist[r - 1, v], -1, -1
            for i in range(max(int(adj_start[v]), 0), min(int(adj_start[v + 1]), A)):
                u, e = int(adj_node[i]), int(adj_edge[i])
                if not (0 <= u < V and 0 <= e < E) or not usable(int(edge_status[e]), w[e]):
                    continue
                c = dist[r - 1, u] + w[e]
                if c < best:
                    best, bn, be = c, u, e
            dist[r, v], pn[r - 1, v], pe[r - 1, v] = best, bn, be
            changed[r - 1] += bn >= 0
    hops = np.full(V, -1, np.int32)
    path, path_edge = np.full((V, H + 1), -1, np.int32), np.full((V, H), -1, np.int32)
    for v in range(V):
        r, x, nodes_back, edges_back = H, v, [v], []
        while x != source:
            while r > 0 and pn[r - 1, x] < 0:
                r -= 1
            if r == 0:
                break
            edges_back.append(int(pe[r - 1, x]))
            x = int(pn[r - 1, x])
            nodes_back.append(x)
            r -= 1
        if x != source:
            continue
        hops[v] = len(edges_back)
        path[v, :len(nodes_back)] = nodes_back[::-1]
        path_edge[v, :len(edges_back)] = edges_back[::-1]
    return {"dist": dist, "pred_node": pn, "pred_edge": pe, "hops": hops, "path": path, "path_edge": path_edge, "changed": changed}


def brute_force(V, ea, eb, edge_status, edge_length, source, H):
    """[V]: the least left-to-right float sum over all simple paths of at most H usable edges from ``source``; inf: none."""
    best = np.full(V, INF)
    best[source] = 0.0
    good = [e for e in range(len(ea)) if 0 <= ea[e] < V and 0 <= eb[e] < V and usable(int(edge_status[e]), edge_length[e])]

    def walk(x, acc, seen, left):
        if acc < best[x]:
            best[x] = acc
        if not left:
            return
        for e in good:
            for a, b in ((ea[e], eb[e]), (eb[e], ea[e])):
                if a == x and b not in seen:
                    walk(b, acc + np.float64(edge_length[e]), seen | {b}, left - 1)
    walk(source, np.float64(0.0), {source}, H)
    return best


def sum_along(path_edge_row, edge_length):
    acc = np.float64(0.0)
    for e in path_edge_row:
        if e >= 0:
            acc = acc + np.float64(edge_length[e])
    return float(acc)


def graph(V, edge_list, status=None, lengths=None, source=0):
    ea, eb = [a for a, _ in edge_list], [b for _, b in edge_list]
    E = len(edge_list)
    start, node, edge = adjacency(V, ea, eb)
    return {"V": V, "ea": np.array(ea, np.int32).reshape(-1), "eb": np.array(eb, np.int32).reshape(-1), "adj_start": start,
            "adj_node": node, "adj_edge": edge, "source": source,
            "status": np.zeros(E, np.int32) if status is None else np.array(status, np.int32),
            "length": np.ones(E) if lengths is None else np.array(lengths, dtype=np.float64)}


def hand_graphs():
    """name -> graph (see tests/test_roadmap_reference.py for what each must give)."""
    out = {}
    out["chain"] = graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)], lengths=[0.1, 0.2, 0.3, 0.4])
    out["short-3-against-long-1"] = graph(4, [(0, 3), (0, 1), (1, 2), (2, 3)], lengths=[1.0, 0.1, 0.2, 0.3])
    out["two-equal-routes"] = graph(4, [(0, 1), (0, 2), (2, 3), (1, 3)], lengths=[0.5, 0.5, 0.25, 0.25])
    # node 1 only over bad edges, node 2 over the one good edge among them
    out["unusable"] = graph(3, [(0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 2)], status=[1, 2, 3, 0, 0, 0, 0],
                            lengths=[1.0, 1.0, 1.0, float("nan"), -1.0, INF, 2.0])
    # slots: node 0: 0 1 2, node 1: 3 4, node 2: 5 (from 1 over edge 1), 6 (from 0 over edge 2), 7 (from 0 over edge 3)
    g = graph(3, [(0, 1), (1, 2), (0, 2), (0, 2)], lengths=[1.0, 1.0, 5.0, 4.0])
    g["adj_node"][5] = 3           # node 2's short route names node V
    g["adj_edge"][7] = 4           # its 4.0 route names edge E: the 5.0 route is what is left
    g["adj_node"][4] = -1
    out["indices-out-of-range"] = g
    out["isolated-source"] = graph(3, [(1, 2)], source=0)
    out["one-node"] = graph(1, [])
    out["duplicates"] = graph(3, [(0, 1), (0, 1), (1, 2), (1, 2)], lengths=[2.0, 1.0, 3.0, 3.0])
    out["source-2"] = graph(4, [(0, 1), (1, 2), (2, 3)], lengths=[1.0, 2.0, 4.0], source=2)
    return out


def random_graph(V, E, seed, bad=0.3):
    rng = np.random.default_rng(seed)
    el = [(int(a), int(b)) for a, b in rng.integers(0, V, (E, 2))] if V > 0 else []
    status = np.where(rng.random(E) < bad, rng.integers(1, 4, E), 0)
    return graph(V, el, status=status, lengths=rng.uniform(0.05, 2.0, E), source=int(rng.integers(0, V)))


# ---- one round's roadmap on the host --------------------------------------------------------------------------------------------------
def roadmap(table, tab, nodes, ok, K, H, margin, depth, max_evals, offset=None):
    """(edge_a, edge_b, results, paths): ``edges``, ``segment_clearance_reference.search`` on the host's kinematics for every
    edge that is not skipped (None for those), and ``paths`` on their status and ``length``."""
    import segment_clearance_reference as SR
    nodes = np.asarray(nodes, dtype=np.float64)
    ea, eb, start, node, edge = edges(nodes, ok, K)
    results, status, w = [], [], []
    for a, b in zip(ea, eb):
        if a < 0:
            results.append(None)
            status.append(3)
            w.append(float("nan"))
            continue
        res = SR.search(SR.host_kin(table, nodes[a], nodes[b], offset), tab, nodes[b] - nodes[a], margin, depth[0], depth[1], max_evals)
        results.append(res)
        status.append(res["status"])
        w.append(length(nodes[a], nodes[b]))
    return ea, eb, results, paths(start, node, edge, np.array(status, np.int32), np.array(w), nodes.shape[0], 0, H)
